"""The closest-point query on the GPU (``include/qf_closest_point.h``) against its numpy restatement
``tests/closest_point_reference.py``: ``tri``, ``bary``, ``dist2`` and ``counts`` bit for bit on every case of
``tests/test_closest_point_host.py`` and on meshes that exercise the tree (1, 8, 9 and 65 triangles, duplicated and
zero-area faces, the singular meshes, a lattice grid where every query is a many-way tie, the level-5 icosphere); the
same bytes from every tree and after a refit; ``max_distance``; the table transfer, the mesh distance and the example.

The restatement is brute force over all pairs; on the large meshes it runs with ``prefilter=True``, which drops pairs
by the bounding-box premise and is checked against the plain loop on the host."""
import functools
import importlib.util
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import closest_point_cases as cases
from tests import closest_point_reference as cp
from tests import singular_meshes as sm

pytestmark = pytest.mark.gpu

F32, F64 = np.float32, np.float64
EPS32, EPS64 = float(np.finfo(np.float32).eps), float(np.finfo(np.float64).eps)


def _intersector(vertices, faces, device, **kw):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    return RayIntersector(TriMesh(np.asarray(vertices, F64), np.asarray(faces, np.int64)), device=device, **kw)


def _query(inter, points, max_distance=math.inf):
    """The device's answer as the restatement returns it: (tri int32, bary, dist2, counts) on the host."""
    out = inter.closest_points(torch.from_numpy(np.array(points, F64)).to(inter.device), max_distance)
    assert out.tri.dtype == torch.int64 and out.bary.dtype == out.dist2.dtype == torch.float64 and out.counts.dtype == torch.int64
    assert all(t.is_cuda for t in out)
    return out.tri.cpu().numpy().astype(np.int32), out.bary.cpu().numpy(), out.dist2.cpu().numpy(), out.counts.cpu().numpy()


def _assert_same(got, want, what=""):
    for name, g, w in zip(("tri", "bary", "dist2", "counts"), got, want):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g.reshape(g.shape[0], -1) != w.reshape(w.shape[0], -1)).any(axis=1))[0]
            raise AssertionError(f"{what}: {name} differs in {bad.size} rows, first {bad[:5].tolist()}: "
                                 f"{g[bad[:3]].tolist()} != {w[bad[:3]].tolist()}")


def _check(vertices, faces, points, device, what, prefilter=False, max_distance=math.inf, **kw):
    inter = _intersector(vertices, faces, device, **kw)
    got = _query(inter, points, max_distance)
    want = cp.closest_points(cp.triangles_of(vertices, faces), points, max_distance, prefilter=prefilter)
    _assert_same(got, want, what)
    return inter, got


# ---------------------------------------------------------------------------------------------- the host tests' cases
def test_hand_worked_triangle(device):
    q = np.array([h[0] for h in cases.HAND], F64)
    _, got = _check(cases.HAND_TRIANGLE[0], [[0, 1, 2]], q, device, "hand")
    assert got[2].tolist() == [h[3] for h in cases.HAND] and got[1][:, 1:].tolist() == [list(h[2]) for h in cases.HAND]


@pytest.mark.parametrize("name", sorted(cases.zero_area_triangles()))
def test_zero_area_triangles(device, name):
    t32 = cases.zero_area_triangles()[name]
    _, got = _check(t32[0], [[0, 1, 2]], cases.box_queries(100_000, seed=3), device, name)
    assert np.isfinite(got[2]).all() and got[3].tolist() == [0, 0]


def test_noise_triangles(device):
    rng = np.random.default_rng(5)
    t32 = rng.uniform(-1, 1, (65, 3, 3)).astype(F32)
    t32[:, 2] = t32[:, 0] + rng.uniform(0, 1, (65, 1)).astype(F32) * (t32[:, 1] - t32[:, 0])
    _check(t32.reshape(-1, 3), np.arange(195).reshape(65, 3), cases.box_queries(4096, seed=6), device, "noise")


def test_grid_ties_and_the_duplicated_face(device):
    v, f = cases.grid_mesh(5)
    q, want, height = cases.grid_tie_queries(5)
    _, got = _check(v, f, q, device, "grid")
    assert np.array_equal(got[0], want) and np.array_equal(got[2], height * height)
    v, f = cases.duplicated_face_mesh(5, 7)
    q = np.concatenate([q, cases.box_queries(2048, seed=8, half=1.0) * [1, 1, 0.25] + [0.5, 0.5, 0]])
    _, got = _check(v, f, q, device, "duplicated face")
    assert (got[0] != f.shape[0] - 1).all() and (got[0] == 7).any()


def test_level_2_sphere_against_brute_force(device):
    v, f = cases.sphere(2)
    _check(v, f, cases.box_queries(4096, seed=9), device, "sphere2")


# ------------------------------------------------------------------------------------------------------------ query sets
@functools.lru_cache(maxsize=None)
def _sphere3_reference():
    v, f = cases.sphere(3)
    rng = np.random.default_rng(21)
    far = cases.box_queries(512, seed=22, half=100.0)
    bad = cases.box_queries(64, seed=23)
    bad[rng.integers(0, 64, 24), rng.integers(0, 3, 24)] = np.tile([np.nan, np.inf, -np.inf], 8)
    q = np.concatenate([cases.sphere_feature_queries(3), far, bad])
    q.setflags(write=False)
    return q, cp.closest_points(cp.triangles_of(v, f), q, prefilter=True), int((~np.isfinite(bad).all(axis=1)).sum())


def test_queries_on_the_surface_far_outside_and_not_finite(device):
    v, f = cases.sphere(3)
    q, want, n_bad = _sphere3_reference()
    got = _query(_intersector(v, f, device), q)
    _assert_same(got, want, "sphere3")
    n_v = v.shape[0]
    assert (got[2][:n_v] == 0).all() and np.isin(got[1][:n_v], (0.0, 1.0)).all()           # the vertices the tree holds
    assert got[2][n_v:n_v + 4 * f.shape[0]].max() <= (8 * EPS64) ** 2                      # edge midpoints and centroids
    assert got[3].tolist() == [n_bad, 0] and n_bad > 0 and (got[0] < 0).sum() == n_bad


@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 63, 64, 65, 4096])
def test_every_query_count(device, n):
    v, f = cases.sphere(2)
    q = cases.box_queries(4096, seed=9)[:n]
    got = _query(_intersector(v, f, device), q)
    want = _sphere2_reference()
    _assert_same(got, (want[0][:n], want[1][:n], want[2][:n], want[3]), f"N={n}")


@functools.lru_cache(maxsize=None)
def _sphere2_reference():
    v, f = cases.sphere(2)
    return cp.closest_points(cp.triangles_of(v, f), cases.box_queries(4096, seed=9))


# ---------------------------------------------------------------------------------------------------------------- meshes
@pytest.mark.parametrize("name", sorted(cases.small_meshes()))
def test_small_meshes_around_the_leaf_size(device, name):
    v, f = cases.small_meshes()[name]
    _check(v, f, cases.box_queries(1024, seed=31), device, name)
    _check(v, f, cases.box_queries(1024, seed=31), device, name + " device-built", builder="device")


def test_a_handle_without_triangles_and_no_queries(device, lib):
    """Through the C ABI: n_tri == 0 (host- and device-built) and N == 0 are valid and still write the counts."""
    import ctypes
    from quadraturefields_amd import _C
    q = cases.box_queries(9, seed=32)
    q[4, 0] = np.nan
    pts = torch.from_numpy(q).to(device)
    for create in (lambda h: lib.qf_bvh_create_ex(None, 0, 32, ctypes.byref(h)),
                   lambda h: lib.qf_bvh_create_device(None, 0, _C.stream(), ctypes.byref(h))):
        handle = ctypes.c_void_p()
        _C.check(create(handle), "create")
        try:
            tri = torch.full((9,), 5, dtype=torch.int32, device=device)
            bary = torch.full((9, 3), 5.0, dtype=torch.float64, device=device)
            dist2 = torch.full((9,), 5.0, dtype=torch.float64, device=device)
            counts = torch.full((2,), 5, dtype=torch.int64, device=device)
            _C.check(lib.qf_bvh_closest_points(handle, _C.ptr(pts), 9, math.inf, _C.ptr(tri), _C.ptr(bary), _C.ptr(dist2),
                                               _C.ptr(counts), _C.stream()), "qf_bvh_closest_points")
            assert (tri == -1).all() and not bary.any() and torch.isinf(dist2).all() and counts.tolist() == [1, 8]
            counts.fill_(5)
            _C.check(lib.qf_bvh_closest_points(handle, None, 0, math.inf, None, None, None, _C.ptr(counts), _C.stream()),
                     "qf_bvh_closest_points")
            assert counts.tolist() == [0, 0]
            assert lib.qf_bvh_closest_points(handle, _C.ptr(pts), 9, -1.0, _C.ptr(tri), _C.ptr(bary), _C.ptr(dist2),
                                             _C.ptr(counts), _C.stream()) == -1
            assert lib.qf_bvh_closest_points(handle, None, 9, 1.0, _C.ptr(tri), _C.ptr(bary), _C.ptr(dist2),
                                             _C.ptr(counts), _C.stream()) == -1
            assert counts.tolist() == [0, 0]                                   # a refusal launches nothing
            torch.cuda.synchronize()
        finally:
            lib.qf_bvh_destroy(handle)


@pytest.mark.parametrize("name", sorted(sm.MESHES))
def test_singular_meshes(device, name):
    v, f, _ = sm.mesh(name, junk=True)
    lo, hi = v.min(axis=0).astype(F64), v.max(axis=0).astype(F64)
    rng = np.random.default_rng(41)
    lattice = np.round(rng.uniform(lo - 0.25, hi + 0.25, (1024, 3)) / sm.PITCH[name]) * sm.PITCH[name]
    q = np.concatenate([rng.uniform(lo - 0.5, hi + 0.5, (1024, 3)), lattice, v.astype(F64)[:512]])
    _check(v, f, q, device, name, prefilter=True)


def test_lattice_grid_where_every_query_ties(device):
    v, f = cases.grid_mesh(65)                                     # 64 x 64 cells, 8 192 faces
    rng = np.random.default_rng(42)
    ij = rng.integers(0, 65, (2048, 2))
    q = np.concatenate([ij / 64.0, rng.integers(0, 3, (2048, 1)) / 4.0], axis=1)      # on and above lattice vertices
    _, got = _check(v, f, q, device, "grid65", prefilter=True)
    assert np.array_equal(got[2], q[:, 2] ** 2)
    incident = np.array([np.nonzero((f == j * 65 + i).any(axis=1))[0][0] for i, j in ij[:64]])
    assert np.array_equal(got[0][:64], incident)


@functools.lru_cache(maxsize=None)
def _sphere5_reference():
    v, f = cases.sphere(5)
    q = cases.box_queries(2048, seed=43)
    return q, cp.closest_points(cp.triangles_of(v, f), q, prefilter=True)


def test_level_5_sphere(device):
    v, f = cases.sphere(5)
    q, want = _sphere5_reference()
    assert f.shape[0] == 20480
    _assert_same(_query(_intersector(v, f, device), q), want, "sphere5")


# --------------------------------------------------------------------------------------------- tree and state independence
def test_every_tree_gives_the_same_bytes(device):
    v, f = cases.sphere(5)
    q, want = _sphere5_reference()
    for kw in (dict(sah_depth=1), dict(builder="device")):
        inter = _intersector(v, f, device, **kw)
        first = _query(inter, q)
        _assert_same(first, want, str(kw))
        _assert_same(_query(inter, q), first, "second run")


def test_refit_and_rebuild_answer_for_the_new_vertices(device):
    v, f = cases.sphere(3)
    q = _sphere3_reference()[0][-1024:]
    moved = (v + np.random.default_rng(51).uniform(-0.02, 0.02, v.shape)).astype(F32)
    want = cp.closest_points(cp.triangles_of(moved, f), q, prefilter=True)
    for builder in ("host", "device"):
        inter = _intersector(v, f, device, builder=builder)
        inter.update_intersector(torch.from_numpy(moved).to(device))             # device refit
        _assert_same(_query(inter, q), want, builder + " device refit")
        inter.update_intersector(v.astype(F32))                                  # host refit, back again
        _assert_same(_query(inter, q), cp.closest_points(cp.triangles_of(v, f), q, prefilter=True), builder + " host refit")
        inter.rebuild(torch.from_numpy(moved).to(device))
        _assert_same(_query(inter, q), want, builder + " rebuild")


def test_mesh_intersection_forwards(device):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    v, f = cases.sphere(2)
    mi = MeshIntersection(TriMesh(v, f), simplify_mesh=False, num_intersections=4, device=device)
    q = torch.from_numpy(cases.box_queries(64, seed=9)).to(device)
    a, b = mi.closest_points(q, 0.75), mi.rayintersector.closest_points(q.to(torch.float32).to(torch.float64), 0.75)
    want = _sphere2_reference()
    within = want[2][:64] <= 0.75 ** 2
    assert np.array_equal(a.tri.cpu().numpy(), np.where(within, want[0][:64], -1))
    q32 = q.to(torch.float32)                                                    # fp32 queries are widened exactly
    c = mi.closest_points(q32)
    _assert_same(_query(mi.rayintersector, q32.cpu().numpy().astype(F64)), (c.tri.cpu().numpy().astype(np.int32), c.bary.cpu().numpy(),
                                                                            c.dist2.cpu().numpy(), c.counts.cpu().numpy()), "fp32")
    assert b.tri.shape == a.tri.shape
    for bad in (-1.0, float("nan")):
        with pytest.raises(ValueError):
            mi.closest_points(q, bad)


# ---------------------------------------------------------------------------------------------------------- max_distance
def test_max_distance_splits_exactly(device):
    v, f = cases.sphere(3)
    q, free, n_bad = _sphere3_reference()
    inter = _intersector(v, f, device)
    zero = _query(inter, q, 0.0)
    assert np.array_equal(zero[0] >= 0, free[2] == 0) and (zero[0] >= 0).sum() >= v.shape[0]
    assert zero[3].tolist() == [n_bad, int((free[2] > 0).sum()) - n_bad]
    for reach in (1e-9, 0.05, 0.5, 3.0, 150.0):
        got = _query(inter, q, reach)
        within = free[2] <= reach * reach
        want = (np.where(within, free[0], -1).astype(np.int32), np.where(within[:, None], free[1], 0.0),
                np.where(within, free[2], np.inf), np.array([n_bad, int((~within).sum()) - n_bad], np.int64))
        _assert_same(got, want, f"max_distance {reach}")
    assert 0 < int((free[2] <= 0.05 ** 2).sum()) < int((free[2] <= 3.0 ** 2).sum()) < q.shape[0] - n_bad


# -------------------------------------------------------------------------------------------------------------- transfer
def test_identity_transfer_is_bit_for_bit(device):
    from quadraturefields_amd import baking
    v, f = cases.sphere(3)
    inter = _intersector(v, f, device, builder="device")
    table = torch.from_numpy(np.random.default_rng(61).normal(size=(v.shape[0], 46)).astype(F32)).to(device)
    dst = torch.from_numpy(v.astype(F32)).to(device)
    got = baking.transfer_vertex_features(inter, table, dst)
    assert got.dtype == torch.float32 and got.shape == table.shape and got.cpu().numpy().tobytes() == table.cpu().numpy().tobytes()
    want = cp.transfer(cp.triangles_of(v, f), f, table.cpu().numpy(), v.astype(F32).astype(F64))
    assert got.cpu().numpy().tobytes() == want.tobytes()
    with pytest.raises(ValueError, match="have no source triangle"):
        baking.transfer_vertex_features(inter, table, dst * 1.5, max_distance=0.1)
    with pytest.raises(ValueError):
        baking.transfer_vertex_features(inter, table[:-1], dst)


def test_affine_table_on_a_decimated_sphere(device):
    """row = A p + b on the level-4 icosphere, carried to its decimation: A c + b at the closest point c within
    8 eps32 max|row| (the bound of tests/test_closest_point_host.py), and the restatement's bits."""
    from quadraturefields_amd import baking, mc_utils
    v, f = cases.sphere(4)
    out = mc_utils.decimate_mesh_device(torch.from_numpy(v).to(device), torch.from_numpy(f).to(device), f.shape[0] // 4)
    assert out.faces.shape[0] <= f.shape[0] // 4 + 2
    rng = np.random.default_rng(62)
    A, b = rng.normal(size=(7, 3)), rng.normal(size=7)
    table = (v.astype(F32).astype(F64) @ A.T + b).astype(F32)
    inter = _intersector(v, f, device)
    got = baking.transfer_vertex_features(inter, torch.from_numpy(table).to(device), out.vertices).cpu().numpy()
    dst = out.vertices.cpu().numpy()
    t32 = cp.triangles_of(v, f)
    tri, bary, dist2, _ = cp.closest_points(t32, dst, prefilter=True)
    fb = bary.astype(F32)
    rows = table[f[tri]]
    assert got.tobytes() == ((fb[:, 0:1] * rows[:, 0] + fb[:, 1:2] * rows[:, 1]) + fb[:, 2:3] * rows[:, 2]).tobytes()
    c = (bary[:, :, None] * t32.astype(F64)[tri]).sum(axis=1)
    err, bound = np.abs(got.astype(F64) - (c @ A.T + b)).max(), 8 * EPS32 * np.abs(table).max()
    print(f"{dst.shape[0]} vertices, max distance {math.sqrt(dist2.max()):.3e}, max error {err:.3e}, bound {bound:.3e}")
    assert err <= bound and dist2.max() > 0


def test_modules_round_trip_and_quantised_tables_are_refused(device):
    from quadraturefields_amd import baking
    v, f = cases.sphere(2)
    inter = _intersector(v, f, device)
    feats = torch.from_numpy(np.random.default_rng(63).normal(size=(v.shape[0], 3 + 7 * 2 + 1)).astype(F32)).to(device)
    module = baking.VertexBakedFeatures(feats, train_density=False)
    dst = torch.from_numpy(cases.sphere(1)[0]).to(device)
    moved = baking.transfer_vertex_features(inter, module, dst)
    assert isinstance(moved, baking.VertexBakedFeatures) and moved.n_lobes == 2 and moved.train_density is False
    assert moved.table.shape == (dst.shape[0], module.table.shape[1]) and moved.table.device == module.table.device
    assert torch.equal(moved.features(), baking.transfer_vertex_features(inter, feats, dst))
    same = baking.transfer_vertex_features(inter, module, torch.from_numpy(v.astype(F32)).to(device))
    assert torch.equal(same.table, module.table)
    quantised = baking.quantise_vertex_features(feats)
    with pytest.raises(TypeError, match="quantise after"):
        baking.transfer_vertex_features(inter, quantised, dst)


def test_a_frame_renders_on_the_decimated_shells_with_the_transferred_table(device):
    from quadraturefields_amd import baking, mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    from tests import vertex_baked_reference as R
    mesh, field = R.mesh(), R.sg_field(2, device)
    full = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=10)
    table = baking.bake_vertex_features(field, full)
    small_mesh = mc_utils.decimate_mesh(mesh, mesh.faces.shape[0] // 2, device=device)[0]
    small = MeshIntersection(small_mesh, simplify_mesh=False, scale=1.0, num_intersections=10)
    moved = baking.transfer_vertex_features(full, table, small.vertices)
    assert moved.shape == (small_mesh.vertices.shape[0], table.shape[1]) and torch.isfinite(moved).all()
    c2w, focal, o, d = R.camera(64, 64)
    cam = make_camera(c2w, focal, 64, 64)
    frames = []
    for mi, feats in ((full, table), (small, moved)):
        rgb = FrameRenderer(mi, field, bg_color="white").render_vertex_baked(o.to(device), d.to(device), feats, camera=cam)[0]
        assert rgb.shape == (64 * 64, 3) and torch.isfinite(rgb).all()
        frames.append(rgb)
    mse = float(((frames[0] - frames[1]) ** 2).mean())
    print(f"{mesh.faces.shape[0]} -> {small_mesh.faces.shape[0]} faces: PSNR of the decimated asset against the full one "
          f"{-10 * math.log10(mse) if mse > 0 else math.inf:.2f} dB")


# --------------------------------------------------------------------------------------------------------- mesh distance
def _dev(v, f, device):
    return torch.from_numpy(np.asarray(v, F64)).to(device), torch.from_numpy(np.asarray(f, np.int64)).to(device)


def test_mesh_distance(device):
    """A mesh against itself and against its midpoint subdivision is zero: at the vertices exactly, at face centroids
    (which lie in their face's plane only up to their own rounding) within 8 eps64 of the unit extent.  The meshes are
    given with vertices that fp32 holds exactly, the split one on a 2^-10 lattice so that its midpoints are exact too:
    the tree stores fp32, and a mesh that it has to round is another mesh.

    The level-3 icosphere against the level-4 one: every one-sided maximum lies in (0, sag], sag = 1 - cos(theta / 2)
    the radial sag of the coarser sphere under its widest edge angle theta = pi / n (the level-4 vertices over the
    level-3 edge midpoints are exactly that far, so the bound is tight), plus what storing both spheres in fp32 can
    add: a coordinate below 1 moves by at most 2^-25, a vertex by sqrt(3) 2^-25, and the distance is 1-Lipschitz in
    the sample and in the mesh (measured on the restatement: 3.2e-8 above the sag)."""
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh
    v3, f3 = cases.sphere(3)
    r3 = v3.astype(F32).astype(F64)
    same = mc_utils.mesh_distance_device(*_dev(r3, f3, device), *_dev(r3, f3, device))
    assert all(0 <= x <= 8 * EPS64 for x in same), same

    lattice = np.round(v3 * 1024.0) / 1024.0
    split = mc_utils.subdivide_mesh_device(*_dev(lattice, f3, device))
    assert split.faces.shape[0] == 4 * f3.shape[0]
    assert torch.equal(split.vertices, split.vertices.to(torch.float32).to(torch.float64))
    again = mc_utils.mesh_distance_device(split.vertices, split.faces, *_dev(lattice, f3, device))
    assert all(0 <= x <= 8 * EPS64 for x in again), again

    v4, f4 = cases.sphere(4)
    r4 = v4.astype(F32).astype(F64)
    edges = np.concatenate([f3[:, [0, 1]], f3[:, [1, 2]], f3[:, [2, 0]]])
    theta = np.arccos(np.clip((v3[edges[:, 0]] * v3[edges[:, 1]]).sum(axis=1), -1, 1)).max()
    sag = 1.0 - math.cos(theta / 2.0)
    stored = 2 * math.sqrt(3.0) * 2.0 ** -25
    d = mc_utils.mesh_distance_device(*_dev(r3, f3, device), *_dev(r4, f4, device))
    print(f"edge angle {theta:.4f} = pi / {math.pi / theta:.2f}, sag {sag:.6e} (+ {stored:.1e} for fp32), distances {d}")
    assert 0 < d.a_to_b_max <= sag + stored and 0 < d.b_to_a_max <= sag + stored
    assert d.symmetric_max == max(d.a_to_b_max, d.b_to_a_max) > 0.9 * sag
    assert 0 < d.a_to_b_mean <= d.a_to_b_rms <= d.a_to_b_max and 0 < d.b_to_a_mean <= d.b_to_a_rms <= d.b_to_a_max
    assert mc_utils.mesh_distance(TriMesh(r3, f3), TriMesh(r4, f4), device=device) == d


# ------------------------------------------------------------------------------------------------------------ the example
def _example():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decimate_mesh_example", os.path.join(root, "examples", "decimate_mesh.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_example_with_and_without_the_new_flags(device, tmp_path, capsys):
    from quadraturefields_amd import mc_utils
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = cases.sphere(3)
    a, b, c = tmp_path / "plain", tmp_path / "table", tmp_path / "direct"
    for folder in (a, b, c):
        folder.mkdir()
    TriMesh(v, f).export(str(tmp_path / "in.ply"))
    loaded = load_mesh(str(tmp_path / "in.ply"))
    target = f.shape[0] // 4
    example = _example()
    example.main([str(tmp_path / "in.ply"), str(a / "out.ply"), "--target_faces", str(target)])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    # without the flags: the files and the line of the calls the example has always made
    out, face_map, vertex_target, stats = mc_utils.decimate_mesh(loaded, target, return_stats=True, device="cuda")
    out.export(str(c / "out.ply"))
    np.save(c / "face_map.npy", face_map)
    np.save(c / "vertex_target.npy", vertex_target)
    assert sorted(os.listdir(a)) == sorted(os.listdir(c)) == ["face_map.npy", "out.ply", "vertex_target.npy"]
    for name in os.listdir(c):
        assert (a / name).read_bytes() == (c / name).read_bytes(), name
    assert plain == json.loads(json.dumps(dict(stats, boundary="lock", boundary_weight=1.0, faces_in=f.shape[0],
                                               vertices_in=v.shape[0], target_faces=target, faces_out=int(out.faces.shape[0]),
                                               vertices_out=int(out.vertices.shape[0]))))
    assert not any(k.startswith("distance_") for k in plain)

    table = np.random.default_rng(71).normal(size=(v.shape[0], 18)).astype(F32)
    np.save(tmp_path / "table.npy", table)
    example.main([str(tmp_path / "in.ply"), str(b / "out.ply"), "--target_faces", str(target), "--vertex_features",
                  str(tmp_path / "table.npy"), "--out_vertex_features", str(b / "table_out.npy")])
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 1
    line = json.loads(lines[0])
    assert sorted(os.listdir(b)) == ["face_map.npy", "out.ply", "table_out.npy", "vertex_target.npy"]
    for name in os.listdir(c):
        assert (b / name).read_bytes() == (c / name).read_bytes(), name
    new_keys = ["distance_in_to_out_max", "distance_in_to_out_mean", "distance_out_to_in_max", "distance_out_to_in_mean"]
    assert sorted(set(line) - set(plain)) == new_keys and {k: line[k] for k in plain} == plain
    assert all(0 < line[k] < 0.1 for k in new_keys) and line["distance_out_to_in_mean"] <= line["distance_out_to_in_max"]
    lv = np.asarray(loaded.vertices)
    want = cp.transfer(cp.triangles_of(lv, loaded.faces), loaded.faces, table, np.asarray(out.vertices, F64))
    assert np.load(b / "table_out.npy").tobytes() == want.tobytes()
