"""GPU: mesh refinement (``mc_utils.mesh_edges_device`` / ``subdivide_mesh_device``, ``qf_mesh_edges_*`` /
``qf_mesh_subdivide_*``) against its numpy restatement (tests/mesh_subdivide_reference.py), and the
vertex-baked table carried through it.  Every comparison with the restatement is exact: edges, faces, maps, counts, and
vertices by bits."""
import numpy as np
import pytest
import torch

from tests import mesh_subdivide_reference as ref
from tests import stream_harness as sh
from tests import vertex_baked_reference as R
from tests.test_mesh_subdivide_host import HAND_CASES, HAND_EDGES, HAND_FACE_EDGES, HAND_FACES, HAND_VERTS, random_mesh

pytestmark = pytest.mark.gpu

_cache = {}


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _assert_edges_match(f, n_v):
    got = _mc().mesh_edges_device(_dev(np.asarray(f).reshape(-1, 3), np.int64), n_v)
    torch.cuda.synchronize()
    e, fe, c = ref.edges(f, n_v)
    assert got.edges.dtype == got.face_edges.dtype == torch.int64 and got.edges.is_cuda
    assert torch.equal(got.edges.cpu(), torch.from_numpy(e)) and torch.equal(got.face_edges.cpu(), torch.from_numpy(fe))
    assert list(got.stats) == list(ref.EDGE_COUNT_NAMES) and list(got.stats.values()) == c.tolist()
    return got, (e, fe, c)


def _assert_matches(v, f, marks=None):
    """Both stages on the device equal the restatement: returns (device record, reference tuple)."""
    edges, (e, fe, _) = _assert_edges_match(f, len(v))
    got = _mc().subdivide_mesh_device(_dev(v, np.float64), _dev(np.asarray(f).reshape(-1, 3), np.int64),
                                      None if marks is None else _dev(marks, np.uint8), edges.edges, edges.face_edges)
    torch.cuda.synchronize()
    want = ref.subdivide(v, f, marks, e, fe)
    assert got.vertices.dtype == torch.float64 and got.vertices.shape == want[0].shape
    assert torch.equal(got.vertices.cpu().view(torch.int64), torch.from_numpy(want[0]).view(torch.int64))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(want[1])) and torch.equal(got.face_map.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(got.vertex_parents.cpu(), torch.from_numpy(want[3]))
    assert list(got.stats) == list(ref.SPLIT_COUNT_NAMES) and list(got.stats.values()) == want[4].tolist()
    return got, want


def _marks(n_e, share, seed):
    if share == 0.0:
        return np.zeros(n_e, np.uint8)
    if share == 1.0:
        return np.ones(n_e, np.uint8)
    return (np.random.default_rng(seed).random(n_e) < share).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------- 1. the rules
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(device, name):
    marks, faces, face_map, new_parents, counts = HAND_CASES[name]
    edges = _mc().mesh_edges_device(_dev(HAND_FACES, np.int64), 4)
    assert edges.edges.tolist() == HAND_EDGES and edges.face_edges.tolist() == HAND_FACE_EDGES
    assert list(edges.stats.values()) == [5, 0, 0, 4]
    got, _ = _assert_matches(HAND_VERTS, HAND_FACES, marks)
    assert got.faces.tolist() == [list(t) for t in faces] and got.face_map.tolist() == face_map
    assert got.vertex_parents[4:].tolist() == [list(t) for t in new_parents] and list(got.stats.values()) == counts


@pytest.mark.parametrize("n_f", [0, 1, 255, 256, 257, 341, 342])
def test_face_counts_around_workgroup_and_scan_edges(device, n_f):
    """3 F = 765 / 768 / 771 half-edges sit on the workgroup boundary, 1 023 / 1 026 on the scan chunk's."""
    v, f = random_mesh(150, n_f, seed=n_f)
    v[75] = [np.inf, -np.inf, -0.0]                        # coordinates are copied or averaged, never read for a decision
    n_e = ref.edges(f, 150)[2][0]
    for share in (1.0, 0.4, 0.0):
        got, want = _assert_matches(v, f, _marks(n_e, share, n_f))
    got, want = _assert_matches(v, f, None)
    assert got.stats["faces"] == want[4][0] and (n_f == 0) == (got.stats["faces"] == 0)


def test_collision_heavy_soup(device):
    """V = 40, F = 2 000: about 780 pairs for 6 000 half-edges, so many faces per edge, duplicate faces in both windings
    and degenerate faces; every probe sequence of the table is contended."""
    rng = np.random.default_rng(13)
    v = rng.normal(size=(40, 3))
    f = rng.integers(0, 40, size=(2000, 3))
    f[500:600] = f[100:200][:, [1, 2, 0]]                  # rotated duplicates
    f[700:800] = f[100:200][:, [0, 2, 1]]                  # opposite windings
    f[900:950, 1] = f[900:950, 0]                          # (a, a, b)
    f[950:960] = f[950:960, :1]                            # (a, a, a)
    edges, (e, fe, c) = _assert_edges_match(f, 40)
    assert c[0] <= 780 and c[1] >= 60 and (fe[900:960] == -1).all()
    for share in (1.0, 0.5, 0.1):
        got, want = _assert_matches(v, f, _marks(c[0], share, 3))
        assert want[4][2] >= 60                            # the degenerate faces count as unsplit


def _mesh_3000():
    """V = 3 000, F = 9 000, seeded, no degenerate face (the linearity test divides by their area)."""
    if "m3000" not in _cache:
        v, f = random_mesh(3000, 9000, seed=21, degenerate=0.0)
        same = (f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])
        f[same] = (f[same, :1] + np.arange(3)) % 3000
        e, fe, c = ref.edges(f, 3000)
        assert c[1] == 0
        _cache["m3000"] = (v, f, e, fe)
    return _cache["m3000"]


@pytest.mark.parametrize("share", [0.0, 0.1, 0.5, 1.0])
def test_seeded_marks_on_a_larger_mesh(device, share):
    v, f, e, _ = _mesh_3000()
    got, want = _assert_matches(v, f, _marks(len(e), share, 17))
    if share == 0.0:
        assert torch.equal(got.faces.cpu(), torch.from_numpy(f)) and got.stats["vertices"] == 3000
    if share == 1.0:
        assert got.stats["faces"] == 36000 and got.stats["faces_3_marked"] == 9000


def test_grid_past_the_scan_bases_threshold(device):
    """A 363 x 363 quad grid, F = 263 538: the scan of the children (a byte's value, 1 to 4, not a flag) runs over more
    than 262 144 items, from where a thread of the scan's middle launch owns more than one per-workgroup sum; the scans
    of the 790 614 half-edges and of the 396 033 marks are past it too.  A seeded 10 % of the edges is marked."""
    n = 363
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    v = np.stack([i.ravel(), j.ravel(), np.zeros(i.size)], 1) + np.random.default_rng(5).normal(scale=0.1, size=(i.size, 3))
    a = (i[:-1, :-1] * (n + 1) + j[:-1, :-1]).ravel()
    f = np.concatenate([np.stack([a, a + n + 1, a + n + 2], 1), np.stack([a, a + n + 2, a + 1], 1)])
    n_e = 3 * n * n + 2 * n
    assert len(f) == 263538 > 262144 and n_e == 396033
    got, want = _assert_matches(v, f, _marks(n_e, 0.1, 17))
    assert got.stats["faces"] == want[4][0] > len(f) and got.stats["faces_3_marked"] > 0


def test_marks_may_be_bool_or_integer_and_edges_are_optional(device):
    v, f, e, fe = _mesh_3000()
    m = _marks(len(e), 0.5, 17)
    vd, fd = _dev(v, np.float64), _dev(f, np.int64)
    want = _mc().subdivide_mesh_device(vd, fd, _dev(m, np.uint8))
    for marks in (torch.from_numpy(m.astype(bool)).cuda(), m.astype(np.int64) * 7, m.astype(bool)):
        got = _mc().subdivide_mesh_device(vd, fd.to(torch.int32), marks)
        assert all(sh.same_bits(a, b) for a, b in zip(got[:4], want[:4])) and got.stats == want.stats
    with pytest.raises(ValueError, match="edge marks"):
        _mc().subdivide_mesh_device(vd, fd, m[:-1])
    with pytest.raises(TypeError):
        _mc().subdivide_mesh_device(vd, fd, m.astype(np.float32))
    with pytest.raises(ValueError, match="both"):
        _mc().subdivide_mesh_device(vd, fd, m, edges=_dev(e, np.int64))
    # fp32 vertices are widened exactly
    got = _mc().subdivide_mesh_device(vd.to(torch.float32), fd, m)
    ref_v = ref.subdivide(v.astype(np.float32).astype(np.float64), f, m, e, fe)[0]
    assert torch.equal(got.vertices.cpu().view(torch.int64), torch.from_numpy(ref_v).view(torch.int64))
    lengths = _mc().mark_edges_longer_than(vd, _dev(e, np.int64), 2.0)
    d = v[e[:, 0]] - v[e[:, 1]]
    assert torch.equal(lengths.cpu(), torch.from_numpy(((d * d).sum(1) > 4.0).astype(np.uint8))) and 0 < int(lengths.sum()) < len(e)


def test_host_mesh_wrapper_composes_the_levels(device):
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = ref.octahedron(1)
    rng = np.random.default_rng(2)
    uv = rng.random((len(v), 2))
    marks = rng.random(ref.edges(f, len(v))[2][0]) < 0.5
    mesh, face_map, parents = _mc().subdivide_mesh(TriMesh(v, f, uv), marks, levels=2)
    v1, f1, fm1, vp1, _ = ref.subdivide(v, f, marks)
    v2, f2, fm2, vp2, _ = ref.subdivide(v1, f1)
    assert np.array_equal(mesh.faces, f2) and np.array_equal(mesh.vertices.view(np.int64), v2.view(np.int64))
    assert np.array_equal(face_map, fm1[fm2]) and np.array_equal(parents, np.concatenate([vp1, vp2[len(vp1):]]))
    # chains end at input vertices, and positions and uv follow the parents
    new = np.arange(len(v), len(parents))
    assert (parents[new] < new[:, None]).all() and (parents[:len(v)] == np.arange(len(v))[:, None]).all()
    assert np.array_equal(mesh.vertices[new], 0.5 * (mesh.vertices[parents[new, 0]] + mesh.vertices[parents[new, 1]]))
    assert np.array_equal(mesh.visual.uv[new], 0.5 * (mesh.visual.uv[parents[new, 0]] + mesh.visual.uv[parents[new, 1]]))
    assert np.array_equal(mesh.visual.uv[:len(v)], uv) and ref.directed_edge_balance(mesh.faces) == 0


def test_closed_manifold_edge_balance_on_device_output(device):
    v, f = ref.octahedron(2)
    for seed, share in ((0, 0.3), (1, 0.5), (2, 0.8)):
        marks = np.random.default_rng(seed).random(192) < share
        got = _mc().subdivide_mesh_device(_dev(v, np.float64), _dev(f, np.int64), marks)
        faces = got.faces.cpu().numpy()
        assert ref.directed_edge_balance(faces) == 0
        assert _mc().mesh_edges_device(got.faces, got.vertices.shape[0]).stats["boundary_edges"] == 0


# ------------------------------------------------------------------------------------------- 2. determinism, capacities
def test_two_runs_give_identical_bytes(device):
    v, f, e, _ = _mesh_3000()
    m = _marks(len(e), 0.5, 17)
    runs = []
    for _ in range(2):
        edges = _mc().mesh_edges_device(_dev(f, np.int64), 3000)
        runs.append((edges, _mc().subdivide_mesh_device(_dev(v, np.float64), _dev(f, np.int64), m)))
    for k in (0, 1):
        n = 2 if k == 0 else 4
        assert all(sh.same_bits(a, b) for a, b in zip(runs[0][k][:n], runs[1][k][:n]))
        assert runs[0][k].stats == runs[1][k].stats


def _raw_args(v, f, fe, n_e, marks, device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    t = dict(v=_dev(v, np.float64), f=_dev(f, np.int64), fe=_dev(fe, np.int64), m=_dev(marks, np.uint8))
    n_bytes = int(lib.qf_mesh_subdivide_workspace_bytes(len(v), len(f), n_e))
    t["ws"] = torch.empty((n_bytes,), dtype=torch.uint8, device=device)
    args = (_C.ptr(t["f"]), len(f), len(v), _C.ptr(t["fe"]), n_e, _C.ptr(t["m"]), _C.ptr(t["ws"]), n_bytes)
    return lib, t, args


def test_emit_with_short_capacities_writes_nothing_beyond_them(device):
    from quadraturefields_amd import _C
    v, f, e, fe = _mesh_3000()
    m = _marks(len(e), 0.5, 17)
    want = ref.subdivide(v, f, m, e, fe)
    lib, t, args = _raw_args(v, f, fe, len(e), m, device)
    counts = torch.full((7,), -5, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_subdivide_count(*args, _C.ptr(counts), _C.stream()), "count")
    n_f, n_v = counts.tolist()[:2]
    assert (n_f, n_v) == (len(want[1]), len(want[0]))
    for cut_v, cut_f in ((5, 7), (n_v - 3000 + 10, n_f), (n_v, 0)):      # the last rows; below V: no new vertex; nothing
        ov = torch.full((n_v, 3), -7.0, dtype=torch.float64, device=device)
        vp = torch.full((n_v, 2), -7, dtype=torch.int64, device=device)
        of = torch.full((n_f, 3), -7, dtype=torch.int64, device=device)
        fm = torch.full((n_f,), -7, dtype=torch.int64, device=device)
        _C.check(lib.qf_mesh_subdivide_emit(_C.ptr(t["v"]), *args, _C.ptr(ov), n_v - cut_v, _C.ptr(of), n_f - cut_f,
                                            _C.ptr(fm), _C.ptr(vp), _C.stream()), "emit")
        torch.cuda.synchronize()
        kv, kf = n_v - cut_v, n_f - cut_f
        assert torch.equal(ov[:kv].cpu().view(torch.int64), torch.from_numpy(want[0][:kv]).view(torch.int64))
        assert torch.equal(vp[:kv].cpu(), torch.from_numpy(want[3][:kv]))
        assert torch.equal(of[:kf].cpu(), torch.from_numpy(want[1][:kf])) and torch.equal(fm[:kf].cpu(), torch.from_numpy(want[2][:kf]))
        assert bool((ov[kv:] == -7).all()) and bool((vp[kv:] == -7).all()) and bool((of[kf:] == -7).all()) and bool((fm[kf:] == -7).all())
    # the maps may be NULL
    ov = torch.empty((n_v, 3), dtype=torch.float64, device=device)
    of = torch.empty((n_f, 3), dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_subdivide_emit(_C.ptr(t["v"]), *args, _C.ptr(ov), n_v, _C.ptr(of), n_f, None, None, _C.stream()), "emit")
    assert torch.equal(of.cpu(), torch.from_numpy(want[1]))
    # stage A: a short edge capacity
    n_bytes = int(lib.qf_mesh_edges_workspace_bytes(3000, 9000))
    ws = torch.empty((n_bytes,), dtype=torch.uint8, device=device)
    c4 = torch.empty((4,), dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_edges_count(_C.ptr(t["f"]), 9000, 3000, _C.ptr(ws), n_bytes, _C.ptr(c4), _C.stream()), "count")
    assert c4.tolist()[0] == len(e)
    oe = torch.full((len(e), 2), -7, dtype=torch.int64, device=device)
    ofe = torch.full((9000, 3), -7, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_edges_emit(_C.ptr(t["f"]), 9000, 3000, _C.ptr(ws), n_bytes, _C.ptr(oe), len(e) - 9, _C.ptr(ofe),
                                    _C.stream()), "emit")
    assert torch.equal(oe[:-9].cpu(), torch.from_numpy(e[:-9])) and bool((oe[-9:] == -7).all())
    assert torch.equal(ofe.cpu(), torch.from_numpy(fe))


def test_invalid_indices_produce_nothing_and_report_the_count(device):
    from quadraturefields_amd import _C
    v, f, e, fe = _mesh_3000()
    bad = f.copy()
    bad[17, 1], bad[4500, 2], bad[8999, 0] = 3000, -1, 2 ** 40
    with pytest.raises(ValueError, match=r"\b3 faces have an index outside \[0, 3000\)"):
        _mc().mesh_edges_device(_dev(bad, np.int64), 3000)
    with pytest.raises(ValueError, match=r"\b3 faces have"):
        _mc().subdivide_mesh_device(_dev(v, np.float64), _dev(bad, np.int64), None, _dev(e, np.int64), _dev(fe, np.int64))
    lib = _C.lib()
    fd = _dev(bad, np.int64)
    n_bytes = int(lib.qf_mesh_edges_workspace_bytes(3000, 9000))
    ws = torch.empty((n_bytes,), dtype=torch.uint8, device=device)
    counts = torch.full((4,), -5, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_edges_count(_C.ptr(fd), 9000, 3000, _C.ptr(ws), n_bytes, _C.ptr(counts), _C.stream()), "count")
    assert counts.tolist() == [0, 0, 3, 0]
    oe = torch.full((27000, 2), -7, dtype=torch.int64, device=device)
    ofe = torch.full((9000, 3), -7, dtype=torch.int64, device=device)
    _C.check(lib.qf_mesh_edges_emit(_C.ptr(fd), 9000, 3000, _C.ptr(ws), n_bytes, _C.ptr(oe), 27000, _C.ptr(ofe), _C.stream()), "emit")
    torch.cuda.synchronize()
    assert bool((oe == -7).all()) and bool((ofe == -7).all())
    # stage B: a vertex index out of range, and an edge id out of range on a face that is not degenerate
    bad_fe = fe.copy()
    bad_fe[5, 0], bad_fe[6, 2] = len(e), -1
    for faces, face_edges, n_bad in ((bad, fe, 3), (f, bad_fe, 2)):
        lib, t, args = _raw_args(v, faces, face_edges, len(e), np.ones(len(e), np.uint8), device)
        c7 = torch.full((7,), -5, dtype=torch.int64, device=device)
        _C.check(lib.qf_mesh_subdivide_count(*args, _C.ptr(c7), _C.stream()), "count")
        assert c7.tolist() == [0, 0, 0, 0, 0, 0, n_bad]
        ov = torch.full((3000 + len(e), 3), -7.0, dtype=torch.float64, device=device)
        of = torch.full((36000, 3), -7, dtype=torch.int64, device=device)
        fm = torch.full((36000,), -7, dtype=torch.int64, device=device)
        vp = torch.full((3000 + len(e), 2), -7, dtype=torch.int64, device=device)
        _C.check(lib.qf_mesh_subdivide_emit(_C.ptr(t["v"]), *args, _C.ptr(ov), ov.shape[0], _C.ptr(of), 36000, _C.ptr(fm),
                                            _C.ptr(vp), _C.stream()), "emit")
        torch.cuda.synchronize()
        assert bool((ov == -7).all()) and bool((of == -7).all()) and bool((fm == -7).all()) and bool((vp == -7).all())


def test_bad_sizes_return_the_status_before_any_launch(device):
    from quadraturefields_amd import _C
    v, f, e, fe = _mesh_3000()
    lib, t, args = _raw_args(v, f, fe, len(e), np.ones(len(e), np.uint8), device)
    counts = torch.full((7,), -5, dtype=torch.int64, device=device)
    fp, fep, mp, wp, need = args[0], args[3], args[5], args[6], args[7]

    def count(F=9000, V=3000, E=len(e), ws_bytes=need, f_=fp, fe_=fep, m_=mp, w_=wp, c_=_C.ptr(counts)):
        return lib.qf_mesh_subdivide_count(f_, F, V, fe_, E, m_, w_, ws_bytes, c_, _C.stream())

    for bad in (dict(V=0), dict(V=2 ** 31), dict(F=-1), dict(F=2 ** 29), dict(E=-1), dict(E=27001), dict(ws_bytes=need - 1),
                dict(f_=None), dict(fe_=None), dict(m_=None), dict(w_=None), dict(c_=None)):
        assert count(**bad) == -1, bad
    torch.cuda.synchronize()
    assert counts.tolist() == [-5] * 7                     # nothing ran
    assert count() == 0
    need_a = int(lib.qf_mesh_edges_workspace_bytes(3000, 9000))
    for bad in (dict(V=0), dict(F=2 ** 30), dict(ws_bytes=need_a - 1)):
        a = dict(dict(F=9000, V=3000, ws_bytes=need_a), **bad)
        assert lib.qf_mesh_edges_count(fp, a["F"], a["V"], wp, a["ws_bytes"], _C.ptr(counts), _C.stream()) == -1, bad


# ------------------------------------------------------------------------------------------------ 3. the vertex table
def test_linearity_ties_the_maps_to_the_renderer(device):
    """A table carried along by ``subdivide_vertex_features`` (no field) renders the function it rendered: the blend of a
    point in a child, from the new table, is its blend in ``face_map[child]`` from the old one.  Between the two blends
    lie about 17 fp32 roundings of magnitude <= max|table| (three products, two sums, three barycentric casts, one
    averaged row per new vertex); 64 ulps of max(1, max|table|) is a fourfold margin.  A wrong parent or child pattern
    gives O(1) differences."""
    from quadraturefields_amd import baking, utils
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    v, f, e, fe = _mesh_3000()
    rng = np.random.default_rng(31)
    out = _mc().subdivide_mesh_device(_dev(v, np.float64), _dev(f, np.int64), _marks(len(e), 0.5, 17))
    new_v, new_f, face_map = out.vertices.cpu().numpy(), out.faces.cpu().numpy(), out.face_map.cpu().numpy()
    table = torch.from_numpy(rng.normal(size=(3000, 3 + 7 * 2 + 1)).astype(np.float32)).cuda()
    new_table = baking.subdivide_vertex_features(table, out.vertex_parents)
    assert new_table.shape == (len(new_v), 18) and torch.equal(new_table[:3000], table)
    n = 20000
    child = rng.integers(0, len(new_f), size=n)
    w = rng.dirichlet(np.ones(3), size=n)                            # fp64 barycentrics inside the child
    points = torch.from_numpy(np.einsum("nk,nkc->nc", w, new_v[new_f[child]]).astype(np.float32)).cuda()
    dirs = rng.normal(size=(n, 3))
    dirs = torch.from_numpy((dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)).cuda()
    kw = dict(simplify_mesh=False, scale=1.0, num_intersections=5, device=device, bvh_builder="device")
    mi_old, mi_new = MeshIntersection(TriMesh(v, f), **kw), MeshIntersection(TriMesh(new_v, new_f), **kw)
    fine = utils.shade_vertex_baked_points(mi_new, new_table, points, torch.from_numpy(child).cuda(), dirs, want_features=True)[2]
    coarse = utils.shade_vertex_baked_points(mi_old, table, points, torch.from_numpy(face_map[child]).cuda(), dirs,
                                             want_features=True)[2]
    bound = 64 * 2.0 ** -24 * max(1.0, float(table.abs().max()))
    diff = float((fine - coarse).abs().max())
    print(f"linearity: max |fine - coarse| = {diff:.3e}, bound {bound:.3e}, max|table| = {float(table.abs().max()):.3f}")
    assert torch.isfinite(fine).all() and diff <= bound
    # the test has power: the blend in a wrong parent is O(1) away
    wrong = utils.shade_vertex_baked_points(mi_old, table, points, torch.from_numpy((face_map[child] + 1) % 9000).cuda(), dirs,
                                            want_features=True)[2]
    assert float((wrong - coarse).abs().max()) > 0.5


def test_rows_from_the_field_equal_a_bake_of_the_refined_mesh(device):
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    mesh, field = R.mesh(), R.sg_field(2, device)
    kw = dict(simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    old = baking.bake_vertex_features(field, MeshIntersection(mesh, **kw))
    n_e = ref.edges(mesh.faces, len(mesh.vertices))[2][0]
    out = _mc().subdivide_mesh_device(_dev(mesh.vertices, np.float64), _dev(mesh.faces, np.int64), _marks(n_e, 0.5, 4))
    got = baking.subdivide_vertex_features(old, out.vertex_parents, radiance_field=field, vertices=out.vertices)
    refined = TriMesh(out.vertices.cpu().numpy(), out.faces.cpu().numpy())
    want = baking.bake_vertex_features(field, MeshIntersection(refined, **kw))
    n_old = len(mesh.vertices)
    assert got.shape == want.shape and got.shape[0] > n_old
    assert sh.same_bits(got[:n_old], old) and sh.same_bits(got[n_old:], want[n_old:]) and sh.same_bits(got, want)
    averaged = baking.subdivide_vertex_features(old, out.vertex_parents)
    assert sh.same_bits(averaged[:n_old], old) and not torch.equal(averaged[n_old:], got[n_old:])
    with pytest.raises(TypeError, match="quantise after refining"):
        baking.subdivide_vertex_features(baking.quantise_vertex_features(old), out.vertex_parents)


def test_refine_vertex_baked_on_the_shell_mesh(device):
    from quadraturefields_amd import baking, synthetic
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    mesh, field = synthetic.shell_mesh(), R.sg_field(2, device)
    n_v0, n_f0 = len(mesh.vertices), len(mesh.faces)
    step = 0.005
    # a tolerance that a part of the edges exceeds: the 0.9 quantile of the input mesh's own errors
    edges0 = _mc().mesh_edges_device(_dev(mesh.faces, np.int64), n_v0).edges
    table0 = baking.bake_vertex_features(field, MeshIntersection(mesh, simplify_mesh=False, device=device, bvh_builder="device"))
    err0 = baking.vertex_edge_error(field, _dev(mesh.vertices, np.float64), edges0, table0, step)
    assert err0.shape == (edges0.shape[0],) and bool(torch.isfinite(err0).all()) and float(err0.min()) >= 0.0
    tol = float(torch.quantile(err0[::7], 0.9))
    assert 0.0 < tol < float(err0.max())

    def check(result, budget):
        n_v = n_v0
        for rec in result.levels:
            err, marks = rec["errors"], rec["marks"].bool()
            assert rec["vertices"] == n_v and rec["marked"] == int(marks.sum())
            assert bool((err[marks] > tol).all())                      # every marked edge had e > tol
            if budget is None:
                assert bool(((err > tol) == marks).all())              # and no edge with e <= tol was split
            elif rec["marked"] < rec["above_tol"]:                     # the budget cut: the largest errors went first
                assert n_v + rec["marked"] == budget
                assert rec["marked"] == 0 or float(err[marks].min()) >= float(err[~marks & (err > tol)].max())
            n_v += rec["marked"]
        assert n_v == len(result.mesh.vertices) == result.table.shape[0] == len(result.vertex_parents)
        assert budget is None or n_v <= budget
        return n_v

    free = baking.refine_vertex_baked(mesh, field, tol, max_levels=1, render_step_size=step, keep_level_arrays=True)
    assert torch.equal(free.levels[0]["errors"], err0) and free.levels[0]["marked"] == int((err0 > tol).sum()) > 0
    check(free, None)
    budget = n_v0 + 5000
    res = baking.refine_vertex_baked(mesh, field, tol, max_levels=2, max_vertices=budget, render_step_size=step,
                                     keep_level_arrays=True)
    assert check(res, budget) == budget and len(res.levels) == 2 and res.levels[1]["marked"] == 0
    # the maps compose: old rows and vertices kept, chains end at input vertices, children lie in the face they name
    v, f, parents = res.mesh.vertices, res.mesh.faces, res.vertex_parents
    assert np.array_equal(v[:n_v0].view(np.int64), np.asarray(mesh.vertices, np.float64).view(np.int64))
    assert sh.same_bits(res.table[:n_v0], table0)
    new = np.arange(n_v0, len(v))
    assert (parents[:n_v0] == np.arange(n_v0)[:, None]).all() and (parents[new] < new[:, None]).all()
    assert np.array_equal(v[new], 0.5 * (v[parents[new, 0]] + v[parents[new, 1]]))
    assert res.face_map.min() >= 0 and res.face_map.max() < n_f0 and len(res.face_map) == len(f)
    tri = np.asarray(mesh.vertices, np.float64)[mesh.faces[res.face_map]]
    centre = v[f].mean(axis=1)
    e0, e1, d = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0], centre - tri[:, 0]
    d00, d01, d11 = (e0 * e0).sum(1), (e0 * e1).sum(1), (e1 * e1).sum(1)
    b1 = ((d * e0).sum(1) * d11 - (d * e1).sum(1) * d01) / (d00 * d11 - d01 * d01)
    b2 = ((d * e1).sum(1) * d00 - (d * e0).sum(1) * d01) / (d00 * d11 - d01 * d01)
    assert min(b1.min(), b2.min(), (1 - b1 - b2).min()) > 1e-3         # a child's centroid is well inside its parent
    assert np.abs(np.einsum("nc,nc->n", d, np.cross(e0, e1))).max() <= 1e-12      # and in its plane
    # the rows of the new vertices are the field's, as a bake of the refined mesh gives them
    mi = MeshIntersection(res.mesh, simplify_mesh=False, num_intersections=5, render_step_size=step, device=device,
                          bvh_builder="device")
    assert sh.same_bits(res.table, baking.bake_vertex_features(field, mi))
    # and a frame renders through it
    c2w, focal, o, d_ = R.camera(64, 64)
    rgb, alpha, depth, n = FrameRenderer(mi, field).render_vertex_baked(o.to(device), d_.to(device), res.table,
                                                                        camera=make_camera(c2w, focal, 64, 64))
    assert n > 0 and bool(torch.isfinite(rgb).all()) and bool(torch.isfinite(alpha).all()) and bool(torch.isfinite(depth).all())
    assert float(alpha.max()) > 0.0


# ------------------------------------------------------------------------------------------------------------ 4. streams
def _stream_faces(seed):
    """Two valid face sets of the same shape (named in ``varies``): the 3 000 / 9 000 mesh and a reseeded one."""
    if seed == 1:
        return _mesh_3000()[1]
    f = random_mesh(3000, 9000, seed=22, degenerate=0.05)[1]
    return f


def _edges_build(seed, device):
    from quadraturefields_amd import _C
    n = int(_C.lib().qf_mesh_edges_workspace_bytes(3000, 9000))
    return dict(faces=torch.from_numpy(_stream_faces(seed)).to(device), tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_counts=torch.zeros((4,), dtype=torch.int64, device=device),
                out_edges=torch.zeros((27000, 2), dtype=torch.int64, device=device),
                out_face_edges=torch.zeros((9000, 3), dtype=torch.int64, device=device))


def _edges_count_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_edges_count(_C.ptr(i["faces"]), 9000, 3000, _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0],
                                          _C.ptr(i["out_counts"]), _C.stream()), "qf_mesh_edges_count")
    return (i["out_counts"],)


def _edges_emit_call(i):
    """Count, then emit at full capacity with no host wait in between: the rows beyond the count keep the sentinel."""
    from quadraturefields_amd import _C
    _edges_count_call(i)
    _C.check(_C.lib().qf_mesh_edges_emit(_C.ptr(i["faces"]), 9000, 3000, _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0],
                                         _C.ptr(i["out_edges"]), 27000, _C.ptr(i["out_face_edges"]), _C.stream()),
             "qf_mesh_edges_emit")
    return i["out_edges"], i["out_face_edges"], i["out_counts"]


def _split_build(seed, device):
    """Same faces and edges in both sets; the vertices (values) and the marks (named in ``varies``) differ."""
    from quadraturefields_amd import _C
    v, f, e, fe = _mesh_3000()
    rng = np.random.default_rng(seed)
    n_e = len(e)
    n = int(_C.lib().qf_mesh_subdivide_workspace_bytes(3000, 9000, n_e))
    return dict(vertices=torch.from_numpy(rng.normal(size=v.shape)).to(device), faces=torch.from_numpy(f).to(device),
                face_edges=torch.from_numpy(fe).to(device),
                edge_mark=torch.from_numpy((rng.random(n_e) < 0.5).astype(np.uint8)).to(device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_counts=torch.zeros((7,), dtype=torch.int64, device=device),
                out_v=torch.zeros((3000 + n_e, 3), dtype=torch.float64, device=device),
                out_vp=torch.zeros((3000 + n_e, 2), dtype=torch.int64, device=device),
                out_f=torch.zeros((36000, 3), dtype=torch.int64, device=device),
                out_fm=torch.zeros((36000,), dtype=torch.int64, device=device))


def _split_args(i):
    from quadraturefields_amd import _C
    return (_C.ptr(i["faces"]), 9000, 3000, _C.ptr(i["face_edges"]), i["edge_mark"].shape[0], _C.ptr(i["edge_mark"]),
            _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0])


def _split_count_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_subdivide_count(*_split_args(i), _C.ptr(i["out_counts"]), _C.stream()), "qf_mesh_subdivide_count")
    return (i["out_counts"],)


def _split_emit_call(i):
    from quadraturefields_amd import _C
    _split_count_call(i)
    _C.check(_C.lib().qf_mesh_subdivide_emit(_C.ptr(i["vertices"]), *_split_args(i), _C.ptr(i["out_v"]), i["out_v"].shape[0],
                                             _C.ptr(i["out_f"]), 36000, _C.ptr(i["out_fm"]), _C.ptr(i["out_vp"]), _C.stream()),
             "qf_mesh_subdivide_emit")
    return i["out_v"], i["out_f"], i["out_fm"], i["out_vp"], i["out_counts"]


STREAM_CASES = [
    sh.Case("mesh_edges_count", _edges_build, _edges_count_call, varies=("faces",), entry_points=("qf_mesh_edges_count",)),
    sh.Case("mesh_edges_emit", _edges_build, _edges_emit_call, varies=("faces",), entry_points=("qf_mesh_edges_emit",)),
    sh.Case("mesh_subdivide_count", _split_build, _split_count_call, varies=("edge_mark",),
            entry_points=("qf_mesh_subdivide_count",)),
    sh.Case("mesh_subdivide_emit", _split_build, _split_emit_call, varies=("edge_mark",),
            entry_points=("qf_mesh_subdivide_emit",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_SUBDIVIDE_SIGNATURES)
                             - {"qf_mesh_edges_workspace_bytes", "qf_mesh_subdivide_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
