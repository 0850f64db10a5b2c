"""GPU: the vertex weld (``mc_utils.weld_vertices_device`` / ``qf_mesh_weld_*``) against its numpy
restatements (tests/mesh_weld_reference.py).  Every comparison with a restatement is exact: vertices by bits, faces, both
maps and all eight counts."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_decimate_open_reference as oref
from tests import mesh_decimate_reference as ref
from tests import mesh_manifold_reference as mref
from tests import mesh_weld_reference as wref
from tests import stream_harness as sh
from tests.test_mesh_weld_host import HAND_CASES, NAN_A, REFUSED_CASES, same

pytestmark = pytest.mark.gpu


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


def _faces(f, dtype=np.int64):
    return None if f is None else _dev(np.asarray(f).reshape(-1, 3), dtype)


def _run(v, f, h, faces_dtype=np.int64, vertices_dtype=np.float64):
    got = _mc().weld_vertices_device(_dev(v, vertices_dtype), _faces(f, faces_dtype), h, return_stats=True)
    torch.cuda.synchronize()
    assert got.vertices.dtype == torch.float64
    assert got.faces.dtype == got.vertex_map.dtype == got.vertex_class.dtype == torch.int64
    return got


def _assert_same(got, want):
    """A device record equals a restatement tuple, bit for bit."""
    out_v, out_f, vmap, vcls, counts = want
    assert list(got.stats) == list(wref.COUNT_NAMES) and list(got.stats.values()) == counts.tolist(), (got.stats, counts)
    assert got.vertices.shape == out_v.shape and torch.equal(_bits(got.vertices), torch.from_numpy(out_v).view(torch.int64))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(out_f).reshape(-1, 3))
    assert torch.equal(got.vertex_map.cpu(), torch.from_numpy(vmap))
    assert torch.equal(got.vertex_class.cpu(), torch.from_numpy(vcls))


def _assert_matches(v, f, h, want=None, **kw):
    got = _run(v, f, h, **kw)
    _assert_same(got, wref.weld(v, f, h) if want is None else want)
    return got


# --------------------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(device, name):
    v, f, h, vertex_class, vertex_map, faces, counts = HAND_CASES[name]
    got = _run(v, f, h)
    assert got.vertex_class.tolist() == vertex_class and got.vertex_map.tolist() == vertex_map
    assert got.faces.tolist() == faces and list(got.stats.values()) == counts
    _assert_matches(v, f, h)


def test_nan_payloads_and_signed_zeros_pass_through(device):
    got = _run(HAND_CASES["loose"][0], None, 0.0)
    assert _bits(got.vertices)[2, 0] == _bits(got.vertices)[3, 0] == NAN_A
    got = _run(HAND_CASES["signed_zero"][0], None, 0.0)
    assert _bits(got.vertices).tolist() == [[-2 ** 63, 0, 0]]
    v = np.array([[0.0, -0.0, 1.0], [-0.0, 0.0, 1.0], [-0.0, -0.0, -0.0], [0.0, 0.0, 0.0]])
    for h in (0.0, 0.125):
        got = _assert_matches(v, None, h)
        assert _bits(got.vertices).tolist() == [[0, -2 ** 63, 0x3FF0000000000000], [-2 ** 63] * 3]


@functools.lru_cache(maxsize=None)
def _lattice(n):
    v = wref.lattice_cloud(n, n)
    return v, np.random.default_rng(n).integers(0, n, (n, 3))


@pytest.mark.parametrize("h", [0.0, 0.75])
@pytest.mark.parametrize("n", [63, 64, 65, 1023, 1024, 1025, 1026])
def test_lattice_clouds_around_a_wave_and_a_scan_chunk(device, n, h):
    v, f = _lattice(n)
    got = _assert_matches(v, f, h)
    assert (n == 63 or got.stats["merged_classes"] > 0) and (n < 1000 or got.stats["collapsed_faces"] > 0)
    assert got.stats["vertices"] == np.unique(v, axis=0).shape[0]             # 0.75 steps link nothing a step apart


@pytest.mark.parametrize("h", [0.0, 1e-4])
def test_one_point_two_thousand_times_among_distinct_ones(device, h):
    v = wref.copies_and_distinct(2048)
    got = _assert_matches(v, None, h)
    assert got.stats["vertices"] == 2049 and got.stats["largest_class"] == 2048 and got.stats["merged_classes"] == 1
    assert got.stats["largest_cell"] == (2048 if h > 0 else 0)
    assert (got.vertex_class[0::2] == 0).all()


@functools.lru_cache(maxsize=None)
def _chain_want(factor):
    v = wref.chain(4096, factor * 0.01)
    return v, wref.weld_cells(v, None, 0.01)


def test_chain_spaced_below_the_tolerance_is_one_class(device):
    v, want = _chain_want(0.9)
    got = _assert_matches(v, None, 0.01, want)
    assert got.stats["vertices"] == 1 and got.stats["largest_class"] == 4096 and got.stats["largest_cell"] < 8


def test_chain_spaced_above_the_tolerance_stays_apart(device):
    v, want = _chain_want(1.1)
    got = _assert_matches(v, None, 0.01, want)
    assert got.stats["vertices"] == 4096 and got.stats["merged_classes"] == 0
    assert torch.equal(_bits(got.vertices), torch.from_numpy(v).view(torch.int64))


@pytest.mark.parametrize("h", [0.5, 0.1])
def test_points_on_cell_borders(device, h):
    """Multiples of the cell edge 2 h on all three axes, negative ones included; every second one has a partner at h
    along an axis: exactly h for h = 0.5, whatever the rounding of k * 0.2 + 0.1 makes of it for h = 0.1 (the brute-force
    restatement decides)."""
    k = np.arange(-4, 5, dtype=np.float64)
    on = np.stack(np.meshgrid(k, k, k, indexing="ij"), axis=-1).reshape(-1, 3) * (2.0 * h)
    partner = on[::2].copy()
    partner[np.arange(partner.shape[0]), np.arange(partner.shape[0]) % 3] += h
    v = np.concatenate([on, partner])
    assert v.shape[0] == 729 + 365
    want = wref.weld_brute(v, None, h)
    assert same(want, wref.weld_cells(v, None, h))
    got = _assert_matches(v, None, h, want)
    assert got.stats["merged_classes"] > 0
    if h == 0.5:
        assert got.stats["vertices"] < 729                                    # the partners chain the lattice together


def test_repeated_icosphere_gives_the_sphere_back(device):
    h = 1e-3
    v, src = wref.repeated_sphere(2, 0, h)
    got = _assert_matches(v, None, h)
    assert got.stats["vertices"] == 162 and got.stats["largest_class"] <= 4
    cls = got.vertex_class.cpu().numpy()
    assert all(len(set(src[cls == c])) == 1 for c in range(162)) and len(set(src[got.vertex_map.cpu().numpy()])) == 162


def test_soup_of_the_icosphere_gives_the_mesh_back(device):
    v, f = ref.icosphere(3)
    sv, sf = wref.soup(v, f)
    assert sv.shape[0] == 3840
    got = _assert_matches(sv, sf, 0.0)
    uniq, first = np.unique(f.reshape(-1), return_index=True)
    rank = np.empty(v.shape[0], dtype=np.int64)
    rank[uniq[np.argsort(first)]] = np.arange(v.shape[0])                     # rule 4: by first appearance
    assert got.stats["vertices"] == 642 and np.array_equal(got.faces.cpu().numpy(), rank[f])
    w = got.vertices.cpu().numpy()
    assert w[got.faces.cpu().numpy()].tobytes() == v[f].tobytes() and w[rank].tobytes() == v.tobytes()
    assert got.stats["collapsed_faces"] == 0 and got.stats["largest_class"] == 6


def test_soup_of_the_grid_past_two_to_the_twenty_corners(device):
    v, f = ref.grid(420)
    sv, sf = wref.soup(v, f)
    assert sv.shape[0] > 2 ** 20
    got = _assert_matches(sv, sf, 0.0)
    assert got.stats["vertices"] == v.shape[0] == 420 * 420
    assert torch.equal(_bits(got.vertices[got.faces]), torch.from_numpy(sv[sf]).view(torch.int64))


# ------------------------------------------------------------------------------------------------------ 2. input variants
def test_int32_faces_fp32_vertices_and_no_faces(device):
    v, f = _lattice(1025)
    _assert_matches(v, f, 0.75, faces_dtype=np.int32)
    v32 = (v + np.random.default_rng(3).uniform(-0.1, 0.1, v.shape)).astype(np.float32)
    for h in (0.0, 0.3):
        _assert_matches(v32.astype(np.float64), f, h, wref.weld(v32.astype(np.float64), f, h), vertices_dtype=np.float32)
    got = _assert_matches(v, None, 0.0)
    assert got.faces.shape == (0, 3)
    plain = _mc().weld_vertices_device(_dev(v, np.float64))
    assert plain.stats is None and torch.equal(plain.vertex_class, got.vertex_class)
    empty = _mc().weld_vertices_device(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda"),
                                       return_stats=True)
    assert empty.vertices.shape == (0, 3) and empty.vertex_map.shape == empty.vertex_class.shape == (0,)
    assert list(empty.stats.values()) == [0] * 8


@pytest.mark.parametrize("h", [0.0, 0.3])
def test_two_runs_give_identical_bytes(device, h):
    v = wref.lattice_cloud(20000, 5) + np.random.default_rng(5).uniform(-0.15, 0.15, (20000, 3)) * (h > 0)
    f = np.random.default_rng(6).integers(0, 20000, (30000, 3))
    dv, df = _dev(v, np.float64), _dev(f, np.int64)
    a = _mc().weld_vertices_device(dv, df, h, return_stats=True)
    b = _mc().weld_vertices_device(dv, df, h, return_stats=True)
    assert a.stats == b.stats and torch.equal(_bits(a.vertices), _bits(b.vertices)) and torch.equal(a.faces, b.faces)
    assert torch.equal(a.vertex_map, b.vertex_map) and torch.equal(a.vertex_class, b.vertex_class)
    assert torch.equal(_bits(dv), torch.from_numpy(v).view(torch.int64)) and torch.equal(df.cpu(), torch.from_numpy(f))   # inputs untouched
    _assert_same(a, wref.weld_cells(v, f, h) if h > 0 else wref.weld_exact(v, f))
    assert a.stats["largest_class"] > 6


def _raw(v, f, device):
    from quadraturefields_amd import _C
    t = dict(v=_dev(v, np.float64), f=_dev(f, np.int64))
    need = int(_C.lib().qf_mesh_weld_workspace_bytes(len(v), len(f)))
    t["ws"] = torch.zeros((need,), dtype=torch.uint8, device=device)
    t["counts"] = torch.full((8,), -7, dtype=torch.int64, device=device)
    t["out_v"] = torch.full((len(v), 3), -7.0, dtype=torch.float64, device=device)
    t["out_f"] = torch.full((len(f), 3), -7, dtype=torch.int64, device=device)
    t["vmap"] = torch.full((len(v),), -7, dtype=torch.int64, device=device)
    t["vcls"] = torch.full((len(v),), -7, dtype=torch.int64, device=device)
    return t, need


def test_refusals_come_before_any_launch(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f, h = HAND_CASES["line"][:3]
    f = np.asarray(f)
    t, need = _raw(v, f, device)
    n_v, n_f = len(v), len(f)

    def count(ws_bytes=need, V=n_v, F=n_f, tol=h, vertices=t["v"], faces=t["f"], ws=t["ws"], counts=t["counts"]):
        return lib.qf_mesh_weld_count(_C.ptr(vertices), V, _C.ptr(faces), F, tol, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream())

    def emit(ws_bytes=need, V=n_v, F=n_f, cap=n_v, vertices=t["v"], faces=t["f"], ws=t["ws"], out_v=t["out_v"], out_f=t["out_f"]):
        return lib.qf_mesh_weld_emit(_C.ptr(vertices), V, _C.ptr(faces), F, _C.ptr(ws), ws_bytes, _C.ptr(out_v), cap,
                                     _C.ptr(out_f), _C.ptr(t["vmap"]), _C.ptr(t["vcls"]), _C.stream())

    for status in (count(ws_bytes=need - 1), count(V=0), count(V=2 ** 31), count(F=-1), count(F=2 ** 31), count(tol=-1e-300),
                   count(tol=float("nan")), count(tol=float("inf")), count(tol=-float("inf")), count(vertices=None),
                   count(faces=None), count(ws=None), count(counts=None),
                   emit(ws_bytes=need - 1), emit(V=0), emit(F=-1), emit(cap=-1), emit(cap=n_v + 1), emit(vertices=None),
                   emit(faces=None), emit(ws=None), emit(out_v=None), emit(out_f=None)):
        assert status == -1
    torch.cuda.synchronize()
    assert (t["counts"] == -7).all() and not t["ws"].any()                              # nothing ran
    assert (t["out_v"] == -7.0).all() and (t["out_f"] == -7).all() and (t["vmap"] == -7).all() and (t["vcls"] == -7).all()
    assert count(faces=None, F=0) == 0                                                  # faces may be NULL with F = 0
    assert count() == 0 and emit() == 0
    torch.cuda.synchronize()
    want = wref.weld(v, f, h)
    n_out = int(t["counts"][0])
    assert t["counts"].tolist() == want[4].tolist() and torch.equal(t["out_f"].cpu(), torch.from_numpy(want[1]))
    assert torch.equal(_bits(t["out_v"][:n_out]), torch.from_numpy(want[0]).view(torch.int64))
    assert torch.equal(t["vmap"][:n_out].cpu(), torch.from_numpy(want[2])) and torch.equal(t["vcls"].cpu(), torch.from_numpy(want[3]))
    assert (t["out_v"][n_out:] == -7.0).all() and (t["vmap"][n_out:] == -7).all()       # rows beyond V' are not written


def test_rows_beyond_a_capacity_are_not_written_and_the_maps_may_be_null(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f = _lattice(1025)
    t, need = _raw(v, f, device)
    want = wref.weld(v, f, 0.0)
    assert want[4][0] > 100
    _C.check(lib.qf_mesh_weld_count(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]), len(f), 0.0, _C.ptr(t["ws"]), need, _C.ptr(t["counts"]),
                                    _C.stream()), "count")
    _C.check(lib.qf_mesh_weld_emit(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]), len(f), _C.ptr(t["ws"]), need, _C.ptr(t["out_v"]), 100,
                                   _C.ptr(t["out_f"]), None, None, _C.stream()), "emit")
    torch.cuda.synchronize()
    assert torch.equal(_bits(t["out_v"][:100]), torch.from_numpy(want[0][:100]).view(torch.int64)) and (t["out_v"][100:] == -7.0).all()
    assert torch.equal(t["out_f"].cpu(), torch.from_numpy(want[1])) and (t["vmap"] == -7).all() and (t["vcls"] == -7).all()
    _C.check(lib.qf_mesh_weld_emit(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]), len(f), _C.ptr(t["ws"]), need, None, 0,
                                   _C.ptr(t["out_f"]), _C.ptr(t["vmap"]), _C.ptr(t["vcls"]), _C.stream()), "emit")
    torch.cuda.synchronize()
    assert (t["vmap"] == -7).all() and torch.equal(t["vcls"].cpu(), torch.from_numpy(want[3]))


@pytest.mark.parametrize("name", sorted(REFUSED_CASES))
def test_refused_meshes_raise_with_their_counts_and_write_nothing(device, name):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f, h, counts = REFUSED_CASES[name]
    f = np.zeros((0, 3), np.int64) if f is None else np.asarray(f)
    match = f"{counts[7]} faces have an index outside" if counts[7] else f"{counts[6]} vertices have a search cell out of range"
    with pytest.raises(ValueError, match=match):
        _mc().weld_vertices_device(_dev(v, np.float64), _dev(f, np.int64), h)
    t, need = _raw(v, f, device)
    _C.check(lib.qf_mesh_weld_count(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]) if len(f) else None, len(f), h, _C.ptr(t["ws"]), need,
                                    _C.ptr(t["counts"]), _C.stream()), "count")
    _C.check(lib.qf_mesh_weld_emit(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]) if len(f) else None, len(f), _C.ptr(t["ws"]), need,
                                   _C.ptr(t["out_v"]), len(v), _C.ptr(t["out_f"]) if len(f) else None, _C.ptr(t["vmap"]),
                                   _C.ptr(t["vcls"]), _C.stream()), "emit")
    torch.cuda.synchronize()
    assert t["counts"].tolist() == counts
    assert (t["out_v"] == -7.0).all() and (t["out_f"] == -7).all() and (t["vmap"] == -7).all() and (t["vcls"] == -7).all()


# ------------------------------------------------------------------------------------------------------- 3. downstream
def _masked_sphere():
    return mref.masked(*ref.icosphere(3), 0)


def _holed_sphere():
    """The level-3 icosphere with a seeded 15 % of its faces removed: bow-ties where two holes touch, and enough interior
    for lock-mode decimation to get somewhere."""
    v, f = ref.icosphere(3)
    return oref._drop_unreferenced(v, f[np.random.default_rng(0).random(f.shape[0]) < 0.85])


@pytest.mark.parametrize("name", ["bowtie", "masked_sphere"])
def test_weld_undoes_the_manifold_cut(device, name):
    v, f = oref.bowtie()[:2] if name == "bowtie" else _masked_sphere()
    assert wref.weld_exact(v, f)[4][0] == v.shape[0]                          # no coincident vertices to begin with
    cut = _mc().make_manifold_device(_dev(v, np.float64), _dev(f, np.int64))
    assert cut.vertices.shape[0] > v.shape[0]
    got = _mc().weld_vertices_device(cut.vertices, cut.faces, 0.0, return_stats=True)
    _assert_same(got, wref.weld_exact(cut.vertices.cpu().numpy(), cut.faces.cpu().numpy()))
    assert got.vertices.shape[0] == v.shape[0]
    assert torch.equal(_bits(got.vertices[got.faces]), torch.from_numpy(v[f]).view(torch.int64))
    assert torch.equal(_bits(got.vertices), torch.from_numpy(v).view(torch.int64)) and torch.equal(got.faces.cpu(), torch.from_numpy(f))


def test_weld_after_lock_mode_decimation_of_a_cut_mesh(device):
    v, f = _holed_sphere()
    cut = _mc().make_manifold_device(_dev(v, np.float64), _dev(f, np.int64))
    dec = _mc().decimate_mesh_device(cut.vertices, cut.faces, f.shape[0] // 2, boundary="lock")
    assert dec.faces.shape[0] < f.shape[0]
    dv, df = dec.vertices.cpu().numpy(), dec.faces.cpu().numpy()
    want = wref.weld_exact(dv, df)
    coinciding = dv.shape[0] - int(want[4][0])                                # copies that still sit on another vertex
    assert coinciding > 0
    got = _mc().weld_vertices_device(dec.vertices, dec.faces, 0.0, return_stats=True)
    _assert_same(got, want)
    assert dec.vertices.shape[0] - got.vertices.shape[0] == coinciding
    assert torch.equal(got.vertices[got.faces], dec.vertices[dec.faces]) and got.stats["collapsed_faces"] == 0


def test_intersection_of_the_welded_atlas_mesh_is_the_original_ones(device):
    from quadraturefields_amd import synthetic, uv_atlas
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    original = synthetic.shell_mesh()
    atlas = uv_atlas.per_triangle_atlas(original, 2048)[0]
    assert atlas.vertices.shape[0] == 3 * original.faces.shape[0] == 2_949_120
    welded, vertex_map, vertex_class = _mc().weld_vertices(atlas, 0.0)
    assert welded.vertices.shape[0] == original.vertices.shape[0] == 491_544 and vertex_class.shape[0] == 2_949_120
    assert np.array_equal(welded.vertices[welded.faces], original.vertices[original.faces])
    assert np.array_equal(welded.visual.uv, atlas.visual.uv[vertex_map])      # the root's uv: the atlas is gone
    rng = np.random.default_rng(0)
    o = rng.normal(size=(4096, 3))
    o = (2.0 * o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    d = (-o + rng.normal(size=o.shape).astype(np.float32) * 0.3)
    d = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    o, d = torch.from_numpy(o).cuda(), torch.from_numpy(d).cuda()
    lists = []
    for mesh in (original, TriMesh(welded.vertices, welded.faces)):
        mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=8, device=device, bvh_builder="device")
        lists.append([t.clone() for t in mi.rayintersector.hits(o, d, 8)])
    assert int(lists[0][2].sum()) > 4096
    for a, b in zip(*lists):
        assert sh.same_bits(a, b)


def test_vertex_baked_frame_of_the_welded_soup_is_the_soups_frame(device):
    """The set-up of the frame test of tests/test_gpu_mesh_manifold.py, at its size: a 64 x 64, K = 5 frame."""
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    from tests import vertex_baked_reference as R
    m = R.mesh()
    c2w, focal, o, d = R.camera(64, 64)
    o, d = o.to(device), d.to(device)
    cam = make_camera(c2w, focal, 64, 64)
    field = R.sg_field(2, device)
    mi = MeshIntersection(TriMesh(m.vertices, m.faces), simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    table = baking.bake_vertex_features(field, mi)
    sv, sf = wref.soup(m.vertices, m.faces)
    repeated = table[torch.from_numpy(np.asarray(m.faces).reshape(-1)).to(device)]
    mi_soup = MeshIntersection(TriMesh(sv, sf), simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    frame = [t.clone() for t in FrameRenderer(mi_soup, field).render_vertex_baked(o, d, repeated, camera=cam)[:3]]
    welded, vertex_map, vertex_class = _mc().weld_vertices(TriMesh(sv, sf), 0.0)
    assert welded.vertices.shape[0] < sv.shape[0] and np.array_equal(welded.vertices[welded.faces], sv[sf])
    carried = baking.weld_vertex_features(repeated, vertex_class, welded.vertices.shape[0], "first")
    assert carried.shape == (len(vertex_map), table.shape[1])
    assert sh.same_bits(carried, baking.remap_vertex_features(repeated, vertex_map))
    mi_welded = MeshIntersection(welded, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    frame_welded = FrameRenderer(mi_welded, field).render_vertex_baked(o, d, carried, camera=cam)[:3]
    assert float(frame[1].sum()) > 0
    for a, b in zip(frame, frame_welded):
        assert sh.same_bits(a, b)
    module = baking.weld_vertex_features(baking.VertexBakedFeatures(repeated), torch.from_numpy(vertex_class), len(vertex_map))
    assert isinstance(module, baking.VertexBakedFeatures) and sh.same_bits(module.features(), carried[:, :module.width])
    with pytest.raises(TypeError, match="QuantisedVertexFeatures"):
        baking.weld_vertex_features(baking.quantise_vertex_features(table), vertex_class[:table.shape[0]], len(vertex_map))


def test_mean_of_a_table_is_the_stated_formula_twice(device):
    from quadraturefields_amd import baking
    v, src = wref.repeated_sphere(2, 1, 1e-3)
    got = _run(v, None, 1e-3)
    cls = got.vertex_class.cpu().numpy()
    rng = np.random.default_rng(2)
    table = (rng.normal(size=(v.shape[0], 16)) * 10.0 ** rng.integers(-6, 7, (v.shape[0], 16))).astype(np.float32)
    want = np.empty((162, 16), dtype=np.float32)
    for c in range(162):
        members = np.flatnonzero(cls == c)                                    # increasing vertex index
        total = table[members[0]].astype(np.float64)
        for i in members[1:]:
            total = total + table[i].astype(np.float64)
        want[c] = (total / np.float64(members.shape[0])).astype(np.float32)
    dev_table = torch.from_numpy(table).cuda()
    a = baking.weld_vertex_features(dev_table, got.vertex_class, 162, reduce="mean")
    b = baking.weld_vertex_features(dev_table, got.vertex_class, 162, reduce="mean")
    assert a.dtype == torch.float32 and a.cpu().numpy().tobytes() == want.tobytes() and sh.same_bits(a, b)
    first = baking.weld_vertex_features(dev_table, got.vertex_class, 162)
    assert first.cpu().numpy().tobytes() == table[got.vertex_map.cpu().numpy()].tobytes()


def test_host_wrappers_carry_uv_compact_and_downsample(device):
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = ref.icosphere(2)
    sv, sf = wref.soup(v, f)
    sf = np.concatenate([sf, sf[:3], [[0, 0, 1]]])                            # three duplicate faces and a degenerate one
    sv = np.concatenate([sv, [[9.0, 9.0, 9.0]]])                              # a vertex nothing uses
    uv = np.random.default_rng(1).random((sv.shape[0], 2))
    want = wref.weld_exact(sv, sf)
    mesh, vertex_map, vertex_class, stats = _mc().weld_vertices(TriMesh(sv, sf, uv), return_stats=True)
    assert mesh.vertices.tobytes() == want[0].tobytes() and np.array_equal(mesh.faces, want[1])
    assert np.array_equal(vertex_map, want[2]) and np.array_equal(vertex_class, want[3]) and np.array_equal(mesh.visual.uv, uv[want[2]])
    assert list(stats.values()) == want[4].tolist() and len(_mc().weld_vertices(TriMesh(sv, sf))) == 3
    cleaned, face_map, vmap, vcls = _mc().weld_vertices(TriMesh(sv, sf, uv), compact=True)
    assert cleaned.faces.shape[0] == f.shape[0] and cleaned.vertices.shape[0] == 162 and np.array_equal(face_map, np.arange(f.shape[0]))
    assert np.array_equal(cleaned.vertices, sv[vmap]) and np.array_equal(cleaned.visual.uv, uv[vmap])
    assert vcls[-1] == -1 and (vcls[:-1] >= 0).all() and np.array_equal(cleaned.vertices[vcls[:-1]], sv[:-1])
    assert np.array_equal(cleaned.vertices[cleaned.faces], sv[sf[face_map]])
    # downsample_mesh: None is the clustered mesh bit for bit, a tolerance welds it afterwards
    gv, gf = ref.icosphere(4)
    plain = _mc().downsample_mesh(TriMesh(gv, gf), 8)
    same = _mc().downsample_mesh(TriMesh(gv, gf), 8, merge_tolerance=None)
    assert plain.vertices.tobytes() == same.vertices.tobytes() and np.array_equal(plain.faces, same.faces)
    merged = _mc().downsample_mesh(TriMesh(gv, gf), 8, merge_tolerance=0.2)
    want = wref.weld(plain.vertices, plain.faces, 0.2)
    assert merged.vertices.tobytes() == want[0].tobytes() and np.array_equal(merged.faces, want[1])
    assert merged.vertices.shape[0] < plain.vertices.shape[0]


def _example(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(root, "examples", name + ".py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_weld_example_writes_the_mesh_and_both_maps(device, tmp_path, capsys):
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = ref.icosphere(2)
    sv, sf = wref.soup(v.astype(np.float32).astype(np.float64), f)
    a, b = tmp_path / "plain", tmp_path / "compact"
    a.mkdir()
    b.mkdir()
    TriMesh(sv, sf).export(str(tmp_path / "in.ply"))
    loaded = load_mesh(str(tmp_path / "in.ply"))
    lv, lf = np.asarray(loaded.vertices, np.float64), np.asarray(loaded.faces, np.int64)
    want = wref.weld_exact(lv, lf)
    _example("weld_mesh").main([str(tmp_path / "in.ply"), str(a / "out.ply"), "--tolerance", "0"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1 and sorted(os.listdir(a)) == ["out.ply", "weld_vertex_class.npy", "weld_vertex_map.npy"]
    stats = json.loads(out[0])
    assert [stats[k] for k in wref.COUNT_NAMES] == want[4].tolist() and stats["vertices_in"] == 960 and stats["vertices_out"] == 162
    assert np.array_equal(np.load(a / "weld_vertex_map.npy"), want[2]) and np.array_equal(np.load(a / "weld_vertex_class.npy"), want[3])
    assert np.array_equal(load_mesh(str(a / "out.ply")).faces, want[1])
    _example("weld_mesh").main([str(tmp_path / "in.ply"), str(b / "out.obj"), "--tolerance", "0.7", "--compact"])
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(b)) == ["out.obj", "weld_face_map.npy", "weld_vertex_class.npy", "weld_vertex_map.npy"]
    big = wref.weld(lv, lf, 0.7)
    assert stats["vertices"] == big[4][0] < 162 and stats["collapsed_faces"] == big[4][3] > 0
    assert stats["faces_out"] == len(np.load(b / "weld_face_map.npy")) < 320


def test_decimate_example_welds_last_with_the_flag_and_is_unchanged_without(device, tmp_path, capsys):
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = _holed_sphere()
    target = f.shape[0] // 2
    a, b = tmp_path / "plain", tmp_path / "weld"
    a.mkdir()
    b.mkdir()
    TriMesh(v, f).export(str(tmp_path / "in.ply"))
    loaded = load_mesh(str(tmp_path / "in.ply"))
    lv, lf = np.asarray(loaded.vertices, np.float64), np.asarray(loaded.faces, np.int64)
    table = np.random.default_rng(4).normal(size=(lv.shape[0], 16)).astype(np.float32)
    np.save(tmp_path / "table.npy", table)
    example = _example("decimate_mesh")
    example.main([str(tmp_path / "in.ply"), str(a / "out.ply"), "--target_faces", str(target), "--make_manifold"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(a)) == ["cut_vertex_map.npy", "face_map.npy", "out.ply", "vertex_target.npy"]
    assert not any(k.startswith("weld_") for k in plain)
    cv, cf = mref.cut(lv, lf)[:2]
    dec = ref.decimate(cv, cf, target)
    assert np.array_equal(load_mesh(str(a / "out.ply")).faces, dec[1]) and plain["faces_out"] == dec[1].shape[0]

    example.main([str(tmp_path / "in.ply"), str(b / "out.ply"), "--target_faces", str(target), "--make_manifold", "--weld", "0",
                  "--vertex_features", str(tmp_path / "table.npy"), "--out_vertex_features", str(b / "table_out.npy")])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    stats = json.loads(out[0])
    assert sorted(os.listdir(b)) == ["cut_vertex_map.npy", "face_map.npy", "out.ply", "table_out.npy", "vertex_target.npy",
                                     "weld_vertex_class.npy", "weld_vertex_map.npy"]
    want = wref.weld_exact(dec[0], dec[1])
    assert stats["weld_tolerance"] == 0.0 and stats["weld_vertices_removed"] == dec[0].shape[0] - want[4][0] > 0
    assert stats["weld_merged_classes"] == want[4][1] and stats["weld_largest_class"] == want[4][2]
    assert stats["weld_collapsed_faces"] == 0 and stats["vertices_out"] == want[4][0] and stats["faces_out"] == plain["faces_out"]
    assert np.array_equal(np.load(b / "weld_vertex_map.npy"), want[2]) and np.array_equal(np.load(b / "weld_vertex_class.npy"), want[3])
    assert np.array_equal(np.load(b / "vertex_target.npy"), np.load(a / "vertex_target.npy"))
    assert np.array_equal(load_mesh(str(b / "out.ply")).faces, want[1])
    assert np.load(b / "table_out.npy").shape == (want[4][0], 16)
