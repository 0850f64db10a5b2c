"""GPU: the manifold repair (``mc_utils.make_manifold_device`` / ``qf_mesh_manifold_*``) against its
numpy restatement (tests/mesh_manifold_reference.py).  Every comparison with the restatement is exact: vertices by bits,
faces, the map and the counts."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import mesh_decimate_open_reference as oref
from tests import mesh_decimate_reference as ref
from tests import mesh_manifold_reference as mref
from tests import stream_harness as sh
from tests.test_mesh_manifold_host import HAND_CASES, masked_sphere

pytestmark = pytest.mark.gpu


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


def _run(v, f, faces_dtype=np.int64):
    got = _mc().make_manifold_device(_dev(v, np.float64), _dev(np.asarray(f).reshape(-1, 3), faces_dtype), return_stats=True)
    torch.cuda.synchronize()
    assert got.vertices.dtype == torch.float64 and got.faces.dtype == got.vertex_map.dtype == torch.int64
    return got


def _assert_same(got, want):
    """A device record equals a restatement tuple, bit for bit."""
    out_v, out_f, vmap, counts = want
    assert list(got.stats) == list(mref.COUNT_NAMES) and list(got.stats.values()) == counts.tolist(), (got.stats, counts)
    assert got.vertices.shape == out_v.shape and torch.equal(_bits(got.vertices), torch.from_numpy(out_v).view(torch.int64))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(out_f).reshape(-1, 3))
    assert torch.equal(got.vertex_map.cpu(), torch.from_numpy(vmap))


def _assert_matches(v, f, faces_dtype=np.int64):
    got = _run(v, f, faces_dtype)
    _assert_same(got, mref.cut(v, f))
    return got


# --------------------------------------------------------------------------------------------------------- 1. the rule
@pytest.mark.parametrize("name", sorted(HAND_CASES))
def test_hand_worked_case(device, name):
    build, faces, vertex_map, counts = HAND_CASES[name]
    v, f = build()
    got = _run(v, f)
    assert got.faces.tolist() == faces and got.vertex_map.tolist() == vertex_map and list(got.stats.values()) == counts
    _assert_matches(v, f)


def test_nan_payloads_and_fp32_vertices_move_bit_for_bit(device):
    v, f = mref.book(3)
    v = v.copy()
    v.view(np.uint64)[0, 0] = 0x7FF8000000ABCDEF                 # a NaN with a payload, at a vertex that is split
    v.view(np.uint64)[1, 2] = 0xFFF0000000000001
    _assert_matches(v, f)
    v32 = np.random.default_rng(0).normal(size=(5, 3)).astype(np.float32)
    got = _mc().make_manifold_device(torch.from_numpy(v32).cuda(), _dev(f, np.int64))
    assert got.stats is None and torch.equal(_bits(got.vertices), torch.from_numpy(mref.cut(v32.astype(np.float64), f)[0]).view(torch.int64))


@pytest.mark.parametrize("level,seed", [(3, 0), (3, 1), (5, 0)])
def test_masked_icospheres(device, level, seed):
    v, f = masked_sphere(level, seed)
    got = _assert_matches(v, f)
    assert got.stats["split_vertices"] > 0 and got.stats["complex_edges"] == 0


@pytest.mark.parametrize("n_faces", [63, 64, 65, 341, 342])
def test_strips_around_a_wave_and_a_scan_chunk(device, n_faces):
    """63 / 64 / 65 faces cross a wave of face threads; 341 / 342 faces are 1 023 / 1 026 corners, across a scan chunk."""
    v, f = mref.strip(n_faces)
    assert f.shape[0] == n_faces
    got = _assert_matches(v, f)
    assert got.stats["split_vertices"] > 0
    g = np.concatenate([f[: n_faces // 2], [[0, 0, 1]], f[n_faces // 2:]])             # a degenerate face in the middle
    assert _assert_matches(v, g).stats["degenerate_faces"] == 1


def test_pinched_fan_has_one_class_per_triangle_at_the_apex(device):
    v, f = mref.pinched_fan(48)
    got = _assert_matches(v, f)
    assert got.vertices.shape[0] == 49 + 23 and got.stats["split_vertices"] == 1
    assert got.faces[:, 0].tolist() == [0] + list(range(49, 72)) and (got.vertex_map[49:] == 0).all()


def test_closed_ring_comes_back_as_itself(device):
    v, f = mref.ring(2048)
    got = _assert_matches(v, f)
    assert torch.equal(got.faces.cpu(), torch.from_numpy(f)) and got.vertices.shape[0] == 2048
    assert got.stats["boundary_edges"] == 2048 and got.stats["split_vertices"] == 0
    both = np.concatenate([f, f[:, [1, 0, 2]] + 0])                                   # every face twice, once reversed
    assert _assert_matches(v, both).stats["complex_edges"] > 0


@functools.lru_cache(maxsize=None)
def _grid_420():
    return ref.grid(420)


def test_masked_grid_past_two_to_the_nineteen_corners(device):
    v, f = mref.masked(*_grid_420(), 0)
    assert 3 * f.shape[0] > 2 ** 19 and f.shape[0] > 170_000
    got = _assert_matches(v, f)
    assert got.stats["split_vertices"] > 50_000


def test_full_grid_past_two_to_the_twenty_corners_comes_back_as_itself(device):
    v, f = _grid_420()
    assert 3 * f.shape[0] == 1_053_366
    got = _assert_matches(v, f)
    assert torch.equal(got.faces.cpu(), torch.from_numpy(f)) and torch.equal(_bits(got.vertices), torch.from_numpy(v).view(torch.int64))
    assert got.stats["vertices"] == v.shape[0] and got.stats["boundary_edges"] == 4 * 419


def test_guarantees_on_the_device_output(device):
    v, f = masked_sphere(3, 0)
    got = _run(v, f)
    w, g = got.vertices.cpu().numpy(), got.faces.cpu().numpy()
    assert w[g].tobytes() == v[f].tobytes()
    assert mref.edge_uses(g, w.shape[0])[0].max() <= 2 and mref.complex_vertices(w, g) == 0
    again = _run(w, g)                                                                 # idempotent on the device
    assert torch.equal(again.faces, got.faces) and torch.equal(_bits(again.vertices), _bits(got.vertices))
    assert torch.equal(again.vertex_map.cpu(), torch.arange(w.shape[0])) and again.stats["split_vertices"] == 0


# ------------------------------------------------------------------------------------------------------ 2. run to run
def test_int32_faces_give_the_same_result(device):
    v, f = masked_sphere(3, 1)
    _assert_matches(v, f, faces_dtype=np.int32)


def test_two_runs_give_identical_bytes(device):
    v, f = masked_sphere(5, 0)
    dv, df = _dev(v, np.float64), _dev(f, np.int64)
    a = _mc().make_manifold_device(dv, df, return_stats=True)
    b = _mc().make_manifold_device(dv, df, return_stats=True)
    assert a.stats == b.stats and torch.equal(_bits(a.vertices), _bits(b.vertices)) and torch.equal(a.faces, b.faces)
    assert torch.equal(a.vertex_map, b.vertex_map)
    assert torch.equal(_bits(dv), torch.from_numpy(v).view(torch.int64)) and torch.equal(df.cpu(), torch.from_numpy(f))   # inputs untouched


def test_host_mesh_wrapper_carries_uv(device):
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = masked_sphere(3, 0)
    uv = np.random.default_rng(1).random((v.shape[0], 2))
    want = mref.cut(v, f)
    mesh, vertex_map, stats = _mc().make_manifold(TriMesh(v, f, uv), return_stats=True)
    assert mesh.vertices.tobytes() == want[0].tobytes() and np.array_equal(mesh.faces, want[1])
    assert np.array_equal(vertex_map, want[2]) and np.array_equal(mesh.visual.uv, uv[want[2]])
    assert list(stats.values()) == want[3].tolist()
    assert len(_mc().make_manifold(TriMesh(v, f))) == 2
    empty = _mc().make_manifold_device(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda"))
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3) and empty.vertex_map.shape == (0,)


def _raw(v, f, device, n_edges=None):
    from quadraturefields_amd import _C
    e, fe = mref.edges(f, len(v))
    n_e = len(e) if n_edges is None else n_edges
    t = dict(v=_dev(v, np.float64), f=_dev(f, np.int64), fe=_dev(fe, np.int64))
    need = int(_C.lib().qf_mesh_manifold_workspace_bytes(len(v), len(f), n_e))
    t["ws"] = torch.zeros((need,), dtype=torch.uint8, device=device)
    t["counts"] = torch.full((8,), -7, dtype=torch.int64, device=device)
    cap = len(v) + 3 * len(f)
    t["out_v"] = torch.full((cap, 3), -7.0, dtype=torch.float64, device=device)
    t["out_f"] = torch.full((len(f), 3), -7, dtype=torch.int64, device=device)
    t["vmap"] = torch.full((cap,), -7, dtype=torch.int64, device=device)
    return t, n_e, need


def test_refusals_come_before_any_launch(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f = mref.book(4)
    t, n_e, need = _raw(v, f, device)
    n_v, n_f = len(v), len(f)

    def count(ws_bytes=need, V=n_v, F=n_f, E=n_e, faces=t["f"], fe=t["fe"], ws=t["ws"], counts=t["counts"]):
        return lib.qf_mesh_manifold_count(_C.ptr(faces), F, V, _C.ptr(fe), E, _C.ptr(ws), ws_bytes, _C.ptr(counts), _C.stream())

    def emit(ws_bytes=need, V=n_v, F=n_f, cap=n_v + 3 * n_f, vertices=t["v"], faces=t["f"], ws=t["ws"], out_v=t["out_v"],
             out_f=t["out_f"]):
        return lib.qf_mesh_manifold_emit(_C.ptr(vertices), _C.ptr(faces), F, V, _C.ptr(ws), ws_bytes, _C.ptr(out_v), cap,
                                         _C.ptr(out_f), _C.ptr(t["vmap"]), _C.stream())

    for status in (count(ws_bytes=need - 1), count(V=0), count(V=2 ** 31), count(F=-1), count(F=2 ** 31 // 3 + 1), count(E=-1),
                   count(E=2 ** 31), count(faces=None), count(fe=None), count(ws=None), count(counts=None),
                   emit(ws_bytes=0), emit(V=0), emit(F=-1), emit(cap=-1), emit(cap=n_v + 3 * n_f + 1), emit(vertices=None),
                   emit(faces=None), emit(ws=None), emit(out_v=None), emit(out_f=None)):
        assert status == -1
    torch.cuda.synchronize()
    assert (t["counts"] == -7).all() and not t["ws"].any()                              # nothing ran
    assert (t["out_v"] == -7.0).all() and (t["out_f"] == -7).all() and (t["vmap"] == -7).all()
    assert count() == 0 and emit() == 0
    torch.cuda.synchronize()
    want = mref.cut(v, f)
    n_out = int(t["counts"][0])
    assert t["counts"].tolist() == want[3].tolist() and torch.equal(t["out_f"].cpu(), torch.from_numpy(want[1]))
    assert torch.equal(_bits(t["out_v"][:n_out]), torch.from_numpy(want[0]).view(torch.int64))
    assert torch.equal(t["vmap"][:n_out].cpu(), torch.from_numpy(want[2]))
    assert (t["out_v"][n_out:] == -7.0).all() and (t["vmap"][n_out:] == -7).all()       # rows beyond V' are not written


def test_rows_beyond_a_capacity_are_not_written_and_the_map_may_be_null(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f = mref.book(4)
    t, n_e, need = _raw(v, f, device)
    want = mref.cut(v, f)
    _C.check(lib.qf_mesh_manifold_count(_C.ptr(t["f"]), len(f), len(v), _C.ptr(t["fe"]), n_e, _C.ptr(t["ws"]), need,
                                        _C.ptr(t["counts"]), _C.stream()), "count")
    _C.check(lib.qf_mesh_manifold_emit(_C.ptr(t["v"]), _C.ptr(t["f"]), len(f), len(v), _C.ptr(t["ws"]), need, _C.ptr(t["out_v"]),
                                       8, _C.ptr(t["out_f"]), None, _C.stream()), "emit")
    torch.cuda.synchronize()
    assert torch.equal(_bits(t["out_v"][:8]), torch.from_numpy(want[0][:8]).view(torch.int64)) and (t["out_v"][8:] == -7.0).all()
    assert torch.equal(t["out_f"].cpu(), torch.from_numpy(want[1])) and (t["vmap"] == -7).all()


def test_invalid_faces_raise_with_their_count_and_write_nothing(device):
    from quadraturefields_amd import _C
    lib = _C.lib()
    v, f = mref.book(4)
    bad = f.copy()
    bad[1, 0], bad[3, 2] = -1, 6
    with pytest.raises(ValueError, match="2 faces have an index outside"):
        _mc().make_manifold_device(_dev(v, np.float64), _dev(bad, np.int64))
    # the raw calls: stage A's rows for the valid faces, then the same with an edge count that two rows leave
    for faces, n_edges, n_bad in ((bad, None, 2), (f, 4, 3)):
        t, n_e, need = _raw(v, f, device, n_edges)
        t["f"] = _dev(faces, np.int64)
        _C.check(lib.qf_mesh_manifold_count(_C.ptr(t["f"]), len(f), len(v), _C.ptr(t["fe"]), n_e, _C.ptr(t["ws"]), need,
                                            _C.ptr(t["counts"]), _C.stream()), "count")
        _C.check(lib.qf_mesh_manifold_emit(_C.ptr(t["v"]), _C.ptr(t["f"]), len(f), len(v), _C.ptr(t["ws"]), need,
                                           _C.ptr(t["out_v"]), len(v) + 3 * len(f), _C.ptr(t["out_f"]), _C.ptr(t["vmap"]),
                                           _C.stream()), "emit")
        torch.cuda.synchronize()
        assert t["counts"].tolist() == [0] * 7 + [n_bad]
        assert t["counts"].tolist() == mref.cut(v, faces, mref.edges(f, len(v))[1], n_e)[3].tolist()
        assert (t["out_v"] == -7.0).all() and (t["out_f"] == -7).all() and (t["vmap"] == -7).all()


# ------------------------------------------------------------------------------------------------------- 3. downstream
@pytest.mark.parametrize("seed", [0, 1])
def test_collapse_mode_gets_further_on_the_cut_mesh(device, seed):
    v, f = masked_sphere(3, seed)
    target = f.shape[0] // 10
    cut = _run(v, f)
    got = _mc().decimate_mesh_device(cut.vertices, cut.faces, target, return_stats=True, boundary="collapse")
    plain = _mc().decimate_mesh_device(_dev(v, np.float64), _dev(f, np.int64), target, return_stats=True, boundary="collapse")
    out_v, out_f = mref.cut(v, f)[:2]
    want = oref.decimate(out_v, out_f, target)
    print(f"seed {seed}: as it is {plain.faces.shape[0]} ({plain.stats['stop']}), cut {got.faces.shape[0]} ({got.stats['stop']})")
    assert torch.equal(_bits(got.vertices), torch.from_numpy(want[0]).view(torch.int64))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(want[1])) and torch.equal(got.face_map.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(got.vertex_target.cpu(), torch.from_numpy(want[3]))
    assert got.stats["rounds"] == want[4]["rounds"] and got.stats["stop"] == want[4]["stop"]
    assert got.faces.shape[0] < plain.faces.shape[0]


def test_intersection_of_the_cut_bowtie_is_the_uncut_ones(device):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    v, f, _ = oref.bowtie()
    cut = _mc().make_manifold(TriMesh(v, f))[0]
    assert cut.vertices.shape[0] == 50
    rng = np.random.default_rng(0)
    o = np.concatenate([rng.uniform(0.0, 2.0, (256, 2)), np.full((256, 1), 1.0)], axis=1)
    o[0, :2] = 1.0                                                                      # through the shared vertex
    d = rng.normal(size=(256, 3)) * 0.2
    d[:, 2] = -1.0
    d[0, :2] = 0.0
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    o, d = torch.from_numpy(o.astype(np.float32)).cuda(), torch.from_numpy(d.astype(np.float32)).cuda()
    lists = []
    for mesh in (TriMesh(v, f), cut):
        mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=4, device=device)
        lists.append([t.clone() for t in mi.rayintersector.hits(o, d, 4)])
    assert int(lists[0][2].sum()) > 64
    for a, b in zip(*lists):
        assert sh.same_bits(a, b)


def test_vertex_baked_frame_of_the_cut_mesh_is_the_uncut_frame(device):
    """The set-up of the soup-equality test of tests/test_gpu_mesh_compact.py, at its size: a 64 x 64, K = 5 frame."""
    from quadraturefields_amd import baking
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection, make_camera
    from quadraturefields_amd.render import FrameRenderer
    from tests import vertex_baked_reference as R
    m = R.mesh()
    keep = np.random.default_rng(5).random(len(m.faces)) < 0.5
    uncut = TriMesh(m.vertices, m.faces[keep], m.visual.uv)
    cut, vertex_map, stats = _mc().make_manifold(uncut, return_stats=True)
    assert stats["split_vertices"] > 0 and np.array_equal(cut.vertices[cut.faces], uncut.vertices[uncut.faces])
    c2w, focal, o, d = R.camera(64, 64)
    o, d = o.to(device), d.to(device)
    cam = make_camera(c2w, focal, 64, 64)
    field = R.sg_field(2, device)
    mi = MeshIntersection(uncut, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    table = baking.bake_vertex_features(field, mi)
    frame = [t.clone() for t in FrameRenderer(mi, field).render_vertex_baked(o, d, table, camera=cam)[:3]]
    mi_cut = MeshIntersection(cut, simplify_mesh=False, scale=1.0, num_intersections=5, device=device)
    carried = baking.remap_vertex_features(table, vertex_map)
    assert carried.shape == (len(vertex_map), table.shape[1])
    frame_cut = FrameRenderer(mi_cut, field).render_vertex_baked(o, d, carried, camera=cam)[:3]
    assert float(frame[1].sum()) > 0
    for a, b in zip(frame, frame_cut):
        assert sh.same_bits(a, b)
    with pytest.raises(TypeError):
        baking.remap_vertex_features(baking.quantise_vertex_features(table), vertex_map)


def _example():
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decimate_mesh_example", os.path.join(root, "examples", "decimate_mesh.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_example_cuts_first_with_the_flag_and_is_unchanged_without(device, tmp_path, capsys):
    import json
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = masked_sphere(3, 0)
    target = f.shape[0] // 10
    a, b = tmp_path / "plain", tmp_path / "cut"
    a.mkdir()
    b.mkdir()
    TriMesh(v, f).export(str(tmp_path / "in.ply"))
    loaded = load_mesh(str(tmp_path / "in.ply"))
    lv, lf = np.asarray(loaded.vertices, np.float64), np.asarray(loaded.faces, np.int64)
    example = _example()
    example.main([str(tmp_path / "in.ply"), str(a / "out.ply"), "--target_faces", str(target), "--boundary", "collapse"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert sorted(os.listdir(a)) == ["face_map.npy", "out.ply", "vertex_target.npy"]
    assert not any(k.startswith("cut_") for k in plain)
    want = oref.decimate(lv, lf, target)
    assert plain["faces_out"] == want[1].shape[0] and np.array_equal(load_mesh(str(a / "out.ply")).faces, want[1])
    assert sorted(plain) == sorted(list(want[4]) + ["boundary", "boundary_weight", "faces_in", "vertices_in", "target_faces",
                                                     "faces_out", "vertices_out"])

    example.main([str(tmp_path / "in.ply"), str(b / "out.ply"), "--target_faces", str(target), "--boundary", "collapse",
                  "--make_manifold"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    stats = json.loads(out[0])
    assert sorted(os.listdir(b)) == ["cut_vertex_map.npy", "face_map.npy", "out.ply", "vertex_target.npy"]
    cv, cf, cmap, counts = mref.cut(lv, lf)
    want = oref.decimate(cv, cf, target)
    assert stats["cut_vertices_added"] == counts[0] - lv.shape[0] > 0 and stats["cut_split_vertices"] == counts[1]
    assert stats["cut_complex_edges"] == 0 and stats["vertices_in"] == lv.shape[0] and stats["faces_in"] == lf.shape[0]
    assert np.array_equal(np.load(b / "cut_vertex_map.npy"), cmap)
    assert np.array_equal(np.load(b / "vertex_target.npy"), want[3]) and len(want[3]) == cv.shape[0]
    assert np.array_equal(np.load(b / "face_map.npy"), want[2])
    assert np.array_equal(load_mesh(str(b / "out.ply")).faces, want[1]) and stats["faces_out"] < plain["faces_out"]
