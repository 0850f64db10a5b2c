"""GPU: mesh decimation (``mc_utils.decimate_mesh_device``, ``qf_mesh_vertex_quadrics`` / ``qf_mesh_collapse_*``, DESIGN.md
section 3.9d) against its numpy restatement (tests/mesh_decimate_reference.py).  Every comparison with the restatement is
exact: vertices by bits, faces, both maps, the per-round counts and the stop reason."""
import functools

import numpy as np
import pytest
import torch

from tests import mesh_decimate_reference as ref
from tests import mesh_subdivide_reference as sub
from tests import stream_harness as sh

pytestmark = pytest.mark.gpu

STAT_LISTS = ("faces", "candidates", "legal", "selected", "taken")


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _bits(t):
    return t.cpu().contiguous().view(torch.int64)


def _assert_same(got, want):
    """A device record equals a restatement tuple (or another device record), bit for bit."""
    if not isinstance(want, tuple) or not isinstance(want[0], np.ndarray):
        want = tuple(x.cpu().numpy() if isinstance(x, torch.Tensor) else x for x in want)
    assert got.vertices.dtype == torch.float64 and got.faces.dtype == got.face_map.dtype == got.vertex_target.dtype == torch.int64
    for name in ("rounds", "stop") + STAT_LISTS:
        assert got.stats[name] == want[4][name], (name, got.stats[name], want[4][name])
    assert got.vertices.shape == want[0].shape and torch.equal(_bits(got.vertices), torch.from_numpy(want[0]).view(torch.int64))
    assert torch.equal(got.faces.cpu(), torch.from_numpy(want[1]))
    assert torch.equal(got.face_map.cpu(), torch.from_numpy(want[2]))
    assert torch.equal(got.vertex_target.cpu(), torch.from_numpy(want[3]))


def _assert_matches(v, f, target, faces_dtype=np.int64, **options):
    got = _mc().decimate_mesh_device(_dev(v, np.float64), _dev(f, faces_dtype), target, return_stats=True, **options)
    torch.cuda.synchronize()
    _assert_same(got, ref.decimate(v, f, target, **options))
    return got


@functools.lru_cache(maxsize=None)
def _sphere(level):
    return ref.icosphere(level)


def test_flat_grid_full_run(device):
    v, f = ref.grid(9)
    got = _assert_matches(v, f, 64)
    assert got.faces.shape[0] == 64 and got.stats["stop"] == ref.STOP_TARGET


@pytest.mark.parametrize("level", [2, 3])
def test_icosphere_full_run_to_a_quarter(device, level):
    v, f = _sphere(level)
    got = _assert_matches(v, f, f.shape[0] // 4, max_rounds=64)
    assert got.faces.shape[0] == f.shape[0] // 4 and got.stats["stop"] == ref.STOP_TARGET


def test_icosphere_level_5_one_round(device):
    """20 480 faces, 30 720 edges: several workgroups in every sort and launch."""
    v, f = _sphere(5)
    got = _assert_matches(v, f, f.shape[0] // 4, max_rounds=1)
    assert got.stats["stop"] == ref.STOP_MAX_ROUNDS and got.stats["taken"][0] > 256


def test_budget_binds_in_the_first_round(device):
    v, f = _sphere(3)
    got = _assert_matches(v, f, f.shape[0] - 10, max_rounds=3)
    assert got.stats["taken"] == [5] and got.stats["selected"][0] > 5


def test_marching_cubes_ball_with_repeated_index_faces(device):
    n = 12
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    # r^2 = 18.75 passes exactly through lattice points such as (2.5, 2.5, 2.5) and (0.5, 2.5, 3.5) (the squares of
    # half-integers are exact in fp32): the crossed edges that end there share one vertex, which leaves faces with a
    # repeated index
    vol = 18.75 - (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    verts, faces = _mc().marching_cubes(vol, 0.0)
    v, f = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64)
    repeated = int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
    print(f"marching cubes: {len(v)} vertices, {len(f)} faces, {repeated} with a repeated index")
    assert repeated > 0
    got = _assert_matches(v, f, f.shape[0] // 4, max_rounds=6)
    assert sum(got.stats["taken"]) > 0
    # fp32 vertices are widened exactly by the wrapper
    again = _mc().decimate_mesh_device(verts, faces, f.shape[0] // 4, max_rounds=6, return_stats=True)
    _assert_same(again, got)


@pytest.mark.parametrize("n_edges", [63, 64, 65, 1025])
def test_padded_meshes_around_workgroup_edges(device, n_edges):
    v, f, n_e = ref.padded(n_edges)
    got = _assert_matches(v, f, f.shape[0] // 2, max_rounds=4)
    assert int(got.vertex_target[-1]) == (-1 if sum(got.stats["taken"]) else v.shape[0] - 1)      # the isolated vertex
    lock = np.zeros(v.shape[0], np.uint8)
    lock[::2] = 1
    _assert_matches(v, f, f.shape[0] // 2, max_rounds=2, vertex_lock=lock, max_cost=1e-3)


def test_no_faces(device):
    v = np.zeros((3, 3))
    got = _assert_matches(v, np.zeros((0, 3), np.int64), 0)
    assert got.stats["rounds"] == 0 and got.vertices.shape == (3, 3) and got.faces.shape == (0, 3)
    got = _mc().decimate_mesh_device(torch.zeros((0, 3), device="cuda"), torch.zeros((0, 3), dtype=torch.int64, device="cuda"), 5)
    assert got.vertices.shape == (0, 3) and got.vertex_target.shape == (0,) and got.stats is None


def test_target_at_or_above_the_face_count_returns_the_same_bits(device):
    v, f = _sphere(2)
    for target in (f.shape[0], f.shape[0] + 1):
        got = _assert_matches(v, f, target)
        assert got.stats["rounds"] == 0
        assert torch.equal(_bits(got.vertices), torch.from_numpy(v).view(torch.int64)) and torch.equal(got.faces.cpu(), torch.from_numpy(f))
        assert torch.equal(got.face_map.cpu(), torch.arange(f.shape[0])) and torch.equal(got.vertex_target.cpu(), torch.arange(v.shape[0]))


def test_tetrahedron_fan_and_locks_take_nothing(device):
    v, f = ref.tetrahedron()
    assert _assert_matches(v, f, 2).stats["stop"] == ref.STOP_NO_EDGE
    v, f = ref.fan()
    assert _assert_matches(v, f, 1).stats["candidates"] == [0]
    v, f = _sphere(2)
    got = _assert_matches(v, f, 10, vertex_lock=np.ones(v.shape[0], np.uint8))
    assert torch.equal(_bits(got.vertices), torch.from_numpy(v).view(torch.int64)) and got.stats["stop"] == ref.STOP_NO_EDGE
    assert _assert_matches(v, f, 10, max_cost=0.0).stats["candidates"] == [0]
    _assert_matches(v, f, 80, vertex_lock=(np.arange(v.shape[0]) % 3 == 0), max_rounds=8)


def test_int32_faces_give_the_same_result(device):
    v, f = _sphere(2)
    a = _assert_matches(v, f, 80, faces_dtype=np.int32)
    b = _mc().decimate_mesh_device(_dev(v, np.float64), _dev(f, np.int64), 80, return_stats=True)
    _assert_same(a, b)


def test_two_runs_give_identical_bytes(device):
    v, f = _sphere(3)
    dv, df = _dev(v, np.float64), _dev(f, np.int64)
    a = _mc().decimate_mesh_device(dv, df, 320, return_stats=True)
    b = _mc().decimate_mesh_device(dv, df, 320, return_stats=True)
    _assert_same(a, b)
    assert torch.equal(_bits(dv), torch.from_numpy(v).view(torch.int64)) and torch.equal(df.cpu(), torch.from_numpy(f))   # inputs untouched


def test_host_mesh_wrappers(device):
    from quadraturefields_amd.mesh_io import TriMesh
    mc = _mc()
    v, f = _sphere(2)
    want = ref.decimate(v, f, 32)
    uv = np.stack([np.arange(len(v)), -np.arange(len(v))], axis=1).astype(np.float64)
    mesh, face_map, vertex_target, stats = mc.decimate_mesh(TriMesh(v, f, uv), 32, return_stats=True)
    assert mesh.vertices.tobytes() == want[0].tobytes() and np.array_equal(mesh.faces, want[1])
    assert np.array_equal(face_map, want[2]) and np.array_equal(vertex_target, want[3]) and stats["rounds"] == want[4]["rounds"]
    kept = mesh.visual.uv[:, 0].astype(np.int64)             # the input vertex whose uv an output vertex carries
    assert np.array_equal(vertex_target[kept], np.arange(len(kept))) and np.array_equal(mesh.visual.uv[:, 1], -mesh.visual.uv[:, 0])
    down = mc.down_sample_quadraic(TriMesh(v, f), agg=7)
    assert down.vertices.tobytes() == want[0].tobytes() and np.array_equal(down.faces, want[1])
    doubled = TriMesh(v, np.concatenate([f, f[:5]]))
    cleaned = mc.clean_mesh(doubled, agg=0, remove_duplicate_faces=True)
    assert np.array_equal(cleaned.faces, f) and cleaned.vertices.tobytes() == v.tobytes()
    assert np.array_equal(mc.clean_mesh(doubled, agg=5, remove_duplicate_faces=True).faces, want[1])
    assert mc.clean_mesh(doubled, agg=None).faces.shape[0] == f.shape[0] + 5
    with pytest.raises(NotImplementedError):
        mc.clean_mesh(doubled, agg=1, remove_non_manifold_edges=True)


def test_example_writes_the_mesh_the_maps_and_one_json_line(device, tmp_path, capsys):
    import importlib.util
    import json
    import os
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("decimate_mesh_example", os.path.join(root, "examples", "decimate_mesh.py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    v, f = _sphere(2)
    v = v.astype(np.float32).astype(np.float64)              # what a PLY keeps
    TriMesh(v, f).export(str(tmp_path / "in.ply"))
    example.main([str(tmp_path / "in.ply"), str(tmp_path / "out.ply"), "--ratio", "0.25"])
    want = ref.decimate(v, f, 80)
    stats = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert stats["faces_out"] == 80 and stats["stop"] == ref.STOP_TARGET and stats["taken"] == want[4]["taken"]
    out = load_mesh(str(tmp_path / "out.ply"))
    assert np.array_equal(out.faces, want[1]) and np.array_equal(out.vertices.astype(np.float32), want[0].astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "face_map.npy"), want[2])
    assert np.array_equal(np.load(tmp_path / "vertex_target.npy"), want[3])


def _raw(v, f, device):
    """Device tensors and the arguments of a raw select call on mesh (v, f)."""
    from quadraturefields_amd import _C
    e, fe, _ = sub.edges(f, len(v))
    t = dict(v=_dev(v, np.float64), f=_dev(f, np.int64), e=_dev(e, np.int64), fe=_dev(fe, np.int64),
             q=_dev(ref.vertex_quadrics(v, f), np.float64))
    need = int(_C.lib().qf_mesh_decimate_workspace_bytes(len(v), len(f), len(e)))
    t["ws"] = torch.zeros((need,), dtype=torch.uint8, device=device)
    t["counts"] = torch.full((6,), -7, dtype=torch.int64, device=device)
    return t, len(e), need


def test_refusals_come_before_any_launch(device):
    from quadraturefields_amd import _C
    mc, lib = _mc(), _C.lib()
    v, f = _sphere(1)
    bad_v = v.copy()
    bad_v[3, 1], bad_v[5, 0] = np.nan, np.inf
    with pytest.raises(ValueError, match="2 vertices are not finite"):
        mc.decimate_mesh_device(_dev(bad_v, np.float64), _dev(f, np.int64), 10)
    bad_f = f.copy()
    bad_f[4, 2], bad_f[9, 0] = len(v), -1
    with pytest.raises(ValueError, match="2 faces have an index outside"):
        mc.decimate_mesh_device(_dev(v, np.float64), _dev(bad_f, np.int64), 10)
    with pytest.raises(ValueError):
        mc.decimate_mesh_device(torch.from_numpy(v), torch.from_numpy(f), 10)             # host tensors
    with pytest.raises(ValueError):
        mc.decimate_mesh_device(_dev(v, np.float64), _dev(f, np.int64), -1)
    with pytest.raises(ValueError):
        mc.decimate_mesh_device(_dev(v, np.float64), _dev(f, np.int64), 10, max_cost=-1.0)
    with pytest.raises(ValueError):
        mc.decimate_mesh_device(_dev(v, np.float64), _dev(f, np.int64), 10, vertex_lock=np.zeros(3, np.uint8))

    t, n_e, need = _raw(v, f, device)
    n_v, n_f = len(v), len(f)

    def select(ws_bytes=need, V=n_v, F=n_f, E=n_e, max_cost=float("inf"), rnd=0, take=5, q=t["q"], counts=t["counts"]):
        return lib.qf_mesh_collapse_select(_C.ptr(t["v"]), V, _C.ptr(t["f"]), F, _C.ptr(t["e"]), E, _C.ptr(t["fe"]), _C.ptr(q),
                                           None, max_cost, rnd, take, _C.ptr(t["ws"]), ws_bytes, _C.ptr(counts), _C.stream())

    for status in (select(ws_bytes=need - 1), select(V=0), select(F=-1), select(E=2 ** 31), select(max_cost=-1.0),
                   select(max_cost=float("nan")), select(rnd=-1), select(take=-1), select(q=None), select(counts=None)):
        assert status == -1
    assert lib.qf_mesh_decimate_workspace_bytes(0, 0, 0) == -1 and lib.qf_mesh_decimate_workspace_bytes(5, 2 ** 30, 0) == -1
    q_out = torch.zeros((n_v, 10), dtype=torch.float64, device=device)
    assert lib.qf_mesh_vertex_quadrics(_C.ptr(t["v"]), n_v, _C.ptr(t["f"]), n_f, _C.ptr(q_out), _C.ptr(t["ws"]), 16,
                                       _C.ptr(t["counts"]), _C.stream()) == -1
    vt = torch.arange(n_v, dtype=torch.int64, device=device)
    assert lib.qf_mesh_collapse_apply(_C.ptr(t["v"]), n_v, _C.ptr(t["f"]), n_f, _C.ptr(t["e"]), n_e, _C.ptr(t["q"]), 5,
                                      _C.ptr(vt), n_v, _C.ptr(t["ws"]), need - 1, _C.stream()) == -1
    assert lib.qf_mesh_collapse_gather(_C.ptr(t["q"]), None, _C.ptr(vt), n_v, n_f, _C.ptr(vt), n_v + 1, _C.ptr(vt), 0,
                                       _C.ptr(q_out), None, None, _C.ptr(vt), n_v, _C.ptr(t["ws"]), need, _C.stream()) == -1
    torch.cuda.synchronize()
    assert (t["counts"] == -7).all() and not t["ws"].any() and not q_out.any()          # nothing ran
    assert torch.equal(_bits(t["v"]), torch.from_numpy(v).view(torch.int64)) and torch.equal(t["f"].cpu(), torch.from_numpy(f))
    assert select() == 0
    torch.cuda.synchronize()
    assert t["counts"][0] == n_e and t["counts"][5] == 0


def test_raw_quadrics_equal_the_restatement(device):
    from quadraturefields_amd import _C
    v, f, _ = ref.padded(65)
    t, _, need = _raw(v, f, device)
    q_out = torch.zeros((len(v), 10), dtype=torch.float64, device=device)
    counts = torch.zeros((2,), dtype=torch.int64, device=device)
    _C.check(_C.lib().qf_mesh_vertex_quadrics(_C.ptr(t["v"]), len(v), _C.ptr(t["f"]), len(f), _C.ptr(q_out), _C.ptr(t["ws"]),
                                              need, _C.ptr(counts), _C.stream()), "qf_mesh_vertex_quadrics")
    assert torch.equal(_bits(q_out), _bits(t["q"])) and counts.tolist() == [0, 0]


def test_intersection_of_the_decimated_sphere(device):
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import MeshIntersection
    v, f = _sphere(3)
    mesh = _mc().decimate_mesh(TriMesh(v, f), 320)[0]
    assert mesh.faces.shape[0] == 320
    mi = MeshIntersection(mesh, simplify_mesh=False, scale=1.0, num_intersections=16)
    d = np.random.default_rng(0).normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    out = mi.sampling_raytrace_numpy(d.astype(np.float32), (-1.5 * d).astype(np.float32))
    assert (np.bincount(out[2], minlength=64) == 2).all()


# ---------------------------------------------------------------------------------------------------------------- streams
@functools.lru_cache(maxsize=None)
def _stream_mesh(seed):
    """The level-3 sphere with seeded jitter (the values that vary), its edges (the same in both sets) and quadrics."""
    v, f = _sphere(3)
    v = v + np.random.default_rng(seed).uniform(-0.02, 0.02, v.shape)
    e, fe, _ = sub.edges(f, len(v))
    return v, f, e, fe, ref.vertex_quadrics(v, f)


def _stream_build(seed, device):
    from quadraturefields_amd import _C
    v, f, e, fe, q = _stream_mesh(seed)
    n = int(_C.lib().qf_mesh_decimate_workspace_bytes(len(v), len(f), len(e)))
    return dict(vertices=torch.from_numpy(v).to(device), faces=torch.from_numpy(f).to(device), edges=torch.from_numpy(e).to(device),
                face_edges=torch.from_numpy(fe).to(device), quadrics=torch.from_numpy(q).to(device),
                vertex_target=torch.arange(len(v), dtype=torch.int64, device=device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_q=torch.zeros((len(v), 10), dtype=torch.float64, device=device),
                out_qcounts=torch.zeros((2,), dtype=torch.int64, device=device),
                out_counts=torch.zeros((6,), dtype=torch.int64, device=device))


def _quadrics_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_vertex_quadrics(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                              _C.ptr(i["out_q"]), _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.ptr(i["out_qcounts"]),
                                              _C.stream()), "qf_mesh_vertex_quadrics")
    return i["out_q"], i["out_qcounts"]


def _select_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_collapse_select(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                              _C.ptr(i["edges"]), i["edges"].shape[0], _C.ptr(i["face_edges"]), _C.ptr(i["quadrics"]),
                                              None, float("inf"), 0, 1000, _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0],
                                              _C.ptr(i["out_counts"]), _C.stream()), "qf_mesh_collapse_select")
    return (i["out_counts"],)


def _apply_call(i):
    """Select, then apply with no host wait in between; vertices, faces, quadrics and the targets change in place (the
    harness reloads them before every call)."""
    from quadraturefields_amd import _C
    _select_call(i)
    _C.check(_C.lib().qf_mesh_collapse_apply(_C.ptr(i["vertices"]), i["vertices"].shape[0], _C.ptr(i["faces"]), i["faces"].shape[0],
                                             _C.ptr(i["edges"]), i["edges"].shape[0], _C.ptr(i["quadrics"]), 1000,
                                             _C.ptr(i["vertex_target"]), i["vertex_target"].shape[0], _C.ptr(i["tmp_ws"]),
                                             i["tmp_ws"].shape[0], _C.stream()), "qf_mesh_collapse_apply")
    return i["vertices"], i["faces"], i["quadrics"], i["vertex_target"], i["out_counts"]


def _gather_build(seed, device):
    """Maps that drop every fourth vertex and every third face (the same in both sets); the quadrics vary."""
    from quadraturefields_amd import _C
    v, f, _, _, q = _stream_mesh(seed)
    n_v, n_f = len(v), len(f)
    vertex_map = torch.arange(n_v, dtype=torch.int64)[torch.arange(n_v) % 4 != 0]
    face_map = torch.arange(n_f, dtype=torch.int64)[torch.arange(n_f) % 3 != 0]
    n = int(_C.lib().qf_mesh_decimate_workspace_bytes(n_v, n_f, 0))
    return dict(quadrics=torch.from_numpy(q).to(device), lock=(torch.arange(n_v) % 5 == 0).to(torch.uint8).to(device),
                face_map=(torch.arange(n_f, dtype=torch.int64) * 2).to(device), vertex_map=vertex_map.to(device),
                compact_face_map=face_map.to(device), vertex_target=torch.arange(n_v, dtype=torch.int64, device=device),
                tmp_ws=torch.zeros((n,), dtype=torch.uint8, device=device),
                out_q=torch.zeros((len(vertex_map), 10), dtype=torch.float64, device=device),
                out_lock=torch.zeros((len(vertex_map),), dtype=torch.uint8, device=device),
                out_fm=torch.zeros((len(face_map),), dtype=torch.int64, device=device))


def _gather_call(i):
    from quadraturefields_amd import _C
    _C.check(_C.lib().qf_mesh_collapse_gather(_C.ptr(i["quadrics"]), _C.ptr(i["lock"]), _C.ptr(i["face_map"]), i["quadrics"].shape[0],
                                              i["face_map"].shape[0], _C.ptr(i["vertex_map"]), i["vertex_map"].shape[0],
                                              _C.ptr(i["compact_face_map"]), i["compact_face_map"].shape[0], _C.ptr(i["out_q"]),
                                              _C.ptr(i["out_lock"]), _C.ptr(i["out_fm"]), _C.ptr(i["vertex_target"]),
                                              i["vertex_target"].shape[0], _C.ptr(i["tmp_ws"]), i["tmp_ws"].shape[0], _C.stream()),
             "qf_mesh_collapse_gather")
    return i["out_q"], i["out_lock"], i["out_fm"], i["vertex_target"]


STREAM_CASES = [
    sh.Case("mesh_vertex_quadrics", _stream_build, _quadrics_call, entry_points=("qf_mesh_vertex_quadrics",)),
    sh.Case("mesh_collapse_select", _stream_build, _select_call, entry_points=("qf_mesh_collapse_select",)),
    sh.Case("mesh_collapse_apply", _stream_build, _apply_call, entry_points=("qf_mesh_collapse_apply",)),
    sh.Case("mesh_collapse_gather", _gather_build, _gather_call, entry_points=("qf_mesh_collapse_gather",)),
]


def test_every_device_entry_point_has_a_stream_case():
    from quadraturefields_amd import _C
    covered = sorted(ep for c in STREAM_CASES for ep in c.entry_points)
    assert covered == sorted(set(_C._MESH_DECIMATE_SIGNATURES) - {"qf_mesh_decimate_workspace_bytes"})
    assert not any(c.host_wait for c in STREAM_CASES)


def test_gather_equals_indexing(device):
    i = _gather_build(1, device)
    q, lock, fm, vt = (x.clone() for x in (i["quadrics"], i["lock"], i["face_map"], i["vertex_target"]))
    out_q, out_lock, out_fm, out_vt = _gather_call(i)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out_q), _bits(q[i["vertex_map"]])) and torch.equal(out_lock, lock[i["vertex_map"]])
    assert torch.equal(out_fm, fm[i["compact_face_map"]])
    inverse = torch.full((len(q),), -1, dtype=torch.int64, device=device)
    inverse[i["vertex_map"]] = torch.arange(len(i["vertex_map"]), device=device)
    assert torch.equal(out_vt, inverse[vt])


@pytest.mark.parametrize("name", [c.name for c in STREAM_CASES])
def test_entry_point_runs_entirely_on_the_callers_stream(device, lib, name):
    case = {c.name: c for c in STREAM_CASES}[name]
    issue_ms, delay_ms = sh.run_case(case, device)
    print(f"{name}: issue {issue_ms:.3f} ms, delay {delay_ms:.0f} ms")
