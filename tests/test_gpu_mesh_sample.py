"""GPU: surface sampling (``mc_utils.sample_surface_device`` / ``qf_mesh_sample_*``) against its
numpy restatement (tests/mesh_sample_reference.py), bit for bit: points and barycentrics as 64-bit words, faces and all
six counts; and ``mesh_distance_device(..., samples=N)`` on pairs whose surface integral is known in closed form."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_sample_reference as ref
from tests.test_mesh_sample_host import ONE_THREE, UNIT, check_properties

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A


def _mc():
    from quadraturefields_amd import mc_utils
    return mc_utils


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _assert_matches(v, f, n, seed=0, w=None, faces_dtype=np.int64, vertices_dtype=np.float64, want=None):
    """The wrapper's output equals the restatement's, bit for bit, and has the properties the rule promises."""
    got, stats = _mc().sample_surface_device(_dev(v, vertices_dtype), _dev(f, faces_dtype), n, seed,
                                             face_weight=None if w is None else _dev(w, np.float64), return_stats=True)
    torch.cuda.synchronize()
    assert got.points.dtype == got.bary.dtype == torch.float64 and got.face.dtype == torch.int64
    points, face, bary, counts = ref.sample(v, f, n, seed, w) if want is None else want
    assert list(stats) == list(ref.COUNT_NAMES) and list(stats.values()) == counts.tolist(), (stats, counts)
    gp, gf, gb = got.points.cpu().numpy(), got.face.cpu().numpy(), got.bary.cpu().numpy()
    assert gf.shape == face.shape and np.array_equal(gf, face)
    assert gb.shape == bary.shape and np.array_equal(_bits(gb), _bits(bary))
    assert gp.shape == points.shape and np.array_equal(_bits(gp), _bits(points))
    check_properties(v, f, w, n, gp, gf, gb)
    return got, stats


# --------------------------------------------------------------------------------------------------------- 1. the rule
def test_hand_worked_cases(device):
    got, _ = _assert_matches(*UNIT, 1)
    r1, r2 = (0x6E789E6AA1B965F4 >> 11) * 2.0 ** -53, (0x06C45D188009454F >> 11) * 2.0 ** -53
    assert got.points.tolist() == [[r1, r2, 0.0]] and got.bary.tolist() == [[(1.0 - r1) - r2, r1, r2]]
    got, stats = _assert_matches(*ONE_THREE, 4)
    assert got.face.tolist() == [0, 3, 3, 3] and stats["unsampled_faces"] == 2
    _assert_matches(*ONE_THREE, 1000, seed=1000)


@functools.lru_cache(maxsize=None)
def _soup(n_faces):
    return ref.soup(n_faces, n_faces)


@pytest.mark.parametrize("n_faces", [1, 2, 7, 255, 256, 257, 1025, 65_537])
def test_face_counts_around_a_workgroup_and_a_scan_block(device, n_faces):
    v, f = _soup(n_faces)
    for n in (1, 257, 4097):
        _assert_matches(v, f, n, seed=n_faces)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097, 65_537])
def test_sample_counts_around_a_wave_and_a_workgroup(device, n):
    v, f = _soup(1025)
    got, _ = _assert_matches(v, f, n, seed=7)
    assert got.points.shape == (n, 3) and got.face.shape == (n,) and got.bary.shape == (n, 3)


@functools.lru_cache(maxsize=None)
def _icosphere3():
    return ref.icosphere(3)


@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1])
def test_icosphere_and_both_ends_of_the_seed_range(device, seed):
    v, f = _icosphere3()
    got, stats = _assert_matches(v, f, 20_000, seed=seed)
    assert stats["unsampled_faces"] == 0 and np.unique(got.face.cpu().numpy()).shape[0] == f.shape[0] == 1280
    # the points lie on the faces of a polyhedron inscribed in the unit sphere
    r = got.points.norm(dim=1)
    assert float(r.max()) <= 1.0 + 1e-15 and float(r.min()) > 0.98


def test_different_seeds_differ_and_two_runs_do_not(device):
    v, f = _icosphere3()
    dv, df = _dev(v, np.float64), _dev(f, np.int64)
    a = _mc().sample_surface_device(dv, df, 5000, 3)
    b = _mc().sample_surface_device(dv, df, 5000, 3)
    c = _mc().sample_surface_device(dv, df, 5000, 4)
    for x, y in zip(a, b):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    assert not torch.equal(a.points, c.points) and not torch.equal(a.bary, c.bary)


def test_marching_cubes_ball_with_repeated_index_faces_and_int32_faces(device):
    n = 12
    ax = torch.arange(n, device="cuda", dtype=torch.float32) - (n - 1) / 2
    # r^2 = 18.75 passes exactly through lattice points (tests/test_gpu_mesh_decimate.py): faces with a repeated index
    vol = 18.75 - (ax[:, None, None] ** 2 + ax[None, :, None] ** 2 + ax[None, None, :] ** 2)
    verts, faces = _mc().marching_cubes(vol, 0.0)
    assert verts.dtype == torch.float32 and faces.dtype == torch.int32
    v, f = verts.cpu().numpy().astype(np.float64), faces.cpu().numpy().astype(np.int64)
    repeated = int(((f[:, 0] == f[:, 1]) | (f[:, 1] == f[:, 2]) | (f[:, 0] == f[:, 2])).sum())
    assert repeated > 0
    want = ref.sample(v, f, 3000, 5)
    assert want[3][4] >= repeated
    _assert_matches(v, f, 3000, seed=5, want=want)
    # fp32 vertices are widened exactly and int32 faces taken as they are
    _assert_matches(v, f, 3000, seed=5, want=want, faces_dtype=np.int32, vertices_dtype=np.float32)


def test_soup_with_a_third_of_the_faces_without_area(device):
    v, f = ref.soup(3000, 3, zero_every=3)
    got, stats = _assert_matches(v, f, 10_000, seed=1)
    assert stats["unsampled_faces"] == 1000 and (got.face % 3 != 0).all()


def test_weights(device):
    v, f = _icosphere3()
    w = np.random.default_rng(8).uniform(0.0, 1.0, size=f.shape[0]) ** 4
    w[::7] = 0.0
    got, stats = _assert_matches(v, f, 9000, seed=2, w=w)
    face = got.face.cpu().numpy()
    assert (w[face] > 0).all() and stats["unsampled_faces"] >= (w == 0).sum()
    again, _ = _assert_matches(v, f, 9000, seed=2, w=4.0 * w)
    for x, y in zip(got, again):
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    plain, _ = _assert_matches(v, f, 9000, seed=2)
    ones, _ = _assert_matches(v, f, 9000, seed=2, w=np.ones(f.shape[0]))
    assert torch.equal(plain.points.view(torch.int64), ones.points.view(torch.int64))
    assert not torch.equal(plain.face, got.face)
    # fp32 weights are widened exactly
    w32 = w.astype(np.float32)
    half = _mc().sample_surface_device(_dev(v, np.float64), _dev(f, np.int64), 500, 2, face_weight=_dev(w32, np.float32))
    want = ref.sample(v, f, 500, 2, w32.astype(np.float64))
    assert np.array_equal(_bits(half.points.cpu().numpy()), _bits(want[0]))


def test_uniform_inside_a_face_on_the_device(device):
    n = 32_768
    got, _ = _assert_matches(*UNIT, n)
    bary = got.bary.cpu().numpy()
    corner = [int((bary[:, k] > 0.5).sum()) for k in range(3)]
    assert corner + [n - sum(corner)] == [8142, 8228, 8268, 8130]          # within 6 sigma = 470 of N / 4


# ------------------------------------------------------------------------------------------------------ 2. the raw calls
class Raw:
    """The two calls on buffers of the test's own: outputs are sentinel-filled, so what emit leaves alone shows."""

    def __init__(self, v, f, w=None):
        from quadraturefields_amd import _C
        self.C, self.lib = _C, _C.lib()
        self.v, self.f = _dev(v, np.float64), _dev(f, np.int64)
        self.w = None if w is None else _dev(w, np.float64)
        self.n_v, self.n_f = self.v.shape[0], self.f.shape[0]
        self.bytes = int(self.lib.qf_mesh_sample_workspace_bytes(self.n_v, self.n_f))
        assert self.bytes > 0
        self.ws = torch.zeros((self.bytes,), dtype=torch.uint8, device="cuda")
        self.counts = torch.full((6,), -1, dtype=torch.int64, device="cuda")

    def prepare(self, **kw):
        a = dict(v=self.C.ptr(self.v), n_v=self.n_v, f=self.C.ptr(self.f), n_f=self.n_f,
                 w=None if self.w is None else self.C.ptr(self.w), ws=self.C.ptr(self.ws), bytes=self.bytes,
                 counts=self.C.ptr(self.counts))
        a.update(kw)
        return self.lib.qf_mesh_sample_prepare(a["v"], a["n_v"], a["f"], a["n_f"], a["w"], a["ws"], a["bytes"], a["counts"],
                                               self.C.stream())

    def emit(self, n, seed, rows=None, **kw):
        rows = max(n, 1) if rows is None else rows
        self.points = torch.zeros((rows, 3), dtype=torch.float64, device="cuda")
        self.face = torch.zeros((rows,), dtype=torch.int64, device="cuda")
        self.bary = torch.zeros((rows, 3), dtype=torch.float64, device="cuda")
        for t in (self.points, self.face, self.bary):
            t.view(torch.uint8).fill_(SENTINEL)
        a = dict(v=self.C.ptr(self.v), n_v=self.n_v, f=self.C.ptr(self.f), n_f=self.n_f, ws=self.C.ptr(self.ws),
                 bytes=self.bytes, n=n, points=self.C.ptr(self.points), face=self.C.ptr(self.face), bary=self.C.ptr(self.bary))
        a.update(kw)
        return self.lib.qf_mesh_sample_emit(a["v"], a["n_v"], a["f"], a["n_f"], a["ws"], a["bytes"], a["n"], seed, a["points"],
                                            a["face"], a["bary"], self.C.stream())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((t.view(torch.uint8) == SENTINEL).all()) for t in (self.points, self.face, self.bary))

    def out(self, n):
        torch.cuda.synchronize()
        return self.points[:n].cpu().numpy(), self.face[:n].cpu().numpy(), self.bary[:n].cpu().numpy()


def test_two_emits_after_one_prepare(device):
    v, f = _soup(1025)
    raw = Raw(v, f)
    assert raw.prepare() == 0
    for n, seed in ((777, 1), (4097, 2 ** 64 - 1), (777, 1)):
        assert raw.emit(n, seed) == 0
        want = ref.sample(v, f, n, seed)
        for got, w in zip(raw.out(n), want[:3]):
            assert np.array_equal(_bits(got) if got.dtype == np.float64 else got, _bits(w) if w.dtype == np.float64 else w)
    assert raw.counts.tolist() == want[3].tolist()


def test_emit_writes_exactly_n_rows(device):
    v, f = _soup(7)
    raw = Raw(v, f)
    assert raw.prepare() == 0
    for n in (1, 255, 256, 257):
        assert raw.emit(n, 3, rows=n + 1) == 0               # buffers of n + 1 rows, of which n are asked for
        torch.cuda.synchronize()
        want = ref.sample(v, f, n, 3)
        assert np.array_equal(_bits(raw.points[:n].cpu().numpy()), _bits(want[0]))
        assert np.array_equal(_bits(raw.bary[:n].cpu().numpy()), _bits(want[2]))
        for t in (raw.points, raw.face, raw.bary):
            assert bool((t[n:].contiguous().view(torch.uint8) == SENTINEL).all())


REFUSED = {
    # name -> (vertices, faces, weights, counts)
    "nan_vertex": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.nan, 0, 0]], dtype=np.float64), [[0, 1, 2], [0, 1, 3]], None,
                   [1, 0, 0, 1, 0, 0]),
    "loose_infinite_vertex": (np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [np.inf, 0, 0]], dtype=np.float64), [[0, 1, 2]], None,
                              [1, 0, 0, 0, 0, 0]),
    "face_out_of_range": (UNIT[0], [[0, 1, 2], [0, 1, 3], [-1, 1, 2]], None, [0, 2, 0, 0, 0, 0]),
    "negative_weight": (ONE_THREE[0], ONE_THREE[1], [1.0, 1.0, 1.0, -0.5], [0, 0, 1, 0, 0, 0]),
    "nan_and_infinite_weights": (ONE_THREE[0], ONE_THREE[1], [np.nan, np.inf, 1.0, np.inf], [0, 0, 3, 2, 0, 0]),
    "overflowing_measure": (ONE_THREE[0] * 1e200, ONE_THREE[1], None, [0, 0, 0, 2, 0, 0]),
    "all_degenerate": (ONE_THREE[0], [[0, 1, 0], [0, 5, 1], [2, 2, 2]], None, [0, 0, 0, 0, 0, 1]),
    "all_weights_zero": (ONE_THREE[0], ONE_THREE[1], [0.0, 0.0, 0.0, 0.0], [0, 0, 0, 0, 0, 1]),
}


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_refused_mesh_counts_and_emit_writes_nothing(device, name):
    v, f, w, counts = REFUSED[name]
    f = np.asarray(f, dtype=np.int64)
    assert ref.sample(v, f, 300, 0, w)[3].tolist() == counts and ref.sample(v, f, 300, 0, w)[0] is None
    raw = Raw(v, f, w)
    assert raw.prepare() == 0 and raw.emit(300, 0) == 0
    assert raw.untouched() and raw.counts.tolist() == counts
    with pytest.raises(ValueError, match=r"nonfinite_vertices=%d, invalid_faces=%d, bad_weights=%d" % tuple(counts[:3])):
        _mc().sample_surface_device(_dev(v, np.float64), _dev(f, np.int64), 300, face_weight=None if w is None else _dev(w, np.float64))
    if w is not None:
        # the same workspace prepared again without the weights serves emit: the flag is prepare's, not the workspace's
        raw.w = None
        assert raw.prepare() == 0 and raw.emit(4, 0) == 0
        assert raw.out(4)[1].tolist() == [0, 3, 3, 3]


def test_argument_refusals_on_the_device(device):
    raw = Raw(*ONE_THREE)
    invalid = -1
    assert raw.prepare(bytes=raw.bytes - 1) == invalid and raw.prepare(v=None) == invalid and raw.prepare(f=None) == invalid
    assert raw.prepare(ws=None) == invalid and raw.prepare(counts=None) == invalid
    assert raw.prepare(n_v=0) == invalid and raw.prepare(n_f=0) == invalid and raw.prepare(n_v=2 ** 31) == invalid
    assert raw.prepare(n_f=(2 ** 31 + 2) // 3) == invalid
    torch.cuda.synchronize()
    assert raw.counts.tolist() == [-1] * 6                   # refused before the first launch
    assert raw.prepare() == 0
    assert raw.emit(4, 0, bytes=raw.bytes - 1) == invalid and raw.emit(-1, 0) == invalid and raw.emit(2 ** 31, 0) == invalid
    assert raw.emit(4, 0, points=None) == invalid and raw.emit(4, 0, face=None) == invalid and raw.emit(4, 0, bary=None) == invalid
    assert raw.emit(4, 0, ws=None) == invalid and raw.emit(4, 0, v=None) == invalid and raw.emit(4, 0, f=None) == invalid
    assert raw.untouched()
    assert raw.emit(0, 0, points=None, face=None, bary=None) == 0 and raw.untouched()
    mc, tv, tf = _mc(), _dev(UNIT[0], np.float64), _dev(UNIT[1], np.int64)
    with pytest.raises(ValueError):
        mc.sample_surface_device(tv, tf, 4, face_weight=torch.ones(2, device="cuda"))
    with pytest.raises(ValueError):
        mc.sample_surface_device(tv, tf[:0], 4)
    with pytest.raises(ValueError, match="vertices on"):
        mc.sample_surface_device(tv, tf, 4, face_weight=torch.ones(1))


def test_trimesh_wrapper(device):
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = _icosphere3()
    w = np.linspace(0.0, 1.0, f.shape[0])
    out, stats = _mc().sample_surface(TriMesh(v, f), 1234, seed=6, face_weight=w, return_stats=True)
    want = ref.sample(v, f, 1234, 6, w)
    assert isinstance(out.points, np.ndarray) and list(stats.values()) == want[3].tolist()
    assert np.array_equal(_bits(out.points), _bits(want[0])) and np.array_equal(out.face, want[1])
    assert np.array_equal(_bits(out.bary), _bits(want[2]))
    plain = _mc().sample_surface(TriMesh(v, f), 10)
    assert plain.points.shape == (10, 3)


# ---------------------------------------------------------------------------------------------------- 3. mesh distance
def test_two_tessellation_square_against_a_slanted_plane(device):
    """Half of the unit square is a 32 x 64 grid, the other half two triangles; the plane z = x / 2 is d(x) = (x / 2) /
    sqrt(1.25) away, whose mean over the square is 0.25 / sqrt(1.25).  The vertex-and-centroid mean sees almost only the
    fine half, where d is small: more than 0.4 relative off.  4096 area-weighted samples: the coarse half holds 2048 plain
    Monte Carlo samples of d in [0.5, 1] / sqrt(5) (sigma 0.0645), the fine half is stratified; six standard errors of the
    mean are 1.9e-2 relative."""
    va, fa = ref.two_tessellation_square()
    vb, fb = ref.slanted_plane()
    args = [_dev(va, np.float64), _dev(fa, np.int64), _dev(vb, np.float64), _dev(fb, np.int64)]
    exact = 0.25 / np.sqrt(1.25)
    default = _mc().mesh_distance_device(*args)
    sampled = _mc().mesh_distance_device(*args, samples=4096, seed=0)
    print(f"exact {exact:.6f}, default {default.a_to_b_mean:.6f}, samples=4096 {sampled.a_to_b_mean:.6f} "
          f"({abs(sampled.a_to_b_mean / exact - 1.0):.2e} relative)")
    assert abs(default.a_to_b_mean / exact - 1.0) > 0.4
    assert abs(sampled.a_to_b_mean / exact - 1.0) <= 1.9e-2
    # the rms likewise: the mean of d^2 = x^2 / 5 is 1 / 15.  On the coarse half x^2 / 5 has sigma 0.0434; 2048 samples on
    # half the area give 0.00048 on the mean, 0.72 % of 1 / 15 and half that of its root: six of them are 2.2e-2
    assert abs(sampled.a_to_b_rms / np.sqrt(1.0 / 15.0) - 1.0) <= 2.2e-2
    assert sampled.a_to_b_max <= 0.5 / np.sqrt(1.25) * (1 + 1e-6) and sampled.symmetric_max >= sampled.a_to_b_max
    # samples=None is the call without the argument, bit for bit
    assert _mc().mesh_distance_device(*args, samples=None) == default
    assert _mc().mesh_distance_device(*args, samples=None, seed=5) == default
    assert _mc().mesh_distance_device(*args, samples=4096, seed=0) == sampled
    with pytest.raises(ValueError, match="samples"):
        _mc().mesh_distance_device(*args, samples=0)


def test_square_against_its_shifted_copy_is_a_quarter_everywhere(device):
    from quadraturefields_amd.mesh_io import TriMesh
    va, fa = ref.two_tessellation_square()
    vb = va + np.array([0.0, 0.0, 0.25])
    d = _mc().mesh_distance(TriMesh(va, fa), TriMesh(vb, fa), samples=5000, seed=3)
    assert d == (0.25,) * 7
    assert _mc().mesh_distance(TriMesh(va, fa), TriMesh(vb, fa)) == _mc().mesh_distance(TriMesh(va, fa), TriMesh(vb, fa), samples=None)


# ------------------------------------------------------------------------------------------------------- 4. the examples
def _example(name):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(root, "examples", name + ".py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_sample_surface_example(device, tmp_path, capsys):
    from quadraturefields_amd.mesh_io import TriMesh, load_mesh
    v, f = ref.icosphere(2)
    TriMesh(v.astype(np.float32).astype(np.float64), f).export(str(tmp_path / "in.ply"))
    loaded = load_mesh(str(tmp_path / "in.ply"))
    lv, lf = np.asarray(loaded.vertices, np.float64), np.asarray(loaded.faces, np.int64)
    w = np.arange(lf.shape[0], dtype=np.float64) % 3
    np.save(tmp_path / "w.npy", w)
    _example("sample_surface").main([str(tmp_path / "in.ply"), str(tmp_path / "out.npz"), "--n", "999", "--seed", "4"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    stats, want, got = json.loads(out[0]), ref.sample(lv, lf, 999, 4), np.load(tmp_path / "out.npz")
    assert [stats[k] for k in ref.COUNT_NAMES] == want[3].tolist() and stats["samples"] == 999 and not stats["weighted"]
    assert np.array_equal(_bits(got["points"]), _bits(want[0])) and np.array_equal(got["face"], want[1])
    assert np.array_equal(_bits(got["bary"]), _bits(want[2]))
    _example("sample_surface").main([str(tmp_path / "in.ply"), str(tmp_path / "weighted.npz"), "--n", "999", "--seed", "4",
                                     "--face_weights", str(tmp_path / "w.npy")])
    stats, want = json.loads(capsys.readouterr().out.strip().splitlines()[-1]), ref.sample(lv, lf, 999, 4, w)
    assert stats["weighted"] and stats["unsampled_faces"] == want[3][4] >= 106
    assert np.array_equal(np.load(tmp_path / "weighted.npz")["face"], want[1])


def test_decimate_example_with_and_without_distance_samples(device, tmp_path, capsys):
    from quadraturefields_amd.mesh_io import TriMesh
    v, f = _icosphere3()
    a, b = tmp_path / "plain", tmp_path / "sampled"
    a.mkdir()
    b.mkdir()
    TriMesh(v, f).export(str(tmp_path / "in.ply"))
    example = _example("decimate_mesh")
    example.main([str(tmp_path / "in.ply"), str(a / "out.ply"), "--target_faces", "400"])
    plain = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert not any(k.startswith("distance_") for k in plain)
    example.main([str(tmp_path / "in.ply"), str(b / "out.ply"), "--target_faces", "400", "--distance_samples", "4096"])
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    sampled = json.loads(out[0])
    new = sorted(set(sampled) - set(plain))
    assert new == sorted(["distance_samples"] + [f"distance_sampled_{d}_{s}" for d in ("out_to_in", "in_to_out")
                                                 for s in ("mean", "rms", "max")])
    assert {k: sampled[k] for k in plain} == plain and sorted(os.listdir(a)) == sorted(os.listdir(b))
    assert sampled["distance_samples"] == 4096
    for d in ("out_to_in", "in_to_out"):
        mean, rms, top = (sampled[f"distance_sampled_{d}_{s}"] for s in ("mean", "rms", "max"))
        # 400 equilateral faces on a unit sphere would have edges of 0.27 and sit 0.012 inside it: 0.1 is eight times that
        assert 0.0 < mean <= rms <= top < 0.1
