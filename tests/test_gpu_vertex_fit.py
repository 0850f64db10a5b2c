"""GPU: the surface fit of the vertex table (``baking.fit_vertex_table_device`` / ``qf_vertex_fit_*``, DESIGN.md section
3.9i) against its numpy restatement (tests/vertex_fit_reference.py), bit for bit: gram, mass and right-hand side as 64-bit
words, the table as 32-bit words, stats and all counts, two runs each; then the wrappers on the synthetic SG scene and
the two examples with and without their new flag."""
import functools
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

from tests import mesh_sample_reference as sampler
from tests import vertex_fit_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A
LAMBDA = 1.0 / 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype))).cuda()


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def _padded(a, pad):
    """The rows of float32 ``a`` inside a sentinel-filled buffer ``pad`` floats wider."""
    buf = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), dtype=torch.float32).cuda()
    buf.view(torch.uint8).fill_(SENTINEL)
    buf[:, :a.shape[1]] = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    return buf


def device_fit(faces, n_v, face, bary, y, x0, lam, steps, mask, pads=(0, 0, 0)):
    """Both entry points through the raw binding: (gram, mass, rhs, out buffer, stats, counts after assemble, counts)."""
    from quadraturefields_amd import _C
    lib = _C.lib()
    n_f, n, n_c = faces.shape[0], face.shape[0], x0.shape[1]
    f, sf, sb = _dev(faces.reshape(-1, 3), np.int64), _dev(face, np.int64), _dev(bary.reshape(-1, 3), np.float64)
    ty, tx = _padded(y.reshape(n, n_c), pads[0]), _padded(x0, pads[1])
    out = torch.empty((n_v, n_c + pads[2]), dtype=torch.float32).cuda()
    out.view(torch.uint8).fill_(SENTINEL)
    ws_bytes = int(lib.qf_vertex_fit_workspace_bytes(n_v, n_f, n, n_c))
    assert ws_bytes > 0
    ws = torch.empty((ws_bytes,), dtype=torch.uint8).cuda()
    ws.fill_(SENTINEL)
    gram = torch.full((n_f, 9), np.nan, dtype=torch.float64).cuda()
    mass = torch.full((n_v,), np.nan, dtype=torch.float64).cuda()
    rhs = torch.full((n_v, n_c), np.nan, dtype=torch.float64).cuda()
    stats = torch.full((n_c, 2), np.nan, dtype=torch.float64).cuda()
    counts = torch.full((8,), -1, dtype=torch.int64).cuda()
    p = _C.ptr
    _C.check(lib.qf_vertex_fit_assemble(p(f) if n_f else None, n_f, n_v, p(sf) if n else None, p(sb) if n else None, n,
                                        p(ty) if n else None, ty.shape[1], p(tx), tx.shape[1], n_c, lam,
                                        p(gram) if n_f else None, p(mass), p(rhs), p(ws), ws_bytes, p(counts), _C.stream()),
             "qf_vertex_fit_assemble")
    first = counts.cpu().numpy().copy()
    _C.check(lib.qf_vertex_fit_solve(p(f) if n_f else None, n_f, n_v, p(tx), tx.shape[1], n_c, p(gram) if n_f else None,
                                     p(mass), p(rhs), steps, mask, p(ws), ws_bytes, p(out), out.shape[1], p(stats), p(counts),
                                     _C.stream()), "qf_vertex_fit_solve")
    torch.cuda.synchronize()
    return (gram.cpu().numpy(), mass.cpu().numpy(), rhs.cpu().numpy(), out.cpu().numpy(), stats.cpu().numpy(), first,
            counts.cpu().numpy())


def assert_matches(faces, n_v, face, bary, y, x0, lam=LAMBDA, steps=32, mask=None, pads=(0, 0, 0)):
    """The device equals the restatement bit for bit, twice; returns the restatement's (table, stats, counts, assembled)."""
    n_c = x0.shape[1]
    mask = (1 << (n_c - 1)) if mask is None else mask
    faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    y = np.asarray(y, dtype=np.float32).reshape(-1, n_c)
    want = ref.fit(faces, n_v, face, bary, y, x0, lam, steps, mask)
    table, stats, counts, a = want
    for run in range(2):
        gram, mass, rhs, out, got_stats, first, got_counts = device_fit(faces, n_v, face, bary, y, x0, lam, steps, mask, pads)
        assert got_counts.tolist() == counts.tolist(), (run, got_counts, counts)
        assert first[:6].tolist() == counts[:6].tolist() and first[6] == 0 and first[7] == counts[7]
        assert np.array_equal(_bits(gram), _bits(a.gram)), run
        assert np.array_equal(_bits(mass), _bits(a.mass)), run
        assert np.array_equal(_bits(rhs), _bits(a.rhs)), run
        assert np.array_equal(_bits(got_stats), _bits(stats)), (run, got_stats, stats)
        sentinel = np.full(out.shape, SENTINEL * 0x01010101, dtype=np.uint32)
        if table is not None:
            sentinel[:, :n_c] = _bits(table)
        assert np.array_equal(_bits(out), sentinel), run
    return want


def _values(n, n_v, n_c, seed):
    """Targets and a prior: normal entries, the last column positive (a density)."""
    rng = np.random.default_rng(seed)
    y, x0 = rng.normal(size=(n, n_c)).astype(np.float32), rng.normal(size=(n_v, n_c)).astype(np.float32)
    y[:, -1], x0[:, -1] = np.exp(2 * y[:, -1]), np.exp(2 * x0[:, -1])
    return y, x0


@functools.lru_cache(maxsize=None)
def _sphere(level, n, seed=0):
    v, f = sampler.icosphere(level)
    _, face, bary, _ = sampler.sample(v, f, n, seed=seed)
    return v, f, face, bary


def _strip(n_v):
    """A zig-zag strip of n_v vertices and n_v - 2 faces."""
    i = np.arange(n_v)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.1 * np.sin(i)], axis=1)
    return v, np.stack([i[:-2], i[1:-1], i[2:]], axis=1)


# --------------------------------------------------------------------------------------------------------- 1. the rule
def test_one_triangle_by_hand(device):
    faces, face = np.array([[0, 1, 2]]), np.array([0, 0, 0])
    bary = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.5, 0.5, 0.0]])
    y, x0 = np.array([[1.0], [2.0], [4.0]], dtype=np.float32), np.array([[0.0], [0.0], [7.0]], dtype=np.float32)
    table, stats, counts, a = assert_matches(faces, 3, face, bary, y, x0, lam=0.5, steps=2, mask=0)
    assert table[:, 0].tolist() == [np.float32(80.0 / 63.0), np.float32(116.0 / 63.0), 7.0] and stats[0, 0] == 5.0


@pytest.mark.parametrize("level", [2, 3])
def test_icospheres(device, level):
    v, f, face, bary = _sphere(level, 8 * sampler.icosphere(level)[1].shape[0])
    y, x0 = _values(face.shape[0], v.shape[0], 4, level)
    table, stats, counts, _ = assert_matches(f, v.shape[0], face, bary, y, x0, pads=(3, 12, 12))
    assert counts[3:6].tolist() == [0, 0, 0] and (stats[:, 1] < 1e-11 * stats[:, 0]).all()


def test_fan_with_a_300_face_hub(device):
    n = 300
    ang = 2 * np.pi * np.arange(n) / n
    v = np.concatenate([[[0.0, 0.0, 0.2]], np.stack([np.cos(ang), np.sin(ang), 0 * ang], axis=1)])
    f = np.stack([np.zeros(n, dtype=np.int64), 1 + np.arange(n), 1 + (np.arange(n) + 1) % n], axis=1)
    _, face, bary, _ = sampler.sample(v, f, 4 * n, seed=3)
    y, x0 = _values(face.shape[0], n + 1, 4, 5)
    _, _, _, a = assert_matches(f, n + 1, face, bary, y, x0)
    assert a.clen[0] == 300


def test_two_face_square_with_ten_thousand_samples(device):
    v = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [1.0, 1.0, 0.0], [0.0, 1.0, 0.0]])
    f = np.array([[0, 1, 2], [0, 2, 3]])
    _, face, bary, _ = sampler.sample(v, f, 10_000, seed=1)
    y, x0 = _values(10_000, 4, 4, 6)
    assert_matches(f, 4, face, bary, y, x0)


def test_isolated_vertices_keep_their_rows(device):
    v, f = sampler.icosphere(1)
    n_v = v.shape[0] + 5
    f = np.where(f >= 7, f + 5, f)                                        # vertices 7 .. 11 are in no face
    vv = np.concatenate([v[:7], np.zeros((5, 3)), v[7:]])
    _, face, bary, _ = sampler.sample(vv, f, 4 * f.shape[0], seed=2)
    y, x0 = _values(face.shape[0], n_v, 4, 7)
    table, _, counts, _ = assert_matches(f, n_v, face, bary, y, x0, mask=0b1111)
    assert counts[5] == 5 and np.array_equal(_bits(table[7:12]), _bits(x0[7:12]))


def test_repeated_index_and_out_of_range_faces_take_no_part(device):
    v, f = sampler.icosphere(1)
    f = f.copy()
    f[3, 1] = f[3, 0]                                                     # a repeated index
    f[10, 2] = v.shape[0]                                                 # an index one past the end
    f[11, 0] = -1
    rng = np.random.default_rng(8)
    face = np.sort(rng.integers(0, f.shape[0], 400))                      # the skipped faces have samples too
    bary = rng.dirichlet(np.ones(3), 400)
    y, x0 = _values(400, v.shape[0], 4, 8)
    _, _, counts, a = assert_matches(f, v.shape[0], face, bary, y, x0)
    assert counts[3] == 3 and counts[4] == np.isin(face, [3, 10, 11]).sum() > 0
    assert not a.gram[[3, 10, 11]].any()


# ------------------------------------------------------------------------------------------------------------ 2. sizes
@pytest.mark.parametrize("n_v", [255, 256, 257, 513])
def test_vertex_counts_around_a_dot_leaf(device, n_v):
    v, f = _strip(n_v)
    _, face, bary, _ = sampler.sample(v, f, 4 * f.shape[0], seed=n_v)
    y, x0 = _values(face.shape[0], n_v, 4, n_v)
    assert_matches(f, n_v, face, bary, y, x0, pads=(0, 12, 12))


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, 80])
def test_sample_counts(device, n):
    """Level-2 icosphere, F = 320: around a wave and a workgroup, none at all, and F / 4 = 80."""
    v, f, face, bary = _sphere(2, n, seed=n)
    y, x0 = _values(n, v.shape[0], 4, 100 + n)
    table, _, counts, a = assert_matches(f, v.shape[0], face, bary, y, x0)
    inactive = ~a.active
    assert counts[5] == inactive.sum() and np.array_equal(_bits(table[inactive]), _bits(x0[inactive]))
    if n == 0:
        assert np.array_equal(_bits(table), _bits(x0))
    if n <= 80:
        assert counts[5] > 0


@pytest.mark.parametrize("n_c,pads", [(1, (0, 0, 0)), (1, (2, 15, 15)), (4, (1, 12, 12)), (46, (0, 2, 2)), (46, (5, 0, 2)),
                                      (60, (4, 4, 4)), (64, (0, 0, 0)), (64, (3, 16, 32))])
def test_column_counts_with_padded_strides(device, n_c, pads):
    v, f, face, bary = _sphere(2, 4 * 320)
    y, x0 = _values(face.shape[0], v.shape[0], n_c, n_c)
    assert_matches(f, v.shape[0], face, bary, y, x0, pads=pads)


# ------------------------------------------------------------------------------------------------ 3. solver parameters
@pytest.mark.parametrize("steps", [0, 1, 32])
@pytest.mark.parametrize("lam", [0.0, LAMBDA])
@pytest.mark.parametrize("mask_name", ["none", "last", "all"])
def test_steps_prior_weights_and_clamp_masks(device, steps, lam, mask_name):
    v, f, face, bary = _sphere(2, 4 * 320)
    n_c = 6
    y, x0 = _values(face.shape[0], v.shape[0], n_c, 9)
    mask = {"none": 0, "last": 1 << (n_c - 1), "all": (1 << n_c) - 1}[mask_name]
    table, _, counts, a = assert_matches(f, v.shape[0], face, bary, y, x0, lam=lam, steps=steps, mask=mask)
    if mask and steps == 32:
        assert counts[6] > 0 and (table[:, -1] > 0).all()
        cols = [c for c in range(n_c) if mask >> c & 1]
        assert (table[:, cols] >= a.lo[:, cols]).all() and (table[:, cols] <= a.hi[:, cols]).all()
    if not mask:
        assert counts[6] == 0


def test_a_second_solve_after_one_assemble(device):
    """solve may run again on what one assemble left, with another step count and mask."""
    from quadraturefields_amd import _C
    v, f, face, bary = _sphere(2, 4 * 320)
    y, x0 = _values(face.shape[0], v.shape[0], 4, 10)
    a = ref.assemble(f, v.shape[0], face, bary, y, x0, LAMBDA)
    lib, p = _C.lib(), _C.ptr
    n_v, n_f, n, n_c = v.shape[0], f.shape[0], face.shape[0], 4
    tf, sf, sb, ty, tx = _dev(f, np.int64), _dev(face, np.int64), _dev(bary, np.float64), _dev(y, np.float32), _dev(x0, np.float32)
    ws_bytes = int(lib.qf_vertex_fit_workspace_bytes(n_v, n_f, n, n_c))
    ws = torch.empty((ws_bytes,), dtype=torch.uint8).cuda()
    gram, mass, rhs = (torch.empty(s, dtype=torch.float64).cuda() for s in ((n_f, 9), (n_v,), (n_v, n_c)))
    counts, stats = torch.empty((8,), dtype=torch.int64).cuda(), torch.empty((n_c, 2), dtype=torch.float64).cuda()
    _C.check(lib.qf_vertex_fit_assemble(p(tf), n_f, n_v, p(sf), p(sb), n, p(ty), n_c, p(tx), n_c, n_c, LAMBDA, p(gram), p(mass),
                                        p(rhs), p(ws), ws_bytes, p(counts), _C.stream()), "assemble")
    for steps, mask in [(32, 0b1111), (3, 0), (32, 0b1000)]:
        out = torch.empty((n_v, n_c), dtype=torch.float32).cuda()
        _C.check(lib.qf_vertex_fit_solve(p(tf), n_f, n_v, p(tx), n_c, n_c, p(gram), p(mass), p(rhs), steps, mask, p(ws),
                                         ws_bytes, p(out), n_c, p(stats), p(counts), _C.stream()), "solve")
        table, want_stats, want_counts = ref.solve(a, steps, mask)
        assert np.array_equal(_bits(out.cpu().numpy()), _bits(table)) and counts.tolist() == want_counts.tolist()
        assert np.array_equal(_bits(stats.cpu().numpy()), _bits(want_stats))


# -------------------------------------------------------------------------------------------------------- 4. refusals
@pytest.mark.parametrize("name", ["unsorted", "face_past_the_end", "negative_face", "nan_target", "inf_bary", "nan_prior"])
def test_invalid_input_leaves_the_output_alone(device, name):
    v, f, face, bary = _sphere(2, 4 * 320)
    y, x0 = _values(face.shape[0], v.shape[0], 4, 11)
    face, bary = face.copy(), bary.copy()
    if name == "unsorted":
        face[[100, 700]] = face[[700, 100]]
    elif name == "face_past_the_end":
        face[-1] = f.shape[0]
    elif name == "negative_face":
        face[0] = -1
    elif name == "nan_target":
        y[500, 2] = np.nan
    elif name == "inf_bary":
        bary[17, 1] = np.inf
    else:
        x0[3, 0] = np.nan
    table, stats, counts, a = assert_matches(f, v.shape[0], face, bary, y, x0, pads=(0, 4, 4))
    assert table is None and counts[7] == 1 and counts[:3].sum() >= 1 and counts[3:7].tolist() == [0, 0, 0, 0]
    from quadraturefields_amd import baking
    with pytest.raises(ValueError, match="cannot be fitted"):
        baking.fit_vertex_table_device(_dev(f, np.int64), v.shape[0], _dev(face, np.int64), _dev(bary, np.float64),
                                       _dev(y, np.float32), _dev(x0, np.float32))


# -------------------------------------------------------------------------------------------------------- 5. wrappers
def test_table_wrapper_matches_the_restatement(device):
    from quadraturefields_amd import _C, baking
    v, f, face, bary = _sphere(2, 8 * 320)
    y, x0 = _values(face.shape[0], v.shape[0], 46, 12)
    args = (_dev(f, np.int32), v.shape[0], _dev(face, np.int64), _dev(bary, np.float64), _dev(y, np.float32))
    got, stats = baking.fit_vertex_table_device(*args, _dev(x0, np.float32), return_stats=True)
    table, want_stats, counts, _ = ref.fit(f, v.shape[0], face, bary, y, x0, LAMBDA, 32, 1 << 45)
    assert got.dtype == torch.float32 and np.array_equal(_bits(got.cpu().numpy()), _bits(table))
    assert [stats[k] for k in _C.VERTEX_FIT_COUNTS] == counts.tolist()
    assert stats["rhs_norm"] == want_stats[:, 0].tolist() and stats["residual_norm"] == want_stats[:, 1].tolist()
    module = baking.VertexBakedFeatures(torch.from_numpy(x0), device="cuda", train_density=False)
    assert module.table.shape[1] == 48
    fitted = baking.fit_vertex_table_device(*args, module)
    assert isinstance(fitted, baking.VertexBakedFeatures) and fitted is not module and not fitted.train_density
    assert np.array_equal(_bits(fitted.features().cpu().numpy()), _bits(table))
    assert np.array_equal(_bits(module.features().cpu().numpy()), _bits(x0))           # the prior is read, not written
    strided = torch.zeros((v.shape[0], 64), dtype=torch.float32).cuda()
    strided[:, :46] = _dev(x0, np.float32)
    again = baking.fit_vertex_table_device(*args, strided[:, :46], clamp_columns=[45])
    assert np.array_equal(_bits(again.cpu().numpy()), _bits(table))
    free = baking.fit_vertex_table_device(*args, _dev(x0, np.float32), clamp_columns=None, iterations=5, prior_weight=0.25)
    assert np.array_equal(_bits(free.cpu().numpy()), _bits(ref.fit(f, v.shape[0], face, bary, y, x0, 0.25, 5, 0)[0]))


@functools.lru_cache(maxsize=None)
def _scene():
    from quadraturefields_amd import synthetic
    from tests import vertex_baked_reference as vb
    return synthetic.shell_mesh(n_shells=2, subdivisions=3), vb.sg_field(6, "cuda")


def test_field_wrapper_on_the_synthetic_scene(device):
    """The fit lowers the feature-space error on its own samples, column by column: CG never raises the objective it
    minimises, and that objective is this error plus a non-negative prior term.  The
    density column is clamped afterwards and is left out of that comparison.  ``vertex_surface_error``'s pixel-unit
    figures of the fitted table are below the point bake's on the fit's own seed too; those on a fresh seed are printed."""
    from quadraturefields_amd import baking, mc_utils
    mesh, sg = _scene()
    n_f, n_v = mesh.faces.shape[0], mesh.vertices.shape[0]
    bake = baking._field_features(sg, torch.from_numpy(np.asarray(mesh.vertices, np.float32)).cuda())
    fitted, stats = baking.fit_vertex_features(sg, mesh, return_stats=True)
    assert fitted.shape == bake.shape == (n_v, 46) and fitted.dtype == torch.float32 and stats["refused"] == 0
    # What 32 steps promise whatever the mesh: the spectrum of the preconditioned operator lies in [1/64, 1 + 1/64], so
    # kappa <= 65 and CG's energy-norm error falls by 2 ((sqrt(65) - 1) / (sqrt(65) + 1))^32 = 6.9e-4; as a residual in the
    # preconditioner's norm that is at most sqrt(65) times as much, 5.5e-3, and the plain norms of the stats differ from it
    # by at most the square root of the spread of a_v, measured here.  (On an icosphere the smallest eigenvalue is near
    # 0.2 and the same 32 steps reach 1e-13: tests/test_vertex_fit_host.py.)
    ratio = [r / b for r, b in zip(stats["residual_norm"], stats["rhs_norm"]) if b > 0]
    print("relative residual per column:", " ".join(f"{r:.1e}" for r in ratio))
    print("rhs norm per column:", " ".join(f"{b:.1e}" for b in stats["rhs_norm"]))
    assert (fitted[:, -1] >= 0).all()
    # the same samples and targets through the restatement
    v64 = torch.from_numpy(np.asarray(mesh.vertices, np.float64)).cuda()
    faces = torch.from_numpy(np.asarray(mesh.faces, np.int64)).cuda()
    samples = mc_utils.sample_surface_device(v64, faces, 8 * n_f, 0)
    targets = baking._field_features(sg, samples.points.to(torch.float32))
    want, _, _, a = ref.fit(np.asarray(mesh.faces), n_v, samples.face.cpu().numpy(), samples.bary.cpu().numpy(),
                            targets.cpu().numpy(), bake.cpu().numpy(), LAMBDA, 32, 1 << 45)
    assert np.array_equal(_bits(fitted.cpu().numpy()), _bits(want))
    spread = float(a.inv[a.active].max() / a.inv[a.active].min())
    print(f"a_v spreads by a factor of {spread:.1f}")
    assert max(ratio) < 5.5e-3 * np.sqrt(spread)
    own = {k: baking.vertex_surface_error(sg, mesh, t, 8 * n_f, seed=0) for k, t in (("bake", bake), ("fit", fitted))}
    fresh = {k: baking.vertex_surface_error(sg, mesh, t, 8 * n_f, seed=77) for k, t in (("bake", bake), ("fit", fitted))}
    for k in ("mean", "rms", "max"):
        print(f"surface error {k}: own seed {own['bake'][k]:.4e} -> {own['fit'][k]:.4e}, "
              f"fresh seed {fresh['bake'][k]:.4e} -> {fresh['fit'][k]:.4e}")
    # in pixel units nothing is promised by the mathematics; on this scene all three figures fall (measured: mean 8.28e-3
    # -> 6.68e-3, RMS 1.58e-2 -> 1.27e-2, maximum 0.487 -> 0.448), and the whole pipeline is deterministic
    for k in ("mean", "rms", "max"):
        assert own["fit"][k] < own["bake"][k], k
    b, t = np.array(own["bake"]["feature_rms"][:-1]), np.array(own["fit"]["feature_rms"][:-1])
    print("feature rms, fit / bake, own seed:", np.round(t / np.maximum(b, 1e-30), 3).tolist())
    assert (t <= b * (1 + 1e-5) + 1e-7).all()           # fp32 rounding of the table and of the scorer's blend
    assert (t * t).sum() < 0.9 * (b * b).sum()
    # a module comes back as a module, a weighted and an explicit sample count are passed on
    module = baking.VertexBakedFeatures(bake)
    again = baking.fit_vertex_features(sg, mesh, prior=module)
    assert isinstance(again, baking.VertexBakedFeatures) and np.array_equal(_bits(again.features().cpu().numpy()), _bits(want))
    few = baking.fit_vertex_features(sg, mesh, n_samples=1000, seed=3, face_weight=np.ones(n_f), iterations=4)
    assert few.shape == bake.shape and bool(torch.isfinite(few).all())
    with pytest.raises(TypeError, match="QuantisedVertexFeatures"):
        baking.fit_vertex_features(sg, mesh, prior=baking.quantise_vertex_features(bake))


# ------------------------------------------------------------------------------------------------------- 6. the examples
def _example(name):
    spec = importlib.util.spec_from_file_location(name + "_example", os.path.join(ROOT, "examples", name + ".py"))
    example = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(example)
    return example


def test_lod_example_with_and_without_the_fit(device, tmp_path, capsys):
    example = _example("lod_vertex_baked")
    base = ["--synthetic", "--root", str(tmp_path), "--log2_hashmap_size", "14", "--size", "100", "--views", "2"]
    plain = example.main(base)
    text = capsys.readouterr().out
    assert json.loads(text.strip().splitlines()[-1]) == plain and "fitted" not in text
    assert [k for k in plain if isinstance(plain[k], dict)] == ["full", "transferred", "rebaked"]
    fit = example.main(base + ["--fit_samples_per_face", "8"])
    text = capsys.readouterr().out
    assert json.loads(text.strip().splitlines()[-1]) == fit
    assert [k for k in fit if isinstance(fit[k], dict)] == ["full", "transferred", "rebaked", "fitted", "fitted_decimated"]
    assert {k: fit[k] for k in plain} == plain
    assert fit["fitted"]["vertices"] == plain["full"]["vertices"] and fit["fitted_decimated"]["faces"] == plain["rebaked"]["faces"]
    print({k: round(fit[k]["psnr"], 2) for k in fit if isinstance(fit[k], dict)})
    assert all(np.isfinite(fit[k]["psnr"]) for k in ("fitted", "fitted_decimated"))


def test_evaluate_example_with_and_without_the_fit(device, tmp_path, capsys):
    example = _example("evaluate_vertex_baked")
    base = ["--synthetic", "--root", str(tmp_path), "--log2_hashmap_size", "14", "--size", "100", "--views", "2"]
    plain = example.main(base)
    text = capsys.readouterr().out
    assert json.loads(text.strip().splitlines()[-1]) == plain and "fit" not in " ".join(plain)
    fit = example.main(base + ["--fit_samples_per_face", "8"])
    text = capsys.readouterr().out
    assert json.loads(text.strip().splitlines()[-1]) == fit and "fitted table (8 samples per face)" in text
    assert {k: fit[k] for k in plain} == plain
    assert sorted(set(fit) - set(plain)) == ["fit_psnr", "fit_samples_per_face", "fit_ssim", "fit_surface_error_rms",
                                             "surface_error_rms"]
    print({k: fit[k] for k in ("psnr", "fit_psnr", "surface_error_rms", "fit_surface_error_rms")})
    assert np.isfinite(fit["fit_psnr"])
