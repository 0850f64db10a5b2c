"""Every capped-grid kernel past its cap (``tests/grid_caps.py``): inputs sized from the device's CU count so that some
workgroups take a second trip of their grid-stride loop, others one, and the last trip is ragged.

Three kinds of check, no tolerance of this module's own:

* stateful loops (LDS tables, barriers, fills in front of a tile loop) against the references the existing tests use, at
  those tests' bars: ``qf_mesh_update_d`` against an fp64 ``np.bincount`` under the summation bound
  ``(k + 1) * 2^-24 * sum|term|`` for a row of k fp32 terms (any order of k fp32 additions, plus nothing for the products:
  the reference adds the same fp32 products), ``qf_vertex_shade_points_backward`` against the float64 reference at
  ``test_gpu_vertex_train.TOL``, the three tile compositors against the unfused routes bit for bit;
* per-item kernels: the whole batch equals, bit for bit, the concatenation of the same call on consecutive pieces of at
  most cap / 2 items -- the kernel below its cap, which the existing tests pin to the oracle;
* rows with a cheap vectorised reference against it, at the existing tests' bars.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from tests import grid_caps as GC

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cu(lib, device):
    c = lib.qf_device_cu_count()
    assert c > 0
    return c


def _C():
    from quadraturefields_amd import _C as c
    return c


def _ok(status, what):
    _C().check(status, what)


def _P(t):
    return _C().ptr(t)


def _st():
    return _C().stream()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bits(t):
    """The tensor as integers of its element size: equality of bits, NaN and -0.0 included."""
    if t.dtype == torch.float32:
        return t.contiguous().view(torch.int32)
    if t.dtype == torch.float64:
        return t.contiguous().view(torch.int64)
    return t


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(_bits(a), _bits(b))


def _cuts(n, piece):
    """Consecutive [a, b) of at most ``piece`` items covering [0, n), of nearly equal sizes."""
    k = -(-n // piece)
    edges = [n * i // k for i in range(k + 1)]
    assert max(b - a for a, b in zip(edges, edges[1:])) <= piece and k >= 3
    return list(zip(edges, edges[1:]))


def _whole_equals_pieces(n, cap, run, names):
    """``run(a, b)``: the call on items [a, b) with everything rebased, as a tuple of per-item tensors."""
    assert n > cap
    whole = run(0, n)
    parts = [run(a, b) for a, b in _cuts(n, cap // 2)]
    torch.cuda.synchronize()
    for k, name in enumerate(names):
        got = torch.cat([p[k] for p in parts])
        assert _same(whole[k], got), f"{name}: the whole batch differs from its pieces at " \
            f"{int((_bits(whole[k]) != _bits(got)).reshape(whole[k].shape[0], -1).any(dim=1).nonzero()[0])}"


# ====================================================================================================================
# a. stateful loops
# ====================================================================================================================
def _update_d(lib, d, w, ids, n_faces, device):
    cache = torch.zeros(n_faces, 4, device=device)
    skipped = torch.zeros(1, dtype=torch.int32, device=device)
    _ok(lib.qf_mesh_update_d(_P(d), _P(w), _P(ids), ids.shape[0], n_faces, _P(cache), _P(skipped), _st()), "qf_mesh_update_d")
    return cache.cpu().numpy(), int(skipped.item())


def _update_d_check(lib, device, ids, n_faces, n_bad, label):
    n = ids.shape[0]
    rng = np.random.default_rng(n % 1000 + n_faces % 1000)
    d = (rng.standard_normal((n, 3)) * 0.01).astype(np.float32)
    w = rng.random(n).astype(np.float32)
    assert int(((ids < 0) | (ids >= n_faces)).sum()) == n_bad > 0
    ref, bound, k = GC.update_d_reference(d, w, ids, n_faces)
    dt, wt, it = (torch.from_numpy(a).to(device) for a in (d, w, ids))
    for with_d in (True, False):
        got, skipped = _update_d(lib, dt if with_d else None, wt, it, n_faces, device)
        assert skipped == n_bad, (label, with_d, skipped, n_bad)
        cols = slice(0, 4) if with_d else slice(3, 4)
        err = np.abs(got[:, cols].astype(np.float64) - ref[:, cols])
        worst = float((err / np.maximum(bound[:, cols], 1e-300)).max())
        print(f"update_d {label} d={'given' if with_d else 'NULL'}: n {n}, faces {n_faces}, rows hit {int((k > 0).sum())}, "
              f"largest row {int(k.max())} samples, worst err / bound {worst:.3f}")
        assert bool((err <= bound[:, cols]).all()), (label, with_d, worst)
        assert not got.view(np.int32)[k == 0].any(), f"{label}: a row that received nothing is not bit-zero"
        if not with_d:
            assert not got.view(np.int32)[:, :3].any(), f"{label}: d == NULL wrote a displacement column"


@pytest.mark.parametrize("kind", GC.UPDATE_D_KINDS)
def test_mesh_update_d_past_the_cap(lib, device, cu, kind):
    """More chunks than 8 CU workgroups: the hash-table reset and the trailing barrier of the chunk loop are reused.  Seven
    faces (every sample of a chunk in seven slots), about 2^22 faces with nearly every id of a chunk distinct (a table
    half full), and keys that hash to slot 2047 so that the probe wraps to slot 0."""
    row = GC.BY_KEY["update_d_merged"]
    n = GC.past(row, cu)
    assert n > GC.cap_items(row, cu) and -(-n // 1024) > 8 * cu
    ids, n_faces, n_bad = GC.update_d_ids(kind, n)
    _update_d_check(lib, device, ids, n_faces, n_bad, kind)


@pytest.mark.parametrize("n", [8191, 8192])
def test_mesh_update_d_on_both_sides_of_the_route_switch(lib, device, n):
    ids, n_faces, n_bad = GC.update_d_ids("wrap", n)
    _update_d_check(lib, device, ids, n_faces, n_bad, f"route-{n}")


def _vertex_frame(cu):
    """The vertex-baked scene's frame whose K = 25 sample count exceeds ``past``: the scene has about 5.07 samples a ray at
    every frame size (the camera's view does not change with it), 4.5 are counted on."""
    need = GC.past(GC.BY_KEY["vertex_train"], cu)
    s = math.sqrt(need / 4.5 / (37 * 29))
    return int(math.ceil(37 * s)) | 1, int(math.ceil(29 * s)) | 1, need


@pytest.mark.parametrize("lobes", [1, 6])
def test_vertex_backward_past_the_cap(device, cu, lobes):
    """int64 and int32 ids on more samples than one sweep of the grid: the barrier at the end of the loop ("the rows are
    rewritten by the next trip") is what keeps a wave's LDS rows from being overwritten under its neighbours."""
    from quadraturefields_amd import baking
    from tests import test_gpu_vertex_train as VT
    from tests import vertex_baked_reference as R
    from tests import vertex_train_reference as G
    w, h, n = _vertex_frame(cu)
    s = VT._samples(device, w, h, 25)
    xyzs, dirs, _, _, index_tri, _ = s["data"]
    assert xyzs.shape[0] >= n > GC.cap_items(GC.BY_KEY["vertex_train"], cu), (xyzs.shape[0], n)
    c = _C()
    points, dirs, tri = c.f32c(xyzs[:n]), c.f32c(dirs[:n]), index_tri[:n].contiguous()
    feats = VT._table(device, "random", lobes, 25)
    module = baking.VertexBakedFeatures(torch.from_numpy(feats), device=device)
    g = _gen(17)
    d_rgb, d_sigma = torch.randn(n, 3, generator=g), torch.randn(n, generator=g)
    m = R.mesh()
    want = G.table_gradient(feats, m.vertices, m.faces, points.cpu().numpy(), tri.cpu().numpy(), dirs.cpu().numpy(), d_rgb,
                            d_sigma, lobes)
    wdt = R.row_width(lobes)
    touched = torch.from_numpy(G.contributions(m.vertices.shape[0], m.faces, tri.cpu().numpy()) > 0).to(device)
    for ids32 in (False, True):
        grad = VT._backward(device, module, s["mi"], points, tri, dirs, d_rgb.to(device), d_sigma.to(device), ids32=ids32)
        assert not bool(grad[:, wdt:].any()) and not bool(grad[~touched].any())
        ratio = G.column_ratio(grad[:, :wdt].cpu().numpy(), want)
        print(f"vertex backward {lobes} lobes, {'int32' if ids32 else 'int64'} ids, {n} samples of a {w}x{h} frame: "
              f"ratio {ratio:.3e} (tol {VT.TOL:.3e})")
        assert ratio <= VT.TOL, ratio


def _tile_frame(cu):
    """A frame of more than 32 CU tiles, neither side a multiple of 8 (733 x 725 at 256 CUs)."""
    tx = int(math.isqrt(32 * cu)) + 2
    ty = tx - 1
    assert tx * ty > 32 * cu
    return 8 * tx - 3, 8 * ty - 3


def _assert_frames_equal(got, want, what):
    for name, a, b in zip(("rgb", "alpha", "depth"), got[:3], want[:3]):
        assert _same(a, b), f"{what}: {name} differs"


@pytest.mark.parametrize("kind", ["vertex", "quant", "texture"])
def test_tile_compositors_past_the_cap(device, cu, kind):
    """One frame each of more tiles than 4 x 8 CU, so that a workgroup's waves take a second tile behind the table and LDS
    fills: the fused frame equals the unfused ray-major route bit for bit, and with ``early_stop_eps = 1e-3`` the
    truncated unfused route, counts included."""
    from quadraturefields_amd import utils
    from quadraturefields_amd.datasets.utils import Rays
    w, h = _tile_frame(cu)
    n_tiles = ((w + 7) // 8) * ((h + 7) // 8)
    assert n_tiles > GC.cap_items(GC.BY_KEY[f"{kind}_tiles"], cu) and w % 8 and h % 8
    assert w * h > GC.cap_items(GC.BY_KEY["camera_rays_check"], cu)
    eps = 1e-3
    if kind == "texture":
        from tests import test_gpu_baked_termination as BT
        s = BT._scene(device, w, h, 5, 6, "white", "sigmoid", "extremes")
        fr, ri = s["fr"], s["mi"].rayintersector
        render = lambda e: fr.render_baked(s["o"], s["d"], s["uv"], s["comp"], camera=s["cam"], early_stop_eps=e)   # noqa: E731
        reference = lambda e: BT._reference(s, e)                                                                    # noqa: E731
    else:
        from tests import test_gpu_vertex_baked as VB
        from tests import test_gpu_vertex_quant as VQ
        from tests import vertex_baked_reference as R
        cfg = (w, h, 5, 6, "white")
        s = VB._scene(device, *cfg)
        fr, ri = s["fr"], s["mi"].rayintersector
        if kind == "vertex":
            table, stop_table = s["feats"], R.override_density(s["feats"])
        else:
            table, stop_table = VQ._quantised_scene(device, cfg, "linear")[1], VQ._quantised_scene(device, cfg, "linear", True)[1]
        major = utils.render_image_finetune_baking_with_occgrid(
            None if kind == "quant" else fr.radiance_field, None, Rays(origins=s["o"], viewdirs=s["d"]), s["data"],
            render_step_size=VB.DELTA, mesh_intersect=s["mi"], vertex_features=table, bg_color=s["bg"])
        render = lambda e: fr.render_vertex_baked(s["o"], s["d"], stop_table if e else table, camera=s["cam"],      # noqa: E731
                                                  early_stop_eps=e)
        reference = lambda e: VB._stopping_reference(s, stop_table, e)                                               # noqa: E731
    mismatches = ri.camera_mismatch_frames
    n = int(s["counts"].sum())
    got = render(0.0)
    assert got[3] == n and ri.last_frame.shaded_count.cpu().numpy().tolist() == s["counts"].tolist()
    if kind == "texture":
        kept0, *want = reference(0.0)
        assert kept0.tolist() == s["counts"].tolist()
        _assert_frames_equal(got, want, "texture frame against shade-points + derive_properties")
    else:
        assert major[3] == n
        _assert_frames_equal(got, major, f"{kind} frame against the ray-major route")
        if kind == "quant":
            dec = fr.render_vertex_baked(s["o"], s["d"], VQ._quantised_scene(device, cfg, "linear")[2], camera=s["cam"])
            _assert_frames_equal(got, dec, "quantised frame against the fp32 route on the decoded table")
    kept, *want = reference(eps)
    stop = render(eps)
    shaded = ri.last_frame.shaded_count.cpu().numpy()
    print(f"{kind} {w}x{h}: {n_tiles} tiles (cap {32 * cu}), {n} samples, eps {eps}: {int(shaded.sum())} shaded")
    assert stop[3] == n and shaded.tolist() == kept.tolist() and int(shaded.sum()) < n
    _assert_frames_equal(stop, want, f"{kind} frame with early_stop_eps against the truncated unfused route")
    assert ri.camera_mismatch_frames == mismatches          # the ray check (camera_rays_check_kernel, n_rays > 2048 CU) passed


def _march_scene(device, n):
    """The ``image16`` scene of test_gpu_volumetric_frame.py widened to ``n`` rays: its grid, its camera, a wider image."""
    from quadraturefields_amd import synthetic
    from tests import test_gpu_volumetric_frame as VF
    b = VF._scene("image16")[0]
    w = int(math.isqrt(n * 3 // 2)) | 1
    h = -(-n // w) + 1
    c2w = synthetic.orbit_cameras(1, radius=3.0, seed=5)[0]
    o, d = synthetic.camera_rays(c2w, synthetic.lego_focal(800) * w / 800.0 * 0.4, w, h, device=device)
    assert o.shape[0] >= n
    return VF, b, VF._estimator(b, device), o[:n].contiguous(), d[:n].contiguous()


def test_occupancy_march_past_the_cap(device, cu):
    """qf_grid_march_count / qf_grid_march_write on more rays than 64 x 64 CU: the whole batch equals its pieces (ray ids
    rebased here), and 2 000 random rays of it equal ``oracle.occgrid.march``, bit for bit."""
    from oracle import occgrid as oocc
    row = GC.BY_KEY["grid_march"]
    n, cap = GC.past(row, cu), GC.cap_items(row, cu)
    VF, b, est, o, d = _march_scene(device, n)
    near, far = 0.0, 1e10

    def run(a, e):
        return est.sampling(o[a:e], d[a:e], near_plane=near, far_plane=far, render_step_size=VF.STEP)

    assert n > cap
    ridx, ts, te = run(0, n)
    parts = [run(a, e) for a, e in _cuts(n, cap // 2)]
    ridx_p = torch.cat([p[0] + a for p, (a, _) in zip(parts, _cuts(n, cap // 2))])
    print(f"march: {n} rays (cap {cap}), {ridx.shape[0]} samples")
    assert ridx.shape[0] > 100000 and torch.equal(ridx, ridx_p)
    assert _same(ts, torch.cat([p[1] for p in parts])) and _same(te, torch.cat([p[2] for p in parts]))
    sel = np.sort(np.random.default_rng(3).choice(n, 2000, replace=False))
    sel[-1] = n - 1                                               # the last ray of the ragged trip
    sel_d = torch.from_numpy(sel).to(device)
    r_o, ts_o, te_o = oocc.march(VF.AABB, b, o[sel_d].cpu().numpy(), d[sel_d].cpu().numpy(), near, far, VF.STEP)
    mask = torch.isin(ridx, sel_d)
    assert np.array_equal(torch.searchsorted(sel_d, ridx[mask]).cpu().numpy(), r_o) and r_o.shape[0] > 2000
    assert np.array_equal(ts[mask].cpu().numpy(), ts_o) and np.array_equal(te[mask].cpu().numpy(), te_o)


def _round(lib, est, o, d, near, alive, opacity, quota, step):
    """One count / scan / write / accumulate round on the C ABI with a quota of ``quota`` samples a ray; the field is an
    elementwise function of the sample's position, so a piece evaluates it to the same bits as the whole."""
    n, dev = o.shape[0], o.device
    near, alive, opacity = near.clone(), alive.clone(), opacity.clone()
    state = torch.zeros(8, dtype=torch.int64, device=dev)
    state[0] = n // quota
    count = torch.empty(n, dtype=torch.int32, device=dev)
    term = torch.zeros(n, device=dev)                           # a dead ray's plane is not written
    aabb, res = est._host_geometry()
    march = (aabb, res, _P(est.binaries[0].contiguous()), _P(o), _P(d), _P(near), _P(alive), n, 0.0, 1e10, step, _P(state))
    _ok(lib.qf_grid_march_round_count(*march, 0, _P(count), _P(term), _st()), "qf_grid_march_round_count")
    assert int(state[4]) == quota, (int(state[4]), quota, n)
    csum = torch.cumsum(count.to(torch.int64), dim=0)
    total = int(csum[-1])
    ts, te = torch.empty(total, device=dev), torch.empty(total, device=dev)
    ridx = torch.empty(total, dtype=torch.int64, device=dev)
    xyz, dirs = torch.empty(total, 3, device=dev), torch.empty(total, 3, device=dev)
    _ok(lib.qf_grid_march_round_write(*march, 0, _P(count), _P(csum), total, _P(ts), _P(te), _P(ridx), _P(xyz), _P(dirs), _st()),
        "qf_grid_march_round_write")
    sigma = (xyz[:, 0].abs() * 30.0).contiguous()
    rgbs = (xyz * 0.25 + 0.5).clamp(0.0, 1.0).contiguous()
    rgb, depth = torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev)
    _ok(lib.qf_volumetric_accumulate(_P(ts), _P(te), _P(sigma), _P(rgbs), _P(count), _P(csum), _P(term), n, total, 1e-2, 1e-2,
                                     _P(state), 0, _P(rgb), _P(opacity), _P(depth), _P(near), _P(alive), _st()),
        "qf_volumetric_accumulate")
    return dict(per_ray=(count, term, rgb, opacity, depth, near, alive), per_sample=(ts, te, xyz, dirs), ridx=ridx,
                state=state.cpu().tolist())


@pytest.mark.parametrize("quota", [7, 64])
def test_volumetric_round_past_the_cap(lib, device, cu, quota):
    """qf_grid_march_round_count, qf_grid_march_round_write and qf_volumetric_accumulate on more rays than 64 x 64 CU (and
    than 2048 CU): the whole batch equals its pieces bit for bit, the survivor and sample counters add up."""
    row = GC.BY_KEY["march_round_count"]
    n = GC.past(row, cu)
    cap = min(GC.cap_items(row, cu), GC.cap_items(GC.BY_KEY["volumetric_accumulate"], cu))
    assert n > GC.cap_items(row, cu) >= cap
    VF, b, est, o, d = _march_scene(device, n)
    g = _gen(31)
    near = (torch.rand(n, generator=g) * 0.5).to(device)
    alive = (torch.rand(n, generator=g) < 0.8).to(torch.uint8).to(device)
    opacity = (torch.rand(n, generator=g) * 0.5).to(device)
    whole = _round(lib, est, o, d, near, alive, opacity, quota, VF.STEP)
    cuts = _cuts(n, cap // 2)
    parts = [_round(lib, est, o[a:e].contiguous(), d[a:e].contiguous(), near[a:e], alive[a:e], opacity[a:e], quota, VF.STEP)
             for a, e in cuts]
    print(f"round quota {quota}: {n} rays (caps {GC.cap_items(row, cu)}, {cap}), {whole['ridx'].shape[0]} samples, state "
          f"{whole['state'][:5]}")
    assert whole["ridx"].shape[0] > 100000 and whole["state"][1] < int(alive.sum())
    assert whole["state"][1] > 0 or quota == 64                 # no ray of this box has 64 samples left: every ray ends
    assert torch.equal(whole["ridx"], torch.cat([p["ridx"] + a for p, (a, _) in zip(parts, cuts)]))
    for key in ("per_ray", "per_sample"):
        for k, t in enumerate(whole[key]):
            assert _same(t, torch.cat([p[key][k] for p in parts])), (key, k)
    for slot in (1, 2, 3):                                     # survivors, kept samples, samples of the round
        assert whole["state"][slot] == sum(p["state"][slot] for p in parts), slot
    assert whole["state"][1] == int(whole["per_ray"][6].sum())


def test_mark_visited_cells_past_the_cap(lib, device, cu):
    row = GC.BY_KEY["mark_visited"]
    n, cap, m = GC.past(row, cu), GC.cap_items(row, cu), 96
    g = _gen(5)
    p = torch.rand(n, 3, generator=g) * 1.02 - 0.01
    p[::9] = (torch.randint(0, m, (p[::9].shape[0], 3), generator=g).float() / (m - 1))       # on the lattice: floor == ceil
    p[-1] = torch.tensor([1.0, 1.0, 1.0])
    p = p.to(device)

    def run(a, e):
        mask = torch.zeros(m * m * m, dtype=torch.uint8, device=device)
        bad = torch.zeros(1, dtype=torch.int64, device=device)
        _ok(lib.qf_mark_visited_cells(_P(p[a:e].contiguous()), e - a, m, _P(mask), _P(bad), _st()), "qf_mark_visited_cells")
        return mask, int(bad)

    assert n > cap
    mask, bad = run(0, n)
    parts = [run(a, e) for a, e in _cuts(n, cap // 2)]
    union = torch.stack([q[0] for q in parts]).amax(dim=0)
    outside = int((~((p >= 0) & (p <= 1)).all(dim=1)).sum())
    assert torch.equal(mask, union) and bad == sum(q[1] for q in parts) == outside > 100
    assert int(mask[-1]) == 1 and 0 < int(mask.sum()) < m ** 3


# ====================================================================================================================
# b. qf_scatter_max
# ====================================================================================================================
def _scatter_max(lib, values, index, out):
    _ok(lib.qf_scatter_max(_P(values), _P(index), values.shape[0], out.shape[0], _P(out), _st()), "qf_scatter_max")
    return out


def test_scatter_max_of_negative_zero(lib, device):
    """-0.0 is a contribution like any other: max(-1, -0.0) = 0."""
    out = _scatter_max(lib, torch.tensor([-0.0], device=device), torch.tensor([0], device=device), torch.tensor([-1.0], device=device))
    assert out.cpu().tolist() == [0.0]


@pytest.mark.parametrize("fill", [0.0, -1.0, -math.inf], ids=["zeros", "minus-one", "minus-inf"])
def test_scatter_max_past_the_cap(lib, device, cu, fill):
    """Values of both signs, +-0, +-inf, NaN (skipped) and ids out of range on more values than one sweep of the grid,
    against ``np.fmax.at`` as values.  Rows 0..49 receive nothing but -0.0 and negative values: their maximum is 0."""
    row = GC.BY_KEY["scatter_max"]
    n, cap, n_out = GC.past(row, cu), GC.cap_items(row, cu), 4099
    rng = np.random.default_rng(11)
    v = rng.standard_normal(n).astype(np.float32)
    idx = rng.integers(50, n_out - 10, n)                       # the last ten rows receive nothing
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], dtype=np.float32)
    at = rng.choice(n, n // 20, replace=False)
    v[at] = special[rng.integers(0, 5, at.shape[0])]
    low = rng.choice(n, 4000, replace=False)                    # rows 0..49: -0.0 and negative values only
    idx[low] = rng.integers(0, 50, 4000)
    v[low] = -np.abs(rng.standard_normal(4000)).astype(np.float32) - 0.5
    v[low[::4]] = -0.0
    v[low[-1]], idx[low[-1]] = -0.0, 49
    bad = rng.choice(n, 300, replace=False)
    idx[bad] = np.array([-1, n_out, n_out + 12345, -2 ** 40, 2 ** 40])[rng.integers(0, 5, 300)]
    v[n - 1], idx[n - 1] = 7.5, n_out - 11                      # the last value of the ragged trip
    assert n > cap and np.signbit(v[v == 0]).any() and (~np.signbit(v[v == 0])).any()
    want = GC.scatter_max_reference(fill, n_out, idx, v)
    out = _scatter_max(lib, torch.from_numpy(v).to(device), torch.from_numpy(idx).to(device),
                       torch.full((n_out,), fill, device=device)).cpu().numpy()
    assert not np.isnan(want).any() and want[n_out - 11] >= 7.5 and (want[-10:] == fill).all()
    assert (want[:50] == (0.0 if fill <= 0 else fill)).all()
    assert np.array_equal(out, want), np.flatnonzero(out != want)[:10]


# ====================================================================================================================
# c. every other row: the whole batch equals its pieces, or a vectorised reference
# ====================================================================================================================
def _frame_samples(device, cu, n):
    """``n`` ray-major samples of the tile compositors' vertex-baked frame (positions on the mesh, triangle ids, unit
    directions): computed once with that frame."""
    from tests import test_gpu_vertex_baked as VB
    w, h = _tile_frame(cu)
    s = VB._scene(device, w, h, 5, 6, "white")
    assert s["xyzs"].shape[0] >= n, (s["xyzs"].shape[0], n)
    c = _C()
    return s, c.f32c(s["xyzs"][:n]), s["index_tri"][:n].contiguous(), c.f32c(s["dirs"][:n])


def _segments(n_seg, seed, longest=3):
    """Segment lengths 0..longest (a tenth empty) as (counts, starts, n)."""
    counts = torch.randint(0, longest + 1, (n_seg,), generator=_gen(seed))
    counts[::10] = 0
    counts[-1] = longest
    starts = torch.cumsum(counts, 0) - counts
    return counts, starts, int(counts.sum())


def _case_mark_pack_boundaries(lib, device, cu):
    row = GC.BY_KEY["mark_boundaries"]
    n = GC.past(row, cu)
    ridx = torch.repeat_interleave(torch.arange(n), torch.randint(0, 4, (n,), generator=_gen(1)))[:n].contiguous().to(device)

    def run(a, e):
        lo = max(a - 1, 0)                                      # a sample's flag looks at its predecessor
        out = torch.empty(e - lo, dtype=torch.uint8, device=device)
        _ok(lib.qf_mark_pack_boundaries(_P(ridx[lo:e].contiguous()), e - lo, _P(out), _st()), "qf_mark_pack_boundaries")
        return (out[a - lo:],)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["boundary"])


def _case_exponential_integration(lib, device, cu):
    row, c = GC.BY_KEY["exp_integration"], 3
    n_seg = -(-GC.past(row, cu) // c)
    counts, starts, n = _segments(n_seg, 2)
    g = _gen(3)
    feats, tau = torch.rand(n, c, generator=g).to(device), (torch.rand(n, generator=g) * 2.0).to(device)
    starts = starts.to(device)
    edge = torch.cat([starts, torch.tensor([n], device=device)])

    def run(a, e):                                              # segments [a, e): their samples, starts rebased
        lo, hi = int(edge[a]), int(edge[e])
        out, wts = torch.empty(e - a, c, device=device), torch.empty(hi - lo, device=device)
        _ok(lib.qf_exponential_integration(_P(feats[lo:hi].contiguous()), c, _P(tau[lo:hi].contiguous()),
                                           _P((starts[a:e] - lo).contiguous()), e - a, hi - lo, 1, _P(out), _P(wts), _st()),
            "qf_exponential_integration")
        return out, wts

    assert n_seg * c > GC.cap_items(row, cu)
    whole = run(0, n_seg)
    cuts = _cuts(n_seg, GC.cap_items(row, cu) // 2 // c)
    parts = [run(a, e) for a, e in cuts]
    assert _same(whole[0], torch.cat([p[0] for p in parts])) and _same(whole[1], torch.cat([p[1] for p in parts]))


def _packed(n_rays, seed, device, longest=3):
    counts, starts, n = _segments(n_rays, seed, longest)
    return torch.stack([starts, counts], dim=1).contiguous().to(device), n


def _case_exclusive_scan(lib, device, cu):
    row = GC.BY_KEY["exclusive_scan"]
    n_rays = GC.past(row, cu)
    info, n = _packed(n_rays, 4, device)
    x = (torch.rand(n, generator=_gen(5)) + 0.25).to(device)

    def run(a, e, mode):
        lo, hi = int(info[a, 0]), int(info[e - 1, 0] + info[e - 1, 1])
        piece = info[a:e].clone()
        piece[:, 0] -= lo
        out = torch.full((hi - lo,), float("nan"), device=device)
        _ok(lib.qf_exclusive_scan(_P(x[lo:hi].contiguous()), _P(piece), e - a, hi - lo, mode, _P(out), _st()), "qf_exclusive_scan")
        return (out,)

    for mode in (0, 1):
        _whole_equals_pieces_rays(n_rays, GC.cap_items(row, cu), lambda a, e: run(a, e, mode), [f"exclusive scan mode {mode}"])


def _whole_equals_pieces_rays(n_rays, cap, run, names):
    """As ``_whole_equals_pieces`` for outputs of different lengths per piece (per-ray and per-sample tensors)."""
    assert n_rays > cap
    whole = run(0, n_rays)
    parts = [run(a, e) for a, e in _cuts(n_rays, cap // 2)]
    for k, name in enumerate(names):
        assert _same(whole[k], torch.cat([p[k] for p in parts])), name


def _case_render_from_density(lib, device, cu):
    row = GC.BY_KEY["render_from_density"]
    n_rays = GC.past(row, cu)
    info, n = _packed(n_rays, 6, device)
    g = _gen(7)
    ts = (torch.rand(n, generator=g) * 3 + 2).to(device)
    te = ts + 0.01 + (torch.rand(n, generator=g) * 0.05).to(device)
    sig, rgbs = (torch.rand(n, generator=g) * 60).to(device), torch.rand(n, 3, generator=g).to(device)
    bk = torch.tensor([0.25, 0.5, 1.0], device=device)

    def run(a, e):
        lo, hi = int(info[a, 0]), int(info[e - 1, 0] + info[e - 1, 1])
        piece = info[a:e].clone()
        piece[:, 0] -= lo
        m, r = hi - lo, e - a
        outs = [torch.empty(m, device=device) for _ in range(3)] + [torch.empty(r, 3, device=device), torch.empty(r, device=device),
                                                                    torch.empty(r, device=device)]
        _ok(lib.qf_render_from_density(_P(ts[lo:hi].contiguous()), _P(te[lo:hi].contiguous()), _P(sig[lo:hi].contiguous()),
                                       _P(rgbs[lo:hi].contiguous()), _P(piece), r, m, _P(bk), *[_P(t) for t in outs], _st()),
            "qf_render_from_density")
        return tuple(outs)

    _whole_equals_pieces_rays(n_rays, GC.cap_items(row, cu), run, ["weights", "trans", "alphas", "colors", "opacities", "depths"])


def _case_apply_deformation(lib, device, cu):
    row = GC.BY_KEY["apply_deformation"]
    n = GC.past(row, cu)
    g = _gen(8)
    f, xyz, ts = torch.randn(n, generator=g).to(device), torch.randn(n, 3, generator=g).to(device), torch.rand(n, generator=g).to(device)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(device)

    def run(a, e):
        m = e - a
        outs = torch.empty(m, 3, device=device), torch.empty(m, device=device), torch.empty(m, 3, device=device)
        _ok(lib.qf_apply_deformation(_P(f[a:e].contiguous()), 0.04, _P(dirs[a:e].contiguous()), _P(xyz[a:e].contiguous()),
                                     _P(ts[a:e].contiguous()), m, *[_P(t) for t in outs], _st()), "qf_apply_deformation")
        return outs

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["xyz", "ts", "dh"])


def _random_mesh(n_faces, seed, device, bad=True):
    g = _gen(seed)
    n_v = 5003
    v = torch.randn(n_v, 3, generator=g, dtype=torch.float64).to(device)
    f = torch.randint(0, n_v, (n_faces, 3), generator=g)
    f[7] = f[7, 0]                                              # a degenerate face
    if bad:
        f[11, 1], f[n_faces - 2, 2] = n_v, -1                   # ids out of range
    return v, f.to(device), n_v


def _case_vertex_records_pack(lib, device, cu):
    row = GC.BY_KEY["vertex_records"]
    n = GC.past(row, cu)
    v, f, n_v = _random_mesh(n, 9, device)

    def run(a, e):
        rec = torch.zeros(e - a, 128, dtype=torch.uint8, device=device)
        _ok(lib.qf_vertex_records_pack(_P(v), n_v, _P(f[a:e].contiguous()), e - a, _P(rec), _st()), "qf_vertex_records_pack")
        return (rec,)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["records"])


def _case_texel_records_pack(lib, device, cu):
    row = GC.BY_KEY["texel_records"]
    n = GC.past(row, cu)
    v, f, n_v = _random_mesh(n, 10, device, bad=False)
    uv = (torch.rand(n_v, 2, generator=_gen(11)) * 255).to(device)

    def run(a, e):
        rec = torch.zeros(e - a, 128, dtype=torch.uint8, device=device)
        _ok(lib.qf_texel_records_pack(_P(v), _P(f[a:e].contiguous()), _P(uv), e - a, _P(rec), _st()), "qf_texel_records_pack")
        return (rec,)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["records"])


def _case_vertex_shade_points(lib, device, cu, ids32):
    from quadraturefields_amd import utils
    row = GC.BY_KEY["vertex_shade32" if ids32 else "vertex_shade64"]
    n = GC.past(row, cu)
    s, pts, tri, dirs = _frame_samples(device, cu, n)
    tri = tri.to(torch.int32) if ids32 else tri

    def run(a, e):
        rgb, sigma, feats = utils.shade_vertex_baked_points(s["mi"], s["feats"], pts[a:e], tri[a:e], dirs[a:e], want_features=True)
        return rgb, sigma, feats

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["rgb", "sigma", "features"])


def _case_vertex_quant_shade_points(lib, device, cu, ids32):
    from quadraturefields_amd import utils
    from tests import test_gpu_vertex_quant as VQ
    row = GC.BY_KEY["quant_shade32" if ids32 else "quant_shade64"]
    n = GC.past(row, cu)
    s, pts, tri, dirs = _frame_samples(device, cu, n)
    q = VQ._quantised_scene(device, _tile_frame(cu) + (5, 6, "white"), "linear")[1]
    tri = tri.to(torch.int32) if ids32 else tri

    def run(a, e):
        return utils._shade_vertex_quant_points(s["mi"], q, pts[a:e], tri[a:e], dirs[a:e], None, True)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["rgb", "sigma", "features"])


def _case_vertex_quant_decode(lib, device, cu):
    from quadraturefields_amd import baking
    from tests import test_gpu_vertex_quant as VQ
    row, lobes = GC.BY_KEY["quant_decode"], 3
    n = GC.past(row, cu)
    rows = VQ._codec_table(lobes, seed=14)
    table = rows[torch.randint(0, rows.shape[0], (n,), generator=_gen(12))].to(device)
    q = baking.quantise_vertex_features(table, compression_type="sigma", lambda_thres=7.5)
    rec = q.records()[:n]                                       # the records of the asset's square texture, one per vertex first
    assert rec.shape == (n, 64)
    stride = _C().vertex_row_stride(lobes)

    def run(a, e):
        out = torch.full((e - a, stride), float("nan"), device=device)
        _ok(lib.qf_vertex_quant_decode(_P(rec[a:e].contiguous()), e - a, lobes, q.sigmoid_codec, 7.5, _P(out), stride, _st()),
            "qf_vertex_quant_decode")
        return (out,)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["table"])
    assert _same(run(0, n)[0], q.dequantise(padded=True))


def _baked_scene(device, cu):
    from tests import test_gpu_baked_termination as BT
    w, h = _tile_frame(cu)
    return BT._scene(device, w, h, 5, 6, "white", "sigmoid", "extremes"), BT


def _baked_samples(device, cu, n):
    """``n`` ray-major samples of the baked-texture frame of the tile compositor's test."""
    s, BT = _baked_scene(device, cu)
    k = s["mi"]
    xyzs, dirs, _, _, index_tri, _ = k.sampling_raytrace_device(s["d"], s["o"], camera=s["cam"], layout=False)
    assert xyzs.shape[0] >= n
    c = _C()
    return s, BT, c.f32c(xyzs[:n]), index_tri[:n].contiguous(), c.f32c(dirs[:n])


def _case_texel_indices_packed(lib, device, cu):
    from quadraturefields_amd import utils
    row = GC.BY_KEY["texel_indices"]
    n = GC.past(row, cu)
    s, BT, pts, tri, _ = _baked_samples(device, cu, n)
    _whole_equals_pieces(n, GC.cap_items(row, cu), lambda a, e: (utils.texel_indices(s["mi"], s["uv"], pts[a:e], tri[a:e], BT.SIZE),),
                         ["texel"])


def _case_texture_fetch_and_shade_packed(lib, device, cu, which):
    from quadraturefields_amd import utils
    row = GC.BY_KEY[which]
    n = GC.past(row, cu)
    s, BT, pts, tri, dirs = _baked_samples(device, cu, n)
    texel = utils.texel_indices(s["mi"], s["uv"], pts, tri, BT.SIZE)
    comp = s["comp"]
    if which == "texture_fetch":
        _whole_equals_pieces(n, GC.cap_items(row, cu), lambda a, e: (comp.get_features_from_texture_map(texel[a:e]),), ["features"])
    else:
        _whole_equals_pieces(n, GC.cap_items(row, cu), lambda a, e: comp.shade(texel[a:e], dirs[a:e]), ["rgb", "sigma"])


def _case_texture_shade_points(lib, device, cu, ids32):
    from quadraturefields_amd import utils
    row = GC.BY_KEY["texture_shade32" if ids32 else "texture_shade64"]
    n = GC.past(row, cu)
    s, BT, pts, tri, dirs = _baked_samples(device, cu, n)
    tri = tri.to(torch.int32) if ids32 else tri
    _whole_equals_pieces(n, GC.cap_items(row, cu),
                         lambda a, e: utils.shade_baked_points(s["mi"], s["uv"], s["comp"], pts[a:e], tri[a:e], dirs[a:e]),
                         ["rgb", "sigma"])


def _case_bake_encode_texels(lib, device, cu):
    from tests.test_gpu_bake import _planes
    row, lobes = GC.BY_KEY["bake_encode"], 2
    n = GC.past(row, cu)
    t = math.isqrt(n) + 2
    g = _gen(13)
    feats = (torch.randn(n, 3 + 7 * lobes + 1, generator=g) * 3.0).to(device)
    sigma = (torch.rand(n, generator=g) * 400.0).to(device)
    texel = torch.randperm(t * t, generator=g)[:n].to(torch.int32).to(device)
    short = 37                                                   # n_device below the capacity: the last slots are not encoded

    def encode(cuts):
        comp = _planes(t, lobes, 7, device)("sigma", 7.5)
        tex = comp.texture_set()
        for a, e in cuts:
            n_dev = torch.tensor([min(e, n - short) - a], dtype=torch.int64, device=device)
            _ok(lib.qf_bake_encode_texels(ctypes.byref(tex), _P(feats[a:e].contiguous()), feats.shape[1], _P(sigma[a:e].contiguous()),
                                          _P(texel[a:e].contiguous()), e - a, _P(n_dev), _st()), "qf_bake_encode_texels")
        return [comp.alpha, comp.diffuse] + [comp.sg_colors[l] for l in range(lobes)] + [comp.lambdas[l] for l in range(lobes)]

    assert n > GC.cap_items(row, cu)
    whole, pieces = encode([(0, n)]), encode(_cuts(n, GC.cap_items(row, cu) // 2))
    assert all(torch.equal(a, b) for a, b in zip(whole, pieces))
    flat = whole[0].reshape(-1)
    assert bool((flat[texel[-short:].long()] == 7).all()) and float((flat != 7).float().mean()) > 0.5


def _case_grid_encode(lib, device, cu):
    row = GC.BY_KEY["grid_encode"]
    n = -(-GC.past(row, cu) // 16)
    c = _C()
    desc = c.make_grid_desc(16, 14, 16, 1.4472692012786865)
    table = ((torch.rand(int(desc.offset[16]), 2, generator=_gen(14)) * 2 - 1) * 1e-1).to(device)
    x = torch.rand(n, 3, generator=_gen(15))
    x[::50] = torch.tensor([0.0, 1.0, 0.5])
    x = x.to(device)

    def run(a, e):
        out = torch.empty(e - a, 32, device=device)
        _ok(lib.qf_grid_encode(ctypes.byref(desc), _P(table), _P(x[a:e].contiguous()), e - a, _P(out), _st()), "qf_grid_encode")
        return (out,)

    assert n * 16 > GC.cap_items(row, cu)
    whole = run(0, n)
    parts = [run(a, e) for a, e in _cuts(n, GC.cap_items(row, cu) // 2 // 16)]
    assert _same(whole[0], torch.cat([p[0] for p in parts])) and bool(whole[0].abs().sum() > 0)


def _case_sg_features_to_rgb(lib, device, cu):
    row, lobes = GC.BY_KEY["sg_features_to_rgb"], 3
    n, stride = GC.past(row, cu), 3 + 7 * 3 + 1
    g = _gen(16)
    feats = torch.randn(n, stride, generator=g).to(device)
    dirs = torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).to(device)

    def run(a, e):
        rgb = torch.empty(e - a, 3, device=device)
        _ok(lib.qf_sg_features_to_rgb(_P(feats[a:e].contiguous()), stride, _P(dirs[a:e].contiguous()), e - a, lobes, _P(rgb), _st()),
            "qf_sg_features_to_rgb")
        return (rgb,)

    _whole_equals_pieces(n, GC.cap_items(row, cu), run, ["rgb"])


def _case_frame_images_u8(lib, device, cu):
    row = GC.BY_KEY["frame_images_u8"]
    n_pix = -(-GC.past(row, cu) // 3)
    g = _gen(17)
    rgb = (torch.rand(n_pix, 3, generator=g) * 1.2 - 0.1).to(device)
    pix, depth = torch.rand(n_pix, 3, generator=g).to(device), (torch.rand(n_pix, generator=g) * 4.0).to(device)
    record = torch.tensor([0.0, 0.0, 0.0, 4.5], dtype=torch.float64, device=device)

    def run(a, e):                                              # rows of a one-pixel-wide image
        m = e - a
        outs = (torch.empty(m, 3, dtype=torch.uint8, device=device), torch.empty(m, 3, dtype=torch.uint8, device=device),
                torch.empty(m, dtype=torch.uint8, device=device))
        _ok(lib.qf_frame_images_u8(_P(rgb[a:e].contiguous()), _P(pix[a:e].contiguous()), _P(depth[a:e].contiguous()), _P(record), m, 1,
                                   *[_P(t) for t in outs], _st()), "qf_frame_images_u8")
        return outs

    assert 3 * n_pix > GC.cap_items(row, cu)
    whole = run(0, n_pix)
    parts = [run(a, e) for a, e in _cuts(n_pix, GC.cap_items(row, cu) // 2 // 3)]
    for k in range(3):
        assert torch.equal(whole[k], torch.cat([p[k] for p in parts])), k
    assert int(whole[2].max()) > 200 and int(whole[0].max()) == 255


def _case_mark_hit_faces(lib, device, cu):
    row, k, n_faces = GC.BY_KEY["mark_hit_faces"], 5, 30011
    n_rays = -(-GC.past(row, cu) // k)
    g = _gen(18)
    tri = torch.randint(0, 20000, (n_rays, k), generator=g, dtype=torch.int32)     # the faces 20 000.. are never hit
    tri[torch.rand(n_rays, k, generator=g) < 0.01] = n_faces + 5
    count = torch.randint(0, k + 2, (n_rays,), generator=g, dtype=torch.int32)
    tri, count = tri.to(device), count.to(device)

    def run(a, e):
        mask = torch.zeros(n_faces, dtype=torch.uint8, device=device)
        bad = torch.zeros(1, dtype=torch.int64, device=device)
        _ok(lib.qf_mark_hit_faces(_P(tri[a:e].contiguous()), _P(count[a:e].contiguous()), e - a, k, n_faces, _P(mask), _P(bad), _st()),
            "qf_mark_hit_faces")
        return mask, int(bad)

    assert n_rays * k > GC.cap_items(row, cu)
    mask, bad = run(0, n_rays)
    parts = [run(a, e) for a, e in _cuts(n_rays, GC.cap_items(row, cu) // 2 // k)]
    considered = torch.arange(k, device=device)[None] < count.clamp(max=k)[:, None]
    assert torch.equal(mask, torch.stack([p[0] for p in parts]).amax(dim=0))
    assert bad == sum(p[1] for p in parts) == int((considered & (tri >= n_faces)).sum()) > 100
    assert not bool(mask[20000:].any()) and int(mask.sum()) > 10000


def _case_resort_by_depth(lib, device, cu):
    row = GC.BY_KEY["resort"]
    n = GC.past(row, cu)
    counts = torch.randint(0, 6, (n,), generator=_gen(19))
    ridx = torch.repeat_interleave(torch.arange(n), counts)[:n].contiguous()
    assert ridx.shape[0] == n
    depth = torch.rand(n, generator=_gen(20))
    ridx_d, depth_d = ridx.to(device), depth.to(device)
    first = torch.cat([torch.tensor([True]), ridx[1:] != ridx[:-1]]).nonzero().flatten()      # pieces end where a ray ends

    def run(a, e):
        perm = torch.empty(e - a, dtype=torch.int64, device=device)
        _ok(lib.qf_resort_by_depth(_P(ridx_d[a:e].contiguous()), _P(depth_d[a:e].contiguous()), e - a, _P(perm), _st()),
            "qf_resort_by_depth")
        return perm + a

    cap = GC.cap_items(row, cu)
    assert n > cap
    whole = run(0, n)
    edges = [0] + [int(first[torch.searchsorted(first, b)]) for _, b in _cuts(n, cap // 2 - 8)[:-1]] + [n]
    assert max(b - a for a, b in zip(edges, edges[1:])) <= cap // 2
    assert torch.equal(whole, torch.cat([run(a, e) for a, e in zip(edges, edges[1:])]))
    # ... and the order itself: by ray, then by depth
    assert np.array_equal(whole.cpu().numpy(), np.lexsort((depth.numpy(), ridx.numpy())))


_WHOLE_CASES = {
    "mark_pack_boundaries": _case_mark_pack_boundaries,
    "exponential_integration": _case_exponential_integration,
    "exclusive_scan": _case_exclusive_scan,
    "render_from_density": _case_render_from_density,
    "apply_deformation": _case_apply_deformation,
    "vertex_records_pack": _case_vertex_records_pack,
    "texel_records_pack": _case_texel_records_pack,
    "vertex_shade_points-int32": lambda *a: _case_vertex_shade_points(*a, True),
    "vertex_shade_points-int64": lambda *a: _case_vertex_shade_points(*a, False),
    "vertex_quant_shade_points-int32": lambda *a: _case_vertex_quant_shade_points(*a, True),
    "vertex_quant_shade_points-int64": lambda *a: _case_vertex_quant_shade_points(*a, False),
    "vertex_quant_decode": _case_vertex_quant_decode,
    "texel_indices_packed": _case_texel_indices_packed,
    "texture_fetch": lambda *a: _case_texture_fetch_and_shade_packed(*a, "texture_fetch"),
    "texture_shade_packed": lambda *a: _case_texture_fetch_and_shade_packed(*a, "texture_shade_packed"),
    "texture_shade_points-int32": lambda *a: _case_texture_shade_points(*a, True),
    "texture_shade_points-int64": lambda *a: _case_texture_shade_points(*a, False),
    "bake_encode_texels": _case_bake_encode_texels,
    "grid_encode": _case_grid_encode,
    "sg_features_to_rgb": _case_sg_features_to_rgb,
    "frame_images_u8": _case_frame_images_u8,
    "mark_hit_faces": _case_mark_hit_faces,
    "resort_by_depth": _case_resort_by_depth,
}


@pytest.mark.parametrize("name", list(_WHOLE_CASES))
def test_whole_equals_pieces(lib, device, cu, name):
    """Per-item kernels past their cap: the whole batch equals, bit for bit, the concatenation of the same call on
    consecutive pieces of at most cap / 2 items (indices and offsets rebased by the case)."""
    _WHOLE_CASES[name](lib, device, cu)


def test_texture_pack_past_the_cap(lib, device, cu):
    """A texture of more texels than one sweep, tiled from a 64 x 64 one: every record equals the small texture's record
    of the same texel -- the kernel below its cap -- byte for byte."""
    from quadraturefields_amd import synthetic
    from quadraturefields_amd.texture_utils import FeatureCompression
    row, lobes, t = GC.BY_KEY["texture_pack"], 3, 64
    reps = -(-(math.isqrt(GC.past(row, cu)) + 1) // t)
    big = t * reps
    assert big * big > GC.cap_items(row, cu)
    tex = synthetic.random_textures(t, lobes, seed=3)
    tile = lambda p: np.tile(p, (reps, reps) + (1,) * (p.ndim - 2))                          # noqa: E731
    make = lambda f: FeatureCompression.from_arrays(f(tex["alpha"]), f(tex["diffuse"]), [f(p) for p in tex["colors"]],      # noqa: E731
                                                    [f(p) for p in tex["lambdas"]], compression_type="sigmoid", lambda_thres=7.5,
                                                    device=device)
    small, whole = make(lambda p: p).records(), make(tile).records()
    assert whole.shape == (big * big, 64)
    r = torch.arange(big, device=device)
    src = ((r % t)[:, None] * t + (r % t)[None, :]).reshape(-1)
    assert torch.equal(whole, small[src])


def test_generate_rays_past_the_cap(device, cu):
    """qf_generate_rays on more pixels than one sweep, at the bars of test_generate_rays_with_general_intrinsics: origins
    exact, directions within 1.2e-7 of the host arithmetic."""
    from tests import asymmetric_inputs as asym
    row = GC.BY_KEY["generate_rays"]
    w = math.isqrt(GC.past(row, cu)) | 1
    h = -(-GC.past(row, cu) // w)
    assert w * h > GC.cap_items(row, cu)
    c = _C()
    for opengl in (True, False):
        cam, c2w, k = asym.general_camera(w, h)
        o = torch.full((w * h, 3), float("nan"), device=device)
        d = torch.full((w * h, 3), float("nan"), device=device)
        _ok(c.lib().qf_generate_rays(ctypes.byref(cam), 1 if opengl else 0, _P(o), _P(d), _st()), "qf_generate_rays")
        o_t, d_t = asym.rays_from_k(c2w, *k, w, h, opengl=opengl)
        assert torch.equal(o.cpu(), o_t)
        assert torch.allclose(d.cpu(), d_t, rtol=0, atol=1.2e-7), float((d.cpu() - d_t).abs().max())


def test_segment_sums_against_reduceat(lib, device, cu):
    """qf_pack_info (exact), qf_sum_reduce and qf_accumulate_along_rays on more rays x channels than one sweep against
    ``np.add.reduceat`` in fp64, at the bar of tests/test_gpu_composite.py (``_close``: atol 1e-6, rtol 1e-5)."""
    from tests.test_gpu_composite import _close
    c = 4
    n_rays = max(GC.past(GC.BY_KEY["pack_info"], cu), -(-GC.past(GC.BY_KEY["sum_reduce"], cu) // c))
    assert n_rays > GC.cap_items(GC.BY_KEY["pack_info"], cu) and n_rays * c > GC.cap_items(GC.BY_KEY["accumulate"], cu)
    counts, starts, n = _segments(n_rays, 21, longest=4)
    ridx = torch.repeat_interleave(torch.arange(n_rays), counts).contiguous()
    g = _gen(22)
    wts, vals = torch.rand(n, generator=g), torch.rand(n, c, generator=g)
    info = torch.full((n_rays, 2), -1, dtype=torch.int64, device=device)
    _ok(lib.qf_pack_info(_P(ridx.to(device)), n, n_rays, _P(info), _st()), "qf_pack_info")
    assert torch.equal(info[:, 1].cpu(), counts)
    assert torch.equal(info[:, 0].cpu()[counts > 0], starts[counts > 0])

    def reduceat(x):                                            # fp64 sums per ray; empty rays give 0
        return torch.from_numpy(GC.segment_sums(x.numpy(), starts.numpy(), counts.numpy()))

    out = torch.full((n_rays, c), float("nan"), device=device)
    _ok(lib.qf_accumulate_along_rays(_P(wts.to(device)), _P(vals.to(device)), c, _P(info), n_rays, n, _P(out), _st()),
        "qf_accumulate_along_rays")
    _close(out, reduceat(wts[:, None] * vals).float())
    one = torch.full((n_rays, 1), float("nan"), device=device)
    _ok(lib.qf_accumulate_along_rays(_P(wts.to(device)), None, 1, _P(info), n_rays, n, _P(one), _st()), "qf_accumulate_along_rays")
    _close(one, reduceat(wts[:, None]).float())
    # sum_reduce takes the first sample of every non-empty segment
    seg = starts[counts > 0].contiguous()
    n_seg = seg.shape[0]
    assert n_seg * c > GC.cap_items(GC.BY_KEY["sum_reduce"], cu)
    red = torch.full((n_seg, c), float("nan"), device=device)
    _ok(lib.qf_sum_reduce(_P(vals.to(device)), c, _P(seg.to(device)), n_seg, n, _P(red), _st()), "qf_sum_reduce")
    _close(red, reduceat(vals)[counts > 0].float())


def test_derive_properties_fills_every_ray(lib, device, cu):
    """fill_background_kernel on more rays than one sweep: every ray without a sample holds the background."""
    from quadraturefields_amd import utils
    n_rays = GC.past(GC.BY_KEY["fill_background"], cu)
    ridx = torch.tensor([3, 3, n_rays - 1], device=device)
    rgb, alpha, _, depth, _ = utils.derive_properties(torch.full((3, 3), 0.5, device=device), torch.full((3,), 1e4, device=device),
                                                       torch.tensor([1.0, 2.0, 3.0], device=device), 5e-3, None, ridx, bg_color="white",
                                                       N=n_rays)
    hit = torch.zeros(n_rays, dtype=torch.bool, device=device)
    hit[ridx] = True
    assert n_rays > GC.cap_items(GC.BY_KEY["fill_background"], cu)
    assert bool((rgb[~hit] == 1.0).all()) and not bool(alpha[~hit].any()) and not bool(depth[~hit].any())
    assert torch.allclose(rgb[hit], torch.full((2, 3), 0.5, device=device), atol=1e-6) and bool((alpha[hit] > 0.999).all())


@pytest.mark.parametrize("maximize", [False, True])
def test_adam_past_the_cap(device, cu, maximize):
    """qf_adam_step on more floats than 16 x 256 x 4 x CU with n % 4 == 3, two steps, against torch.optim.Adam at the bar of
    test_fused_adam_is_torch_adam (rtol 2e-6, atol 1e-7)."""
    from quadraturefields_amd.optim import Adam
    row = GC.BY_KEY["adam"]
    n = GC.past(row, cu)
    n += (3 - n) % 4
    assert n % 4 == 3 and n > GC.cap_items(row, cu)
    g = torch.Generator(device=device).manual_seed(3)
    init = torch.randn(n, generator=g, device=device)
    pa, pb = torch.nn.Parameter(init.clone()), torch.nn.Parameter(init.clone())
    kwargs = dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=0.01, maximize=maximize)
    oa, ob = Adam([pa], **kwargs), torch.optim.Adam([pb], **kwargs)
    for _ in range(2):
        gr = torch.randn(n, generator=g, device=device)
        gr[::7] = 0.0
        pa.grad, pb.grad = gr.clone(), gr.clone()
        oa.step()
        ob.step()
    assert torch.allclose(pa, pb, rtol=2e-6, atol=1e-7), float((pa - pb).abs().max())
    assert float((pa - init).abs().min()) >= 0.0 and float((pa[-3:] - init[-3:]).abs().min()) > 0.0      # the tail moved


def test_split_layout_past_the_cap(lib, device, cu):
    """split_rays_kernel on more rays than one sweep: the per-ray counts and offsets of qf_split_layout against bincount and
    cumsum, exactly; the order and its inverse are permutations of each other."""
    need = GC.past(GC.BY_KEY["split_rays"], cu)
    w = math.isqrt(need) | 1
    h = -(-need // w)
    n_rays = w * h
    assert n_rays + 1 > GC.cap_items(GC.BY_KEY["split_rays"], cu) and w % 8 and n_rays < 2 ** 31
    counts, starts, n = _segments(n_rays, 23)
    index_ray = torch.repeat_interleave(torch.arange(n_rays), counts).contiguous().to(device)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    hit_count = torch.full((n_rays,), -1, dtype=torch.int32, device=device)
    ray_offset = torch.full((n_rays + 1,), -1, dtype=torch.int64, device=device)
    tile_base = torch.full((tiles,), -1, dtype=torch.int64, device=device)
    invalid = torch.full((1,), 7, dtype=torch.int32, device=device)
    order, inverse = (torch.full((n,), -1, dtype=torch.int32, device=device) for _ in range(2))
    _ok(lib.qf_split_layout(_P(index_ray), n, w, h, _P(hit_count), _P(ray_offset), _P(tile_base), _P(invalid), _P(order), _P(inverse),
                            _st()), "qf_split_layout")
    assert int(invalid) == 0
    assert torch.equal(hit_count.cpu(), counts.to(torch.int32))
    assert torch.equal(ray_offset.cpu(), torch.cat([starts, torch.tensor([n])]))
    assert int(tile_base[0]) == 0 and bool((tile_base[1:] >= tile_base[:-1]).all()) and int(tile_base[-1]) <= n
    arange = torch.arange(n, dtype=torch.int32, device=device)
    assert torch.equal(inverse[order.long()], arange) and torch.equal(torch.sort(order).values, arange)


_big = {}


def _big_mesh(cu):
    """Nested shells of 81 920 faces each, more faces than 2048 CU (737 280 at 256 CUs): built once."""
    from quadraturefields_amd import synthetic
    if "mesh" not in _big:
        shells = -(-GC.past(GC.BY_KEY["bvh_morton_keys"], cu) // 81920)
        _big["mesh"] = synthetic.shell_mesh(n_shells=shells, subdivisions=6)
    return _big["mesh"]


def _bvh_lists(lib, ri, o, d, k, width=0):
    n = o.shape[0]
    width = width or n
    tri = torch.full((n, k), -7, dtype=torch.int32, device=o.device)
    t = torch.full((n, k), float("nan"), device=o.device)
    cnt = torch.full((n,), -7, dtype=torch.int32, device=o.device)
    _ok(lib.qf_bvh_intersect(ri._handle, _P(o), _P(d), n, k, width, _P(tri), _P(t), _P(cnt), _st()), "qf_bvh_intersect")
    return tri, t, cnt


def test_device_bvh_past_the_cap(lib, device, cu):
    """The device BVH build (morton_keys_kernel, gather_tris_kernel) and the device refit (refit_tris_kernel) on more
    triangles than one sweep: the hit lists of 20 000 rays equal those of the host-built, host-refitted BVH bit for bit
    (both return the K nearest hits in (t, triangle) order), and the build's triangle order is a permutation."""
    from quadraturefields_amd.mesh_io import TriMesh
    from quadraturefields_amd.mesh_utils import RayIntersector
    from tests import test_gpu_bvh_device_build as DB
    mesh = _big_mesh(cu)
    n_tri, k = mesh.faces.shape[0], 5
    assert n_tri > GC.cap_items(GC.BY_KEY["bvh_morton_keys"], cu)
    plain = TriMesh(np.asarray(mesh.vertices), np.asarray(mesh.faces))
    dev = RayIntersector(plain, max_hits=k, min_separation=0, builder="device")
    host = RayIntersector(plain, max_hits=k, min_separation=0, builder="host")
    ids = np.full(n_tri, -1, dtype=np.int32)
    assert lib.qf_bvh_copy_tri_ids(dev._handle, ids.ctypes.data_as(ctypes.c_void_p), n_tri) == 0
    assert np.array_equal(np.sort(ids), np.arange(n_tri, dtype=np.int32))
    o, d = (torch.from_numpy(a).to(device) for a in DB._special_rays(20000, seed=3))
    moved = np.asarray(mesh.vertices, dtype=np.float32) * np.array([0.9, 1.1, 1.0], np.float32) + np.array([0.05, 0.0, -0.05], np.float32)
    for step in ("build", "refit"):
        if step == "refit":
            dev.update_intersector(torch.from_numpy(moved).to(device))       # on the device: refit_tris_kernel
            host.update_intersector(moved)                                   # on the host
        got, want = _bvh_lists(lib, dev, o, d, k), _bvh_lists(lib, host, o, d, k)
        assert torch.equal(got[2], want[2]) and int(got[2].sum()) > 20000, step
        valid = torch.arange(k, device=device)[None] < got[2].clamp(max=k)[:, None]
        assert torch.equal(got[0][valid], want[0][valid]) and _same(got[1][valid], want[1][valid]), step


def test_uv_atlas_histogram_past_the_cap(device, cu):
    """histogram_kernel on more faces than one sweep: the class counts of the per-triangle atlas equal the bincount of the
    classes the faces were given (written by another launch, one thread per face)."""
    from quadraturefields_amd import uv_atlas
    from quadraturefields_amd.mesh_io import TriMesh
    mesh = _big_mesh(cu)
    n_f = mesh.faces.shape[0]
    assert n_f > GC.cap_items(GC.BY_KEY["uv_histogram"], cu)
    _, info = uv_atlas.per_triangle_atlas(TriMesh(np.asarray(mesh.vertices), np.asarray(mesh.faces)), 4096)
    classes = info.face_class.cpu().numpy()
    counts = np.asarray(info.class_counts)
    print(f"atlas of {n_f} faces: rho {info.rho:.4g}, classes {np.flatnonzero(counts).tolist()}")
    assert counts.sum() == n_f and np.array_equal(np.bincount(classes, minlength=counts.shape[0]), counts)
    assert (counts > 0).sum() >= 2


def _raster_mesh_key(cu, n_rays):
    """Shells of 20 480 faces: the fewest whose chunk list (n_tri * lanes / 256 workgroups) is longer than 8 CU."""
    from tests import test_gpu_raster_passes as RP
    for shells in range(1, 40):
        n_tri = shells * 20480
        if n_tri * RP.raster_lanes(n_rays, n_tri) // 256 > 8 * cu * 11 // 10:
            return (shells, 5), n_tri
    raise AssertionError("no mesh")


@pytest.mark.parametrize("route", ["plain", "culled", "slabs"])
def test_camera_passes_past_the_cap(lib, device, cu, route):
    """The camera-coherent passes on a frame of more rays than 2048 CU (camera_rays_check_kernel on the pass without a cull
    launch, slab_ray_records_kernel between the slabs) and a mesh whose chunk list is longer than the 8 CU resident
    workgroups of the culled and the slab pass: no overflow, no ray flag, and every ray's hits -- sorted by (t, triangle)
    -- equal qf_bvh_intersect's, bit for bit, without the repair launch."""
    from tests import test_gpu_raster_passes as RP
    w, h = _tile_frame(cu)
    key, n_tri = _raster_mesh_key(cu, w * h)
    assert w * h > GC.cap_items(GC.BY_KEY["camera_rays_check"], cu)
    k = 25                                                       # a ray crosses the shells 2 x 8 times, a grazing one more often
    if ("view", w, h) not in _big:
        _big["view", w, h] = RP._view("orbit", focal_scale=w / 96.0, w=w, h=h)
    view, ri = _big["view", w, h], RP._ri(key)
    assert view.n == w * h and ri.mesh.faces.shape[0] == n_tri
    if route == "slabs":
        out = RP._call(lib, ri, view, k, "slabs", wide=k + 7, slabs=2)
    else:
        out = RP._call(lib, ri, view, k, "plain", cull=int(route == "culled"))
    assert out.flag == 0
    o, d = RP._dev_rays(view, device)
    tri_b, t_b, cnt_b = _bvh_lists(lib, ri, o, d, k, width=w)
    full = cnt_b < k                                             # every hit of the ray fits: the pass answers it by itself
    print(f"{route}: {w}x{h} rays, {n_tri} triangles, {int(cnt_b.sum())} hits, longest list {int(cnt_b.max())}, overflow {out.overflow}")
    assert float(full.float().mean()) > 0.99 and int(cnt_b.sum()) > w * h
    assert torch.equal(out.dev.cnt[full], cnt_b[full]) and (out.overflow == 0 or not bool(full.all()))

    def keys(t, tri, cnt):
        valid = torch.arange(k, device=device)[None] < cnt[:, None]
        key64 = (t.contiguous().view(torch.int32).to(torch.int64) << 32) | tri.to(torch.int64)
        return torch.sort(torch.where(valid, key64, torch.full_like(key64, 2 ** 62)), dim=1).values

    assert torch.equal(keys(out.dev.t, out.dev.tri, out.dev.cnt)[full], keys(t_b, tri_b, cnt_b)[full])
    valid = torch.arange(k, device=device)[None] < cnt_b[:, None]
    assert bool((out.dev.tri[full][~valid[full]] == RP.SENT_TRI).all())      # no slot behind a ray's hits was written
