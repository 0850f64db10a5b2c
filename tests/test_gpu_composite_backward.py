"""The per-ray compositing kernels of csrc/composite.hip against the float64 reference of tests/composite_reference.py:
``qf_derive_properties_backward`` over the whole optical-depth range, and the forward kernels at the same inputs.

One generator (``composite_reference.make_case``) feeds everything.  Families: mild tau (<= 0.24); one spike of tau =
250, 1.6e4, 1e6 or the largest finite fp32 number, first, in the middle or last on the ray; several spikes on one ray;
sigma = +inf (with delta > 0: inf * 0 is outside the domain of the kernels and is not a case); rays without density;
tau ~ 1e-8 (1 - expf(-tau) = 0 in fp32, grad_sigma = gw T delta is not); delta = 0 samples; ray lengths 1, 2, 25, 64,
400, 2 500; empty rays between the others (every family); ray ids < 0 and >= n_rays; one sample; and more samples than
one sweep of the backward kernel's grid (2048 x compute units) plus a ragged tail, with a ray across the boundary.
Each with the four background modes.  Outputs are pre-filled with NaN and carry spare rows that must stay NaN.

Assertion: |got - ref| <= bar u M for every element of every gradient (u = 2^-24, M the reference's sum of term
magnitudes, floored per ray at 2^-20 of its maximum and at 2^-102, the fp32 underflow limit); nothing is excluded.  For sigma = +inf additionally: all finite,
and exactly zero grad_color / grad_depth behind the opaque sample.

Bars.  The prefix-kept fp32 restatement of the algorithm (numpy, on the host; it measures the arithmetic, never the
kernel) has these worst ratios against float64 over all families and modes, and each bar is 4 x that, rounded up to a
power of two (device expf within 1-2 ulp of numpy's, contraction of the backward's products and sums):

    quantity        restatement   bar     kernels, MI355X (this commit)
    grad_color      2.49          16      1.48
    grad_sigma      3.13          16      2.56
    grad_depth      2.46          16      1.31
    weights         2.12          16      0.96
    rgb             2.10          16      1.32
    alpha           0.88           4      0.46
    depth           0.90           4      0.45
    trans           2.17          16      0.99
    alphas          1.08           8      0.51
    depth_norm      0.31           2      0.31
    weights_incl    1.16           8      0.60   (qf_exponential_integration, exclusive = 0)
    feats_incl      0.87           4      0.53

Before this commit the backward kernel rebuilt each sample's exclusive optical depth as ``cum -= tau`` from the ray's
total.  That kernel, on the same cases, failed every spike family and the multi, lengths, outside, big and +inf
families (72 of the 96 backward and route tests).  Its worst ratios, grad_color / grad_sigma / grad_depth: spike 250
125 / 43 / 126; spike 1.6e4 7.9e3 / 1.2e3 / 7.6e3; spike 1e6 4.9e5 / 1.5e5 / 4.9e5; largest finite tau 6.0e7 / 1.5e7 /
6.0e7; through ``rendering`` 4.9e5 / 8.2e4; and for sigma = +inf NaN in 2 280 of 3 454 grad_sigma values (every sample
in front of an opaque one).  Mild, zero, tiny, zero_delta and single measured the same on both kernels (<= 2.6).
"""
import os

import numpy as np
import pytest
import torch

from tests import composite_reference as R

pytestmark = pytest.mark.gpu

SPARE = 16
NAN = float("nan")
MODES = (R.BG_WHITE, R.BG_BLACK, R.BG_CUSTOM, R.BG_NONE)
GRADS = ("grad_color", "grad_sigma", "grad_depth")


def _report(kind, case, name, value):
    """One line per measured maximum of err / (u M); collected into the pull request's numbers."""
    print(f"ERR_RATIO {kind} {case} {name} {value:.3g}")
    path = os.environ.get("QF_ERR_RATIO_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{kind} {case} {name} {value:.6g}\n")


def _p(t, dtype=None):
    from quadraturefields_amd import _C
    return _C.ptr(t) if dtype is None else _C.ptr(t, dtype)


def _dev(case, device):
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(device)
         for k in ("sigma", "delta", "rgb", "depth", "index_ray", "g_rgb", "g_alpha", "g_depth")}
    t["bkgd"] = torch.tensor(R.BKGD, dtype=torch.float32, device=device)
    return t


def _nan(rows, cols, device):
    shape = (rows + SPARE,) if cols == 0 else (rows + SPARE, cols)
    return torch.full(shape, NAN, dtype=torch.float32, device=device)


def run_backward(lib, case, t, mode, g_alpha=True, g_depth=True, grad_depth=True, delta_const=None):
    from quadraturefields_amd import _C
    n, dev = len(case["sigma"]), t["sigma"].device
    gc, gs = _nan(n, 3, dev), _nan(n, 0, dev)
    gd = _nan(n, 0, dev) if grad_depth else None
    _C.check(lib.qf_derive_properties_backward(
        _p(t["rgb"]), _p(t["sigma"]), _p(t["depth"]), None if delta_const is not None else _p(t["delta"]),
        0.0 if delta_const is None else float(delta_const), _p(t["index_ray"]), n, int(case["n_rays"]), mode,
        _p(t["bkgd"]) if mode == R.BG_CUSTOM else None, _p(t["g_rgb"]), _p(t["g_alpha"]) if g_alpha else None,
        _p(t["g_depth"]) if g_depth else None, _p(gc), _p(gs), _p(gd), _C.stream()), "qf_derive_properties_backward")
    torch.cuda.synchronize()
    return {"grad_color": gc, "grad_sigma": gs, "grad_depth": gd}


def check(kind, label, names, got, ref, rows, bars=R.BARS, bar_names=None):
    """Rows < n within the bar, spare rows untouched; returns the worst ratios."""
    worst = {}
    for i, name in enumerate(names):
        g = got[name]
        if g is None:
            continue
        assert bool(torch.isnan(g[rows[name]:]).all()), f"{kind} {label}: {name} wrote past its last row"
        val, mag = ref[name]
        r = R.err_ratio(g[:rows[name]].cpu().numpy(), val, mag)
        worst[name] = float(r.max(initial=0.0))
        _report(kind, label, name, worst[name])
    for i, name in enumerate(worst):
        bar = bars[bar_names[name] if bar_names else name]
        assert worst[name] <= bar, (kind, label, name, worst[name], bar)
    return worst


def _behind_opaque(case):
    starts, counts, _ = R.ray_runs(case["index_ray"])
    inf = np.isinf(case["sigma"])
    seen = np.zeros(len(inf), dtype=bool)
    for s, c in zip(starts, counts):
        seen[s:s + c] = np.cumsum(inf[s:s + c]) - inf[s:s + c] > 0
    return seen


@pytest.fixture(scope="module")
def stride(lib, device):
    cu = lib.qf_device_cu_count()
    assert cu > 0
    return 2048 * cu


_cases = {}


def _case(family, stride, device):
    if family not in _cases:
        _cases.clear()                                    # one family's tensors at a time
        case = R.make_case(family, stride=stride)
        _cases[family] = (case, _dev(case, device))
    return _cases[family]


# ------------------------------------------------------------------------------------------------------- backward
@pytest.mark.parametrize("mode", MODES, ids=[R.BG_NAMES[m] for m in MODES])
@pytest.mark.parametrize("family", R.FAMILIES)
def test_backward_vs_fp64(lib, device, stride, family, mode):
    case, t = _case(family, stride, device)
    n = len(case["sigma"])
    if family == "big":
        starts, counts, _ = R.ray_runs(case["index_ray"])
        assert n > stride and n % 256 != 0 and bool(((starts < stride) & (starts + counts > stride)).any())
    got = run_backward(lib, case, t, mode)
    ref = R.reference(case, mode, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"])
    rows = {k: n for k in GRADS}
    if family == "inf":                                   # finite first: the ratios below would only say "inf"
        for k in GRADS:
            bad = int((~torch.isfinite(got[k][:n])).sum())
            _report("backward", f"inf-{R.BG_NAMES[mode]}", f"{k}_nonfinite", bad)
        for k in GRADS:
            assert bool(torch.isfinite(got[k][:n]).all()), (k, "not finite for sigma = +inf")
        behind = torch.from_numpy(_behind_opaque(case)).to(device)
        assert int(behind.sum()) > 100
        assert not bool(got["grad_color"][:n][behind].any()) and not bool(got["grad_depth"][:n][behind].any())
    if family == "outside":
        out = torch.from_numpy((case["index_ray"] < 0) | (case["index_ray"] >= case["n_rays"])).to(device)
        assert int(out.sum()) > 50
        for k in GRADS:
            assert not bool(got[k][:n][out].any()), (k, "gradient on a ray id outside the image")
    check("backward", f"{family}-{R.BG_NAMES[mode]}", GRADS, got, ref, rows)


@pytest.mark.parametrize("mode", (R.BG_WHITE, R.BG_NONE), ids=["white", "none"])
def test_backward_optional_pointers(lib, device, stride, mode):
    """g_alpha NULL, g_depth NULL and grad_depth NULL; a deltas tensor and the equal delta_const give the same bits."""
    case, t = _case("spike-1e6-mid", stride, device)
    n = len(case["sigma"])
    rows = {k: n for k in GRADS}
    full = run_backward(lib, case, t, mode)
    for ga, gd in ((False, True), (True, False), (False, False)):
        got = run_backward(lib, case, t, mode, g_alpha=ga, g_depth=gd)
        ref = R.reference(case, mode, R.BKGD, case["g_rgb"], case["g_alpha"] if ga else None, case["g_depth"] if gd else None)
        check("backward", f"null-alpha{int(not ga)}-depth{int(not gd)}-{R.BG_NAMES[mode]}", GRADS, got, ref, rows)
        if not gd:
            assert not bool(got["grad_depth"][:n].any())
    got = run_backward(lib, case, t, mode, grad_depth=False)
    assert got["grad_depth"] is None
    assert torch.equal(got["grad_color"][:n], full["grad_color"][:n]) and torch.equal(got["grad_sigma"][:n], full["grad_sigma"][:n])
    assert case["delta_const"] == R.DELTA and bool((t["delta"] == R.DELTA).all())
    const = run_backward(lib, case, t, mode, delta_const=R.DELTA)
    for k in GRADS:
        assert torch.equal(const[k][:n], full[k][:n]), k


def _leaf(x):
    return x.clone().requires_grad_(True)


@pytest.mark.parametrize("bg", ["white", "black", "custom"])
@pytest.mark.parametrize("family", ["spike-1e6-mid", "inf"])
def test_derive_properties_under_autograd(lib, device, stride, family, bg):
    from quadraturefields_amd import utils
    case, t = _case(family, stride, device)
    n, n_rays = len(case["sigma"]), int(case["n_rays"])
    mode = {"white": R.BG_WHITE, "black": R.BG_BLACK, "custom": R.BG_CUSTOM}[bg]
    with torch.enable_grad():
        c, s, d = _leaf(t["rgb"]), _leaf(t["sigma"]), _leaf(t["depth"])
        rgb, alpha, _, depth, _ = utils.derive_properties(c, s, d, t["delta"], None, t["index_ray"], render_bkgd=t["bkgd"],
                                                          bg_color=bg, N=n_rays)
        torch.autograd.backward([rgb, alpha, depth], [t["g_rgb"], t["g_alpha"][:, None], t["g_depth"][:, None]])
    ref = R.reference(case, mode, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"])
    got = {"grad_color": torch.cat([c.grad, _nan(0, 3, device)]), "grad_sigma": torch.cat([s.grad, _nan(0, 0, device)]),
           "grad_depth": torch.cat([d.grad, _nan(0, 0, device)])}
    assert all(bool(torch.isfinite(g[:n]).all()) for g in got.values())
    check("autograd", f"{family}-{bg}", GRADS, got, ref, {k: n for k in GRADS})
    fwd = {"rgb": torch.cat([rgb.detach(), _nan(0, 3, device)]), "alpha": torch.cat([alpha.detach().reshape(-1), _nan(0, 0, device)]),
           "depth": torch.cat([depth.detach().reshape(-1), _nan(0, 0, device)])}
    check("autograd", f"{family}-{bg}", ("rgb", "alpha", "depth"), fwd, ref, {k: n_rays for k in fwd})


@pytest.mark.parametrize("bkgd", [None, R.BKGD], ids=["nobkgd", "bkgd"])
def test_rendering_training_branch_vs_fp64(lib, device, stride, bkgd):
    """field_rendering.rendering with autograd recording: compositing in mode none, depth / max(A, eps) and the
    render_bkgd blend in torch, end to end against the reference at a spike case."""
    from quadraturefields_amd import field_rendering as fr
    case0, t = _case("spike-1e6-mid", stride, device)
    n, n_rays = len(case0["sigma"]), int(case0["n_rays"])
    ts = t["depth"] - 0.5 * t["delta"]
    te = ts + t["delta"]
    case = dict(case0, delta=(te - ts).cpu().numpy(), depth=((ts + te) / 2.0).cpu().numpy())
    bk = None if bkgd is None else torch.tensor(bkgd, dtype=torch.float32, device=device)
    g_o, g_d = t["g_alpha"][:, None], t["g_depth"][:, None]
    with torch.enable_grad():
        c, s = _leaf(t["rgb"]), _leaf(t["sigma"])
        colors, opac, depths, extras = fr.rendering(ts, te, t["index_ray"], n_rays, rgb_sigma_fn=lambda a, b, r: (c, s),
                                                    render_bkgd=bk)
        torch.autograd.backward([colors, opac, depths], [t["g_rgb"], g_o, g_d])
    ref, ref_colors = R.rendering_reference(case, bkgd, case["g_rgb"], case["g_alpha"], case["g_depth"])
    ref = dict(ref, colors=ref_colors)
    got = {"grad_color": torch.cat([c.grad, _nan(0, 3, device)]), "grad_sigma": torch.cat([s.grad, _nan(0, 0, device)])}
    check("rendering", f"train-{'bkgd' if bkgd else 'nobkgd'}", ("grad_color", "grad_sigma"), got, ref, {"grad_color": n, "grad_sigma": n})
    fwd = {"colors": torch.cat([colors.detach(), _nan(0, 3, device)]), "alpha": torch.cat([opac.detach().reshape(-1), _nan(0, 0, device)]),
           "depth_norm": torch.cat([depths.detach().reshape(-1), _nan(0, 0, device)]),
           "weights": torch.cat([extras["weights"].detach(), _nan(0, 0, device)])}
    check("rendering", f"train-{'bkgd' if bkgd else 'nobkgd'}", ("colors", "alpha", "depth_norm", "weights"), fwd, ref,
          {"colors": n_rays, "alpha": n_rays, "depth_norm": n_rays, "weights": n}, bar_names={"colors": "rgb", "alpha": "alpha", "depth_norm": "depth_norm", "weights": "weights"})


# ------------------------------------------------------------------------------------------------------- forward
FORWARD_FAMILIES = ["mild", "spike-250-mid", "spike-1.6e4-last", "spike-1e6-mid", "spike-max-mid", "multi", "inf", "zero",
                    "tiny", "zero_delta", "lengths", "outside", "single", "big"]


def run_forward(lib, case, t, mode, sample_index=None, rgb=None, sigma=None):
    from quadraturefields_amd import _C
    n, n_rays, dev = len(case["sigma"]), int(case["n_rays"]), t["sigma"].device
    out = {"rgb": _nan(n_rays, 3, dev), "alpha": _nan(n_rays, 0, dev), "depth": _nan(n_rays, 0, dev), "weights": _nan(n, 0, dev)}
    _C.check(lib.qf_derive_properties(
        _p(t["rgb"] if rgb is None else rgb), _p(t["sigma"] if sigma is None else sigma), _p(t["depth"]), _p(t["delta"]), 0.0,
        _p(t["index_ray"]), n, n_rays, mode, _p(t["bkgd"]) if mode == R.BG_CUSTOM else None,
        None if sample_index is None else _p(sample_index, torch.int32), _p(out["rgb"]), _p(out["alpha"]), _p(out["depth"]),
        _p(out["weights"]), _C.stream()), "qf_derive_properties")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("mode", MODES, ids=[R.BG_NAMES[m] for m in MODES])
@pytest.mark.parametrize("family", FORWARD_FAMILIES)
def test_derive_properties_forward_vs_fp64(lib, device, stride, family, mode):
    """The chunked kernel (1024-sample chunks + halo, long-ray tail from global memory) and its sample_index form."""
    case, t = _case(family, stride, device)
    n, n_rays = len(case["sigma"]), int(case["n_rays"])
    got = run_forward(lib, case, t, mode)
    ref = R.reference(case, mode)
    names = ("weights", "rgb", "alpha", "depth")
    rows = {"weights": n, "rgb": n_rays, "alpha": n_rays, "depth": n_rays}
    if family == "inf":
        assert all(bool(torch.isfinite(got[k][:rows[k]]).all()) for k in names)
    check("forward", f"{family}-{R.BG_NAMES[mode]}", names, got, ref, rows)
    if mode in (R.BG_WHITE, R.BG_NONE):
        g = torch.Generator().manual_seed(n)
        perm = torch.randperm(n, generator=g).to(device)
        inv = torch.empty(n, dtype=torch.int32, device=device)
        inv[perm] = torch.arange(n, dtype=torch.int32, device=device)
        got2 = run_forward(lib, case, t, mode, sample_index=inv, rgb=t["rgb"][perm].contiguous(), sigma=t["sigma"][perm].contiguous())
        for k in names:
            assert torch.equal(got2[k][:rows[k]], got[k][:rows[k]]), (k, "sample_index form differs")


def _frame_case(spike, w, h, k=25):
    """An image of w x h rays with up to k samples each and a constant delta, one spike on most rays."""
    rng = np.random.default_rng(w * 100 + h)
    counts = rng.integers(0, k + 1, size=w * h)
    counts[rng.random(w * h) < 0.3] = 0
    counts[0], counts[-1] = k, 0
    case = R._assemble(rng, counts)
    s, c, _ = R.ray_runs(case["index_ray"])
    at = R._spike_at(rng, s, c, "mid")[::2]
    if np.isinf(spike):
        case["sigma"][at] = np.inf
    else:
        R._set_tau(case, at, spike)
    return case, counts.astype(np.int32)


@pytest.mark.parametrize("mode", MODES, ids=[R.BG_NAMES[m] for m in MODES])
@pytest.mark.parametrize("spike", [250.0, 1.6e4, 1e6, float("inf")])
@pytest.mark.parametrize("w,h", [(50, 37), (8, 8)])
def test_composite_tiles_on_spike_inputs(lib, device, spike, w, h, mode):
    """qf_composite_tiles against the reference, and bit for bit equal to the chunked kernel, on spike inputs."""
    from quadraturefields_amd import _C
    case, counts = _frame_case(spike, w, h)
    t = _dev(case, device)
    n, n_rays, k = len(case["sigma"]), w * h, 25
    hit = torch.from_numpy(counts).to(device)
    offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).long().to(device)
    tiles = ((w + 7) // 8) * ((h + 7) // 8)
    totals = torch.empty((tiles,), dtype=torch.int64, device=device)
    _C.check(lib.qf_tile_totals(_p(hit), w, h, _p(totals), _C.stream()), "qf_tile_totals")
    tile_base = (torch.cumsum(totals, 0) - totals).contiguous()
    inverse = torch.empty((n,), dtype=torch.int32, device=device)
    _C.check(lib.qf_coherent_layout(_p(hit), _p(offsets), _p(tile_base), w, h, None, _p(inverse), 0, _C.stream()), "qf_coherent_layout")
    inv = inverse.long()
    assert int(inv.min()) == 0 and int(inv.max()) == n - 1 and len(torch.unique(inv)) == n
    rgb_c, sigma_c, depth_c = torch.empty_like(t["rgb"]), torch.empty_like(t["sigma"]), torch.empty_like(t["depth"])
    rgb_c[inv], sigma_c[inv], depth_c[inv] = t["rgb"], t["sigma"], t["depth"]
    out = {"rgb": _nan(n_rays, 3, device), "alpha": _nan(n_rays, 0, device), "depth": _nan(n_rays, 0, device), "weights": _nan(n, 0, device)}
    _C.check(lib.qf_composite_tiles(_p(rgb_c), _p(sigma_c), _p(depth_c), R.DELTA, _p(hit), k, _p(tile_base), w, h, mode,
                                    _p(t["bkgd"]) if mode == R.BG_CUSTOM else None, _p(out["rgb"]), _p(out["alpha"]), _p(out["depth"]),
                                    _p(out["weights"]), None, _C.stream()), "qf_composite_tiles")
    torch.cuda.synchronize()
    chunked = run_forward(lib, case, t, mode)
    for name in ("rgb", "alpha", "depth"):
        assert torch.equal(out[name][:n_rays], chunked[name][:n_rays]), name
    assert torch.equal(out["weights"][:n][inv], chunked["weights"][:n])
    out["weights"] = torch.cat([out["weights"][:n][inv], out["weights"][n:]])
    ref = R.reference(case, mode)
    check("tiles", f"spike{spike:g}-{w}x{h}-{R.BG_NAMES[mode]}", ("weights", "rgb", "alpha", "depth"), out, ref,
          {"weights": n, "rgb": n_rays, "alpha": n_rays, "depth": n_rays})


@pytest.mark.parametrize("bkgd", [None, R.BKGD], ids=["nobkgd", "bkgd"])
@pytest.mark.parametrize("family", [f for f in FORWARD_FAMILIES if f != "outside"])      # pack_info has rows for image rays only
def test_render_from_density_vs_fp64(lib, device, stride, family, bkgd):
    """weights, trans, alphas, colours, opacities and depth / max(A, eps) (0 / eps = 0 on rays without density)."""
    from quadraturefields_amd import _C
    case0, t = _case(family, stride, device)
    n, n_rays = len(case0["sigma"]), int(case0["n_rays"])
    ts = t["depth"] - 0.5 * t["delta"]
    te = ts + t["delta"]
    delta32, mid32 = (te - ts).cpu().numpy(), ((ts + te) / 2.0).cpu().numpy()
    if family == "zero_delta":                            # keep the exact zeros
        te = torch.where(t["delta"] == 0, ts, te)
        delta32 = (te - ts).cpu().numpy()
        mid32 = ((ts + te) / 2.0).cpu().numpy()
        assert int((delta32 == 0).sum()) > 100
    case = dict(case0, delta=delta32, depth=mid32)
    info = torch.empty((n_rays, 2), dtype=torch.int64, device=device)
    _C.check(lib.qf_pack_info(_p(t["index_ray"]), n, n_rays, _p(info), _C.stream()), "qf_pack_info")
    bk = None if bkgd is None else torch.tensor(bkgd, dtype=torch.float32, device=device)
    out = {"weights": _nan(n, 0, device), "trans": _nan(n, 0, device), "alphas": _nan(n, 0, device),
           "colors": _nan(n_rays, 3, device), "alpha": _nan(n_rays, 0, device), "depth_norm": _nan(n_rays, 0, device)}
    _C.check(lib.qf_render_from_density(_p(ts.contiguous()), _p(te.contiguous()), _p(t["sigma"]), _p(t["rgb"]), _p(info), n_rays, n,
                                        _p(bk), _p(out["weights"]), _p(out["trans"]), _p(out["alphas"]), _p(out["colors"]),
                                        _p(out["alpha"]), _p(out["depth_norm"]), _C.stream()), "qf_render_from_density")
    torch.cuda.synchronize()
    ref = R.reference(case, R.BG_NONE)
    (C, mC), (A, mA) = ref["plain"], ref["alpha"]
    b = np.zeros(3) if bkgd is None else np.float32(bkgd).astype(np.float64)
    ref["colors"] = (C + b[None, :] * (1.0 - A)[:, None], mC + np.abs(b)[None, :] * (1.0 + mA)[:, None])
    names = ("weights", "trans", "alphas", "colors", "alpha", "depth_norm")
    rows = {"weights": n, "trans": n, "alphas": n, "colors": n_rays, "alpha": n_rays, "depth_norm": n_rays}
    if family == "zero":
        dead = torch.from_numpy(A == 0).to(device)
        assert int(dead.sum()) > 50 and not bool(out["depth_norm"][:n_rays][dead].any())
    check("render_from_density", f"{family}-{'bkgd' if bkgd else 'nobkgd'}", names, out, ref, rows,
          bar_names={"weights": "weights", "trans": "trans", "alphas": "alphas", "colors": "rgb", "alpha": "alpha", "depth_norm": "depth_norm"})


@pytest.mark.parametrize("exclusive", [1, 0], ids=["exclusive", "inclusive"])
@pytest.mark.parametrize("family", FORWARD_FAMILIES)
def test_exponential_integration_vs_fp64(lib, device, stride, family, exclusive):
    """kaolin's exponential_integration, both modes: exclusive T_j = exp(-cum_j), inclusive T_j = exp(-(cum_j + tau_j))."""
    from quadraturefields_amd import _C
    case, t = _case(family, stride, device)
    n = len(case["sigma"])
    starts, counts, ids = R.ray_runs(case["index_ray"])
    tau = (t["sigma"] * t["delta"]).contiguous()
    seg = torch.from_numpy(starts).to(device)
    n_seg = len(starts)
    out = {"feats": _nan(n_seg, 3, device), "weights": _nan(n, 0, device)}
    _C.check(lib.qf_exponential_integration(_p(t["rgb"]), 3, _p(tau), _p(seg), n_seg, n, exclusive, _p(out["feats"]), _p(out["weights"]),
                                            _C.stream()), "qf_exponential_integration")
    torch.cuda.synchronize()
    # one ray per run, every run inside the image: the reference's rows are the runs
    runs = dict(case, index_ray=np.repeat(np.arange(n_seg), counts), n_rays=n_seg)
    ref = R.reference(runs, R.BG_NONE, inclusive=not exclusive)
    ref = {"feats": ref["plain"], "weights": ref["weights"]}
    bar_names = {"feats": "rgb", "weights": "weights"} if exclusive else {"feats": "feats_incl", "weights": "weights_incl"}
    check("exp_integration", f"{family}-{'excl' if exclusive else 'incl'}", ("feats", "weights"), out, ref, {"feats": n_seg, "weights": n},
          bar_names=bar_names)


@pytest.mark.parametrize("n_rays,max_per", [(1, 1), (300, 25), (20, 400)])
def test_exclusive_scan_product_with_exact_zeros_and_ones(lib, device, n_rays, max_per):
    """Product mode: out_j = prod_{k<j} x_k.  An exact 1 changes nothing, everything behind an exact 0 is exactly 0, and
    j sequential fp32 products are within j u of the float64 product (one rounding each, (1 + u/2)^j - 1 < j u)."""
    from quadraturefields_amd import _C
    rng = np.random.default_rng(n_rays)
    counts = rng.integers(1, max_per + 1, n_rays)
    counts[rng.random(n_rays) < 0.2] = 0
    counts[0] = max_per
    n = int(counts.sum())
    x = (0.5 + 0.5 * rng.random(n)).astype(np.float32)
    x[rng.random(n) < 0.3] = 1.0
    x[rng.random(n) < 0.03] = 0.0
    starts = np.cumsum(counts) - counts
    info = torch.from_numpy(np.stack([starts, counts], 1).astype(np.int64)).to(device)
    out = _nan(n, 0, device)
    _C.check(lib.qf_exclusive_scan(_p(torch.from_numpy(x).to(device)), _p(info), n_rays, n, 1, _p(out), _C.stream()), "qf_exclusive_scan")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out[n:]).all())
    got = out[:n].cpu().numpy().astype(np.float64)
    worst = 0.0
    for s, c in zip(starts, counts):
        ref = np.concatenate([[1.0], np.cumprod(x[s:s + c].astype(np.float64))[:-1]]) if c else np.zeros(0)
        g = got[s:s + c]
        assert not g[ref == 0].any()
        if c and x[s] == 1.0:
            assert g[0] == 1.0 and g[1] == 1.0 if c > 1 else g[0] == 1.0
        j = np.arange(c)
        ok = np.abs(g - ref) <= j * R.U * ref
        assert ok.all(), (s, int(np.argmin(ok)))
        live = (ref > 0) & (j > 0)
        if live.any():
            worst = max(worst, float((np.abs(g - ref)[live] / (j[live] * R.U * ref[live])).max()))
    _report("exclusive_scan", f"prod-{n_rays}x{max_per}", "out", worst)
