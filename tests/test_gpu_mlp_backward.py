"""The fused MLP backward kernels (qf_ngp_mlp_backward, qf_sg_mlp_backward, qf_deform_mlp_backward) and
qf_sg_features_to_rgb_backward against the float64 reference of tests/mlp_backward_reference.py, at training sizes.

Each MLP kernel is a persistent grid-stride loop: a wave takes groups of 16 points, keeps its weight-gradient tiles in
registers across iterations and flushes them with atomics at the end.  One sweep of the grid covers S = 64 * CUs points
(2S for the deformation decoder), so the sizes below straddle one sweep, several sweeps and 2^20 + 5 points, where
every wave carries its accumulators through many iterations and the ragged last group lands in a late one.

Bars, with M the reference's magnitude of each element and u = 2^-24:
  * per point (d_enc, d_x01): |got - ref| <= 2^-16 M, except points with a ReLU margin below 2^-22, which must be
    fewer than 0.1 % of n and finite;
  * full-batch weight gradients: |got - ref| <= 2^-14 M;
  * sparse probes (upstream gradients zero except on ~112 points in chosen groups): the weight gradients match the
    probe-only reference at 2^-16 M_probe -- a dropped, doubled or leaking group moves them by far more.
The ReLU-margin threshold is 2^-22 rather than 2^-14: with random inputs at grid-feature scale 3.4 % of points have
some pre-activation within 2^-14 of its magnitude, and for the SG head at S + 1 points still 0.11 % within 2^-20, more
than the 0.1 % the check allows.  Points within the margin get no upstream gradient (the reference is recomputed
without them): a ReLU branch that fp32 takes differently there would otherwise move a full-batch weight gradient by
that point's whole contribution, which no rounding bar can absorb.
"""
import ctypes
import math
import os

import pytest
import torch

from oracle import fields as ofields
from quadraturefields_amd import synthetic
from tests import mlp_backward_reference as R

PT_BAR = 2.0 ** -16 / R.U            # in units of u * M
W_BAR = 2.0 ** -14 / R.U
MARGIN = 2.0 ** -22
SPARE = 16
NAN = float("nan")

pytestmark = pytest.mark.gpu


def _report(kind, case, name, value):
    """One line per measured maximum of err / (u M); collected into the pull request's numbers."""
    print(f"ERR_RATIO {kind} {case} {name} {value:.3g}")
    path = os.environ.get("QF_ERR_RATIO_LOG")
    if path:
        with open(path, "a") as f:
            f.write(f"{kind} {case} {name} {value:.6g}\n")


@pytest.fixture(scope="module")
def sweep(lib, device):
    cu = lib.qf_device_cu_count()
    assert cu > 0
    return 64 * cu


def _size(expr, s):
    return int(eval(expr.replace("^", "**"), {"S": s}))


def _gen(device, seed):
    return torch.Generator(device=device).manual_seed(seed)


def _inputs(n, device, seed):
    """enc at grid-feature scale, unit dirs, a selector ~20 % zeros with runs, upstream gradients with exact zeros
    (and nonzero d_sigma on unselected points)."""
    g = _gen(device, seed)
    enc = (torch.rand(n, 32, generator=g, device=device) * 2 - 1) * 0.5
    dirs = torch.randn(n, 3, generator=g, device=device)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    sel = torch.rand(n, generator=g, device=device) > 0.15
    for start in torch.randint(0, n, (max(1, n // 4096),), generator=g, device=device).tolist():
        sel[start:start + 40] = False                                     # runs of unselected points
    d_rgb = torch.randn(n, 3, generator=g, device=device) * 0.1
    d_rgb[torch.rand(n, generator=g, device=device) < 0.1] = 0.0
    d_rgb[torch.rand(n, 3, generator=g, device=device) < 0.05] = 0.0
    d_sigma = torch.randn(n, generator=g, device=device) * 0.01
    d_sigma[torch.rand(n, generator=g, device=device) < 0.1] = 0.0
    return enc, dirs, sel.to(torch.uint8).contiguous(), d_rgb, d_sigma


def _ngp_weights(device):
    st = synthetic.seeded_ngp_state(10, 16)
    return st["mlp_base.params"][:3072].to(device), st["mlp_head.params"].to(device)


def _sg_weights(device, lobes):
    st = synthetic.seeded_ngp_state(10, 16, sg_lobes=lobes)
    keys = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "lout.weight", "lout.bias")
    head = {k: st[f"mlp_head.{s}"].to(device).contiguous() for k, s in zip(R.SG_HEAD_NAMES, keys)}
    return st["mlp_base.params"][:3072].to(device), head


def _deform_weights(device):
    st = synthetic.seeded_deform_state(16)
    keys = ("layers.0.weight", "layers.0.bias", "layers.1.weight", "layers.1.bias", "lout.weight", "lout.bias")
    return {k: st[f"decoder_field.{s}"].to(device).contiguous() for k, s in zip(R.DEFORM_NAMES, keys)}


def _p(t):
    from quadraturefields_amd import _C
    return _C.ptr(t)


def _nan_rows(n, cols, device):
    return torch.full((n + SPARE, cols), NAN, dtype=torch.float32, device=device)


def run_ngp(lib, enc, dirs, sel, d_rgb, d_sigma, base_w, head_w, g_base, g_head):
    from quadraturefields_amd import _C
    n = enc.shape[0]
    d_enc = _nan_rows(n, 32, enc.device)
    _C.check(lib.qf_ngp_mlp_backward(_p(enc), _p(dirs), _p(sel), _p(d_rgb), _p(d_sigma), _p(base_w), _p(head_w), n,
                                     _p(d_enc), _p(g_base), _p(g_head), _C.stream()), "qf_ngp_mlp_backward")
    return d_enc


def run_sg(lib, enc, sel, d_feat, d_sigma, base_w, head, lobes, g_base, g_head):
    from quadraturefields_amd import _C
    n = enc.shape[0]
    d_enc = _nan_rows(n, 32, enc.device)
    h = _C.SGHead(*[_p(head[k]) for k in R.SG_HEAD_NAMES])
    gh = _C.SGHead(*[_p(g_head[k]) for k in R.SG_HEAD_NAMES])
    _C.check(lib.qf_sg_mlp_backward(_p(enc), _p(sel), _p(d_feat), d_feat.shape[1], _p(d_sigma), _p(base_w),
                                    ctypes.byref(h), lobes, n, _p(d_enc), _p(g_base), ctypes.byref(gh), _C.stream()),
             "qf_sg_mlp_backward")
    return d_enc


def run_deform(lib, enc, x01, d_out, w, grads):
    from quadraturefields_amd import _C
    n = enc.shape[0]
    d_enc, d_x01 = _nan_rows(n, 32, enc.device), _nan_rows(n, 3, enc.device)
    _C.check(lib.qf_deform_mlp_backward(_p(enc), _p(x01), _p(d_out), *[_p(w[k]) for k in R.DEFORM_NAMES[:5]], n,
                                        _p(d_enc), _p(d_x01), *[_p(grads[k]) for k in R.DEFORM_NAMES], _C.stream()),
             "qf_deform_mlp_backward")
    return d_enc, d_x01


def check_points(kind, case, name, got, ref, margin, n, bar=PT_BAR):
    """Rows < n written, finite and within bar (unless flagged by the ReLU margin); the spare rows untouched."""
    val, mag = ref
    assert bool(torch.isnan(got[n:]).all()), f"{kind} {case}: {name} wrote past row n"
    got = got[:n]
    assert bool(torch.isfinite(got).all()), f"{kind} {case}: {name} has non-finite rows < n"
    flagged = margin < MARGIN
    n_flag = int(flagged.sum())
    assert n_flag <= n // 1000, f"{kind} {case}: {n_flag} of {n} points within the ReLU margin"
    r = R.err_ratio(got, val, mag).amax(dim=1)
    worst = float(r[~flagged].max()) if n_flag < n else 0.0
    _report(kind, case, name, worst)
    assert worst <= bar, (kind, case, name, worst, int(r[~flagged].argmax()))


def check_weights(kind, case, name, got, ref, g0=None, bar=W_BAR):
    val, mag = ref
    if g0 is not None:
        val, mag = val + g0.double(), mag + g0.double().abs()
    assert bool(torch.isfinite(got).all()), f"{kind} {case}: {name} not finite"
    r = R.err_ratio(got.reshape(val.shape), val, mag)
    worst = float(r.max())
    _report(kind, case, name, worst)
    assert worst <= bar, (kind, case, name, worst, int(r.argmax()))


def _g0(ref_mag, device, seed):
    """Random prefill of a gradient buffer at the scale of the gradient itself (the kernels ACCUMULATE)."""
    g = _gen(device, seed)
    return (torch.randn(ref_mag.shape, generator=g, device=device) * float(ref_mag.mean())).float()


SIZES = ["1", "17", "S-1", "S", "S+1", "S+17", "3*S+7", "2^20+5"]


# ------------------------------------------------------------------------------------------------------- NGP
def _ngp_case(lib, device, n, seed, enc=None, probes=None, prefill=True):
    base_w, head_w = _ngp_weights(device)
    e, dirs, sel, d_rgb, d_sigma = _inputs(n, device, seed)
    enc = e if enc is None else enc
    if probes is not None:
        keep = torch.zeros(n, dtype=torch.bool, device=device)
        keep[probes] = True
        d_rgb, d_sigma = d_rgb * keep[:, None], d_sigma * keep
    ref = R.ngp_backward(enc, dirs, sel, d_rgb, d_sigma, base_w, head_w)
    live = ref["margin"] >= MARGIN
    if not bool(live.all()):
        d_rgb, d_sigma = d_rgb * live[:, None], d_sigma * live
        ref = R.ngp_backward(enc, dirs, sel, d_rgb, d_sigma, base_w, head_w)
    g0b = _g0(ref["grad_base_w"][1], device, seed + 1) if prefill else torch.zeros(3072, device=device)
    g0h = _g0(ref["grad_head_w"][1], device, seed + 2) if prefill else torch.zeros(7168, device=device)
    gb, gh = g0b.clone(), g0h.clone()
    d_enc = run_ngp(lib, enc, dirs, sel, d_rgb, d_sigma, base_w, head_w, gb, gh)
    torch.cuda.synchronize()
    return dict(inputs=(enc, dirs, sel, d_rgb, d_sigma, base_w, head_w), ref=ref, d_enc=d_enc, gb=gb, gh=gh,
                g0b=g0b, g0h=g0h, live=live)


@pytest.mark.parametrize("size", SIZES)
def test_ngp_mlp_backward_vs_fp64(lib, device, sweep, size):
    n = _size(size, sweep)
    c = _ngp_case(lib, device, n, seed=11 + n % 997)
    ref = c["ref"]
    check_points("ngp", size, "d_enc", c["d_enc"], ref["d_enc"], ref["margin"], n)
    check_weights("ngp", size, "grad_base_w", c["gb"], ref["grad_base_w"], c["g0b"])
    check_weights("ngp", size, "grad_head_w", c["gh"], ref["grad_head_w"], c["g0h"])


# ------------------------------------------------------------------------------------------------------- SG
def _sg_case(lib, device, n, lobes, seed, enc=None, probes=None, prefill=True):
    base_w, head = _sg_weights(device, lobes)
    e, _, sel, _, d_sigma = _inputs(n, device, seed)
    enc = e if enc is None else enc
    n_out = 3 + 7 * lobes
    g = _gen(device, seed + 5)
    d_feat = torch.full((n, n_out + 5), NAN, device=device)          # d_stride = n_out + 5, NaN padding
    d_feat[:, :n_out] = torch.randn(n, n_out, generator=g, device=device) * 0.05
    d_feat[:, :n_out][torch.rand(n, generator=g, device=device) < 0.1] = 0.0
    if probes is not None:
        keep = torch.zeros(n, dtype=torch.bool, device=device)
        keep[probes] = True
        d_feat[:, :n_out] *= keep[:, None]
        d_sigma = d_sigma * keep
    ref = R.sg_backward(enc, sel, d_feat, d_sigma, base_w, head, lobes)
    live = ref["margin"] >= MARGIN
    if not bool(live.all()):
        d_feat[:, :n_out] *= live[:, None]
        d_sigma = d_sigma * live
        ref = R.sg_backward(enc, sel, d_feat, d_sigma, base_w, head, lobes)
    g0 = {k: (_g0(ref[k][1], device, seed + i) if prefill else torch.zeros_like(ref[k][1], dtype=torch.float32))
          for i, k in enumerate(("grad_base_w",) + R.SG_HEAD_NAMES)}
    gb = g0["grad_base_w"].clone()
    gh = {k: g0[k].clone().reshape(head[k].shape) for k in R.SG_HEAD_NAMES}
    d_enc = run_sg(lib, enc, sel, d_feat, d_sigma, base_w, head, lobes, gb, gh)
    torch.cuda.synchronize()
    return dict(ref=ref, d_enc=d_enc, gb=gb, gh=gh, g0=g0, enc=enc, d_feat=d_feat, sel=sel, d_sigma=d_sigma, live=live)


def _sg_checks(c, size, lobes, n, bar_w=W_BAR, prefill=True):
    ref, kind = c["ref"], f"sg{lobes}"
    check_points(kind, size, "d_enc", c["d_enc"], ref["d_enc"], ref["margin"], n)
    check_weights(kind, size, "grad_base_w", c["gb"], ref["grad_base_w"], c["g0"]["grad_base_w"] if prefill else None,
                  bar=bar_w)
    for k in R.SG_HEAD_NAMES:
        check_weights(kind, size, k, c["gh"][k], ref[k], c["g0"][k].reshape(ref[k][0].shape) if prefill else None,
                      bar=bar_w)


@pytest.mark.parametrize("lobes,size", [(L, s) for L in (1, 2, 4, 5, 7, 8) for s in ("17", "S+1", "3*S+7")]
                         + [(8, "2^20+5")])
def test_sg_mlp_backward_vs_fp64(lib, device, sweep, lobes, size):
    n = _size(size, sweep)
    c = _sg_case(lib, device, n, lobes, seed=100 * lobes + n % 997)
    _sg_checks(c, size, lobes, n)


# ------------------------------------------------------------------------------------------------------- deform
def _deform_case(lib, device, n, seed, probes=None, prefill=True):
    w = _deform_weights(device)
    g = _gen(device, seed)
    enc = (torch.rand(n, 32, generator=g, device=device) * 2 - 1) * 0.5
    x01 = torch.rand(n, 3, generator=g, device=device)
    d_out = torch.randn(n, generator=g, device=device) * 0.1
    d_out[torch.rand(n, generator=g, device=device) < 0.1] = 0.0
    if probes is not None:
        keep = torch.zeros(n, dtype=torch.bool, device=device)
        keep[probes] = True
        d_out = d_out * keep
    ref = R.deform_backward(enc, x01, d_out, *[w[k] for k in R.DEFORM_NAMES[:5]])
    live = ref["margin"] >= MARGIN
    if not bool(live.all()):
        d_out = d_out * live
        ref = R.deform_backward(enc, x01, d_out, *[w[k] for k in R.DEFORM_NAMES[:5]])
    g0 = {k: (_g0(ref[k][1], device, seed + i).reshape(w[k].shape) if prefill else torch.zeros_like(w[k]))
          for i, k in enumerate(R.DEFORM_NAMES)}
    grads = {k: v.clone() for k, v in g0.items()}
    d_enc, d_x01 = run_deform(lib, enc, x01, d_out, w, grads)
    torch.cuda.synchronize()
    return dict(ref=ref, d_enc=d_enc, d_x01=d_x01, grads=grads, g0=g0, enc=enc, x01=x01, d_out=d_out, live=live)


def _deform_checks(c, size, n, bar_w=W_BAR, prefill=True):
    ref = c["ref"]
    check_points("deform", size, "d_enc", c["d_enc"], ref["d_enc"], ref["margin"], n)
    check_points("deform", size, "d_x01", c["d_x01"], ref["d_x01"], ref["margin"], n)
    for k in R.DEFORM_NAMES:
        check_weights("deform", size, k, c["grads"][k], ref[k], c["g0"][k].reshape(ref[k][0].shape) if prefill else None,
                      bar=bar_w)


@pytest.mark.parametrize("size", SIZES)
def test_deform_mlp_backward_vs_fp64(lib, device, sweep, size):
    n = _size(size.replace("S", "(2*S)"), sweep)             # the deformation kernel's sweep is 2S
    c = _deform_case(lib, device, n, seed=23 + n % 997)
    _deform_checks(c, size, n)


# ------------------------------------------------------------------------------------------------------- probes
def _probe_points(n, sweep_pts, device):
    """~112 points: groups 0, 1, W-1, W, W+1 (W = groups per sweep), the last wave's group of the last full sweep and
    the ragged last group, which holds point n - 1 (where invalid lanes clamp to)."""
    W = sweep_pts // 16
    n_groups = (n + 15) // 16
    late = max(1, n_groups // W - 1) * W + W - 1
    groups = sorted({gq for gq in (0, 1, W - 1, W, W + 1, late, n_groups - 1) if 0 <= gq < n_groups})
    pts = torch.cat([torch.arange(16 * gq, min(n, 16 * gq + 16)) for gq in groups])
    return pts.to(device), groups


@pytest.mark.parametrize("size", ["S+17", "3*S+7", "2^20+5"])
@pytest.mark.parametrize("kind", ["ngp", "sg5", "deform"])
def test_sparse_probes_catch_a_lost_or_doubled_group(lib, device, sweep, kind, size):
    sw = 2 * sweep if kind == "deform" else sweep
    n = _size(size.replace("S", f"({sw})"), sweep)
    pts, groups = _probe_points(n, sw, device)
    assert len(pts) <= 128 and (n - 1) in pts.tolist() and sw // 16 in groups
    case = f"{size}-probes"
    if kind == "ngp":
        c = _ngp_case(lib, device, n, seed=31, probes=pts, prefill=False)
        enc, dirs, sel, d_rgb, d_sigma, base_w, head_w = c["inputs"]
        rp = R.ngp_backward(enc[pts], dirs[pts], sel[pts], d_rgb[pts], d_sigma[pts], base_w, head_w)
        check_weights(kind, case, "grad_base_w", c["gb"], rp["grad_base_w"], bar=PT_BAR)
        check_weights(kind, case, "grad_head_w", c["gh"], rp["grad_head_w"], bar=PT_BAR)
        d_enc = c["d_enc"]
    elif kind == "sg5":
        c = _sg_case(lib, device, n, 5, seed=37, probes=pts, prefill=False)
        base_w, head = _sg_weights(device, 5)
        rp = R.sg_backward(c["enc"][pts], c["sel"][pts], c["d_feat"][pts], c["d_sigma"][pts], base_w, head, 5)
        check_weights(kind, case, "grad_base_w", c["gb"], rp["grad_base_w"], bar=PT_BAR)
        for k in R.SG_HEAD_NAMES:
            check_weights(kind, case, k, c["gh"][k], rp[k], bar=PT_BAR)
        d_enc = c["d_enc"]
    else:
        c = _deform_case(lib, device, n, seed=41, probes=pts, prefill=False)
        rp = R.deform_backward(c["enc"][pts], c["x01"][pts], c["d_out"][pts],
                               *[_deform_weights(device)[k] for k in R.DEFORM_NAMES[:5]])
        for k in R.DEFORM_NAMES:
            check_weights(kind, case, k, c["grads"][k], rp[k], bar=PT_BAR)
        d_enc = c["d_enc"]
    assert bool(c["live"][pts].sum() >= len(pts) - 2) and bool(c["live"][n - 1])
    # the probes' own rows follow the reference; every other row is exactly 0
    off = torch.ones(n, dtype=torch.bool, device=device)
    off[pts] = False
    assert bool((d_enc[:n][off] == 0).all())
    check_points(kind, case, "d_enc", d_enc[pts], rp["d_enc"], rp["margin"], len(pts))


# ------------------------------------------------------------------------------------------------------- clamp
CLAMP_TARGETS = (-3.0, 14.5, 15.0, 15.5, 20.0, 60.0, 100.0)


def _push_past_clamp(enc, base_w, device, seed, per_target=24):
    """Scale chosen enc rows by alpha > 0 so that raw - 1 lands on each target: the base MLP has no bias and uses ReLU,
    so raw(alpha enc) = alpha raw(enc).  Rows are spread over the whole batch (every sweep)."""
    raw = R.ngp_raw(enc, base_w)
    free = torch.ones_like(raw, dtype=torch.bool)
    g = _gen(device, seed)
    rows = {}
    for t in CLAMP_TARGETS:
        cand = torch.nonzero(free & ((raw > 0.5) if t + 1.0 > 0 else (raw < -0.5))).flatten()
        pick = cand[torch.randperm(len(cand), generator=g, device=device)[:per_target]]
        enc[pick] *= ((t + 1.0) / raw[pick]).float()[:, None]
        free[pick] = False
        rows[t] = pick
    return rows


@pytest.mark.parametrize("kind", ["ngp", "sg8"])
def test_density_gradient_follows_the_clamp(lib, device, sweep, kind):
    """d raw = d_sigma * selector * exp(min(raw - 1, 15)): finite where the fp32 forward density is inf (raw - 1 =
    100), and on the reference's value above 15 (the kernels used exp(raw - 1) before)."""
    n = 3 * sweep + 7
    g = _gen(device, 77)
    enc = (torch.rand(n, 32, generator=g, device=device) * 2 - 1) * 0.5
    base_w = _ngp_weights(device)[0]
    by_target = _push_past_clamp(enc, base_w, device, 78)
    rows = torch.cat(list(by_target.values()))
    raw = R.ngp_raw(enc, base_w)
    assert float((raw - 1).max()) > 99.0 and math.isinf(float(torch.exp(raw.float().max() - 1.0)))
    c = _ngp_case(lib, device, n, seed=79, enc=enc) if kind == "ngp" else _sg_case(lib, device, n, 8, seed=81, enc=enc)
    for t, r_t in by_target.items():                      # per target first: the values a wrong rule gives
        val, mag = c["ref"]["d_enc"]
        _report(kind, f"clamp{t:g}", "d_enc", float(R.err_ratio(c["d_enc"][r_t], val[r_t], mag[r_t]).max()))
    if kind == "ngp":
        ref = c["ref"]
        check_points(kind, "clamp", "d_enc", c["d_enc"], ref["d_enc"], ref["margin"], n)
        check_weights(kind, "clamp", "grad_base_w", c["gb"], ref["grad_base_w"], c["g0b"])
        check_weights(kind, "clamp", "grad_head_w", c["gh"], ref["grad_head_w"], c["g0h"])
        sel, d_sigma = c["inputs"][2], c["inputs"][4]
    else:
        _sg_checks(c, "clamp", 8, n)
        sel, d_sigma = c["sel"], c["d_sigma"]
    live = rows[(sel[rows] > 0) & (d_sigma[rows] != 0)]
    assert len(live) >= 50                                # the clamp rows do carry a density gradient


# ------------------------------------------------------------------------------------------------------- SG mixture
@pytest.mark.parametrize("lobes", range(1, 9))
def test_sg_features_to_rgb_backward_vs_fp64_autograd(lib, device, lobes):
    """qf_sg_features_to_rgb_backward per point against float64 autograd of oracle.fields.features_to_rgb, with
    feat_stride > 3+7L and a wider d_stride whose padding must stay untouched.  M per point: the row's largest
    gradient times (1 + max |lambda|), the exponent's error amplification."""
    from quadraturefields_amd import _C
    n, n_f = 4099, 3 + 7 * lobes
    g = _gen(device, 200 + lobes)
    feats = torch.randn(n, n_f + 3, generator=g, device=device) * 0.7
    lam = feats[:, 3:n_f].view(n, lobes, 7)[:, :, 3]
    lam.mul_(5.0)
    lam[:17] = 0.0                                        # sharpness exactly 0: d|lambda| = 0 as torch.abs gives
    dirs = torch.randn(n, 3, generator=g, device=device)
    dirs = dirs / dirs.norm(dim=-1, keepdim=True)
    d_rgb = torch.randn(n, 3, generator=g, device=device)
    d_rgb[:5] = 0.0
    d_feat = torch.full((n + SPARE, n_f + 2), NAN, device=device)
    _C.check(lib.qf_sg_features_to_rgb_backward(_p(feats), feats.shape[1], _p(dirs), _p(d_rgb), n, lobes, _p(d_feat),
                                                d_feat.shape[1], _C.stream()), "qf_sg_features_to_rgb_backward")
    torch.cuda.synchronize()
    assert bool(torch.isnan(d_feat[n:]).all()) and bool(torch.isnan(d_feat[:n, n_f:]).all())
    got = d_feat[:n, :n_f]
    assert bool(torch.isfinite(got).all())
    with torch.enable_grad():
        f = feats[:, :n_f].double().cpu().requires_grad_(True)
        rgb = ofields.features_to_rgb(f, dirs.double().cpu(), lobes)
        (gf,) = torch.autograd.grad((rgb * d_rgb.double().cpu()).sum(), f)
    gf = gf.to(device)
    amp = 1.0 + lam.abs().double().amax(dim=1, keepdim=True)
    mag = gf.abs().amax(dim=1, keepdim=True) * amp
    r = R.err_ratio(got, gf, mag.expand_as(gf))
    worst = float(r.max())
    _report("sg_rgb", f"L{lobes}", "d_features", worst)
    assert worst <= PT_BAR, (lobes, worst)


# ------------------------------------------------------------------------------------------------------- modules
@pytest.mark.parametrize("cls", ["NGPRadianceField", "NGPRadianceFieldSGNew"])
def test_modules_take_the_clamped_gradient_on_both_routes(lib, device, cls):
    """NGPRadianceField and NGPRadianceFieldSGNew, fused backward and library route: with mlp_base's density row
    scaled so that some points reach raw - 1 > 15, both give the reference's clamped gradient and agree."""
    from quadraturefields_amd import _C
    from quadraturefields_amd import tinycudann as tcnn
    from quadraturefields_amd.radiance_fields import ngp as ngp_mod
    from tests import helpers
    aabb = [-1.5] * 3 + [1.5] * 3
    sg = cls == "NGPRadianceFieldSGNew"
    L = 4
    m = getattr(ngp_mod, cls)(aabb=aabb, log2_hashmap_size=12, **({"use_viewdirs": False, "num_g_lobes": L} if sg else {}))
    st = synthetic.seeded_ngp_state(12, m.mlp_base.grid.n_rows, sg_lobes=L if sg else 0)
    st["mlp_base.params"][2048:2112] *= 5.0                     # the density row of the base MLP's output layer
    m.load_state_dict(st, strict=False)
    m = m.to(device)
    n = 4000
    x, d = helpers.random_points(n, seed=3, outside_frac=0.2)
    x, d = x.to(device), d.to(device)
    g = _gen(device, 4)
    t_rgb, t_sig = torch.randn(n, 3, generator=g, device=device), torch.randn(n, 1, generator=g, device=device) * 1e-3

    selector, x01 = m.normalize(x)
    net_w = m.mlp_base.params.detach()[:3072].contiguous()
    enc = tcnn.grid_encode(_C.f32c(x01), m.mlp_base.params.detach()[3072:].contiguous(), m.mlp_base.grid.desc)
    raw = R.ngp_raw(enc, net_w)
    past = selector & (raw - 1 > 15.0)
    assert int(past.sum()) >= 20, int(past.sum())
    sel = selector.to(torch.uint8)
    if sg:
        f = m.features(x).detach()
        with torch.enable_grad():                         # the oracle runs on the CPU
            fd = f[:, :-1].double().cpu().requires_grad_(True)
            rgb = ofields.features_to_rgb(fd, d.double().cpu(), L)
            (d_feat,) = torch.autograd.grad((rgb * t_rgb.double().cpu()).sum(), fd)
        d_feat = d_feat.to(device)
        h = m.mlp_head
        head = dict(zip(R.SG_HEAD_NAMES, (h.layers[0].weight, h.layers[0].bias, h.layers[1].weight, h.layers[1].bias,
                                          h.lout.weight, h.lout.bias)))
        ref = R.sg_backward(enc, sel, d_feat, t_sig.reshape(-1), net_w, {k: v.detach() for k, v in head.items()}, L)
        named = [("grad_base_w", lambda: m.mlp_base.params.grad[:3072])] + \
                [(k, (lambda v=v: v.grad)) for k, v in head.items()]
    else:
        ref = R.ngp_backward(enc, d, sel, t_rgb, t_sig.reshape(-1), net_w, m.mlp_head.params.detach())
        named = [("grad_base_w", lambda: m.mlp_base.params.grad[:3072]), ("grad_head_w", lambda: m.mlp_head.params.grad)]

    got = {}
    for fused in (True, False):
        m.fused_backward = fused
        for p_ in m.parameters():
            p_.grad = None
        with torch.enable_grad():
            rgb, sigma = m(x, d)
            ((rgb * t_rgb).sum() + (sigma * t_sig).sum()).backward()
        got[fused] = {k: fn().detach().clone() for k, fn in named}
        got[fused]["table"] = m.mlp_base.params.grad[3072:].detach().clone()
        for k, _ in named:
            # the library route sums in a different order and its features differ by fp32 rounding: weight bar
            check_weights(cls, f"fused={fused}", k, got[fused][k], ref[k])
    for k, v in got[True].items():
        assert bool(torch.isfinite(v).all())
        scale = float(got[False][k].abs().max())
        assert float((v - got[False][k]).abs().max()) <= 2e-4 * scale, k
