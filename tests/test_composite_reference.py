"""tests/composite_reference.py against torch float64 autograd and central differences, and the two fp32 restatements
against the bars: the prefix-kept one stays inside them on every case family, the subtracting one (the arithmetic
``derive_properties_backward_kernel`` had) breaks them wherever a tau >= 1.6e4 sits behind live samples.  No GPU."""
import numpy as np
import pytest
import torch

from tests import composite_reference as R

GRADS = ("grad_color", "grad_sigma", "grad_depth")
FORWARD = ("weights", "rgb", "alpha", "depth", "trans", "alphas", "depth_norm")
MODES = (R.BG_WHITE, R.BG_BLACK, R.BG_CUSTOM, R.BG_NONE)


def _torch_composite(case, mode):
    """Straight per-ray loops in torch float64 (autograd supplies the gradients)."""
    f = torch.float64
    sigma = torch.tensor(case["sigma"], dtype=f, requires_grad=True)
    rgb = torch.tensor(case["rgb"], dtype=f, requires_grad=True)
    depth = torch.tensor(case["depth"], dtype=f, requires_grad=True)
    delta = torch.tensor(case["delta"], dtype=f)
    starts, counts, ids = R.ray_runs(case["index_ray"])
    bg = torch.tensor([1.0] * 3 if mode == R.BG_WHITE else (np.float32(R.BKGD).tolist() if mode == R.BG_CUSTOM else [0.0] * 3), dtype=f)
    loss = torch.zeros((), dtype=f)
    for s, c, ray in zip(starts, counts, ids):
        if not 0 <= ray < case["n_rays"]:
            continue
        cum, C, A, D = torch.zeros((), dtype=f), torch.zeros(3, dtype=f), torch.zeros((), dtype=f), torch.zeros((), dtype=f)
        for j in range(s, s + c):
            tau = sigma[j] * delta[j]
            w = torch.exp(-cum) * -torch.expm1(-tau)
            cum = cum + tau
            C, A, D = C + w * rgb[j], A + w, D + w * depth[j]
        px = {R.BG_WHITE: (1 - A) + A * C, R.BG_BLACK: A * C, R.BG_CUSTOM: A * C + (1 - A) * bg, R.BG_NONE: C}[mode]
        loss = loss + (px * torch.tensor(case["g_rgb"][ray], dtype=f)).sum() + A * float(case["g_alpha"][ray]) + D * float(case["g_depth"][ray])
    loss.backward()
    return {"grad_color": rgb.grad.numpy(), "grad_sigma": sigma.grad.numpy(), "grad_depth": depth.grad.numpy()}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", ["mild", "spike-250-mid", "zero", "tiny", "zero_delta", "outside", "single"])
def test_analytic_backward_equals_float64_autograd(family, mode):
    case = R.make_case(family)
    keep = case["index_ray"] < min(case["n_rays"], 40)            # the loops are slow: the first rays
    case = dict(case, **{k: case[k][keep] for k in ("sigma", "delta", "rgb", "depth", "index_ray")})
    ref = R.reference(case, mode, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"])
    with torch.enable_grad():
        want = _torch_composite(case, mode)
    for k in GRADS:
        val, mag = ref[k]
        assert float(R.err_ratio(want[k], val, mag).max(initial=0.0)) <= 2.0 ** -20, k          # 2^-44 M: float64 rounding


def test_central_differences_on_a_few_rays():
    case = R.make_case("mild")
    keep = case["index_ray"] < 6
    case = dict(case, **{k: case[k][keep] for k in ("sigma", "delta", "rgb", "depth", "index_ray")})
    args = (R.BG_CUSTOM, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"])

    def loss(c):
        r = R.reference(c, *args)
        return float((r["rgb"][0] * c["g_rgb"]).sum() + (r["alpha"][0] * c["g_alpha"]).sum() + (r["depth"][0] * c["g_depth"]).sum())
    ref = R.reference(case, *args)
    for name, key, h in (("grad_sigma", "sigma", 2.0 ** -6), ("grad_depth", "depth", 2.0 ** -8), ("grad_color", "rgb", 2.0 ** -8)):
        for j in range(0, len(case["sigma"]), 5):
            idx = (j, 1) if key == "rgb" else (j,)
            hi, lo = dict(case), dict(case)
            hi[key], lo[key] = case[key].copy(), case[key].copy()
            hi[key][idx] += np.float32(h)                             # exactly representable steps
            lo[key][idx] -= np.float32(h)
            step = float(hi[key][idx]) - float(lo[key][idx])
            fd = (loss(hi) - loss(lo)) / step
            want = float(ref[name][0][idx])
            assert abs(fd - want) <= 1e-5 * (abs(want) + float(ref[name][1][idx])), (name, j, fd, want)


def test_infinite_density_has_a_finite_reference():
    """sigma = +inf: finite everywhere, zero colour and depth gradients behind the opaque sample."""
    case = R.make_case("inf")
    ref = R.reference(case, R.BG_WHITE, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"])
    assert all(np.isfinite(ref[k][0]).all() and np.isfinite(ref[k][1]).all() for k in ref)
    behind = _behind_opaque(case)
    assert behind.sum() > 100
    assert not ref["grad_color"][0][behind].any() and not ref["grad_depth"][0][behind].any()
    assert not ref["grad_sigma"][0][np.isinf(case["sigma"])].any()


def _behind_opaque(case):
    starts, counts, _ = R.ray_runs(case["index_ray"])
    seen = np.zeros(len(case["sigma"]), dtype=bool)
    for s, c in zip(starts, counts):
        seen[s:s + c] = np.cumsum(np.isinf(case["sigma"][s:s + c])) - np.isinf(case["sigma"][s:s + c]) > 0
    return seen


def _ratios(case, mode, prefix):
    g = (case["g_rgb"], case["g_alpha"], case["g_depth"])
    ref = R.reference(case, mode, R.BKGD, *g)
    got = R.restate_fp32(case, mode, R.BKGD, *g, prefix=prefix)
    return {k: float(R.err_ratio(got[k], *ref[k]).max(initial=0.0)) for k in GRADS + FORWARD}


_worst = {}


@pytest.mark.parametrize("family", R.FAMILIES)
def test_prefix_kept_restatement_is_inside_the_bars(family):
    """Its worst ratio is at most a quarter of each bar (bar = 4 x maximum, rounded up), and at most the recorded
    maximum, so the constants in composite_reference.py are this measurement."""
    case = R.make_case(family)
    for mode in MODES:
        for k, r in _ratios(case, mode, "keep").items():
            print(f"RESTATEMENT keep {family} {R.BG_NAMES[mode]} {k} {r:.3g}")
            _worst[k] = max(_worst.get(k, 0.0), r)
            assert r <= R.RESTATEMENT_MAX[k] * 1.005 and 4.0 * r <= R.BARS[k], (family, mode, k, r)
    ref = R.reference(case, R.BG_NONE, inclusive=True)
    got = R.restate_fp32(case, R.BG_NONE, inclusive=True)
    for k, name in (("weights", "weights_incl"), ("plain", "feats_incl")):
        r = float(R.err_ratio(got[k], *ref[k]).max(initial=0.0))
        _worst[name] = max(_worst.get(name, 0.0), r)
        assert r <= R.RESTATEMENT_MAX[name] * 1.005 and 4.0 * r <= R.BARS[name], (family, name, r)


def test_bars_are_four_times_the_measured_maxima():
    assert set(R.BARS) == set(R.RESTATEMENT_MAX)
    for k, m in R.RESTATEMENT_MAX.items():
        assert R.BARS[k] == R.bar_from(m), k
    if len(_worst) == len(R.BARS):                                # the whole module ran: the recorded maxima are attained
        for k, m in R.RESTATEMENT_MAX.items():
            assert _worst[k] >= 0.98 * m, (k, _worst[k], m)


@pytest.mark.parametrize("family", R.SPIKE_FAMILIES)
def test_subtracting_restatement_breaks_the_bars(family):
    case = R.make_case(family)
    for mode in MODES:
        r = _ratios(case, mode, "subtract")
        print(f"RESTATEMENT subtract {family} {R.BG_NAMES[mode]} " + " ".join(f"{k} {r[k]:.3g}" for k in GRADS))
        if family.startswith("spike-"):
            assert all(r[k] > 4.0 * R.BARS[k] for k in GRADS), (family, mode, r)
        else:
            assert any(r[k] > 4.0 * R.BARS[k] for k in GRADS), (family, mode, r)


def test_subtracting_restatement_gives_nan_for_infinite_density():
    case = R.make_case("inf")
    got = R.restate_fp32(case, R.BG_WHITE, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"], prefix="subtract")
    assert np.isnan(got["grad_sigma"]).any()
    got = R.restate_fp32(case, R.BG_WHITE, R.BKGD, case["g_rgb"], case["g_alpha"], case["g_depth"], prefix="keep")
    assert all(np.isfinite(got[k]).all() for k in GRADS)


def test_case_families_hold_what_they_claim():
    big = R.make_case("big", stride=4096)
    n = len(big["sigma"])
    starts, counts, _ = R.ray_runs(big["index_ray"])
    assert n > 4096 and n % 256 != 0 and ((starts < 4096) & (starts + counts > 4096)).any()
    assert len(R.make_case("single")["sigma"]) == 1
    out = R.make_case("outside")
    assert (out["index_ray"] < 0).any() and (out["index_ray"] >= out["n_rays"]).any()
    tiny = R.make_case("tiny")
    tau = tiny["sigma"] * tiny["delta"]
    assert float(tau.max()) < 3e-8 and not (np.float32(1) - np.exp(-tau)).any()
    assert sorted(set(R.ray_runs(R.make_case("lengths")["index_ray"])[1]) & {1, 2, 25, 64, 400, 2500}) == [1, 2, 25, 64, 400, 2500]
    assert float(R.make_case("spike-max-mid")["sigma"].max()) == R.FLT_MAX
    zd = R.make_case("zero_delta")
    assert (zd["delta"] == 0).sum() > 100 and np.isfinite(zd["sigma"]).all()
