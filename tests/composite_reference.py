"""float64 reference of the per-ray compositing of csrc/composite.hip, forward and backward, on the host.

Written from the equations, not from ``oracle/volrend.py`` (whose ``seg_cumsum`` forms exclusive sums as
``inclusive - f``).  Samples are packed and sorted by ray; a run of equal ray ids is one ray.  Per ray, in sample order,

    tau_j = sigma_j delta_j        cum_j = sum_{k<j} tau_k  (an explicit prefix sum, never total - suffix)
    T_j = exp(-cum_j)              e_j = exp(-tau_j)          alpha_j = -expm1(-tau_j)        w_j = T_j alpha_j
    C = sum w c,  A = sum w,  D = sum w t

and the blend of ``composite_blend``: white (1 - A) + A C (alpha applied twice, the reference's quirk), black A C,
custom A C + (1 - A) bg, none C.  Rays without samples read 1 (white, custom) or 0 (black, none).  Backward, with
upstream gradients g_rgb, g_alpha, g_depth of the ray (zero for a ray id outside [0, n_rays)):

    gC = A g_rgb (none: g_rgb)     gA = g_alpha + sum_ch g_rgb (C - {1, 0, bg}) (none: g_alpha)
    gw_j = gC . c_j + gA + g_depth t_j
    grad_color_j = w_j gC          grad_depth_j = w_j g_depth
    grad_sigma_j = delta_j (gw_j T_j e_j - sum_{k>j} gw_k w_k)

Every factor T, e, alpha lies in [0, 1] and the prefix sums only add, so tau = +inf needs no special case: the opaque
sample has T e = 0, everything behind it has T = 0, and nothing forms inf - inf.  (sigma = +inf with delta = 0 is
inf * 0 and outside the domain.)

Next to every value the reference returns a scale M, the sum of the magnitudes of the terms an fp32 evaluation of the
kernels' formulas adds up.  The kernels form alpha as ``1 - expf(-tau)`` (the forward kernels are pinned to those bits),
so a weight's scale is M_w = T (1 + e) + w S, not w: for small tau the difference 1 - e cancels and its error is u
relative to 1, and the fp32 running sum cum_j errs by u times the sum S_j of its partial sums (2 500 additions on a
marched ray), which the exponential carries into T.  From there M_A = sum M_w, M_C = sum M_w |c|, M_D = sum M_w |t|, |gC| = M_A |g_rgb|, |gA| = |g_alpha| +
sum |g_rgb| (M_C + |bg|), |gw| = |gC| . |c| + |gA| + |g_depth| |t|, and

    M_color = M_w |gC|     M_depth = M_w |g_depth|     M_sigma = delta (|gw| T e (1 + S) + sum_{k>j} |gw_k| M_w_k).

Per ray every M is floored at 2^-20 of its maximum on that ray, so that a fully occluded sample is judged against its
ray, not against an underflowed scale, and at 2^-102 (u M = 2^-126, the smallest normal fp32 number: a whole ray
behind tau = 250 has gradients near 1e-109 that fp32 returns as 0).  A ray whose M is 0 throughout keeps M = 0.
``err_ratio`` is |got - ref| / (u M) with u = 2^-24; where M = 0 the value
must be exact.

Two fp32 restatements of the backward kernel's algorithm (numpy float32, one sample after the other, same order of
operations) sit beside it: ``prefix="keep"`` remembers each sample's exclusive cum from the forward sweep and is what
the bars of the tests are derived from (4 x its worst ratio, rounded up to a power of two); ``prefix="subtract"``
rebuilds it as ``cum -= tau`` from the total and exists only so that the host test can show the bars reject it.
"""
import numpy as np

U = 2.0 ** -24
FLOOR = 2.0 ** -20
TINY = 2.0 ** -102          # u * TINY = 2^-126, the smallest normal fp32: what underflows there is not resolved
EPS32 = float(np.finfo(np.float32).eps)
FLT_MAX = float(np.finfo(np.float32).max)
BG_WHITE, BG_BLACK, BG_CUSTOM, BG_NONE = 0, 1, 2, 3
BG_NAMES = {BG_WHITE: "white", BG_BLACK: "black", BG_CUSTOM: "custom", BG_NONE: "none"}
BKGD = (0.1, 0.6, 0.3)

#: Worst err_ratio of the prefix-kept fp32 restatement against float64 over every family of ``FAMILIES`` and the four
#: background modes, measured on the host (tests/test_composite_reference.py re-measures and asserts them).
RESTATEMENT_MAX = {"grad_color": 2.49, "grad_sigma": 3.13, "grad_depth": 2.46,
                   "weights": 2.12, "rgb": 2.10, "alpha": 0.88, "depth": 0.90,
                   "trans": 2.17, "alphas": 1.08, "depth_norm": 0.31, "weights_incl": 1.16, "feats_incl": 0.87}
#: 4 x RESTATEMENT_MAX rounded up to a power of two: the device's expf is within 1-2 ulp of numpy's and the compiler
#: may contract the backward's products and sums.
BARS = {"grad_color": 16.0, "grad_sigma": 16.0, "grad_depth": 16.0,
        "weights": 16.0, "rgb": 16.0, "alpha": 4.0, "depth": 4.0,
        "trans": 16.0, "alphas": 8.0, "depth_norm": 2.0, "weights_incl": 8.0, "feats_incl": 4.0}


def bar_from(measured):
    """4 x the restatement's maximum, rounded up to a power of two."""
    return 2.0 ** int(np.ceil(np.log2(4.0 * measured)))


# ------------------------------------------------------------------------------------------------- rays and padding
def ray_runs(index_ray):
    """(starts, counts, ids) of the runs of equal ray ids."""
    r = np.asarray(index_ray, dtype=np.int64)
    n = r.shape[0]
    if n == 0:
        z = np.zeros(0, dtype=np.int64)
        return z, z, z
    head = np.concatenate([[True], r[1:] != r[:-1]])
    starts = np.nonzero(head)[0]
    counts = np.diff(np.concatenate([starts, [n]]))
    return starts, counts, r[starts]


def _groups(counts, short=64):
    """Runs grouped for padding: every run of at most ``short`` samples together, longer ones one length at a time."""
    small = np.nonzero(counts <= short)[0]
    if len(small):
        yield small, int(counts[small].max())
    for k in np.unique(counts[counts > short]):
        yield np.nonzero(counts == k)[0], int(k)


class _Pad:
    def __init__(self, starts, counts, rows, k, n):
        cols = np.arange(k)[None, :]
        self.valid = cols < counts[rows][:, None]
        self.idx = np.minimum(starts[rows][:, None] + cols, n - 1)

    def take(self, x, dtype):
        v = x[self.idx].astype(dtype)
        m = self.valid if v.ndim == 2 else self.valid[..., None]
        return np.where(m, v, dtype(0))

    def put(self, out, val):
        out[self.idx[self.valid]] = val[self.valid]


def _bg(bg_mode, bkgd, dtype):
    if bg_mode == BG_WHITE:
        return np.ones(3, dtype)
    if bg_mode == BG_CUSTOM:
        return np.asarray(bkgd, dtype=np.float32).astype(dtype)
    return np.zeros(3, dtype)


def _ray_grads(ids, n_rays, g, width, dtype):
    """Upstream gradient rows of the runs' rays; zero for ids outside the image or a missing gradient."""
    out = np.zeros((len(ids), width), dtype)
    if g is None:
        return out
    inside = (ids >= 0) & (ids < n_rays)
    out[inside] = np.asarray(g).reshape(n_rays, width)[ids[inside]].astype(dtype)
    return out


def _excl_prefix(x):
    inc = np.cumsum(x, axis=1)
    return np.concatenate([np.zeros_like(x[:, :1]), inc[:, :-1]], axis=1)


def _excl_suffix(x):
    inc = np.cumsum(x[:, ::-1], axis=1)[:, ::-1]
    return np.concatenate([inc[:, 1:], np.zeros_like(x[:, :1])], axis=1)


def _floor(m, valid):
    """Floor M at FLOOR x its maximum over the ray's samples (and channels)."""
    mm = np.where(valid if m.ndim == 2 else valid[..., None], m, 0.0)
    top = mm.max(axis=tuple(range(1, m.ndim)), keepdims=True)
    return np.where(top > 0, np.maximum(np.maximum(mm, FLOOR * top), TINY), 0.0)


# ------------------------------------------------------------------------------------------------- float64 reference
def reference(case, bg_mode, bkgd=BKGD, g_rgb=None, g_alpha=None, g_depth=None, g_alpha_mag=None, g_depth_mag=None,
              inclusive=False):
    """Forward and backward of the compositing in float64 from the fp32 inputs of ``case``.

    Returns a dict of (value, M) pairs.  Per sample [n]: weights, trans, alphas, grad_sigma, grad_depth; [n, 3]:
    grad_color.  Per ray [n_rays]: alpha, depth, depth_norm (D / max(A, eps32)); [n_rays, 3]: rgb, plain (= C).
    ``inclusive``: T_j = exp(-(cum_j + tau_j)) as kaolin's non-exclusive exponential_integration (forward only).
    ``g_*_mag``: magnitudes of the upstream gradients when those were themselves computed in fp32."""
    f = np.float64
    sigma, delta = case["sigma"], case["delta"]
    n, n_rays = sigma.shape[0], int(case["n_rays"])
    starts, counts, ids = ray_runs(case["index_ray"])
    bg = _bg(bg_mode, bkgd, f)
    plain = bg_mode == BG_NONE
    fill = 1.0 if bg_mode in (BG_WHITE, BG_CUSTOM) else 0.0
    per_s = {k: (np.zeros(n, f), np.zeros(n, f)) for k in ("weights", "trans", "alphas", "grad_sigma", "grad_depth")}
    per_s["grad_color"] = (np.zeros((n, 3), f), np.zeros((n, 3), f))
    per_r = {"rgb": (np.full((n_rays, 3), fill, f), np.zeros((n_rays, 3), f)),
             "plain": (np.zeros((n_rays, 3), f), np.zeros((n_rays, 3), f))}
    for k in ("alpha", "depth", "depth_norm"):
        per_r[k] = (np.zeros(n_rays, f), np.zeros(n_rays, f))
    with np.errstate(over="ignore", invalid="raise"):
        for rows, k in _groups(counts):
            p = _Pad(starts, counts, rows, k, n)
            v = p.valid
            tau = p.take(sigma, f) * p.take(delta, f)
            c, t = p.take(case["rgb"], f), p.take(case["depth"], f)
            cum = _excl_prefix(tau)
            T = np.exp(-(cum + tau)) if inclusive else np.exp(-cum)
            e = np.exp(-tau)
            alpha = -np.expm1(-tau)
            w = T * alpha
            # error of the fp32 running sum cum_j: u x the sum of its partial sums, carried into T by the exponential
            S = np.where(T > 0, np.cumsum(np.where(T > 0, cum, 0.0), axis=1), 0.0)
            mw = (T * (1.0 + e) + w * S) * v
            C, A, D = (w[..., None] * c).sum(1), w.sum(1), (w * t).sum(1)
            mC, mA, mD = (mw[..., None] * np.abs(c)).sum(1), mw.sum(1), (mw * np.abs(t)).sum(1)
            if bg_mode == BG_WHITE:
                px, mpx = (1.0 - A)[:, None] + A[:, None] * C, 1.0 + mA[:, None] + mA[:, None] * mC
            elif bg_mode == BG_BLACK:
                px, mpx = A[:, None] * C, mA[:, None] * mC
            elif plain:
                px, mpx = C, mC
            else:
                px = A[:, None] * C + (1.0 - A)[:, None] * bg
                mpx = mA[:, None] * mC + (1.0 + mA)[:, None] * np.abs(bg)
            den = np.maximum(A, EPS32)
            inside = (ids[rows] >= 0) & (ids[rows] < n_rays)
            rid = ids[rows][inside]
            for name, val, mag in (("rgb", px, mpx), ("plain", C, mC), ("alpha", A, mA), ("depth", D, mD),
                                   ("depth_norm", D / den, mD / den + np.abs(D) * mA / den ** 2)):
                per_r[name][0][rid] = val[inside]
                per_r[name][1][rid] = np.where(mag > 0, np.maximum(mag, TINY), 0.0)[inside]
            # backward
            r_ids = ids[rows]
            gr = _ray_grads(r_ids, n_rays, g_rgb, 3, f)
            ga = _ray_grads(r_ids, n_rays, g_alpha, 1, f)[:, 0]
            gd = _ray_grads(r_ids, n_rays, g_depth, 1, f)[:, 0]
            ga_m = np.abs(ga) if g_alpha_mag is None else _ray_grads(r_ids, n_rays, g_alpha_mag, 1, f)[:, 0]
            gd_m = np.abs(gd) if g_depth_mag is None else _ray_grads(r_ids, n_rays, g_depth_mag, 1, f)[:, 0]
            if plain:
                gC, gA = gr, ga
                gC_m, gA_m = np.abs(gr), ga_m
            else:
                gC, gA = A[:, None] * gr, ga + (gr * (C - bg)).sum(1)
                gC_m, gA_m = mA[:, None] * np.abs(gr), ga_m + (np.abs(gr) * (mC + np.abs(bg))).sum(1)
            gw = (c * gC[:, None, :]).sum(2) + gA[:, None] + gd[:, None] * t
            gw_m = (np.abs(c) * gC_m[:, None, :]).sum(2) + gA_m[:, None] + gd_m[:, None] * np.abs(t)
            dl = p.take(delta, f)
            g_sig = dl * (gw * T * e - _excl_suffix(gw * w))
            m_sig = dl * (gw_m * T * e * (1.0 + S) + _excl_suffix(gw_m * mw))
            for name, val, mag in (("weights", w, mw), ("trans", T, T * (1.0 + S)),
                                   ("alphas", alpha, 1.0 + e), ("grad_sigma", g_sig, m_sig),
                                   ("grad_depth", w * gd[:, None], mw * gd_m[:, None]),
                                   ("grad_color", w[..., None] * gC[:, None, :], mw[..., None] * gC_m[:, None, :])):
                p.put(per_s[name][0], val)
                p.put(per_s[name][1], _floor(mag, v))
    out = dict(per_s)
    out.update(per_r)
    return out


def rendering_reference(case, render_bkgd, g_colors, g_opac, g_depths):
    """The training branch of ``field_rendering.rendering``: colors = C + bkgd (1 - A), opacities = A, depths =
    D / max(A, eps32), and the gradients of sum(colors g_colors + opacities g_opac + depths g_depths) w.r.t. the
    samples.  Returns (reference dict in mode none, colors (value, M))."""
    fwd = reference(case, BG_NONE)
    f = np.float64
    A, mA = fwd["alpha"]
    D, mD = fwd["depth"]
    C, mC = fwd["plain"]
    bk = np.zeros(3, f) if render_bkgd is None else np.asarray(render_bkgd, dtype=np.float32).astype(f)
    gc, go, gd = (np.asarray(x, dtype=np.float32).astype(f) for x in (g_colors, g_opac, g_depths))
    go, gd = go.reshape(-1), gd.reshape(-1)
    live = A > EPS32                                             # clamp_min passes no gradient below eps
    den = np.maximum(A, EPS32)
    g_a = go - (gc * bk).sum(1) - np.where(live, gd * D / den ** 2, 0.0)
    g_a_m = np.abs(go) + (np.abs(gc) * np.abs(bk)).sum(1) + np.where(live, np.abs(gd) * (mD / den ** 2 + 2 * np.abs(D) * mA / den ** 3), 0.0)
    g_d = gd / den
    g_d_m = np.abs(gd) * (1.0 / den + mA / den ** 2)
    ref = reference(case, BG_NONE, None, gc, g_a, g_d, g_a_m, g_d_m)
    colors = C + bk[None, :] * (1.0 - A)[:, None]
    m_colors = mC + np.abs(bk)[None, :] * (1.0 + mA)[:, None]
    return ref, (colors, m_colors)


def err_ratio(got, ref, mag):
    """|got - ref| / (u M); 0 where both the error and M are 0; inf where got is not finite or errs against M = 0."""
    got = np.asarray(got, dtype=np.float64).reshape(ref.shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(got - ref)
        r = np.where(err == 0.0, 0.0, err / (U * mag))
    return np.where(np.isfinite(got), r, np.inf)


# ------------------------------------------------------------------------------------------------- fp32 restatements
def restate_fp32(case, bg_mode, bkgd=BKGD, g_rgb=None, g_alpha=None, g_depth=None, prefix="keep", inclusive=False):
    """The kernels' algorithm in numpy float32, sample after sample: a forward sweep that accumulates cum and the sums,
    a backward sweep from the far end.  ``prefix``: "keep" (each sample's exclusive cum remembered from the forward
    sweep) or "subtract" (rebuilt as cum -= tau from the total).  Returns float32 arrays under the names of
    ``reference``."""
    assert prefix in ("keep", "subtract")
    f = np.float32
    sigma, delta = case["sigma"], case["delta"]
    n, n_rays = sigma.shape[0], int(case["n_rays"])
    starts, counts, ids = ray_runs(case["index_ray"])
    bg = _bg(bg_mode, bkgd, f)
    plain = bg_mode == BG_NONE
    fill = 1.0 if bg_mode in (BG_WHITE, BG_CUSTOM) else 0.0
    out = {k: np.zeros(n, f) for k in ("weights", "trans", "alphas", "grad_sigma", "grad_depth")}
    out["grad_color"] = np.zeros((n, 3), f)
    out["rgb"] = np.full((n_rays, 3), fill, f)
    out["plain"] = np.zeros((n_rays, 3), f)
    for k in ("alpha", "depth", "depth_norm"):
        out[k] = np.zeros(n_rays, f)
    one = f(1.0)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for rows, kk in _groups(counts):
            p = _Pad(starts, counts, rows, kk, n)
            sg, dl, c, t = p.take(sigma, f), p.take(delta, f), p.take(case["rgb"], f), p.take(case["depth"], f)
            R = len(rows)
            cum = np.zeros(R, f)
            acc = np.zeros((R, 3), f)
            ca, cd = np.zeros(R, f), np.zeros(R, f)
            pre = np.zeros((R, kk), f)
            w_f, T_f, a_f = np.zeros((R, kk), f), np.zeros((R, kk), f), np.zeros((R, kk), f)
            for j in range(kk):
                tau = sg[:, j] * dl[:, j]
                if inclusive:
                    cum = cum + tau
                al = one - np.exp(-tau)
                T = np.exp(-cum)
                w = T * al
                pre[:, j] = cum
                if not inclusive:
                    cum = cum + tau
                acc = acc + w[:, None] * c[:, j]
                cd = cd + w * t[:, j]
                ca = ca + w
                w_f[:, j], T_f[:, j], a_f[:, j] = w, T, al
            rest = one - ca
            if bg_mode == BG_WHITE:
                px = ca[:, None] * acc + rest[:, None]
            elif bg_mode == BG_BLACK:
                px = ca[:, None] * acc
            elif plain:
                px = acc
            else:
                px = ca[:, None] * acc + rest[:, None] * bg
            inside = (ids[rows] >= 0) & (ids[rows] < n_rays)
            rid = ids[rows][inside]
            out["rgb"][rid], out["plain"][rid], out["alpha"][rid], out["depth"][rid] = px[inside], acc[inside], ca[inside], cd[inside]
            out["depth_norm"][rid] = (cd / np.maximum(ca, f(EPS32)))[inside]
            for name, val in (("weights", w_f), ("trans", T_f), ("alphas", a_f)):
                p.put(out[name], val)
            if inclusive:
                continue
            gr = _ray_grads(ids[rows], n_rays, g_rgb, 3, f)
            ga = _ray_grads(ids[rows], n_rays, g_alpha, 1, f)[:, 0]
            gd = _ray_grads(ids[rows], n_rays, g_depth, 1, f)[:, 0]
            if plain:
                gA, gC = ga, gr
            else:
                gA = ga + (gr[:, 0] * (acc[:, 0] - bg[0]) + gr[:, 1] * (acc[:, 1] - bg[1]) + gr[:, 2] * (acc[:, 2] - bg[2]))
                gC = ca[:, None] * gr
            suffix = np.zeros(R, f)
            g_sig, g_dep, g_col = np.zeros((R, kk), f), np.zeros((R, kk), f), np.zeros((R, kk, 3), f)
            for j in range(kk - 1, -1, -1):
                tau = sg[:, j] * dl[:, j]
                if prefix == "subtract":
                    cum = cum - tau
                else:
                    cum = pre[:, j]
                T, e = np.exp(-cum), np.exp(-tau)
                w = T * (one - e)
                gw = gC[:, 0] * c[:, j, 0] + gC[:, 1] * c[:, j, 1] + gC[:, 2] * c[:, j, 2] + gA + gd * t[:, j]
                g_sig[:, j] = (gw * T * e - suffix) * dl[:, j]
                suffix = suffix + gw * w
                g_col[:, j] = w[:, None] * gC
                g_dep[:, j] = w * gd
            for name, val in (("grad_sigma", g_sig), ("grad_depth", g_dep), ("grad_color", g_col)):
                p.put(out[name], val)
    return out


# ------------------------------------------------------------------------------------------------- cases
SPIKES = {"250": 250.0, "1.6e4": 1.6e4, "1e6": 1e6, "max": FLT_MAX}
POSITIONS = ("first", "mid", "last")
FAMILIES = (["mild"] + [f"spike-{s}-{p}" for s in SPIKES for p in POSITIONS] +
            ["multi", "inf", "zero", "tiny", "zero_delta", "lengths", "outside", "single", "big"])
#: families on which the subtracting restatement must break the bars (one tau >= 1.6e4 in front of live samples)
SPIKE_FAMILIES = [f"spike-{s}-{p}" for s in ("1.6e4", "1e6", "max") for p in ("mid", "last")] + ["multi", "lengths", "big"]
DELTA = 0.005


def _assemble(rng, counts, ids=None, n_rays=None, sigma_scale=48.0):
    """Packed samples for rays of ``counts`` samples (0 = an empty ray): mild densities (tau <= 0.24), colours in
    [0, 1), depths ascending along each ray, upstream gradients with exact zeros."""
    counts = np.asarray(counts, dtype=np.int64)
    ids = np.arange(len(counts), dtype=np.int64) if ids is None else np.asarray(ids, dtype=np.int64)
    n_rays = len(counts) if n_rays is None else n_rays
    n = int(counts.sum())
    index_ray = np.repeat(ids, counts)
    sigma = (rng.random(n) * sigma_scale).astype(np.float32)
    rank = np.arange(n) - np.repeat(np.cumsum(counts) - counts, counts)
    depth = (2.0 + 0.01 * rank + 0.005 * rng.random(n)).astype(np.float32)
    g_rgb = rng.standard_normal((n_rays, 3)).astype(np.float32)
    g_alpha = rng.standard_normal(n_rays).astype(np.float32)
    g_depth = rng.standard_normal(n_rays).astype(np.float32)
    g_rgb[rng.random(n_rays) < 0.05] = 0.0
    g_alpha[rng.random(n_rays) < 0.1] = 0.0
    g_depth[rng.random(n_rays) < 0.1] = 0.0
    return dict(sigma=sigma, delta=np.full(n, DELTA, np.float32), rgb=rng.random((n, 3)).astype(np.float32),
                depth=depth.astype(np.float32), index_ray=index_ray, n_rays=n_rays, g_rgb=g_rgb, g_alpha=g_alpha,
                g_depth=g_depth, delta_const=DELTA)


def _set_tau(case, where, tau):
    """Make tau = sigma * delta equal ``tau`` at samples ``where``; the largest finite fp32 needs delta = 1."""
    if tau >= FLT_MAX:
        case["sigma"][where] = FLT_MAX
        case["delta"][where] = 1.0
        case["delta_const"] = None
    else:
        case["sigma"][where] = np.float32(tau) / case["delta"][where]


def _spike_at(rng, starts, counts, position):
    if position == "first":
        off = np.zeros_like(counts)
    elif position == "last":
        off = counts - 1
    else:
        off = np.minimum(counts - 1, np.maximum(1, (counts * rng.uniform(0.3, 0.8, len(counts))).astype(np.int64)))
    return starts + off


def _random_counts(rng, n_rays, lo=2, hi=25, empty=0.15):
    c = rng.integers(lo, hi + 1, n_rays)
    c[rng.random(n_rays) < empty] = 0
    c[0], c[-1] = hi, lo                                   # the first and last rays are never empty
    return c


def make_case(family, seed=0, stride=2048 * 256):
    """The inputs of one case family (see FAMILIES).  ``stride``: threads of one sweep of the backward kernel's grid
    (2048 x compute units), which the family "big" exceeds."""
    rng = np.random.default_rng([seed, sum(map(ord, family))])
    if family.startswith("spike-"):
        _, mag, pos = family.split("-")
        case = _assemble(rng, _random_counts(rng, 400))
        s, c, _ = ray_runs(case["index_ray"])
        _set_tau(case, _spike_at(rng, s, c, pos), SPIKES[mag])
        return case
    if family == "mild":
        return _assemble(rng, _random_counts(rng, 400))
    if family == "multi":                                  # three spikes of different sizes on every ray, two the largest tau
        case = _assemble(rng, np.where(rng.random(300) < 0.1, 0, 25))
        s, c, _ = ray_runs(case["index_ray"])
        for k, r0 in enumerate(s):
            at = r0 + np.sort(rng.choice(25, 3, replace=False))
            mags = rng.permutation([250.0, 1.6e4, 1e6, FLT_MAX, FLT_MAX])[:3] if k % 4 == 0 else rng.permutation([250.0, 1.6e4, 1e6])
            for a, m in zip(at, mags):
                _set_tau(case, np.array([a]), float(m))
        return case
    if family == "inf":                                    # sigma = +inf, delta > 0
        case = _assemble(rng, _random_counts(rng, 300))
        s, c, _ = ray_runs(case["index_ray"])
        case["sigma"][_spike_at(rng, s, c, "mid")] = np.inf
        case["sigma"][s[::7]] = np.inf                     # first on the ray
        case["sigma"][(s + c - 1)[3::7]] = np.inf          # last, some rays with two
        return case
    if family == "zero":                                   # every third ray has no density at all
        case = _assemble(rng, _random_counts(rng, 300))
        case["sigma"][case["index_ray"] % 3 == 0] = 0.0
        return case
    if family == "tiny":                                   # tau ~ 1e-8: 1 - expf(-tau) = 0 in fp32
        return _assemble(rng, _random_counts(rng, 300), sigma_scale=4e-6)
    if family == "zero_delta":
        case = _assemble(rng, _random_counts(rng, 300))
        case["delta"] = (rng.random(len(case["sigma"])) * 0.01).astype(np.float32)
        case["delta"][rng.random(len(case["sigma"])) < 0.3] = 0.0
        case["delta_const"] = None
        return case
    if family == "lengths":                                # occupancy-grid marching: up to 2 500 samples on a ray
        counts = [1, 2, 25, 0, 64, 400, 0, 0, 2500, 1, 65, 2500, 3, 0, 400, 1089, 64, 2, 1]
        case = _assemble(rng, counts, sigma_scale=8.0)
        s, c, _ = ray_runs(case["index_ray"])
        long_ = c >= 25
        _set_tau(case, _spike_at(rng, s[long_], c[long_], "mid"), 1.6e4)
        _set_tau(case, (s + c - 1)[c == 2500], 1e6)
        return case
    if family == "outside":                                # ray ids < 0 and >= n_rays: no pixel, zero gradient
        counts = _random_counts(rng, 60, empty=0.0)
        ids = np.concatenate([[-7, -3, -1], np.arange(50), [50, 53, 54, 60, 2 ** 40, 2 ** 40 + 1, 2 ** 62]])
        case = _assemble(rng, counts, ids=np.sort(ids)[:60], n_rays=50)
        s, c, _ = ray_runs(case["index_ray"])
        _set_tau(case, _spike_at(rng, s[::2], c[::2], "mid"), 1e6)
        return case
    if family == "single":
        return _assemble(rng, [0, 0, 1, 0])
    if family == "big":                                    # more samples than one sweep of the grid, ragged tail
        counts = list(_random_counts(rng, stride // 10 + 200, empty=0.1))
        cs = np.cumsum(counts)
        cut = int(np.searchsorted(cs, stride - 7 - 40))
        counts = counts[:cut + 1]
        counts += [stride - 7 - int(cs[cut]), 25]            # the 25-sample ray starts 7 samples before the stride boundary
        assert sum(counts) == stride + 18 and 1 <= counts[-2] <= 60
        counts += list(_random_counts(rng, 150, empty=0.1))
        if sum(counts) % 256 == 0:
            counts.append(1)
        case = _assemble(rng, counts)
        s, c, _ = ray_runs(case["index_ray"])
        _set_tau(case, _spike_at(rng, s[::4], c[::4], "mid"), 1e6)
        _set_tau(case, _spike_at(rng, s[1::4], c[1::4], "last"), 1.6e4)
        at = int(np.searchsorted(s, stride - 7))
        assert s[at] == stride - 7 and c[at] == 25
        _set_tau(case, np.array([stride + 9]), 1e6)        # the straddling ray: spike behind the boundary
        return case
    raise KeyError(family)
