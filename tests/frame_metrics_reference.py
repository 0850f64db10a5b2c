"""CPU references of the frame metrics (no project imports).

* ``ssim_torchmetrics(p, t, dtype)``: SSIM in the shape torchmetrics' ``StructuralSimilarityIndexMeasure(data_range=1)``
  computes it -- reflect-pad by 5, stack the five quantities, depthwise ``conv2d`` with the 11x11 Gaussian, crop by 5,
  mean.  In fp64 it is THE REFERENCE of the tests; in fp32 it is THE YARDSTICK: what a user of the reference gets.
* ``ssim_scipy(p, t)``: an independent fp64 statement through ``scipy.ndimage.correlate1d`` on the valid region.
* ``box_downsample64``, ``mse64`` and ``cases()``: seeded (render, ground truth, depth) generators.
"""
import numpy as np
import torch
import torch.nn.functional as F

KERNEL_SIZE, SIGMA, K1, K2 = 11, 1.5, 0.01, 0.03
PAD = (KERNEL_SIZE - 1) // 2
C1, C2 = (K1 * 1.0) ** 2, (K2 * 1.0) ** 2


def gaussian(dtype=torch.float64) -> torch.Tensor:
    """torchmetrics' ``_gaussian(11, 1.5, dtype)``: [11], normalised to sum 1, built in ``dtype``."""
    dist = torch.arange((1 - KERNEL_SIZE) / 2, (1 + KERNEL_SIZE) / 2, 1, dtype=dtype)
    gauss = torch.exp(-torch.pow(dist / SIGMA, 2) / 2)
    return gauss / gauss.sum()


def _nchw(x, dtype) -> torch.Tensor:
    x = torch.as_tensor(np.asarray(x)) if not isinstance(x, torch.Tensor) else x
    return x.detach().cpu().to(dtype).permute(2, 0, 1).unsqueeze(0)


def ssim_windows(p: torch.Tensor, t: torch.Tensor, padding="reflect") -> torch.Tensor:
    """torchmetrics' computation on [1, C, H, W] tensors, in their dtype and on their device: the SSIM of every kept window,
    [1, C, H-10, W-10]."""
    channels = p.shape[1]
    g = gaussian(p.dtype).to(p.device).unsqueeze(0)
    kernel = torch.matmul(g.t(), g).expand(channels, 1, KERNEL_SIZE, KERNEL_SIZE)
    p = F.pad(p, (PAD, PAD, PAD, PAD), mode=padding)
    t = F.pad(t, (PAD, PAD, PAD, PAD), mode=padding)
    stack = torch.cat((p, t, p * p, t * t, p * t))
    out = F.conv2d(stack, kernel, groups=channels)
    mu_p, mu_t, e_pp, e_tt, e_pt = (out[i:i + 1] for i in range(5))
    mu_pp, mu_tt, mu_pt = mu_p * mu_p, mu_t * mu_t, mu_p * mu_t
    s_pp, s_tt, s_pt = e_pp - mu_pp, e_tt - mu_tt, e_pt - mu_pt
    full = ((2 * mu_pt + C1) * (2 * s_pt + C2)) / ((mu_pp + mu_tt + C1) * (s_pp + s_tt + C2))
    return full[..., PAD:-PAD, PAD:-PAD]


def ssim_torchmetrics(p, t, dtype=torch.float64, padding="reflect"):
    """(map [H-10, W-10, 3], mean) of [H, W, 3] images ``p`` (prediction) and ``t`` (target), computed in ``dtype`` on the
    CPU.  ``padding``: "reflect" as torchmetrics pads, or "constant" (zeros): the crop removes every value the padding
    reaches."""
    kept = ssim_windows(_nchw(p, dtype), _nchw(t, dtype), padding)
    return kept[0].permute(1, 2, 0).contiguous(), kept.mean().item()


def ssim_scipy(p, t):
    """fp64 (map [H-10, W-10, 3], mean): the same definition by two 1-D correlations, valid region only."""
    from scipy.ndimage import correlate1d
    p, t = np.asarray(p, dtype=np.float64), np.asarray(t, dtype=np.float64)
    g = gaussian(torch.float64).numpy()

    def blur(x):
        y = correlate1d(correlate1d(x, g, axis=0, mode="constant"), g, axis=1, mode="constant")
        return y[PAD:-PAD, PAD:-PAD]

    mu_p, mu_t = blur(p), blur(t)
    s_pp, s_tt, s_pt = blur(p * p) - mu_p * mu_p, blur(t * t) - mu_t * mu_t, blur(p * t) - mu_p * mu_t
    m = ((2 * mu_p * mu_t + C1) * (2 * s_pt + C2)) / ((mu_p * mu_p + mu_t * mu_t + C1) * (s_pp + s_tt + C2))
    return m, float(m.mean())


def box_downsample64(x, f: int) -> np.ndarray:
    """fp64 mean of every f x f block of [H*f, W*f(, C)]."""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[0] // f, x.shape[1] // f
    return x.reshape(h, f, w, f, *x.shape[2:]).mean(axis=(1, 3))


def box_mean_abs64(x, f: int) -> np.ndarray:
    """fp64 mean of |x| over every f x f block: the scale of the down-sample's rounding error."""
    return box_downsample64(np.abs(np.asarray(x, dtype=np.float64)), f)


def mse64(a, b) -> float:
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return float(np.mean(d * d))


def upsample_with_detail(x: np.ndarray, f: int, rng, amplitude: float) -> np.ndarray:
    """fp32 [H*f, W*f(, C)] whose f x f box average is ``x`` up to rounding: every block is its pixel plus detail of zero
    block mean (``amplitude`` 0: a plain repeat)."""
    x = np.asarray(x, dtype=np.float32)
    if f == 1:
        return x.copy()
    h, w = x.shape[:2]
    rest = x.shape[2:]
    up = np.broadcast_to(x.reshape(h, 1, w, 1, *rest).astype(np.float64), (h, f, w, f, *rest)).copy()
    if amplitude:
        detail = rng.standard_normal(up.shape) * amplitude
        detail -= detail.mean(axis=(1, 3), keepdims=True)
        up += detail
    return up.reshape(h * f, w * f, *rest).astype(np.float32)


def _smooth(h, w, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        fy, fx, ph = rng.uniform(2, 6), rng.uniform(2, 6), rng.uniform(0, 2 * np.pi)
        chans.append(0.5 + 0.35 * np.sin(2 * np.pi * fy * y / h + ph) * np.cos(2 * np.pi * fx * x / w + c))
    return np.stack(chans, axis=-1)


def _depth(h, w, rng):
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    d = 2.0 + 1.5 * np.sin(3.0 * y / h) * np.cos(2.0 * x / w) + 0.05 * rng.standard_normal((h, w))
    d[: h // 5] = 0.0                                         # rows without a hit, as a rendered frame has
    return np.maximum(d, 0.0).astype(np.float32)


# name -> (height, width, kind, noise, detail amplitude of the f > 1 inputs)
CASES = {
    "smooth400": (400, 400, "smooth", 0.05, 0.02),
    "block400": (400, 400, "block", 0.01, 0.02),
    "odd133x77": (133, 77, "smooth", 0.2, 0.02),
    "smooth800": (800, 800, "smooth", 0.02, 0.02),
    "identical": (96, 120, "identical", 0.0, 0.0),
    "constant": (64, 80, "constant", 0.0, 0.0),
}
CONSTANT_A, CONSTANT_B = 0.25, 0.75


def case(name: str, f: int = 1):
    """(render fp32 [H*f, W*f, 3], ground truth fp32 [H, W, 3], depth fp32 [H*f, W*f]) of a named case, seeded."""
    h, w, kind, noise, amplitude = CASES[name]
    rng = np.random.default_rng(sorted(CASES).index(name) + 1000)
    if kind == "smooth":
        truth = _smooth(h, w, rng)
        render = truth + noise * rng.standard_normal(truth.shape)
    elif kind == "block":                                      # the synthetic scenes' look: white with a dark object
        truth = np.ones((h, w, 3))
        truth[h // 4: 3 * h // 4, w // 3: 2 * w // 3] = np.array([0.15, 0.1, 0.2])
        render = truth.copy()
        render[h // 4 + 2: 3 * h // 4 + 2, w // 3 - 1: 2 * w // 3 - 1] = np.array([0.17, 0.1, 0.18])
        render[: h // 4] = 1.0
        render += noise * rng.standard_normal(truth.shape) * (render < 0.99)
    elif kind == "identical":
        truth = _smooth(h, w, rng)
        render = truth
    else:
        truth = np.full((h, w, 3), CONSTANT_B)
        render = np.full((h, w, 3), CONSTANT_A)
    truth = truth.astype(np.float32)
    render = render.astype(np.float32)
    depth = _depth(h, w, rng)
    up_rng = np.random.default_rng(7 * f + sorted(CASES).index(name))
    return (upsample_with_detail(render, f, up_rng, amplitude), truth,
            upsample_with_detail(depth, f, up_rng, amplitude if kind not in ("identical", "constant") else 0.0))


def cases(factors=(1, 2, 3)):
    """Yields (name, f, render, ground truth, depth) for every case and factor."""
    for name in CASES:
        for f in factors:
            yield (name, f) + case(name, f)
