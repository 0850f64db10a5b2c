"""The early-termination rule of the front-to-back baked frame, restated in numpy.  No device.

The rank-k sample of a ray (k < count) contributes iff the optical depth accumulated BEFORE it satisfies
``cum <= stop_tau``; ``cum`` is the fp32 value the compositor keeps, ``cum = cum + sigma * delta`` with the product and
the sum each rounded to fp32 on its own, so ``np.float32`` arithmetic reproduces it exactly.  ``stop_tau = +inf`` never
stops, even at ``cum = +inf``; a ray that has stopped stays stopped."""
import math

import numpy as np


def stop_tau(eps: float) -> np.float32:
    """float32(-log(eps)) for a transmittance threshold in (0, 1); +inf for 0."""
    return np.float32(np.inf) if eps == 0 else np.float32(-math.log(eps))


def contributing_counts(sigma_f32, counts, delta, stop_tau) -> np.ndarray:
    """Per ray, how many of its samples contribute.  ``sigma_f32``: the densities of all samples, ray-major and in depth
    order within a ray (rays without samples take no room); ``counts``: samples per ray.  int64 [len(counts)]."""
    sigma = np.ascontiguousarray(np.asarray(sigma_f32), dtype=np.float32).reshape(-1)
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    assert counts.sum() == sigma.shape[0], (int(counts.sum()), sigma.shape[0])
    delta, stop = np.float32(delta), np.float32(stop_tau)
    assert stop >= 0, "stop_tau must not be NaN or negative"
    never = bool(np.isposinf(stop))
    first = np.concatenate([[0], np.cumsum(counts)[:-1]])
    cum = np.zeros(counts.shape, dtype=np.float32)
    alive = np.ones(counts.shape, dtype=bool)
    kept = np.zeros(counts.shape, dtype=np.int64)
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(int(counts.max()) if counts.size else 0):
            has = counts > k
            if not never:
                alive &= ~has | (cum <= stop)               # the rule, tested where there is a rank-k sample
            go = has & alive
            tau = (sigma[(first + k)[go]] * delta).astype(np.float32)       # one multiply ...
            cum[go] = (cum[go] + tau).astype(np.float32)                     # ... and one add per sample
            kept += go
    return kept


def truncate(counts, kept, *arrays):
    """Drop every ray's non-contributing samples (rank >= kept) from ray-major per-sample arrays (numpy arrays or torch
    tensors, first axis = sample).  Returns the truncated arrays in the order given."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    kept = np.asarray(kept, dtype=np.int64).reshape(-1)
    assert (kept <= counts).all() and (kept >= 0).all()
    rank = np.arange(int(counts.sum())) - np.repeat(np.concatenate([[0], np.cumsum(counts)[:-1]]), counts)
    mask = rank < np.repeat(kept, counts)
    out = []
    for a in arrays:
        if isinstance(a, np.ndarray):
            out.append(a[mask])
        else:                                               # a torch tensor, on any device
            import torch
            out.append(a[torch.from_numpy(mask).to(a.device)])
    return tuple(out)
