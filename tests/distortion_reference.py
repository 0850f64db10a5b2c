"""fp64 CPU references of the distortion loss (numpy).  Both take packed samples -- ``w``, ``m``, ``delta`` [n],
``ray_id`` [n] nondecreasing -- and ``n_rays``, and return ``(loss, dloss/dw)`` in float64.

``pairwise``: the Mip-NeRF-360 definition, O(c^2) per ray:
    L_ray = sum_ij w_i w_j |m_i - m_j| + (1/3) sum_i w_i^2 delta_i,   dL/dw_k = 2 sum_j w_j |m_k - m_j| + (2/3) w_k delta_k
``ordered``: the sum in stored order the kernel computes, O(c) per ray with prefix sums:
    L_ray = sum_i sum_{j<i} 2 w_i w_j (m_i - m_j) + (1/3) sum_i w_i^2 delta_i
    dL/dw_k = 2 (m_k (P_k - S_k) + (SM_k - PM_k)) + (2/3) w_k delta_k
They agree when ``m`` is nondecreasing along every ray.
"""
import numpy as np


def _prepare(w, m, delta, ray_id):
    w = np.asarray(w, dtype=np.float64).reshape(-1)
    m = np.asarray(m, dtype=np.float64).reshape(-1)
    delta = np.broadcast_to(np.asarray(delta, dtype=np.float64), w.shape)
    ray_id = np.asarray(ray_id, dtype=np.int64).reshape(-1)
    assert w.shape == m.shape == ray_id.shape
    assert ray_id.size == 0 or (np.all(np.diff(ray_id) >= 0) and ray_id[0] >= 0)
    bounds = np.flatnonzero(np.diff(ray_id)) + 1 if ray_id.size else np.zeros(0, dtype=np.int64)
    starts = np.concatenate([[0], bounds]) if ray_id.size else bounds
    ends = np.concatenate([bounds, [ray_id.size]]) if ray_id.size else bounds
    return w, m, delta, starts.astype(np.int64), ends.astype(np.int64)


def pairwise(w, m, delta, ray_id, n_rays):
    w, m, delta, starts, ends = _prepare(w, m, delta, ray_id)
    grad = np.zeros_like(w)
    loss = 0.0
    for a, b in zip(starts, ends):
        ww, mm, dd = w[a:b], m[a:b], delta[a:b]
        dist = np.abs(mm[:, None] - mm[None, :])
        loss += float(ww @ dist @ ww) + float(np.sum(ww * ww * dd)) / 3.0
        grad[a:b] = 2.0 * (dist @ ww) + (2.0 / 3.0) * ww * dd
    return loss / n_rays, grad / n_rays


def ordered(w, m, delta, ray_id, n_rays):
    w, m, delta, starts, ends = _prepare(w, m, delta, ray_id)
    grad = np.zeros_like(w)
    loss = 0.0
    for a, b in zip(starts, ends):
        ww, mm, dd = w[a:b], m[a:b], delta[a:b]
        wm = ww * mm
        p = np.cumsum(ww) - ww
        pm = np.cumsum(wm) - wm
        s = np.cumsum(ww[::-1])[::-1] - ww
        sm = np.cumsum(wm[::-1])[::-1] - wm
        loss += float(np.sum(2.0 * ww * (mm * p - pm))) + float(np.sum(ww * ww * dd)) / 3.0
        grad[a:b] = 2.0 * (mm * (p - s) + (sm - pm)) + (2.0 / 3.0) * ww * dd
    return loss / n_rays, grad / n_rays
