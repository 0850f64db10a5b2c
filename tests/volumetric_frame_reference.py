"""CPU restatement of the volumetric frame with early ray termination (the reference's
``render_image_with_occgrid_test``, examples/utils.py:176-350) -- TEST INFRASTRUCTURE.

Marching is numpy fp32, operation by operation, under the rule of ``oracle/occgrid.py`` (whose ``_safe_inv`` it
imports), capped at the round's quota and restarted from every ray's own near plane; compositing is fp64.  The renderer
returns what the device renderer's ``trace`` returns, round by round, and the final 5-tuple.
"""
import numpy as np

from oracle import occgrid as oocc

F = np.float32
ROUND_CAP = 64


def n_samples_for(num_rays: int, n_alive: int) -> int:
    """Samples every alive ray may add in a round (min_samples = 1: one grid level, cone_angle = 0)."""
    return max(min(num_rays // n_alive, ROUND_CAP), 1)


def schedule(num_rays: int, max_samples: int, alive_counts):
    """The (n_samples, iter_samples) of the rounds that run when round i starts with ``alive_counts[i]`` alive rays: the
    bound is tested BEFORE a round, so the last round may overshoot ``max_samples``."""
    out, it = [], 0
    for n_alive in alive_counts:
        if not it < max_samples or n_alive == 0:
            break
        n = n_samples_for(num_rays, n_alive)
        it += n
        out.append((n, it))
    return out


def _ranges(aabb, o, d, near, far_plane):
    lo, hi = aabb[:3], aabb[3:]
    inv = oocc._safe_inv(d)
    a = ((lo - o) * inv).astype(F)
    b = ((hi - o) * inv).astype(F)
    tn, tf = np.minimum(a, b).max(axis=1), np.maximum(a, b).min(axis=1)
    t0, t1 = np.maximum(tn, near), np.minimum(tf, F(far_plane))
    return t0, t1, (tn <= tf) & (t0 < t1)


def march_round(aabb, binaries, rays_o, rays_d, near, alive, quota, far_plane, step, chunk=128):
    """One round: (ray_indices, t_starts, t_ends, count [R], term [R]).  Samples grouped by ray, front to back; ``term`` is
    the t_end of the last kept sample of a ray that filled ``quota``, the clipped exit t1 of any other alive ray, and
    the old near plane of a dead ray."""
    aabb = np.asarray(aabb, dtype=F)
    lo, hi = aabb[:3], aabb[3:]
    res = np.array(binaries.shape, dtype=np.int64)
    resf = res.astype(F)
    step = F(step)
    idx = np.nonzero(alive)[0]
    o, d = rays_o[idx], rays_d[idx]
    t0, t1, hit = _ranges(aabb, o, d, near[idx], far_plane)
    kept = np.zeros(idx.shape[0], dtype=np.int64)
    last_end = np.zeros(idx.shape[0], dtype=F)
    done = ~hit
    rows = []
    k0 = 0
    while not done.all():
        act = np.nonzero(~done)[0]
        k = np.arange(k0, k0 + chunk, dtype=np.int64)
        ts = t0[act, None] + (k.astype(F) * step)[None, :]
        te = t0[act, None] + ((k + 1).astype(F) * step)[None, :]
        tm = (ts + te) * F(0.5)
        before = np.logical_and.accumulate(tm < t1[act, None], axis=1)      # the march stops at the first midpoint past t1
        p = o[act, None, :] + d[act, None, :] * tm[:, :, None]
        u = (p - lo) / (hi - lo) * resf
        f = np.floor(u)
        inside = ((f >= 0) & (f < resf)).all(axis=2)
        c = np.clip(f.astype(np.int64), 0, res - 1)
        keep = before & inside & binaries[c[..., 0], c[..., 1], c[..., 2]]
        rank = kept[act, None] + np.cumsum(keep, axis=1)
        keep &= rank <= quota
        assert ts.dtype == te.dtype == tm.dtype == u.dtype == F
        a, j = np.nonzero(keep)
        rows.append((idx[act[a]], k[j], ts[a, j], te[a, j]))
        full = keep & (rank == quota)
        fa, fj = np.nonzero(full)
        last_end[act[fa]] = te[fa, fj]
        kept[act] += keep.sum(axis=1)
        done[act] = (kept[act] >= quota) | ~before[:, -1]
        k0 += chunk
    count = np.zeros(rays_o.shape[0], dtype=np.int32)
    term = near.copy()
    count[idx] = kept
    term[idx] = np.where(kept == quota, last_end, t1)
    if rows:
        r, k, ts, te = (np.concatenate(x) for x in zip(*rows))
        order = np.lexsort((k, r))
        return r[order].astype(np.int64), ts[order], te[order], count, term
    return np.zeros(0, np.int64), np.zeros(0, F), np.zeros(0, F), count, term


def positions_of(rays_o, rays_d, ray_indices, t_starts, t_ends):
    """o + d * (t_start + t_end) / 2 in fp32, every operation rounded."""
    return rays_o[ray_indices] + (rays_d[ray_indices] * (t_starts + t_ends)[:, None]) / F(2.0)


def composite_round(opacity, rgb, depth, ray_indices, t_starts, t_ends, sigmas, rgbs, count, alpha_thre):
    """fp64 update of the per-ray state in place; returns the number of samples the alpha filter leaves."""
    starts = np.cumsum(count) - count
    cum = np.zeros(opacity.shape[0])
    prefix = 1.0 - opacity
    add_o, add_d, add_c = np.zeros_like(opacity), np.zeros_like(depth), np.zeros_like(rgb)
    passed = 0
    ts64, te64 = t_starts.astype(np.float64), t_ends.astype(np.float64)
    for j in range(int(count.max()) if count.size else 0):
        rr = np.nonzero(count > j)[0]
        s = starts[rr] + j
        sdt = sigmas[s].astype(np.float64) * (te64[s] - ts64[s])
        alpha = 1.0 - np.exp(-sdt)
        w = prefix[rr] * np.exp(-cum[rr]) * alpha
        cum[rr] += sdt                                   # the filter is applied after the weights: T is attenuated anyway
        if alpha_thre > 0:
            vis = alpha >= alpha_thre
            rr, s, w = rr[vis], s[vis], w[vis]
        add_o[rr] += w
        add_d[rr] += w * (ts64[s] + te64[s]) / 2.0
        add_c[rr] += w[:, None] * rgbs[s].astype(np.float64)
        passed += rr.shape[0]
    opacity += add_o
    depth += add_d
    rgb += add_c
    return passed


def render(max_samples, field_fn, aabb, binaries, rays_o, rays_d, near_plane=0.0, far_plane=1e10, render_step_size=1e-3,
           render_bkgd=None, alpha_thre=0.0, early_stop_eps=1e-4):
    """``field_fn(positions fp32 [n,3], dirs fp32 [n,3]) -> (rgb [n,3], sigma [n])``.  Returns (rounds, (rgb [R,3],
    opacity [R], depth [R], total_samples, positions [S,3])); a round is a dict with ``n_alive``, ``n_samples``,
    ``ray_indices``, ``t_starts``, ``t_ends``, ``positions``, and -- after the round -- ``alive``, ``near``, ``opacity``."""
    rays_o, rays_d = np.asarray(rays_o, dtype=F), np.asarray(rays_d, dtype=F)
    binaries = np.asarray(binaries, dtype=bool)
    num_rays = rays_o.shape[0]
    opacity, depth, rgb = np.zeros(num_rays), np.zeros(num_rays), np.zeros((num_rays, 3))
    near = np.full(num_rays, F(near_plane), dtype=F)
    alive = np.ones(num_rays, dtype=bool)
    opc_thre = float(F(1.0 - early_stop_eps))
    rounds, positions_all = [], []
    iter_samples = total_samples = 0
    while iter_samples < max_samples:
        n_alive = int(alive.sum())
        if n_alive == 0:
            break
        n_samples = n_samples_for(num_rays, n_alive)
        iter_samples += n_samples
        ridx, ts, te, count, term = march_round(aabb, binaries, rays_o, rays_d, near, alive, n_samples, far_plane,
                                                render_step_size)
        pos = positions_of(rays_o, rays_d, ridx, ts, te)
        assert pos.dtype == F
        positions_all.append(pos)
        if ridx.shape[0]:
            rgbs, sigmas = field_fn(pos, rays_d[ridx])
            rgbs, sigmas = np.asarray(rgbs).reshape(-1, 3), np.asarray(sigmas).reshape(-1)
        else:
            rgbs, sigmas = np.zeros((0, 3)), np.zeros(0)
        total_samples += composite_round(opacity, rgb, depth, ridx, ts, te, sigmas, rgbs, count, alpha_thre)
        near = term
        alive = alive & (opacity <= opc_thre) & (count == n_samples)
        rounds.append({"n_alive": n_alive, "n_samples": n_samples, "ray_indices": ridx, "t_starts": ts, "t_ends": te,
                       "positions": pos, "count": count, "alive": alive.copy(), "near": near.copy(),
                       "opacity": opacity.copy()})
    if render_bkgd is not None:
        rgb = rgb + np.asarray(render_bkgd, dtype=np.float64)[None, :] * (1.0 - opacity)[:, None]
    positions = np.concatenate(positions_all) if positions_all else np.zeros((0, 3), F)
    return rounds, (rgb, opacity, depth, total_samples, positions)


def threshold_margin(rounds, early_stop_eps):
    """Per ray, the least |opacity - opc_thre| over the ends of the rounds it entered alive (inf for none)."""
    opc_thre = float(F(1.0 - early_stop_eps))
    n = rounds[0]["alive"].shape[0] if rounds else 0
    margin = np.full(n, np.inf)
    entered = np.ones(n, dtype=bool)
    for r in rounds:
        margin[entered] = np.minimum(margin[entered], np.abs(r["opacity"][entered] - opc_thre))
        entered = r["alive"]
    return margin


def mark_visited_cells(p01, m):
    """(mask bool [m,m,m], out_of_range): the numpy restatement of ``qf_mark_visited_cells``."""
    p = np.asarray(p01, dtype=F)
    ok = ((p >= 0) & (p <= 1)).all(axis=1)
    u = p[ok] * F(m - 1)
    mask = np.zeros((m, m, m), dtype=bool)
    for c in (np.floor(u).astype(np.int64), np.ceil(u).astype(np.int64)):
        mask[c[:, 0], c[:, 1], c[:, 2]] = True
    return mask, int((~ok).sum())
