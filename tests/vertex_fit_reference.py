"""Numpy restatement of the surface fit of the vertex table (include/qf_vertex_fit.h), operation
for operation: every floating-point operation is one numpy fp64 operation on exactly widened inputs, rounded on its own,
and every sum runs in the order the rule states (``seg_sum`` adds member k of every run to its run's total for
k = 0, 1, ...: a gather and an add on distinct rows, never ``numpy.sum``).  The device output is compared with this bit
for bit."""
import numpy as np

COUNT_NAMES = ("bad_sample_faces", "unsorted_samples", "nonfinite_entries", "skipped_faces", "skipped_samples",
               "inactive_vertices", "clamped_entries", "refused")
LEAF = 256


def seg_sum(values, start, length):
    """total[r] = values[start[r]] + values[start[r] + 1] + ... left to right from +0.0, for every run r."""
    total = np.zeros((start.shape[0],) + values.shape[1:], dtype=np.float64)
    for k in range(int(length.max()) if length.size else 0):
        has = length > k
        total[has] = total[has] + values[start[has] + k]
    return total


def order_key(x):
    """fp32 values as uint32 keys in the order of the values, -0.0 below +0.0."""
    b = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000))


def order_value(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    return (k ^ np.where(k >> np.uint32(31), np.uint32(0x80000000), np.uint32(0xFFFFFFFF))).view(np.float32)


def seg_extreme(keys, start, length, init, op):
    out = init.copy()
    for k in range(int(length.max()) if length.size else 0):
        has = length > k
        out[has] = op(out[has], keys[start[has] + k])
    return out


class Assembled:
    """What qf_vertex_fit_assemble leaves: rules 1 to 4 and the bounds of rule 8."""


def assemble(faces, n_vertices, sample_face, sample_bary, targets, prior, prior_weight, wide=False):
    """``wide``: take fp64 targets and prior as they are in the arithmetic of rule 4 instead of their fp32 roundings (for
    host checks of the mathematics that need inputs fp32 cannot hold; the device has no such mode)."""
    f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
    sf = np.asarray(sample_face, dtype=np.int64).reshape(-1)
    b = np.asarray(sample_bary, dtype=np.float64).reshape(-1, 3)
    y32 = np.asarray(targets, dtype=np.float32)
    x32 = np.asarray(prior, dtype=np.float32)
    V, F, N, C = int(n_vertices), f.shape[0], sf.shape[0], x32.shape[1]
    assert x32.shape == (V, C) and y32.shape == (N, C) and b.shape == (N, 3) and 1 <= C <= 64
    lam = float(prior_weight)
    a = Assembled()
    a.faces, a.V, a.F, a.N, a.C, a.lam, a.prior = f, V, F, N, C, lam, x32
    a.gram = np.zeros((F, 9))
    a.mass = np.zeros(V)
    a.rhs = np.zeros((V, C))
    counts = np.zeros(8, dtype=np.int64)
    counts[0] = ((sf < 0) | (sf >= F)).sum()
    counts[1] = (sf[1:] < sf[:-1]).sum()
    counts[2] = (~np.isfinite(b)).sum() + (~np.isfinite(y32)).sum() + (~np.isfinite(x32)).sum()
    a.counts = counts
    a.refused = bool(counts[:3].any())
    counts[7] = int(a.refused)
    if a.refused:
        return a
    ok = (((f >= 0) & (f < V)).all(axis=1) & (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 0] != f[:, 2])) \
        if F else np.zeros(0, dtype=bool)
    counts[3] = (~ok).sum()
    ids = np.arange(F, dtype=np.int64)
    s0, s1 = np.searchsorted(sf, ids, "left"), np.searchsorted(sf, ids + 1, "left")
    counts[4] = (s1 - s0)[~ok].sum()
    run_len = np.where(ok, s1 - s0, 0)
    # rule 2
    m = np.stack([seg_sum(b[:, i], s0, run_len) for i in range(3)], axis=1)                   # [F,3]
    for i in range(3):
        for j in range(i, 3):
            g = seg_sum(b[:, i] * b[:, j], s0, run_len)
            a.gram[:, 3 * i + j] = g
            a.gram[:, 3 * j + i] = g
    # corner runs: vertex << 32 | corner, sorted
    corner = np.nonzero(np.repeat(ok, 3))[0]
    keys = np.sort((f.reshape(-1)[corner].astype(np.uint64) << np.uint64(32)) | corner.astype(np.uint64))
    kv, kc = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    a.corner, a.corner_face, a.corner_i = kc, kc // 3, kc % 3
    a.cstart = np.searchsorted(kv, np.arange(V), "left")
    a.clen = np.searchsorted(kv, np.arange(V), "right") - a.cstart
    # rule 3
    a.mass = seg_sum(m.reshape(-1)[kc], a.cstart, a.clen)
    diag = seg_sum(a.gram[a.corner_face, 4 * a.corner_i], a.cstart, a.clen)
    a.ld = lam * a.mass
    av = diag + a.ld
    with np.errstate(divide="ignore"):
        a.inv = np.where(av > 0.0, 1.0 / av, 0.0)
    a.active = a.mass != 0.0
    counts[5] = (~a.active).sum()
    # rule 4
    x64, y64 = x32.astype(np.float64), y32.astype(np.float64)
    if wide:
        x64, y64 = np.asarray(prior, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    tri = f[np.where(ok[sf], sf, 0)] if N else np.zeros((0, 3), dtype=np.int64)
    tri = np.where(ok[sf][:, None], tri, 0) if N else tri
    e = y64 - ((b[:, 0:1] * x64[tri[:, 0]] + b[:, 1:2] * x64[tri[:, 1]]) + b[:, 2:3] * x64[tri[:, 2]])
    g = np.stack([seg_sum(b[:, i:i + 1] * e, s0, run_len) for i in range(3)], axis=1).reshape(3 * F, C)
    a.rhs = seg_sum(g[kc], a.cstart, a.clen)
    # the bounds of rule 8: per face over its run, then per vertex over its corners' faces and its own prior entry
    ykey, big = order_key(y32), np.uint32(0xFFFFFFFF)
    flo = seg_extreme(ykey, s0, run_len, np.full((F, C), big, dtype=np.uint32), np.minimum)
    fhi = seg_extreme(ykey, s0, run_len, np.zeros((F, C), dtype=np.uint32), np.maximum)
    xkey = order_key(x32)
    a.lo = order_value(seg_extreme(flo[a.corner_face], a.cstart, a.clen, xkey, np.minimum)).astype(np.float64)
    a.hi = order_value(seg_extreme(fhi[a.corner_face], a.cstart, a.clen, xkey, np.maximum)).astype(np.float64)
    return a


def apply(a, p):
    """Rule 5."""
    f = a.faces[a.corner_face]
    g = a.gram[a.corner_face].reshape(-1, 3, 3)[np.arange(a.corner.shape[0]), a.corner_i]     # row i of M_f
    term = (g[:, 0:1] * p[f[:, 0]] + g[:, 1:2] * p[f[:, 1]]) + g[:, 2:3] * p[f[:, 2]]
    return seg_sum(term, a.cstart, a.clen) + a.ld[:, None] * p


def dot(x, y):
    """Rule 6: per column."""
    V, C = x.shape
    n_blocks = -(-V // LEAF)
    t = np.zeros((n_blocks * LEAF, C))
    t[:V] = x * y
    t = t.reshape(n_blocks, LEAF, C)
    s = LEAF // 2
    while s >= 1:
        t[:, :s] = t[:, :s] + t[:, s:2 * s]
        s //= 2
    total = np.zeros(C)
    for blk in range(n_blocks):
        total = total + t[blk, 0]
    return total


def _ratio(num, den):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(den > 0.0, num / np.where(den > 0.0, den, 1.0), 0.0)


def iterate(a, iterations):
    """Rule 7: yields Z after 0, 1, ..., K steps, then returns; the last R is left in ``a.R``."""
    Z = np.zeros((a.V, a.C))
    R = a.rhs.copy()
    S = a.inv[:, None] * R
    P = S.copy()
    rho = dot(R, S)
    a.R = R
    yield Z
    for _ in range(int(iterations)):
        q = apply(a, P)
        pi = dot(P, q)
        alpha = _ratio(rho, pi)
        Z = Z + alpha * P
        R = R - alpha * q
        S = a.inv[:, None] * R
        rho_new = dot(R, S)
        beta = _ratio(rho_new, rho)
        P = S + beta * P
        rho = rho_new
        a.R = R
        yield Z


def solve(a, iterations, clamp_mask=0):
    """Rules 7 to 9: (table fp32 [V,C] or None when the input is refused, stats fp64 [C,2], counts int64 [8])."""
    counts = a.counts.copy()
    if a.refused:
        return None, np.zeros((a.C, 2)), counts
    for Z in iterate(a, iterations):
        pass
    stats = np.stack([np.sqrt(dot(a.rhs, a.rhs)), np.sqrt(dot(a.R, a.R))], axis=1)
    X = a.prior.astype(np.float64) + Z
    cols = np.array([(int(clamp_mask) >> c) & 1 for c in range(a.C)], dtype=bool)
    below = (X < a.lo) & cols[None, :] & a.active[:, None]
    above = (X > a.hi) & cols[None, :] & a.active[:, None]
    X = np.where(below, a.lo, np.where(above, a.hi, X))
    counts[6] = below.sum() + above.sum()
    with np.errstate(over="ignore"):
        out = X.astype(np.float32)
    out[~a.active] = a.prior[~a.active]
    return out, stats, counts


def fit(faces, n_vertices, sample_face, sample_bary, targets, prior, prior_weight=1.0 / 64, iterations=32, clamp_mask=0):
    a = assemble(faces, n_vertices, sample_face, sample_bary, targets, prior, prior_weight)
    return solve(a, iterations, clamp_mask) + (a,)


def blend(faces, sample_face, sample_bary, table):
    """What the renderer draws at the samples, fp64."""
    t = np.asarray(table, dtype=np.float64)
    tri = np.asarray(faces)[sample_face]
    b = np.asarray(sample_bary, dtype=np.float64)
    return (b[:, 0:1] * t[tri[:, 0]] + b[:, 1:2] * t[tri[:, 1]]) + b[:, 2:3] * t[tri[:, 2]]


def energy(a, sample_face, sample_bary, targets, X):
    """E(X) of the header, per column (plain numpy sums: a diagnostic, not part of the rule)."""
    r = np.asarray(targets, dtype=np.float64) - blend(a.faces, sample_face, sample_bary, X)
    return (r * r).sum(axis=0) + a.lam * (a.mass[:, None] * (X - a.prior.astype(np.float64)) ** 2).sum(axis=0)


def dense(a, sample_face, sample_bary):
    """G [V,V] and the diagonal d [V] from the samples directly (plain numpy: for the dense checks)."""
    W = np.zeros((a.N, a.V))
    tri = a.faces[sample_face]
    for i in range(3):
        W[np.arange(a.N), tri[:, i]] += np.asarray(sample_bary)[:, i]
    return W.T @ W, W.sum(axis=0)
