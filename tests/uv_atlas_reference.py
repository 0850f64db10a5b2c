"""numpy restatement of the per-triangle UV atlas, the yardstick of ``uv_atlas.per_triangle_atlas``.

Written from the rules, one numpy operation per rounding, fp64 throughout:
  1. measure  u = b - a, w = c - a, n = u x w, len = sqrt((n0 n0 + n1 n1) + n2 n2), l = sqrt(len);
  2. class    q = floor(rho * l); k = N if q >= N, q if q > 0, else 0 (a NaN lands on 0);
  3. order    stable sort by (N - k) << 30 | morton30(quantised centroid);
  4. place    face j of its class run -> block j >> 1, half j & 1, shelves of k + 1 rows, taller classes first;
  5. corners  the staircase's right triangle, shrunk by delta = 1/16, divided by S; the right angle goes to the vertex
              opposite the longest edge;
  6. density  rho given, or searched by doubling and 40 bisection steps.
"""
import numpy as np

DELTA = 1.0 / 16.0
BISECTIONS = 40


def _dot3(x):
    return (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]


def measure(vertices, faces):
    """(l [F] fp64, apex [F] in {0,1,2}, morton [F] uint64) of rules 1, 3 and 5."""
    v = np.asarray(vertices, dtype=np.float64)
    f = np.asarray(faces, dtype=np.int64)
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    with np.errstate(all="ignore"):
        u, w = b - a, c - a
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        ell = np.sqrt(np.sqrt(_dot3(n)))
        # squared edge lengths opposite corners 0, 1, 2; the longest wins, ties (and NaNs) keep the lowest corner
        e = [_dot3(c - b), _dot3(a - c), _dot3(b - a)]
        apex = np.zeros(len(f), dtype=np.int64)
        apex[e[1] > e[0]] = 1
        best = np.where(apex == 1, e[1], e[0])
        apex[e[2] > best] = 2
        lo, hi = v.min(0), v.max(0)
        g = ((a + b) + c) / 3.0
        code = np.zeros(len(f), dtype=np.uint64)
        for axis in range(3):
            if hi[axis] == lo[axis]:
                continue
            t = (g[:, axis] - lo[axis]) / (hi[axis] - lo[axis]) * 1024.0
            q = np.where(t >= 1023.0, 1023.0, np.where(t > 0.0, np.floor(t), 0.0)).astype(np.uint64)
            for bit in range(10):
                code |= ((q >> np.uint64(bit)) & np.uint64(1)) << np.uint64(3 * bit + 2 - axis)
    return ell, apex, code


def classes(rho, ell, N):
    with np.errstate(all="ignore"):
        q = np.floor(np.float64(rho) * ell)
    return np.where(q >= N, float(N), np.where(q > 0, q, 0.0)).astype(np.int64)


def layout(counts, S):
    """(first row Y_k, first sorted position of class k, rows_used, texels_used) for class counts [N+1]."""
    N = len(counts) - 1
    rows = np.zeros(N + 1, dtype=np.int64)
    for k in range(N + 1):
        per_shelf = (S - 1) // (k + 2)
        blocks = (int(counts[k]) + 1) // 2
        rows[k] = -(-blocks // per_shelf) * (k + 1)
    first_row = np.array([rows[k + 1:].sum() for k in range(N + 1)], dtype=np.int64)
    start = np.array([counts[k + 1:].sum() for k in range(N + 1)], dtype=np.int64)
    texels = int(sum(int(counts[k]) * (k + 1) * (k + 2) // 2 for k in range(N + 1)))
    return first_row, start, int(rows.sum()), texels


def probe(rho, ell, S, N):
    """(fits, saturated, class counts): saturated = the faces of class N are at least the faces of positive l, i.e. every
    face that can reach class N is there (with N = 0 that is every face, whatever its area)."""
    counts = np.bincount(classes(rho, ell, N), minlength=N + 1)
    rows_used = layout(counts, S)[2]
    return rows_used <= S - 1, int(counts[N]) >= int((ell > 0).sum()), counts


def capacity(S):
    """Faces an S x S atlas holds when every face is class 0: two per 1 x 2 block."""
    return 2 * ((S - 1) // 2) * (S - 1)


def search(ell, S, N):
    """(rho, hi): the searched density and the bound that ended the search (hi == rho when the histogram saturated)."""
    if not probe(0.0, ell, S, N)[0]:
        raise ValueError(f"{len(ell)} faces do not fit: a {S} x {S} atlas holds at most {capacity(S)} faces")
    lo, hi = 0.0, 1.0
    while True:
        fits, saturated, _ = probe(hi, ell, S, N)
        if not fits:
            break
        if saturated:
            return hi, hi
        lo, hi = hi, hi * 2.0
    for _ in range(BISECTIONS):
        mid = (lo + hi) / 2.0
        if probe(mid, ell, S, N)[0]:
            lo = mid
        else:
            hi = mid
    return lo, hi


def atlas(vertices, faces, S, texels_per_unit=None, N=63):
    """dict(uv [3F,2] fp64, rho, hi, class_counts, face_class, face_origin [F,2], face_half, rows_used, texels_used)."""
    faces = np.asarray(faces, dtype=np.int64)
    F = len(faces)
    ell, apex, code = measure(vertices, faces)
    if texels_per_unit is None:
        rho, hi = search(ell, S, N)
    else:
        rho = hi = float(texels_per_unit)
    k = classes(rho, ell, N)
    counts = np.bincount(k, minlength=N + 1).astype(np.int64)
    first_row, start, rows_used, texels = layout(counts, S)
    if rows_used > S - 1:
        raise ValueError(f"rows_used = {rows_used} exceeds {S - 1}")
    key = ((N - k).astype(np.uint64) << np.uint64(30)) | code
    order = np.argsort(key, kind="stable")
    rank = np.empty(F, dtype=np.int64)
    rank[order] = np.arange(F)
    j = rank - start[k]
    block, half = j >> 1, j & 1
    per_shelf = (S - 1) // (k + 2)
    r0 = (first_row[k] + (block // per_shelf) * (k + 1)).astype(np.float64)
    c0 = ((block % per_shelf) * (k + 2)).astype(np.float64)
    kf = k.astype(np.float64)
    low = half == 0
    # p0, p1, p2 in texels, [F, 3, 2] (row, column)
    p = np.empty((F, 3, 2), dtype=np.float64)
    p[:, 0, 0] = np.where(low, r0 + DELTA, (r0 + (kf + 1)) - DELTA)
    p[:, 0, 1] = np.where(low, c0 + DELTA, (c0 + (kf + 2)) - DELTA)
    p[:, 1, 0] = np.where(low, (r0 + (kf + 1)) - 2 * DELTA, r0 + 2 * DELTA)
    p[:, 1, 1] = p[:, 0, 1]
    p[:, 2, 0] = p[:, 0, 0]
    p[:, 2, 1] = np.where(low, (c0 + (kf + 1)) - 2 * DELTA, (c0 + 1) + 2 * DELTA)
    uv = np.empty((F, 3, 2), dtype=np.float64)
    for corner in range(3):
        which = (corner - apex) % 3                                    # the apex gets p0, the next corner p1
        uv[:, corner] = p[np.arange(F), which] / np.float64(S)
    return dict(uv=uv.reshape(-1, 2), rho=float(rho), hi=float(hi), class_counts=counts, face_class=k.astype(np.int32),
                face_origin=np.stack([r0, c0], 1).astype(np.int32), face_half=half.astype(np.uint8),
                rows_used=rows_used, texels_used=texels)


def staircase(k, origin, half):
    """Texels (r, c) of one face's chart, [n, 2]."""
    dr, dc = np.meshgrid(np.arange(k + 1), np.arange(k + 2), indexing="ij")
    m = (dr + dc <= k) if half == 0 else (dr + dc >= k + 1)
    return np.stack([dr[m] + origin[0], dc[m] + origin[1]], axis=1)


def in_staircase(texel, k, origin, half):
    """Vectorised: is texel[i] inside the chart of (k[i], origin[i], half[i])?"""
    dr, dc = texel[..., 0] - origin[..., 0], texel[..., 1] - origin[..., 1]
    box = (dr >= 0) & (dr <= k) & (dc >= 0) & (dc <= k + 1)
    return box & np.where(half == 0, dr + dc <= k, dr + dc >= k + 1)


def lookup_points(n_faces, n_random=200, seed=0):
    """Barycentric weights [F, 6 + n_random, 3]: the corners, the edge midpoints and Dirichlet(0.3) points."""
    rng = np.random.default_rng(seed)
    fixed = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [.5, .5, 0], [0, .5, .5], [.5, 0, .5]])
    w = rng.dirichlet([0.3] * 3, size=(n_faces, n_random))
    return np.concatenate([np.broadcast_to(fixed, (n_faces, 6, 3)), w], axis=1)


def lookup(uv, S, weights):
    """The baked path's nearest-texel lookup: clip(fp32(uv - 1e-7) * S, 0, S - 1), an fp32 blend, floor."""
    s = np.clip((uv - 1e-7).astype(np.float32) * np.float32(S), 0, S - 1).reshape(-1, 3, 2)
    w = weights.astype(np.float32)
    p = (w[..., 0:1] * s[:, None, 0] + w[..., 1:2] * s[:, None, 1]) + w[..., 2:3] * s[:, None, 2]
    assert p.dtype == np.float32
    return np.floor(p).astype(np.int64)
