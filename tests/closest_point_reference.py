"""The closest-point rule of DESIGN.md section 3.9f (include/qf_closest_point.h) restated in numpy, operation for operation:
every product, sum and comparison below stands in the same place in closest_point.hip (compiled with -ffp-contract=off),
so the device's tri, bary, dist2 and counts are these bit for bit.  All arithmetic is fp64 on the fp32 triangle
vertices widened exactly.

Per triangle: the region walk of Ericson, Real-Time Collision Detection 5.1.5, regions in the order A, B, AB, C, AC,
BC, with two additions that keep zero-length edges and zero-area triangles finite and right:
  * an edge region also needs its denominator > 0 (a zero-length edge claims nothing; the walk goes on);
  * what reaches the end of the walk takes the best of up to four candidates, the earlier one on a tie: the interior
    point when va, vb and vc are all > 0, then the clamped projections onto AB, AC and BC.  On a triangle with area the
    interior point wins; where rounding has eaten the area the edges answer, and every candidate is a point of the
    triangle, so the result is never below the true distance by more than rounding.
The point is b when v == 1, c when w == 1, else (a + v ab) + w ac moved into the triangle's bounding box axis by axis
(which is what makes pruning by box distance exact); dist2 sums the squared differences x, y, z in that order.
Across triangles the answer minimises (dist2, id) among dist2 <= max_distance^2."""
import numpy as np

REGIONS = ("A", "B", "AB", "C", "AC", "BC", "interior", "end:AB", "end:AC", "end:BC")
COUNT_NAMES = ("nonfinite_queries", "no_triangle")
F64 = np.float64


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def _ratio(num, den):
    """num / den where den > 0, else 0."""
    ok = den > 0
    return np.where(ok, num / np.where(ok, den, 1.0), 0.0)


def _bounds(a, b, c):
    lo = np.where(b < a, b, a)
    lo = np.where(c < lo, c, lo)
    hi = np.where(b > a, b, a)
    hi = np.where(c > hi, c, hi)
    return lo, hi


def _point(a, b, c, ab, ac, lo, hi, v, w):
    p = (a + v[..., None] * ab) + w[..., None] * ac
    p = np.where(p < lo, lo, p)
    p = np.where(p > hi, hi, p)
    return np.where((v == 1.0)[..., None], b, np.where((w == 1.0)[..., None], c, p))


def _dist2(q, p):
    e = q - p
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]


def _end_of_walk(q, a, b, c, ab, ac, lo, hi, d1, d2, d3, d6, n_bc, m_bc, t_ab, t_ac, t_bc, va, vb, vc):
    """Flat arrays of the pairs no region claimed -> (v, w, region): the interior point (va, vb, vc all > 0), then the
    clamped projections onto AB, AC, BC; the smallest dist2, the earlier candidate on a tie."""
    zero, one = np.zeros_like(d1), np.ones_like(d1)
    s_ab = np.where(d1 <= 0, zero, np.where(d3 >= 0, one, t_ab))
    s_ac = np.where(d2 <= 0, zero, np.where(d6 >= 0, one, t_ac))
    s_bc = np.where(n_bc <= 0, zero, np.where(m_bc <= 0, one, t_bc))
    cand = [(s_ab, zero, 7), (zero, s_ac, 8), (1.0 - s_bc, s_bc, 9)]
    ev, ew, er = s_ab, zero, np.full(d1.shape, 7, np.int8)
    ed = _dist2(q, _point(a, b, c, ab, ac, lo, hi, ev, ew))
    for kv, kw, code in cand[1:]:
        kd = _dist2(q, _point(a, b, c, ab, ac, lo, hi, kv, kw))
        better = kd < ed
        ev, ew, ed, er = np.where(better, kv, ev), np.where(better, kw, ew), np.where(better, kd, ed), np.where(better, np.int8(code), er)
    inside = (va > 0) & (vb > 0) & (vc > 0)
    denom = 1.0 / np.where(inside, (va + vb) + vc, 1.0)
    iv, iw = np.where(inside, vb * denom, zero), np.where(inside, vc * denom, zero)
    idist = _dist2(q, _point(a, b, c, ab, ac, lo, hi, iv, iw))
    keep = inside & ~(ed < idist)
    return np.where(keep, iv, ev), np.where(keep, iw, ew), np.where(keep, np.int8(6), er)


def closest_on_triangles(q, a, b, c):
    """q, a, b, c: fp64 arrays [..., 3] that broadcast against each other -> (v, w, dist2, region, point)."""
    q, a, b, c = (np.asarray(x, F64) for x in (q, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac = b - a, c - a
        ap = q - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = q - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        cp = q - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vc = d1 * d4 - d3 * d2
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        den_ab, den_ac = d1 - d3, d2 - d6
        n_bc, m_bc = d4 - d3, d5 - d6
        den_bc = n_bc + m_bc
        t_ab, t_ac, t_bc = _ratio(d1, den_ab), _ratio(d2, den_ac), _ratio(n_bc, den_bc)
        zero, one = np.zeros_like(d1), np.ones_like(d1)

        in_a = (d1 <= 0) & (d2 <= 0)
        in_b = (d3 >= 0) & (d4 <= d3)
        in_ab = (vc <= 0) & (d1 >= 0) & (d3 <= 0) & (den_ab > 0)
        in_c = (d6 >= 0) & (d5 <= d6)
        in_ac = (vb <= 0) & (d2 >= 0) & (d6 <= 0) & (den_ac > 0)
        in_bc = (va <= 0) & (n_bc >= 0) & (m_bc >= 0) & (den_bc > 0)

        lo, hi = _bounds(a, b, c)
        claimed = in_a | in_b | in_ab | in_c | in_ac | in_bc
        v, w, region = np.zeros(claimed.shape), np.zeros(claimed.shape), np.zeros(claimed.shape, np.int8)
        for mask, rv, rw, code in ((in_bc, 1.0 - t_bc, t_bc, 5), (in_ac, zero, t_ac, 4), (in_c, zero, one, 3),
                                   (in_ab, t_ab, zero, 2), (in_b, one, zero, 1), (in_a, zero, zero, 0)):
            v, w, region = np.where(mask, rv, v), np.where(mask, rw, w), np.where(mask, np.int8(code), region)
        rest = ~claimed
        if rest.any():                  # the end of the walk, on the pairs that reach it (elementwise: the same bits)
            shape = claimed.shape + (3,)
            sq, sa, sb, sc, sab, sac, slo, shi = (np.broadcast_to(x, shape)[rest] for x in (q, a, b, c, ab, ac, lo, hi))
            ev, ew, er = _end_of_walk(sq, sa, sb, sc, sab, sac, slo, shi, *(x[rest] for x in (d1, d2, d3, d6, n_bc, m_bc, t_ab, t_ac, t_bc, va, vb, vc)))
            v[rest], w[rest], region[rest] = ev, ew, er
        v, w = np.broadcast_arrays(v, w)
        p = _point(a, b, c, ab, ac, lo, hi, v, w)
        return v, w, _dist2(q, p), region, p


def _closest_prefiltered(t, pts, max2):
    """The answer of the plain loop for these queries from the pairs that can matter: dist2 is never below the distance
    from the query to the triangle's bounding box (rule 3 keeps the point inside it; the host tests check it), so with u
    = dist2 of the triangle whose box is nearest, only triangles whose box distance is <= u can hold the minimiser of
    (dist2, id).  Those pairs go through the same elementwise rule, so every bit is the plain loop's."""
    n = pts.shape[0]
    lo, hi = t.min(axis=1), t.max(axis=1)
    bd = box_dist2(pts[:, None, :], lo[None], hi[None])
    first = np.argmin(bd, axis=1)
    upper = closest_on_triangles(pts, t[first, 0], t[first, 1], t[first, 2])[2]
    qi, ti = np.nonzero(bd <= np.where(np.isnan(upper), np.inf, upper)[:, None])          # row-major: ids ascend per query
    v, w, d2, _, _ = closest_on_triangles(pts[qi], t[ti, 0], t[ti, 1], t[ti, 2])
    with np.errstate(all="ignore"):
        ok = d2 <= max2
    key = np.where(ok, d2, np.inf)
    order = np.lexsort((ti, key, qi))                       # per query: the smallest (key, id) first
    head = order[np.r_[True, qi[order][1:] != qi[order][:-1]]]
    tri, bary, dist2 = np.full(n, -1, np.int32), np.zeros((n, 3), F64), np.full(n, np.inf, F64)
    head = head[ok[head]]
    rows = qi[head]
    tri[rows], dist2[rows] = ti[head], d2[head]
    bary[rows] = np.stack([(1.0 - v[head]) - w[head], v[head], w[head]], axis=1)
    return tri, bary, dist2


def closest_points(triangles, points, max_distance=np.inf, chunk_pairs=1 << 17, prefilter=False):
    """triangles fp32 [T,3,3] (id = row), points fp64 [N,3] -> tri int32 [N], bary fp64 [N,3], dist2 fp64 [N],
    counts int64 [2].  ``prefilter``: the same answer, bit for bit, from far fewer pairs (see ``_closest_prefiltered``)."""
    tri32 = np.asarray(triangles)
    assert tri32.dtype == np.float32 and tri32.shape[1:] == (3, 3)
    t = tri32.astype(F64)
    pts = np.ascontiguousarray(points, F64).reshape(-1, 3)
    n, n_tri = pts.shape[0], t.shape[0]
    max2 = F64(max_distance) * F64(max_distance)
    out_tri = np.full(n, -1, np.int32)
    out_bary = np.zeros((n, 3), F64)
    out_d2 = np.full(n, np.inf, F64)
    finite = np.isfinite(pts).all(axis=1)
    if n_tri:
        idx = np.nonzero(finite)[0]
        step = max(1, chunk_pairs // n_tri)
        for s in range(0, idx.size, step):
            sel = idx[s:s + step]
            if prefilter:
                out_tri[sel], out_bary[sel], out_d2[sel] = _closest_prefiltered(t, pts[sel], max2)
                continue
            v, w, d2, _, _ = closest_on_triangles(pts[sel, None, :], t[None, :, 0], t[None, :, 1], t[None, :, 2])
            with np.errstate(all="ignore"):
                ok = d2 <= max2
            key = np.where(ok, d2, np.inf)
            best = np.argmin(key, axis=1)                      # the first minimum: the lowest id on a tie
            rows = np.arange(sel.size)
            found = ok[rows, best]
            bv, bw = v[rows, best], w[rows, best]
            out_tri[sel] = np.where(found, best, -1)
            out_bary[sel] = np.where(found[:, None], np.stack([(1.0 - bv) - bw, bv, bw], axis=1), 0.0)
            out_d2[sel] = np.where(found, d2[rows, best], np.inf)
    counts = np.array([(~finite).sum(), (finite & (out_tri < 0)).sum()], np.int64)
    return out_tri, out_bary, out_d2, counts


def triangles_of(vertices, faces):
    """The fp32 triangle soup [F,3,3] an intersector holds for this mesh."""
    return np.ascontiguousarray(np.asarray(vertices).astype(np.float32)[np.asarray(faces, np.int64)])


def transfer(triangles, faces, table, points, max_distance=np.inf):
    """Rows of an fp32 vertex table blended at the closest point, in fp32, left to right, from the barycentrics rounded
    once to fp32."""
    tri, bary, _, counts = closest_points(triangles, points, max_distance)
    assert counts[0] == 0 and counts[1] == 0
    f = np.asarray(faces, np.int64)[tri]
    b = bary.astype(np.float32)
    tab = np.asarray(table, np.float32)
    return (b[:, 0:1] * tab[f[:, 0]] + b[:, 1:2] * tab[f[:, 1]]) + b[:, 2:3] * tab[f[:, 2]]


# ---- an independent formulation, for the host tests ---------------------------------------------------------------------

def segment_dist2(q, a, b):
    d = b - a
    l2 = (d * d).sum(-1)
    t = np.clip(((q - a) * d).sum(-1) / np.where(l2 > 0, l2, 1.0), 0.0, 1.0)
    t = np.where(l2 > 0, t, 0.0)
    e = q - (a + t[..., None] * d)
    return (e * e).sum(-1)


def segments_dist2(q, a, b, c):
    return np.minimum(np.minimum(segment_dist2(q, a, b), segment_dist2(q, a, c)), segment_dist2(q, b, c))


def plane_or_segments_dist2(q, a, b, c):
    """The plane projection where it falls inside the triangle, else the three segments."""
    n = np.cross(b - a, c - a)
    n2 = (n * n).sum(-1)
    safe = np.where(n2 > 0, n2, 1.0)
    h = ((q - a) * n).sum(-1)
    foot = q - (h / safe)[..., None] * n
    inside = n2 > 0
    for u, v in ((a, b), (b, c), (c, a)):
        inside = inside & ((np.cross(v - u, foot - u) * n).sum(-1) >= 0)
    return np.where(inside, h * h / safe, segments_dist2(q, a, b, c))


def box_dist2(q, lo, hi):
    e = np.maximum(np.maximum(lo - q, q - hi), 0.0)
    return (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
