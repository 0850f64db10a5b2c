/* qf_closest_point.h -- the closest point on a triangle mesh, in libqf_hip.so: for every query
 * point the nearest triangle of a qf_bvh handle, its barycentric coordinates there and the squared distance.  The rule
 * is this project's own (the reference has no such query); it is restated in numpy, operation for operation, in
 * tests/closest_point_reference.py, and the device returns those bits whatever the tree, the build or the launch shape.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`, nothing
 * waits on the host; every refusal comes before the first launch); QF_ABI_VERSION is unchanged.
 *
 * INPUT  the triangles of the handle, fp32, as the last build or refit left them; points fp64 [N,3]; max_distance >= 0,
 * +inf for no limit.  All arithmetic is fp64 on the fp32 vertices widened exactly, no operation is fused, and
 * dot(u, v) = (u.x v.x + u.y v.y) + u.z v.z.
 *   1. per triangle (a, b, c), query q: ab = b - a, ac = c - a; d1 = dot(ab, q - a), d2 = dot(ac, q - a), d3 = dot(ab, q - b),
 *      d4 = dot(ac, q - b), d5 = dot(ab, q - c), d6 = dot(ac, q - c); vc = d1 d4 - d3 d2, vb = d5 d2 - d1 d6,
 *      va = d3 d6 - d5 d4.  The regions of Ericson, Real-Time Collision Detection 5.1.5, tested in this order, the first
 *      that holds gives (v, w):
 *        A   d1 <= 0 and d2 <= 0                                              (0, 0)
 *        B   d3 >= 0 and d4 <= d3                                             (1, 0)
 *        AB  vc <= 0, d1 >= 0, d3 <= 0 and d1 - d3 > 0                        (d1 / (d1 - d3), 0)
 *        C   d6 >= 0 and d5 <= d6                                             (0, 1)
 *        AC  vb <= 0, d2 >= 0, d6 <= 0 and d2 - d6 > 0                        (0, d2 / (d2 - d6))
 *        BC  va <= 0, n = d4 - d3 >= 0, m = d5 - d6 >= 0 and n + m > 0        (1 - t, t), t = n / (n + m)
 *      An edge of length zero has a denominator that is not > 0 and claims nothing.
 *   2. the end of the walk: up to four candidates, the smallest dist2 (rule 3) wins, the earlier one on a tie:
 *        interior, only when va > 0, vb > 0 and vc > 0: r = 1 / ((va + vb) + vc), (vb r, vc r);
 *        AB clamped: s = 0 if d1 <= 0, 1 if d3 >= 0, else d1 / (d1 - d3) (0 when the denominator is not > 0): (s, 0);
 *        AC clamped: s = 0 if d2 <= 0, 1 if d6 >= 0, else d2 / (d2 - d6), likewise: (0, s);
 *        BC clamped: s = 0 if n <= 0, 1 if m <= 0, else n / (n + m), likewise: (1 - s, s).
 *      On a triangle with area the interior point wins.  On a sliver whose area is lost to rounding, and on a zero-area
 *      triangle, va, vb and vc are noise: there the edges answer.  Every candidate is a point of the triangle.
 *   3. the point p is b if v == 1, else c if w == 1, else (a + v ab) + w ac with every coordinate moved into
 *      [min(a, b, c), max(a, b, c)]; dist2 = (ex ex + ey ey) + ez ez, e = q - p.  For finite input v, w and dist2 are
 *      finite (products of coordinates must not overflow fp64: magnitudes below 1e75 are safe) and p lies in the
 *      triangle's bounding box, so dist2 is never below the squared distance from q to any box that holds the triangle;
 *   4. the answer for q minimises (dist2, original triangle id) among the triangles with dist2 <= max_distance
 *      max_distance: ties go to the lower id, and the answer does not depend on the tree;
 *   5. output  tri int32 [N] the original id or -1; bary fp64 [N,3] = ((1 - v) - w, v, w), zeros when tri is -1; dist2
 *      fp64 [N], +inf when tri is -1; counts int64 [2]: queries with a NaN or infinite coordinate (they get -1 and are
 *      never traversed), and the other queries with no triangle within max_distance.
 * The traversal is best-first over the 8-wide tree: a subtree is skipped only when the squared distance from q to its
 * box is strictly greater than the best dist2 so far (or than max_distance squared), so the minimiser of rule 4 is
 * never lost.  A triangle with a NaN vertex is never the answer.                                                       */
#ifndef QF_CLOSEST_POINT_H
#define QF_CLOSEST_POINT_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_CLOSEST_POINT_COUNTS 2

/* Rules 1 to 5 for n_points queries.  n_points == 0 and a handle without triangles are valid (counts is still written).
 * QF_ERR_INVALID_ARGUMENT before any launch for a NULL bvh or counts, n_points < 0, a max_distance that is negative or
 * NaN, or a NULL points / tri / bary / dist2 with n_points > 0; QF_ERR_UNSUPPORTED for a tree whose traversal stack
 * does not fit the LDS or n_points above 2^36.                                                                         */
int qf_bvh_closest_points(const qf_bvh *bvh, const double *points, int64_t n_points, double max_distance,
                          int32_t *tri, double *bary, double *dist2, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_CLOSEST_POINT_H */
