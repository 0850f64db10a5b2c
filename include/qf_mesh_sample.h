/* qf_mesh_sample.h -- points drawn by area from the surface of a triangle mesh, in libqf_hip.so (DESIGN.md section
 * 3.9h): N points, stratified along the mesh's cumulative measure, each with its face and its barycentric coordinates.
 * The measure of a face is its area (twice the area, to be exact: the scale cancels), optionally times a per-face
 * weight, so that per-triangle importances can steer where the samples go.  The rule is this project's own and is
 * restated in numpy in tests/mesh_sample_reference.py.  Every result is the same bit for bit from run to run and from
 * launch shape to launch shape: the only sums are integer sums, the only maximum is exact, and no floating-point atomic
 * is used.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`, nothing
 * waits on the host; every refusal comes before the first launch); QF_ABI_VERSION is unchanged.
 *
 * INPUT  vertices fp64 [V,3]; faces int64 [F,3]; face_weight fp64 [F] or NULL (every weight 1); the number of samples N;
 * a seed, uint64.  V in [1, 2^31), F in [1, 2^31 / 3), N in [0, 2^31).  Every floating-point operation is fp64, rounded
 * on its own, never fused.
 *   1. validity    counted: vertices with a coordinate that is not finite; faces with an index outside [0, V); weights
 *                  that are negative or not finite (a NaN weight is one); faces, among those with every index in range,
 *                  whose measure (rule 2) is not finite.  If any of the four is non-zero nothing is sampled: counts[4]
 *                  and counts[5] are zero and emit writes nothing;
 *   2. measure     for the corners a, b, c of face f: u = b - a, w = c - a, n = (u1 w2 - u2 w1, u2 w0 - u0 w2,
 *                  u0 w1 - u1 w0) (section 3.9's expression), len = sqrt((n0 n0 + n1 n1) + n2 n2), m_f = len * w_f, and
 *                  m_f = len itself with NULL weights.  A face with two equal indices has m_f = 0 by decree, and so has
 *                  a face with an index out of range;
 *   3. quantise    M = max_f m_f (exact, order-free).  If M == 0 nothing can be sampled: counts[5] = 1 and emit writes
 *                  nothing.  Otherwise q_f = floor(m_f / M * 4294967296.0) as uint64: one division, one multiplication
 *                  by 2^32 (exact) and one floor, so q_f in [0, 2^32] and the largest face has exactly 2^32.  A face
 *                  with q_f == 0 (its measure is below 2^-32 of the largest) is never sampled; counts[4] is their number;
 *   4. scan        S_f = sum over g <= f of q_g in uint64, an integer sum, hence exact whatever the scan's shape;
 *                  S = S_{F-1} < 2^63;
 *   5. position    for sample i: h_k = fin(seed + (3 i + k + 1) * 0x9E3779B97F4A7C15 mod 2^64), k = 0, 1, 2, with fin
 *                  splitmix64's finaliser (x ^= x >> 30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB;
 *                  x ^= x >> 31);  xi = (h_0 >> 11) * 2^-53;  u = (double(i) + xi) / double(N);
 *                  t = min(uint64(floor(u * double(S))), S - 1) with double(S) the round-to-nearest-even conversion.
 *                  One sample per stratum [i / N, (i + 1) / N) of the cumulative measure; t is non-decreasing in i;
 *   6. face        f_i = the smallest f with S_f > t: never a face with q_f == 0, and non-decreasing in i;
 *   7. barycentric r1 = (h_1 >> 11) * 2^-53, r2 = (h_2 >> 11) * 2^-53; if r1 + r2 > 1.0 then r1 = 1 - r1 and
 *                  r2 = 1 - r2;  bary = (max((1 - r1) - r2, 0), r1, r2);
 *   8. point       p = (a * bary0 + b * bary1) + c * bary2 per coordinate.
 * OUTPUT points fp64 [N,3], face int64 [N], bary fp64 [N,3]; counts int64 [6]: non-finite vertices, invalid faces, bad
 * weights, faces with a non-finite measure, faces with q == 0, and 1 iff the mesh is valid and has no measure (M == 0).
 * The count of face f is within 2 of N q_f / S (in exact arithmetic the stratification makes it so).
 * Multiplying every weight by a power of two changes no output bit.                                                    */
#ifndef QF_MESH_SAMPLE_H
#define QF_MESH_SAMPLE_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_SAMPLE_COUNTS 6

/* Bytes of workspace the two calls below need for a mesh of this size (host computation); -1 for sizes out of range.   */
int64_t qf_mesh_sample_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Rules 1 to 4, kept in `workspace`; counts[6] is written on the device.  face_weight may be NULL.
 * QF_ERR_INVALID_ARGUMENT before any launch for sizes out of range, a NULL vertices / faces / workspace / counts or a
 * short workspace.                                                                                                     */
int qf_mesh_sample_prepare(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                           const double *face_weight, void *workspace, int64_t workspace_bytes, int64_t *counts,
                           void *stream);

/* Rules 5 to 8 from the workspace qf_mesh_sample_prepare left for the same mesh (workspace_bytes is what it was there);
 * it may be called any number of times after one prepare, with any N and seed.  points [N,3], face [N] and bary [N,3]
 * get every row, unless prepare found the mesh invalid or without measure: then nothing is written (the kernel reads
 * that flag on the device; the caller learns it from counts).  Refusals as above, plus N outside [0, 2^31) and, with
 * N > 0, a NULL points / face / bary.  N == 0 is valid and launches nothing.                                           */
int qf_mesh_sample_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces, void *workspace,
                        int64_t workspace_bytes, int64_t n_samples, uint64_t seed, double *points, int64_t *face,
                        double *bary, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_SAMPLE_H */
