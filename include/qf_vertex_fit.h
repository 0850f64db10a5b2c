/* qf_vertex_fit.h -- the vertex table fitted to a field over the surface, in libqf_hip.so: the
 * least-squares fit of the function the vertex-baked renderer draws (the barycentric blend of three table rows) to target
 * rows given at surface samples, regularised towards a prior table and solved by a fixed number of Jacobi-preconditioned
 * conjugate-gradient steps.  The rule is this project's own and is restated in numpy, operation for operation, in
 * tests/vertex_fit_reference.py.  Every result is the same bit for bit from run to run: every sum has a stated order, no
 * floating-point atomic is used, and the only atomics are integer tallies.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`, nothing
 * waits on the host; every refusal comes before the first launch); QF_ABI_VERSION is unchanged.
 *
 * INPUT  faces int64 [F,3] over V vertices; N samples as face int64 [N], non-decreasing, and bary fp64 [N,3] (what
 * qf_mesh_sample_emit writes); targets y fp32 [N,C], rows y_stride floats apart; the prior table x0 fp32 [V,C], rows
 * x0_stride floats apart (a padded vertex table is read in place); prior_weight lambda >= 0; K >= 0 steps; a 64-bit
 * clamp_mask over the columns (bit c: column c is clamped).  1 <= C <= 64, V in [1, 2^31), F in [0, 2^31 / 3),
 * N in [0, 2^31).  With f0, f1, f2 the indices of a sample's face and b_s0, b_s1, b_s2 its barycentrics, the fit minimises
 *     E(X) = sum_s sum_c (y_s[c] - (b_s0 X[f0][c] + b_s1 X[f1][c] + b_s2 X[f2][c]))^2
 *            + lambda sum_v d_v sum_c (X[v][c] - x0[v][c])^2
 * over X.  Every floating-point operation is fp64 on exactly widened inputs, rounded on its own and never fused; every
 * sum runs left to right from +0.0 in the order written.
 *   1. validity   counted: samples whose face id is outside [0, F); positions s >= 1 with face[s] < face[s-1]; entries of
 *                 bary, y (the C columns of its N rows) or x0 (the C columns of its V rows) that are not finite.  If any
 *                 of the three counts is non-zero the input is refused: face_gram, vertex_mass and rhs are all +0.0,
 *                 counts[3..6] are zero, counts[7] is 1, and solve writes no row of the output table and zero stats.
 *                 A face with an index outside [0, V) or with two equal indices is skipped: it takes no part, and neither
 *                 do its samples; both are counted;
 *   2. per face   over the run of its samples in sample order, for corners i, j in 0..2:
 *                 M_f[i][j] = sum_s b_si * b_sj (face_gram[9 f + 3 i + j]; six distinct numbers) and m_f[i] = sum_s b_si.
 *                 A skipped face and a face without samples have zeros;
 *   3. per vertex over its corners (f, i) of faces that are not skipped, in ascending (f, i):
 *                 d_v = sum m_f[i] (vertex_mass[v]);  a_v = (sum M_f[i][i]) + lambda * d_v;  inv_v = 1 / a_v if a_v > 0,
 *                 else 0.  A vertex with d_v == 0 is inactive: it keeps its prior row bit for bit and is counted;
 *   4. rhs        e_s[c] = y_s[c] - ((b_s0 * x0[f0][c] + b_s1 * x0[f1][c]) + b_s2 * x0[f2][c]);
 *                 g_(f,i)[c] = sum_s b_si * e_s[c] over the run;  B[v][c] = sum of g_(f,i)[c] over the corners of v in the
 *                 order of rule 3 (rhs[v C + c]);
 *   5. operator   (A p)[v][c] = (sum over the corners (f, i) of v: ((M_f[i][0] * p[f0][c] + M_f[i][1] * p[f1][c])
 *                 + M_f[i][2] * p[f2][c])) + (lambda * d_v) * p[v][c];
 *   6. dot        dot(x, y)[c], per column over the vertices: the products x[v][c] * y[v][c] of each block of 256
 *                 consecutive vertices are summed by the stride-halving tree t[i] += t[i + s], s = 128, 64, ..., 1, over
 *                 256 entries (missing entries are +0.0), and the block sums t[0] are then added one by one, from +0.0, in
 *                 ascending block order;
 *   7. solve      for the correction Z (X = x0 + Z), every column on its own:  Z = 0, R = B, S = inv * R, P = S,
 *                 rho = dot(R, S);  then exactly K times:  q = A P;  pi = dot(P, q);  alpha = pi > 0 ? rho / pi : 0;
 *                 Z = Z + alpha * P;  R = R - alpha * q;  S = inv * R;  rho' = dot(R, S);  beta = rho > 0 ? rho' / rho : 0;
 *                 P = S + beta * P;  rho = rho'.  stats[2 c] = sqrt(dot(B, B)[c]), stats[2 c + 1] = sqrt(dot(R, R)[c]) with
 *                 the last R;
 *   8. clamp      for the columns of clamp_mask only: lo_v[c] / hi_v[c] are the least / greatest of x0[v][c] and y_s[c]
 *                 over the samples of the faces at v's corners, in the order in which -0.0 is below +0.0 (exact, hence
 *                 free of the order of evaluation);  X = x0 + Z;  X = lo if X < lo;  X = hi if X > hi;  the entries moved
 *                 are counted;
 *   9. output     X rounded once to fp32 into the first C columns of the output rows (out_stride floats apart; padding
 *                 columns are not touched); an inactive vertex gets the C words of its prior row instead.
 * OUTPUT counts int64 [8]: sample faces out of range, unsorted positions, non-finite entries, skipped faces, samples of
 * skipped faces, inactive vertices, clamped entries (zero until solve writes it), and 1 iff the input is refused.
 *
 * The barycentrics of a sample are convex weights, so z' G z <= z' D z for the Gram matrix G of the blend and the
 * diagonal D of d_v (Jensen's inequality): the eigenvalues of D^-1 (G + lambda D) lie in [lambda, 1 + lambda] whatever the
 * mesh, and the step count needed does not grow with it.  A vertex with hundreds of corners and a face with thousands of
 * samples are walked by one lane per column and stay correct, but slow.                                                  */
#ifndef QF_VERTEX_FIT_H
#define QF_VERTEX_FIT_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_VERTEX_FIT_COUNTS 8
#define QF_VERTEX_FIT_MAX_COLUMNS 64

/* Bytes of workspace the two calls below need (host computation); -1 for sizes out of range.                            */
int64_t qf_vertex_fit_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_samples, int64_t n_columns);

/* Rules 1 to 4, and the bounds of rule 8, kept in `workspace`; face_gram fp64 [F,9], vertex_mass fp64 [V] and rhs fp64
 * [V,C] get every entry; counts[8] is written on the device.  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of
 * range, a stride below C, a prior_weight that is negative or not finite, a NULL faces (with F > 0), sample_face,
 * sample_bary or targets (with N > 0), prior, face_gram (with F > 0), vertex_mass, rhs, workspace or counts, or a short
 * workspace.                                                                                                            */
int qf_vertex_fit_assemble(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *sample_face,
                           const double *sample_bary, int64_t n_samples, const float *targets, int64_t y_stride,
                           const float *prior, int64_t x0_stride, int64_t n_columns, double prior_weight, double *face_gram,
                           double *vertex_mass, double *rhs, void *workspace, int64_t workspace_bytes, int64_t *counts,
                           void *stream);

/* Rules 5 to 9 from what qf_vertex_fit_assemble left for the same input in face_gram, vertex_mass, rhs and `workspace`
 * (every size and workspace_bytes as there).  out fp32 [V, out_stride] gets the first C columns of every row, unless the
 * input was refused; stats fp64 [C,2] and counts[8] get every entry.  It may be called again after one assemble, with any
 * K and clamp_mask.  Refusals as above, plus K outside [0, 2^31) and a NULL out or stats.                               */
int qf_vertex_fit_solve(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const float *prior, int64_t x0_stride,
                        int64_t n_columns, const double *face_gram, const double *vertex_mass, const double *rhs,
                        int64_t iterations, uint64_t clamp_mask, void *workspace, int64_t workspace_bytes, float *out,
                        int64_t out_stride, double *stats, int64_t *counts, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_VERTEX_FIT_H */
