/* qf_mesh_decimate.h -- mesh decimation of libqf_hip.so: rounds of independent quadric edge
 * collapses that bring a triangle mesh down to a face count.  The rules are this project's own (parity with
 * fast_simplification, which the reference calls, is UNPINNED); they are restated in numpy in
 * tests/mesh_decimate_reference.py and every result is the same bit for bit from run to run.  All deciding arithmetic is
 * fp64, every product and sum rounded on its own in the order written below (-ffp-contract=off); the only atomics are
 * integer ones.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer; work is enqueued on `stream`, nothing waits on the host; every refusal comes before the first launch),
 * QF_ABI_VERSION is unchanged.  A round is: qf_mesh_edges_count / _emit (qf_mesh_subdivide.h), qf_mesh_collapse_select,
 * qf_mesh_collapse_apply, qf_mesh_compact_count / _emit (qf_mesh_compact.h) with QF_MESH_REMOVE_DEGENERATE |
 * QF_MESH_REMOVE_UNREFERENCED, qf_mesh_collapse_gather.  Round 0 starts with qf_mesh_vertex_quadrics.
 *
 * QUADRICS (round 0; section 3.9's rule).  The plane of face (i0, i1, i2): u = p1 - p0, w = p2 - p0, n = (u1 w2 - u2 w1,
 * u2 w0 - u0 w2, u0 w1 - u1 w0), len = sqrt((n0 n0 + n1 n1) + n2 n2); if len == 0 the plane is zero, else n = n / len per
 * component and d = -((n0 p0x + n1 p0y) + n2 p0z).  Q[v] is the upper triangle q00 q01 q02 q03 q11 q12 q13 q22 q23 q33 of
 * the sum of (n, d)(n, d)^T over the faces that use v, in ascending face index, starting from +0.0.  A face with two
 * equal indices has the zero plane, which changes no bit of a sum, and is left out.
 *
 * EACH ROUND r = 0, 1, ... on the current mesh (V vertices p, F faces, E edges e = (a, b), a < b, face_edges):
 *   1. uses       uses[e] is the number of half-edges on e (entries of face_edges equal to e);
 *   2. locks      a vertex is locked iff its vertex_lock byte is not zero or it is an end of an edge with uses != 2
 *                 (boundary or non-manifold);
 *   3. candidate  an edge with both ends unlocked.  Qe = Q[a] + Q[b] per component; m = (p[a] + p[b]) * 0.5; with
 *                 a_ij / b = -(q03, q13, q23) of Qe, r_i = b_i - ((a_i0 m0 + a_i1 m1) + a_i2 m2), the cofactors
 *                 c00 = a11 a22 - a12 a12, c01 = a12 a02 - a01 a22, c02 = a01 a12 - a11 a02, c11 = a00 a22 - a02 a02,
 *                 c12 = a01 a02 - a00 a12, c22 = a00 a11 - a01 a01, det = (a00 c00 + a01 c01) + a02 c02,
 *                 t = ((a00 + a11) + a22) / 3: if det > 1e-6 * ((t t) t), z_i = m_i + ((c_i0 r0 + c_i1 r1) + c_i2 r2) /
 *                 det, accepted iff every z_k lies in [min(p[a]_k, p[b]_k) - L, max(p[a]_k, p[b]_k) + L] with
 *                 L = max_k |p[a]_k - p[b]_k|; otherwise z = m.  With s_i = ((q_i0 z0 + q_i1 z1) + q_i2 z2) + q_i3 (rows
 *                 of the symmetric Qe), c = ((s0 z0 + s1 z1) + s2 z2) + s3 and cost = c > 0 ? c : 0.  The edge is dropped
 *                 iff cost > max_cost (max_cost = +inf drops none);
 *   4. legality   with N(v) the vertices that share an edge with v and the faces of v those without two equal indices:
 *                 (L1) |N(a) & N(b)| == uses[e]; (L2) no face of a without b and face of b without a have the same
 *                 other two vertices; (L3) for every face with exactly one of a, b, n = u x w as above before and n'
 *                 after that corner moves to z satisfy (n0 n'0 + n1 n'1) + n2 n'2 > 0;
 *   5. key        (cost_bits >> 52) << 52 | (mix(a << 32 | b, r) & 0x1FFFFF) << 31 | e, where cost_bits is the IEEE
 *                 pattern of cost and mix(x, r) is splitmix64's finaliser of x + (r + 1) * 0x9E3779B97F4A7C15 (mod 2^64):
 *                 s ^= s >> 30, s *= 0xBF58476D1CE4E5B9, s ^= s >> 27, s *= 0x94D049BB133111EB, s ^= s >> 31;
 *   6. selection  m1(v) = min key over the legal candidates at v (integer atomicMin), m2(v) = min of m1 over v and N(v);
 *                 e is selected iff key(e) == m2(a) == m2(b).  No end of a selected edge equals or neighbours an end of
 *                 another, so their face sets are disjoint;
 *   7. budget     the selected edges sorted by (cost_bits, e); the first min(selected, max_take) are taken.  Every
 *                 candidate has exactly two faces, so the caller passes max_take = ceil((F - target_faces) / 2);
 *   8. apply      for a taken edge p[a] = z, Q[a] = Qe, b -> a; faces and vertex_target are remapped; the caller then
 *                 compacts and gathers Q, the locks and the maps through the compaction's maps.
 * Boundary quadrics and collapsing boundary edges are qf_mesh_decimate_open.h's; non-manifold edges never collapse.
 *
 * Invalid input is never followed out of bounds: a face with an index outside [0, V), a face_edges entry outside
 * [-1, E) or an edge that is not 0 <= a < b < V takes no part and is counted.                                        */
#ifndef QF_MESH_DECIMATE_H
#define QF_MESH_DECIMATE_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_QUADRIC_COUNTS 2
#define QF_MESH_COLLAPSE_COUNTS 6

/* Bytes of workspace the calls below need for a mesh of this size (host computation; E = 0 for
 * qf_mesh_vertex_quadrics); -1 for sizes outside V in [1, 2^31), F in [0, 2^31 / 3), E in [0, 2^31).                  */
int64_t qf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges);

/* quadrics fp64 [V,10] by the rule above.  counts int64 [2], written on the device: non-finite vertices, faces with an
 * index outside [0, V) (such a face takes no part).  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of range, a
 * NULL vertices / faces (F > 0) / quadrics / workspace / counts or a workspace below
 * qf_mesh_decimate_workspace_bytes(V, F, 0).                                                                           */
int qf_mesh_vertex_quadrics(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                            double *quadrics, void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);

/* Steps 1 to 7 of round `round`; the taken edges stay in `workspace` for qf_mesh_collapse_apply.  edges int64 [E,2] and
 * face_edges int64 [F,3] are qf_mesh_edges_emit's, vertex_lock uint8 [V] may be NULL, max_cost >= 0 (+inf for none).
 * counts int64 [6], written on the device: candidates (step 3), legal candidates (step 4), selected, taken, locked
 * vertices, invalid faces + edges.  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of range, a NULL vertices /
 * faces (F > 0) / edges (E > 0) / face_edges (F > 0) / quadrics / workspace / counts, a short workspace, a max_cost that
 * is negative or NaN, round < 0 or max_take < 0.                                                                       */
int qf_mesh_collapse_select(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                            const int64_t *edges, int64_t n_edges, const int64_t *face_edges, const double *quadrics,
                            const uint8_t *vertex_lock, double max_cost, int64_t round, int64_t max_take,
                            void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);

/* Step 8 for the edges qf_mesh_collapse_select left in `workspace` (same sizes, edges and max_take): vertices and
 * quadrics are updated in place at the kept ends, every index of faces and every entry of vertex_target (int64
 * [n_targets], may be NULL with n_targets == 0; entries outside [0, V) are left alone) that names a removed end is
 * replaced by the kept one.  Refusals as above.                                                                        */
int qf_mesh_collapse_apply(double *vertices, int64_t n_vertices, int64_t *faces, int64_t n_faces, const int64_t *edges,
                           int64_t n_edges, double *quadrics, int64_t max_take, int64_t *vertex_target,
                           int64_t n_targets, void *workspace, int64_t workspace_bytes, void *stream);

/* After qf_mesh_compact_emit: carries the per-vertex and per-face state through its maps.  vertex_map int64
 * [n_out_vertices] and compact_face_map int64 [n_out_faces] are the compaction's; out_quadrics[j] = quadrics[vertex_map
 * [j]], out_lock[j] = vertex_lock[vertex_map[j]] (both NULL or neither), out_face_map[i] = face_map[compact_face_map[i]],
 * and every entry t of vertex_target in [0, V) becomes the output vertex whose source is t, or -1 if there is none.  Map
 * entries out of range write nothing.  `workspace` needs 4 V bytes.  QF_ERR_INVALID_ARGUMENT before any launch for sizes
 * out of range (n_out_vertices in [0, V], n_out_faces in [0, F]), a NULL pointer where the matching count is above zero
 * or a short workspace.                                                                                                */
int qf_mesh_collapse_gather(const double *quadrics, const uint8_t *vertex_lock, const int64_t *face_map,
                            int64_t n_vertices, int64_t n_faces, const int64_t *vertex_map, int64_t n_out_vertices,
                            const int64_t *compact_face_map, int64_t n_out_faces, double *out_quadrics, uint8_t *out_lock,
                            int64_t *out_face_map, int64_t *vertex_target, int64_t n_targets, void *workspace,
                            int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_DECIMATE_H */
