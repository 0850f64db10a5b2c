/* qf_mesh_decimate_open.h -- decimation of open meshes in libqf_hip.so (boundary = "collapse"):
 * the rounds of qf_mesh_decimate.h with boundary quadrics and boundary edge collapses, so that a mesh with borders reaches
 * its face count instead of keeping every border vertex.  The rules extend that header's (same numbering of steps, same
 * fp64 operation-order discipline, -ffp-contract=off, integer atomics only); they are restated in numpy in
 * tests/mesh_decimate_open_reference.py.  On a mesh without boundary or non-manifold edges every call below computes the
 * bits of its counterpart there.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`; every
 * refusal comes before the first launch); QF_ABI_VERSION is unchanged.  A round is that header's with
 * qf_mesh_collapse_select_open / qf_mesh_collapse_apply_open in place of select / apply; round 0 calls
 * qf_mesh_boundary_quadrics after qf_mesh_vertex_quadrics and qf_mesh_edges_emit.
 *
 * BOUNDARY QUADRICS (round 0).  For every edge e = (a, b) with uses[e] == 1, n the unit normal of its one face (that
 * header's face plane): m = (p[b] - p[a]) x n = (d1 n2 - d2 n1, d2 n0 - d0 n2, d0 n1 - d1 n0) with d = p[b] - p[a],
 * len = sqrt((m0 m0 + m1 m1) + m2 m2); the edge is left out if n is the zero plane or len == 0, else m = m / len per
 * component and d = -((m0 p[a]x + m1 p[a]y) + m2 p[a]z).  Q[v] = Q[v] + boundary_weight * (pl_r * pl_c) per component of
 * the upper triangle, pl = (m, d), over the boundary edges of v in ascending edge index, continuing the face sum.
 *
 * EACH ROUND differs from qf_mesh_decimate.h's in these steps:
 *   2. classes    nb[v] is the number of edges at v with uses == 1; bad[v] iff an edge at v has uses > 2 or uses == 0.
 *                 v is interior iff nb == 0 and not bad, border iff nb == 2 and not bad, else complex.  A vertex is locked
 *                 iff its vertex_lock byte is not zero or it is complex;
 *   3. candidate  an edge with both ends unlocked and (a) uses == 2, both ends interior; or (b) uses == 2, one end interior
 *                 and one border: z is the border end's position, bit for bit, and cost is Qe's at that z by the same
 *                 expression; or (c) uses == 1, unless the three edges of its face all have uses == 1 (an isolated
 *                 triangle).  z of (a) and (c) is that header's.  An edge with uses == 2 and two border ends (a chord) is
 *                 no candidate;
 *   7. budget     the selected edges sorted by (cost_bits, e); the i-th is taken iff the uses of those in front of it sum
 *                 to less than faces_to_remove = F - target_faces: the shortest prefix whose summed uses reaches it, or
 *                 all of them (a device-wide exclusive scan; the count stays on the device);
 *   8. apply      as there, with z of step 3 for the edge's kind.
 * Steps 1, 4 (L1 forbids closing a three-edge hole), 5 and 6 are unchanged.  Collapsing non-manifold edges is out of
 * scope: their ends are locked.
 *
 * Invalid input is never followed out of bounds: it takes no part and is counted, as in qf_mesh_decimate.h.             */
#ifndef QF_MESH_DECIMATE_OPEN_H
#define QF_MESH_DECIMATE_OPEN_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_BOUNDARY_COUNTS 2
#define QF_MESH_COLLAPSE_OPEN_COUNTS 8

/* Bytes of workspace the calls below need (host computation): qf_mesh_decimate_workspace_bytes plus the class, budget and
 * boundary-plane arrays; -1 for sizes outside V in [1, 2^31), F in [0, 2^31 / 3), E in [0, 2^31).                       */
int64_t qf_mesh_decimate_open_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges);

/* Adds the boundary planes to quadrics fp64 [V,10] in place, by the rule above.  edges int64 [E,2] and face_edges int64
 * [F,3] are qf_mesh_edges_emit's.  counts int64 [2], written on the device: boundary edges that gave a plane, invalid
 * edges + face_edges entries.  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of range, a NULL vertices / faces
 * (F > 0) / edges (E > 0) / face_edges (F > 0) / quadrics / workspace / counts, a short workspace or a boundary_weight
 * that is negative or not finite.                                                                                      */
int qf_mesh_boundary_quadrics(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                              const int64_t *edges, int64_t n_edges, const int64_t *face_edges, double *quadrics,
                              double boundary_weight, void *workspace, int64_t workspace_bytes, int64_t *counts,
                              void *stream);

/* Steps 1 to 7 of round `round` in collapse mode; the taken edges, the classes and uses stay in `workspace` for
 * qf_mesh_collapse_apply_open.  Arguments as qf_mesh_collapse_select's, with faces_to_remove = F - target_faces in place
 * of max_take.  counts int64 [8], written on the device: candidates, legal candidates, selected, taken, locked vertices,
 * invalid faces + edges, taken edges with uses == 1, border vertices.  Refusals as there (faces_to_remove < 0).         */
int qf_mesh_collapse_select_open(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                 const int64_t *edges, int64_t n_edges, const int64_t *face_edges, const double *quadrics,
                                 const uint8_t *vertex_lock, double max_cost, int64_t round, int64_t faces_to_remove,
                                 void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);

/* Step 8 for the edges qf_mesh_collapse_select_open left in `workspace` (same sizes, edges and faces_to_remove);
 * otherwise as qf_mesh_collapse_apply.                                                                                 */
int qf_mesh_collapse_apply_open(double *vertices, int64_t n_vertices, int64_t *faces, int64_t n_faces, const int64_t *edges,
                                int64_t n_edges, double *quadrics, int64_t faces_to_remove, int64_t *vertex_target,
                                int64_t n_targets, void *workspace, int64_t workspace_bytes, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_DECIMATE_OPEN_H */
