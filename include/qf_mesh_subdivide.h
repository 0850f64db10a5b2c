/* qf_mesh_subdivide.h -- mesh refinement of libqf_hip.so: the undirected edges of a triangle
 * mesh numbered on the device (stage A), and a conforming midpoint split of the faces along any marked subset of those
 * edges, with the maps that carry a per-vertex table along (stage B).  Integer work only: the one piece of arithmetic is
 * the midpoint 0.5 * (p[min] + p[max]) in fp64; coordinates are never read for a decision, and every result is the same
 * bit for bit from run to run and from launch shape to launch shape.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer; work is enqueued on `stream`, nothing waits on the host; every refusal comes before the first launch),
 * QF_ABI_VERSION is unchanged.
 *
 * STAGE A, the edges of faces int64 [F,3] over V vertices (V in [1, 2^31), F in [0, 2^31 / 3): a half-edge id fits 31
 * bits):
 *   1. validity     a face with an index outside [0, V) is invalid; if any face is, nothing is produced: counts[2] holds
 *                   their number, counts[0], [1] and [3] are zero and emit writes nothing;
 *   2. half-edges   half-edge h = 3 f + k joins v_k and v_{(k+1) mod 3} of face f;
 *   3. degenerate   a face with two equal indices is degenerate: it is counted, its three face_edges are -1 and it
 *                   contributes no edge;
 *   4. undirected   an undirected edge is the pair (min, max) of a half-edge's two indices;
 *   5. ids          edges are numbered in the order of their lowest half-edge (first appearance): edges[e] = (min, max),
 *                   face_edges[f, k] is the id of half-edge 3 f + k;
 *   6. counts       int64 [4]: E, degenerate faces, invalid faces, boundary edges (used by exactly one half-edge).
 *
 * STAGE B, the split of the same faces by edge_mark uint8 [E] (an edge is marked iff its byte is not zero), given stage
 * A's face_edges (F in [0, 2^29), V + E < 2^31, so that V' and F' stay below 2^31 whatever the marks):
 *   1. validity     as above, and a face that is not degenerate whose face_edges row leaves [0, E) is invalid too;
 *                   counts[6] holds their number, the rest is zero and emit writes nothing;
 *   2. vertices     a marked edge e gets vertex V + (number of marked edges with a smaller id), at 0.5 * (p[min] +
 *                   p[max]) per component in fp64 (one add, one multiply), written once, from the edge's lowest marked
 *                   half-edge; vertex_parents is (min, max) for a new vertex and (v, v) for an old one; the first V
 *                   output rows copy the input bit for bit;
 *   3. children     with m_k the vertex of the face's edge k and indices taken mod 3:
 *                     0 marked            (v0, v1, v2)
 *                     1 marked, edge k    u = (v_k, v_{k+1}, v_{k+2}):  (u0, m, u2)  (m, u1, u2)
 *                     2 marked, j not     u = (v_{j+1}, v_{j+2}, v_j), a = mid(u0, u1), b = mid(u1, u2):  the corner
 *                                         (a, u1, b), then the quad (u0, a, b, u2) cut from its original corner with the
 *                                         smaller index: u0 < u2 gives (u0, a, b) (u0, b, u2), else (u0, a, u2) (a, b, u2)
 *                     3 marked            (v0, m0, m2)  (m0, v1, m1)  (m2, m1, v2)  (m0, m1, m2)
 *                   a degenerate face is copied unsplit;
 *   4. order        children keep the parent's winding and are consecutive, in the order above, parents in input order;
 *                   face_map[child] = parent;
 *   5. counts       int64 [7]: F', V', faces with 0, 1, 2 and 3 marked edges (degenerate faces count as 0), invalid
 *                   faces.
 * Every marked edge is split at the same vertex in every face that uses it, so the result has no T-junction whatever
 * the marks are, non-manifold edges included.                                                                         */
#ifndef QF_MESH_SUBDIVIDE_H
#define QF_MESH_SUBDIVIDE_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_EDGES_COUNTS 4
#define QF_MESH_SUBDIVIDE_COUNTS 7

/* Bytes of workspace stage A needs for a mesh of this size (host computation); -1 for sizes out of range.            */
int64_t qf_mesh_edges_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Rules 1 to 5 of stage A, kept in `workspace`; counts[4] is written on the device.  QF_ERR_INVALID_ARGUMENT before any
 * launch for sizes out of range, a NULL faces (F > 0) / workspace / counts or a short workspace.                      */
int qf_mesh_edges_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, void *workspace,
                        int64_t workspace_bytes, int64_t *counts, void *stream);

/* Writes edges (int64 [.,2], capacity n_edges rows: rows beyond it are not written) and face_edges (int64 [F,3], every
 * row) from the workspace qf_mesh_edges_count left for the same faces.  The caller reads counts between the two calls
 * (the one host wait) and passes counts[0].  Refusals as above, plus n_edges outside [0, 3 F], a NULL edges with
 * n_edges > 0 or a NULL face_edges with F > 0.                                                                        */
int qf_mesh_edges_emit(const int64_t *faces, int64_t n_faces, int64_t n_vertices, void *workspace,
                       int64_t workspace_bytes, int64_t *edges, int64_t n_edges, int64_t *face_edges, void *stream);

/* Bytes of workspace stage B needs; -1 for sizes out of range.                                                        */
int64_t qf_mesh_subdivide_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges);

/* The children per face, the output positions of faces and new vertices and the half-edge that writes each new vertex,
 * kept in `workspace`; counts[7] is written on the device.  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of
 * range, a NULL faces / face_edges (F > 0) / edge_mark (E > 0) / workspace / counts or a short workspace.             */
int qf_mesh_subdivide_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *face_edges,
                            int64_t n_edges, const uint8_t *edge_mark, void *workspace, int64_t workspace_bytes,
                            int64_t *counts, void *stream);

/* Writes the refined mesh from the workspace qf_mesh_subdivide_count left, with the same mesh and marks.  Capacities:
 * n_out_vertices rows of out_vertices (fp64 [.,3]) and vertex_parents (int64 [.,2]), n_out_faces rows of out_faces
 * (int64 [.,3]) and face_map (int64); rows beyond a capacity are not written, the two maps may be NULL.  The caller
 * passes counts[1] and counts[0].  Refusals as above, plus a NULL vertices, a capacity outside [0, V + E] / [0, 4 F] or
 * a NULL out_vertices / out_faces with a capacity above zero.                                                         */
int qf_mesh_subdivide_emit(const double *vertices, const int64_t *faces, int64_t n_faces, int64_t n_vertices,
                           const int64_t *face_edges, int64_t n_edges, const uint8_t *edge_mark, void *workspace,
                           int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices, int64_t *out_faces,
                           int64_t n_out_faces, int64_t *face_map, int64_t *vertex_parents, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_SUBDIVIDE_H */
