/* qf_mesh_manifold.h -- making a triangle mesh a manifold with boundary, in libqf_hip.so: the
 * mesh is CUT along its complex edges (three or more faces) and every vertex is SPLIT into one copy per fan of faces.  No
 * face is dropped and no coordinate changes: out_vertices[out_faces] is vertices[faces] bit for bit, so every rendered
 * frame is unchanged, while every edge of the result has at most two faces and every vertex exactly one fan -- the
 * meshes qf_mesh_decimate_open.h can collapse.  This is not open3d's remove_non_manifold_edges (which drops faces).
 * Integer work only, no floating-point operation: coordinates move as 64-bit words and are never read for a decision;
 * every result is the same bit for bit from run to run and from launch shape to launch shape.  The rule is restated in
 * numpy in tests/mesh_manifold_reference.py.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`, nothing
 * waits on the host; every refusal comes before the first launch); QF_ABI_VERSION is unchanged.
 *
 * INPUT  vertices fp64 [V,3], faces int64 [F,3], and face_edges int64 [F,3] with its edge count E from
 * qf_mesh_edges_count / qf_mesh_edges_emit (qf_mesh_subdivide.h, stage A).  V in [1, 2^31), F in [0, 2^31 / 3) (a corner
 * id fits 31 bits), E in [0, 2^31).
 *   1. validity    a face with an index outside [0, V) is invalid, and so is a face that is not degenerate whose
 *                  face_edges row leaves [0, E); if any face is, nothing is produced: counts[7] holds their number, the
 *                  other counts are zero and emit writes nothing;
 *   2. proper      a face with two equal indices is degenerate (stage A's rule 3): it is counted, copied to the output
 *                  unchanged and takes part in nothing below; the other faces are proper;
 *   3. uses        uses[e] is the number of half-edges of proper faces with edge id e;
 *   4. links       corner c = 3 f + k of a proper face is vertex faces[f, k]; half-edge h = 3 f + k touches corners
 *                  3 f + k and 3 f + (k + 1) mod 3.  For every edge with uses == 2, each of the two corners of one face
 *                  on it is linked to the corner of the other face with the same vertex index, whichever way the two
 *                  half-edges run.  Edges with uses == 1 or uses > 2 link nothing;
 *   5. classes     the connected components of the corners under the links; all corners of a class are the same input
 *                  vertex; a class's id is its lowest corner;
 *   6. numbering   of the classes of vertex v the one with the lowest id keeps the index v; every other class is extra
 *                  and gets V + r, r the number of extra classes with a lower id (the order of first appearance).  A
 *                  vertex without a class (unreferenced, or used by degenerate faces only) keeps its row;
 *   7. output      out_vertices fp64 [V',3]: the first V rows are the input, row V + r copies its class's vertex, all
 *                  moved as 64-bit words (NaN payloads included); vertex_map int64 [V'], the source vertex of every row
 *                  (the identity on the first V); out_faces int64 [F,3], same order and winding, every corner of a
 *                  proper face replaced by its class's index.  Faces do not move, so there is no face map;
 *   8. counts      int64 [8]: V'; input vertices with two or more classes; edges with uses > 2; proper faces with at
 *                  least one such edge; edges with uses == 1; edges with uses == 2 whose two half-edges run in the same
 *                  direction (inconsistently wound neighbours: reported, never acted on); degenerate faces; invalid
 *                  faces.
 * A mesh that already has at most two faces on every edge and one fan at every vertex comes back as itself, V' = V, and
 * the pass applied to its own output changes nothing.  Duplicate faces put three or more faces on their edges and are
 * therefore cut apart from their neighbours: drop them first (qf_mesh_compact.h, QF_MESH_REMOVE_DUPLICATES).
 * A face_edges that is not stage A's for these faces is never followed out of bounds: a pair of half-edges that does
 * not join the same two vertices links nothing.                                                                       */
#ifndef QF_MESH_MANIFOLD_H
#define QF_MESH_MANIFOLD_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_MANIFOLD_COUNTS 8

/* Bytes of workspace the two calls below need for a mesh of this size (host computation); -1 for sizes out of range. */
int64_t qf_mesh_manifold_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges);

/* Rules 1 to 6, kept in `workspace`; counts[8] is written on the device.  QF_ERR_INVALID_ARGUMENT before any launch for
 * sizes out of range, a NULL faces / face_edges (F > 0) / workspace / counts or a short workspace.                    */
int qf_mesh_manifold_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *face_edges,
                           int64_t n_edges, void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);

/* Rule 7 from the workspace qf_mesh_manifold_count left for the same faces (workspace_bytes is what it was there).  The
 * caller reads counts[0] between the two calls (the one host wait) and passes it as n_out_vertices, the capacity in rows
 * of out_vertices and vertex_map: rows beyond it are not written; out_faces gets every row; vertex_map may be NULL.
 * Refusals as above, plus a NULL vertices, n_out_vertices outside [0, V + 3 F], a NULL out_vertices with
 * n_out_vertices > 0 or a NULL out_faces with F > 0.                                                                  */
int qf_mesh_manifold_emit(const double *vertices, const int64_t *faces, int64_t n_faces, int64_t n_vertices,
                          void *workspace, int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                          int64_t *out_faces, int64_t *vertex_map, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_MANIFOLD_H */
