/* qf_mesh_weld.h -- welding the vertices of a triangle mesh by position, in libqf_hip.so: two
 * vertices at the same place (tolerance 0) or within a tolerance h of one another become one vertex, transitively, and
 * the faces are renumbered.  No face is dropped and no coordinate is computed: an output row is the row of its class's
 * lowest input vertex, moved as 64-bit words.  The rule is this project's own and is restated in numpy in
 * tests/mesh_weld_reference.py; it is not trimesh's merge_vertices, parity with which is unpinned.  Every result is the
 * same bit for bit from run to run and from launch shape to launch shape.
 *
 * An additive part of the C ABI under qf_hip.h's conventions (device pointers only; work is enqueued on `stream`, nothing
 * waits on the host; every refusal comes before the first launch); QF_ABI_VERSION is unchanged.
 *
 * INPUT  vertices fp64 [V,3]; faces int64 [F,3], which may be NULL with F = 0; a tolerance h, fp64, finite, h >= 0.
 * V in [1, 2^31), F in [0, 2^31).
 *   1. validity    a face with an index outside [0, V) is invalid.  A vertex with a coordinate that is not finite is
 *                  LOOSE: a class of its own that links to nothing (two vertices with the same NaN bits do not merge).
 *                  With h > 0 the search cell of a finite vertex is c = floor(x / s) per axis, one fp64 division and
 *                  one floor, for the cell edge s = 2 max(h, 2^-510), or s = +inf when h * h is not finite (then every
 *                  c is 0); a finite vertex with a c that is not finite or has |c| >= 2^51 is OUT OF RANGE.  If any
 *                  face is invalid or any vertex out of range nothing is produced: counts[6] and counts[7] hold their
 *                  numbers, the other counts are zero and emit writes nothing;
 *   2. link        with h == 0 two finite vertices are linked iff their three coordinates compare equal with ==
 *                  (so -0.0 links with +0.0).  With h > 0 they are linked iff ((dx*dx + dy*dy) + dz*dz) <= h*h with
 *                  dx = xa - xb and so on, every operation in fp64, rounded on its own, never fused: symmetric by
 *                  construction, and a closed ball (a pair at distance exactly h links).  The cells decide nothing:
 *                  they only bound the search (no linked pair lies outside the 27 cells around c);
 *   3. classes     the connected components of the link graph (single linkage: a chain of points each within h of the
 *                  next is one class, however long); a class is named by its lowest vertex index, its ROOT;
 *   4. numbering   output row i is the i-th root in increasing index order; vertex_class int64 [V] is the output row
 *                  of every input vertex, vertex_map int64 [V'] the root of every output row, so
 *                  vertex_class[vertex_map] == arange(V');
 *   5. output      out_vertices[i] is the root's row, moved as 64-bit words (NaN payloads and signed zeros pass
 *                  through); out_faces[f, k] = vertex_class[faces[f, k]], same order and winding.  No face is dropped:
 *                  faces that become degenerate stay and are counted (qf_mesh_compact.h removes them);
 *   6. counts      int64 [8]: V'; classes with two or more members; the size of the largest class; faces that were not
 *                  degenerate (two equal indices) before and are after; with h > 0 the largest population of one
 *                  search cell, else 0; loose vertices; out-of-range vertices; invalid faces.
 * With h == 0 out_vertices[out_faces] == vertices[faces] as values (bit for bit when the mesh has no negative zero).  A
 * mesh with no linked pair comes back as itself.  The weld of its own output at the same h is the identity whenever no
 * two roots are within h, which always holds for h == 0.  With h > 0 a root may sit up to the class's diameter away
 * from a member.  The link pass costs the square of a cell's population: counts[4] reports it.                        */
#ifndef QF_MESH_WELD_H
#define QF_MESH_WELD_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_WELD_COUNTS 8

/* Bytes of workspace the two calls below need for a mesh of this size, whatever the tolerance (host computation); -1
 * for sizes out of range.                                                                                              */
int64_t qf_mesh_weld_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Rules 1 to 4, kept in `workspace`; counts[8] is written on the device.  QF_ERR_INVALID_ARGUMENT before any launch for
 * sizes out of range, a NULL vertices / faces (F > 0) / workspace / counts, a short workspace, or a tolerance that is
 * negative or not finite.                                                                                              */
int qf_mesh_weld_count(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces, double tolerance,
                       void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream);

/* Rule 5 from the workspace qf_mesh_weld_count left for the same mesh (workspace_bytes is what it was there).  The
 * caller reads counts[0] between the two calls (the one host wait) and passes it as n_out_vertices, the capacity in rows
 * of out_vertices and vertex_map: rows beyond it are not written.  out_faces [F,3] and vertex_class [V] get every row;
 * vertex_map and vertex_class may be NULL.  Refusals as above, plus n_out_vertices outside [0, V], a NULL out_vertices
 * with n_out_vertices > 0 or a NULL out_faces with F > 0.                                                             */
int qf_mesh_weld_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces, void *workspace,
                      int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices, int64_t *out_faces,
                      int64_t *vertex_map, int64_t *vertex_class, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_WELD_H */
