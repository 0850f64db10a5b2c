/* qf_mesh_compact.h -- mesh clean-up of libqf_hip.so: faces selected by a keep mask, degenerate
 * and duplicate faces dropped, small connected components ("islands") dropped, unreferenced vertices removed and the
 * faces remapped; and the visibility mask of the reference's prunning_mesh_train_visibility (examples/mc_utils.py:
 * 272-345) marked from an intersector's id lists.  Integer work only: vertex coordinates are copied, never read for a
 * decision, and every result is the same bit for bit from run to run.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer; work is enqueued on `stream`, nothing waits on the host), QF_ABI_VERSION is unchanged.
 *
 * THE RULES, applied in this order to vertices fp64 [V,3], faces int64 [F,3], an optional keep mask uint8 [F], `flags`
 * and `min_component_faces` = M (V in [1, 2^31), F in [0, 2^31)):
 *   1. validity     a face with an index outside [0, V) is invalid; if any face is, nothing is produced: counts[7] holds
 *                   their number, counts[0..6] are zero and emit writes nothing;
 *   2. mask         face f survives iff keep is NULL or keep[f] != 0;
 *   3. degenerate   (QF_MESH_REMOVE_DEGENERATE) a surviving face with two equal indices is dropped; with the flag off it
 *                   stays and takes part in 4 and 5 like any other face;
 *   4. duplicates   (QF_MESH_REMOVE_DUPLICATES) two surviving faces are duplicates iff their index triples are equal
 *                   after sorting each triple (rotations and opposite windings included); the face with the lowest
 *                   index stays.  A face whose earlier copy was dropped by 2 or 3 stays;
 *   5. islands      surviving faces are connected through shared vertex INDICES; a component's size is its number of
 *                   surviving faces; counts[6] is the number of components (always computed, before the drop); with
 *                   M >= 2 the faces of components with fewer than M faces are dropped;
 *   6. vertices     (QF_MESH_REMOVE_UNREFERENCED) a vertex stays iff a surviving face uses it; kept vertices keep their
 *                   relative order, the new index is the number of kept vertices below it, faces are remapped.  With the
 *                   flag off vertices and indices are untouched (V' = V).
 * Output faces keep their input order and winding.
 *
 * counts int64 [8]: kept faces, kept vertices, faces dropped by the mask, as degenerate, as duplicates, as small
 * islands, number of components, invalid faces.                                                                       */
#ifndef QF_MESH_COMPACT_H
#define QF_MESH_COMPACT_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define QF_MESH_REMOVE_DEGENERATE 1
#define QF_MESH_REMOVE_DUPLICATES 2
#define QF_MESH_REMOVE_UNREFERENCED 4
#define QF_MESH_COMPACT_COUNTS 8

/* Bytes of workspace the pair below needs for a mesh of this size (host computation); -1 for sizes out of range.     */
int64_t qf_mesh_compact_workspace_bytes(int64_t n_vertices, int64_t n_faces);

/* Steps 1 to 5, the vertex marks and the output positions, kept in `workspace`; counts[8] is written on the device.
 * keep may be NULL.  QF_ERR_INVALID_ARGUMENT before any launch for sizes out of range, a NULL vertices / faces (F > 0)
 * / workspace / counts, a short workspace, unknown flag bits or min_component_faces outside [0, 2^31).               */
int qf_mesh_compact_count(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                          const uint8_t *keep, int32_t flags, int64_t min_component_faces, void *workspace,
                          int64_t workspace_bytes, int64_t *counts, void *stream);

/* Writes the mesh from the workspace qf_mesh_compact_count left, with the same mesh, keep, flags and M.  Capacities:
 * n_out_vertices rows of out_vertices (fp64 [.,3], copies that keep the input's bits) and vertex_map (int64, the source
 * vertex of each output vertex), n_out_faces rows of out_faces (int64 [.,3]) and face_map (int64, the source face);
 * rows beyond a capacity are not written, the maps may be NULL.  The caller reads counts between the two calls (the one
 * host wait) and passes counts[1] and counts[0].  Refusals as above, plus a capacity outside [0, V] / [0, F] or a NULL
 * out_vertices / out_faces with a capacity above zero.                                                               */
int qf_mesh_compact_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                         const uint8_t *keep, int32_t flags, int64_t min_component_faces, void *workspace,
                         int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices, int64_t *out_faces,
                         int64_t n_out_faces, int64_t *face_map, int64_t *vertex_map, void *stream);

/* The faces some ray hits among its first max_hits hits, as qf_mark_visited_cells does for cells: hit_tri int32
 * [n_rays, max_hits], hit_count int32 [n_rays] or NULL.  For ray r the slots considered are k < min(hit_count[r],
 * max_hits); with hit_count NULL every slot whose id is >= 0 is considered.  For a considered slot mask[id] = 1; an id
 * outside [0, n_faces) writes nothing and adds one to *out_of_range (int64, may be NULL).  The call only ever sets
 * bytes of mask (uint8 [n_faces]), so views accumulate into one mask.  n_rays >= 0, 1 <= max_hits, n_rays * max_hits <
 * 2^40, 0 <= n_faces < 2^31 (else QF_ERR_INVALID_ARGUMENT, before the launch).                                       */
int qf_mark_hit_faces(const int32_t *hit_tri, const int32_t *hit_count, int64_t n_rays, int32_t max_hits, int64_t n_faces,
                      uint8_t *mask, int64_t *out_of_range, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_MESH_COMPACT_H */
