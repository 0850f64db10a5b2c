/* qf_vertex_baked.h -- the vertex-baked renderer of libqf_hip.so: SG features kept at the mesh VERTICES, every
 * quadrature point shaded from the barycentric blend of its triangle's three vertex rows.  Replaces the arithmetic of
 * render_image_finetune_baking_with_occgrid (examples/utils.py:733-861) behind the field evaluation: the barycentrics of
 * :822-823, the blend of :835-836, features_to_rgb of :840.  The reference evaluates the field
 * at the three corners of every sample's triangle; the field depends on the position alone, so the table is evaluated
 * once per vertex and gathered.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer unless documented "host"; work is enqueued on `stream`, nothing waits on the host), QF_ABI_VERSION is
 * unchanged.
 *
 * The vertex table: fp32 [n_vertices, stride], stride = 16 * ceil(W / 16) floats with W = 3 + 7 * n_lobes + 1 (16 / 32 /
 * 48 / 64 for 1 / 2 / 6 / 8 lobes), 16-byte aligned; a row is [diffuse3 | (axis3, lambda, colour3) * n_lobes | sigma |
 * zero pad] -- the columns of NGPRadianceFieldSGNew.features (raw head outputs and the activated density).
 *
 * The arithmetic, every operation rounded on its own: the float64 Cramer barycentrics of the sample in its triangle
 * (b2, b1, b0 = 1 - b1 - b2), each cast to fp32, NOT clamped and NOT renormalised; blend[c] = (f0[c] * b0 + f1[c] * b1)
 * + f2[c] * b2 in fp32 for every column c < W, f_k = the row of the triangle's k-th vertex; sigma = blend[W - 1];
 * rgb = sigmoid(diffuse + sum over lobes of colour * exp(|lambda| (axis / |axis| . dir - 1))) on the blend
 * (qf_sg_features_to_rgb's formula).  A degenerate triangle (1 / det not finite) gives NaN, as in the reference.   */
#ifndef QF_VERTEX_BAKED_H
#define QF_VERTEX_BAKED_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Vertex-triangle records [n_faces * 128 bytes]: the 13 doubles of qf_texel_records_pack's records (corner a, edges e0
 * and e1, d00, d01, d11, 1 / det: the same expressions in the same order), the three vertex ids as int32, 12 zero bytes.
 * vertices float64 [n_vertices, 3] (trimesh keeps float64), faces int64 [n_faces, 3].  One launch, one thread per face.
 * A face with an id outside [0, n_vertices) gets the ids 0, 0, 0 and with them a non-finite 1 / det: it shades NaN and
 * reads nothing out of bounds.  n_vertices must be in [1, 2^31) when n_faces > 0.                                */
#define QF_VERTEX_TRIANGLE_RECORD_BYTES 128
int qf_vertex_records_pack(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces, void *records,
                           void *stream);

/* Samples given by position and triangle -> the blend and its shading, one launch.  The triangle ids come as EXACTLY ONE
 * of index_tri (int64) or index_tri32 (int32); n_device as in qf_texture_shade_points (NULL, or a device count: the
 * kernel handles min(*n_device, n) samples and leaves the rows beyond untouched).  features_out [n, W] or NULL: the
 * blend.  rgb [n,3] and sigma [n]: both set (dirs [n,3] is then required) or both NULL; at least one output is required.
 * stride must be the rule's value for n_lobes.                                                                      */
int qf_vertex_shade_points(const float *table, int32_t stride, int32_t n_lobes, const void *records, const float *points,
                           const int64_t *index_tri, const int32_t *index_tri32, const float *dirs, int64_t n,
                           const int64_t *n_device, float *features_out, float *rgb, float *sigma, void *stream);

/* The vertex-baked frame shaded and composited FRONT TO BACK in one launch with early ray termination:
 * qf_texture_composite_tiles with the texture parameters replaced by the vertex table and the vertex-triangle records.
 * The walk (one wave per 8x8 tile, lane = pixel, rank by rank in depth order), the rule (the rank-k sample contributes
 * iff the optical depth accumulated before it satisfies cum <= stop_tau, cum the compositor's fp32 value; a sample that
 * does not contribute is not shaded; stop_tau = +inf never stops; NaN or negative: QF_ERR_INVALID_ARGUMENT), the
 * outputs and shaded_count are that function's.  With stop_tau = +inf the image equals qf_vertex_shade_points +
 * qf_composite_tiles bit for bit.                                                                                   */
int qf_vertex_composite_tiles(const float *table, int32_t stride, int32_t n_lobes, const void *records, const float *xyz_c,
                              const float *dirs_c, const float *depth_c, const int32_t *tri_c, const int32_t *hit_count,
                              int32_t max_hits, const int64_t *tile_base, int32_t width, int32_t height, float delta_const,
                              int32_t bg_mode, const float *bkgd, float stop_tau, float *out_rgb, float *out_alpha,
                              float *out_depth, float *out_packed, int32_t *shaded_count, void *stream);

/* One vertex-baked camera frame as ONE host call: qf_frame_render_baked's sequence (qf_frame_render up to and including
 * the tile pack, per-ray lists) followed by qf_vertex_composite_tiles on the job's samples, image pointers, delta_const,
 * bg_mode and bkgd.  job->field must be NULL and job->tri_c set; the whole job, the shading struct and stop_tau are
 * validated before the first launch.  Same results as the separate calls, bit for bit.                              */
typedef struct qf_vertex_baked_shading {
    const float *table;                 /* [n_vertices, stride] fp32 */
    const void *records;                /* qf_vertex_records_pack's [n_faces * QF_VERTEX_TRIANGLE_RECORD_BYTES] */
    int64_t n_vertices;
    int32_t stride;
    int32_t n_lobes;
} qf_vertex_baked_shading;
int qf_frame_render_vertex_baked(qf_bvh *bvh, const qf_frame_job *job /* host */,
                                 const qf_vertex_baked_shading *shading /* host */, float stop_tau,
                                 int32_t *shaded_count /* [n_rays] or NULL */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_VERTEX_BAKED_H */
