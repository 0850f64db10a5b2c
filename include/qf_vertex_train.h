/* qf_vertex_train.h -- training through the vertex table of libqf_hip.so: the backward of qf_vertex_shade_points
 * (include/qf_vertex_baked.h), from the gradient of a loss with respect to every sample's colour and density to its
 * gradient with respect to the table.  An extension of this project: the reference only
 * evaluates through render_image_finetune_baking_with_occgrid.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer unless documented "host"; work is enqueued on `stream`, nothing waits on the host), QF_ABI_VERSION is
 * unchanged.  The vertex table, its stride rule and the vertex-triangle records are qf_vertex_baked.h's. */
#ifndef QF_VERTEX_TRAIN_H
#define QF_VERTEX_TRAIN_H

#include "qf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* grad_table [n_vertices, stride] += d(sum_i d_rgb[i] . rgb[i] + d_sigma[i] sigma[i]) / d table, rgb and sigma those of
 * qf_vertex_shade_points on the same table, records, points, ids and dirs.  One launch.  The forward is recomputed (the
 * same barycentrics and the same blend, bit for bit) and nothing is kept between the two calls.  The caller zeroes
 * grad_table; the kernel accumulates with fp32 atomic adds, so the last bits depend on the order of arrival.
 *
 * For a sample with barycentrics b and triangle vertices v_0..v_2: grad_table[v_k][c] += d_blend[c] * b_k, d_blend the
 * gradient of the SG mixture on the blend (qf_sg_features_to_rgb_backward's formula: d|lambda| is 0 at lambda = 0, the
 * axis gradient is projected orthogonally to the unit axis and divided by the norm) in the columns below W - 1 and
 * d_sigma[i] in the density column W - 1.  d_sigma NULL: the density is frozen, its column gets no gradient and is not
 * written.  The pad columns W..stride-1 are never written.
 *
 * A sample contributes NOTHING when its record's 1 / det is not finite (a degenerate face, or a face whose ids
 * qf_vertex_records_pack found out of range and set to 0, 0, 0: the forward's NaN does not reach row 0), when one of its
 * three vertex ids lies outside [0, n_vertices), or when it lies at or beyond min(*n_device, n) (n_device as in
 * qf_vertex_shade_points; NULL: n samples).
 *
 * The triangle ids come as EXACTLY ONE of index_tri (int64) or index_tri32 (int32).  table and grad_table 16-byte
 * aligned, stride the rule's value for n_lobes, n_vertices in [1, 2^31).  n = 0 returns QF_OK at once.           */
int qf_vertex_shade_points_backward(const float *table, int32_t stride, int32_t n_lobes, const void *records,
                                    int64_t n_vertices, const float *points, const int64_t *index_tri,
                                    const int32_t *index_tri32, const float *dirs, int64_t n, const int64_t *n_device,
                                    const float *d_rgb, const float *d_sigma /* or NULL */,
                                    float *grad_table /* [n_vertices, stride], accumulated */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_VERTEX_TRAIN_H */
