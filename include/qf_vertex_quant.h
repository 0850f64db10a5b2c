/* qf_vertex_quant.h -- the QUANTISED vertex-baked renderer of libqf_hip.so: the vertex table of
 * qf_vertex_baked.h kept as one 64-byte uint8 record per vertex, in the texel-record format of the baked textures
 * (qf_texture_pack: [alpha | diffuse3 | (lambda, azimuth, elevation, colour3) * n_lobes | zero pad], the codes of
 * FeatureCompression.compress).  A "vertex texture" is a texture set of size T = ceil(sqrt(V)) whose texel
 * (v / T, v % T) holds vertex v; its texel records [T * T, QF_TEXEL_RECORD_BYTES] are the vertex record table, row v =
 * vertex v.  A sample reads its 128-byte triangle record and three 64-byte vertex records.
 *
 * An additive part of the C ABI: the types, status codes and conventions are qf_hip.h's (every data pointer is a device
 * pointer unless documented "host"; work is enqueued on `stream`, nothing waits on the host), QF_ABI_VERSION is
 * unchanged.
 *
 * Common parameters: records uint8 [>= n_vertices, QF_TEXEL_RECORD_BYTES], 16-byte aligned; n_vertices >= 1 (the rows
 * below it exist); n_lobes in 1..QF_MAX_LOBES (else QF_ERR_UNSUPPORTED); sigmoid_codec and lambda_thres as in
 * qf_texture_set; tri_records = qf_vertex_records_pack's records (qf_vertex_baked.h) built with the same n_vertices,
 * whose vertex ids are thereby confined to [0, n_vertices).
 *
 * THE ARITHMETIC RULE.  The decoded row of vertex v is what qf_texture_fetch returns for that texel: the same
 * dequantiser expressions with all their quirks (the linear colour range of +-12 whatever the codec string says unless
 * it is "sigma", the uint8 wrap of the azimuth code, the 1e-6 floor under the density's logarithm).  DECODE FIRST, THEN
 * BLEND: blend[c] = (f0[c] * b0 + f1[c] * b1) + f2[c] * b2 in fp32 on the three DECODED rows, with the unclamped fp32
 * barycentrics of qf_vertex_baked.h; sigma = blend[W - 1], rgb = the SG shading of the blend, W = 3 + 7 * n_lobes + 1.
 * The codes themselves are never blended (the azimuth code wraps mod 256).  Hence every output of the three shading
 * entry points below equals the fp32 entry point of qf_vertex_baked.h run on qf_vertex_quant_decode's table, bit for
 * bit (a degenerate triangle gives NaN in both, at the same positions).                                              */
#ifndef QF_VERTEX_QUANT_H
#define QF_VERTEX_QUANT_H

#include "qf_vertex_baked.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The records decoded to the fp32 vertex table of qf_vertex_baked.h: table_out [n_vertices, stride], row v =
 * [diffuse3 | (axis3, lambda, colour3) * n_lobes | sigma | zero pad].  stride is the rule's value of that header,
 * 16 * ceil(W / 16), or exactly W (no pad; table_out then needs 4-byte alignment only).  One launch, one thread per
 * vertex.                                                                                                            */
int qf_vertex_quant_decode(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                           float lambda_thres, float *table_out, int32_t stride, void *stream);

/* qf_vertex_shade_points on the quantised table: EXACTLY ONE of index_tri (int64) / index_tri32 (int32); n_device NULL
 * or a device count (min(*n_device, n) samples are handled, the rows beyond stay untouched); features_out [n, W] or
 * NULL; rgb [n,3] and sigma [n] both set (dirs [n,3] is then required) or both NULL; at least one output.            */
int qf_vertex_quant_shade_points(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                                 float lambda_thres, const void *tri_records, const float *points, const int64_t *index_tri,
                                 const int32_t *index_tri32, const float *dirs, int64_t n, const int64_t *n_device,
                                 float *features_out, float *rgb, float *sigma, void *stream);

/* qf_vertex_composite_tiles with the table parameters replaced: the same walk, rule, outputs, shaded_count, refusals
 * and stop_tau semantics (+inf never stops; NaN or negative: QF_ERR_INVALID_ARGUMENT).  With stop_tau = +inf the image
 * equals qf_vertex_quant_shade_points + qf_composite_tiles bit for bit.                                              */
int qf_vertex_quant_composite_tiles(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                                    float lambda_thres, const void *tri_records, const float *xyz_c, const float *dirs_c,
                                    const float *depth_c, const int32_t *tri_c, const int32_t *hit_count, int32_t max_hits,
                                    const int64_t *tile_base, int32_t width, int32_t height, float delta_const,
                                    int32_t bg_mode, const float *bkgd, float stop_tau, float *out_rgb, float *out_alpha,
                                    float *out_depth, float *out_packed, int32_t *shaded_count, void *stream);

/* One quantised vertex-baked camera frame as ONE host call: qf_frame_render_vertex_baked's sequence with the compositor
 * above.  job->field must be NULL and job->tri_c set; the whole job, the shading struct and stop_tau are validated
 * before the first launch.  Same results as the separate calls, bit for bit.                                        */
typedef struct qf_vertex_quant_shading {
    const uint8_t *records;             /* [>= n_vertices, QF_TEXEL_RECORD_BYTES] */
    const void *tri_records;            /* qf_vertex_records_pack's [n_faces * QF_VERTEX_TRIANGLE_RECORD_BYTES] */
    int64_t n_vertices;
    int32_t n_lobes;
    int32_t sigmoid_codec;
    float lambda_thres;
} qf_vertex_quant_shading;
int qf_frame_render_vertex_quant(qf_bvh *bvh, const qf_frame_job *job /* host */,
                                 const qf_vertex_quant_shading *shading /* host */, float stop_tau,
                                 int32_t *shaded_count /* [n_rays] or NULL */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* QF_VERTEX_QUANT_H */
