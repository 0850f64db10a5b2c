// One camera frame of the mesh-quadrature render as ONE host call: the fixed launch sequence of a render-only frame
// (FrameRenderer.render_async: examples/utils.py:510-620 behind nerf_synthetic.py:310-373's camera rays), composed
// from the library's own entry points -- nothing here launches a kernel of its own.  Two sequences: the per-ray lists
// (qf_raster_intersect ... qf_pack_tiles) and, for the plain pass with a field, the hit bins (qf_raster_intersect_tiles
// ... qf_pack_tiles_bins); same frame bit for bit.  qf_frame_prune is the same sequence with the last launch replaced by
// qf_composite_tiles_trimax (the tile compositor that folds its weights into the triangles); qf_frame_render_baked is the
// sampling half (no field) followed by qf_texture_composite_tiles (the baked-texture frame, shaded and composited front to
// back in one launch) and qf_frame_render_vertex_baked the same with qf_vertex_composite_tiles (the vertex-baked frame,
// include/qf_vertex_baked.h) and qf_frame_render_vertex_quant with qf_vertex_quant_composite_tiles (its quantised table,
// include/qf_vertex_quant.h); qf_frame_render_front is the sequence up to the tile pack followed by the rank windows of
// front_frame.hip (select launches + one field launch per window) and their finish: the field frame front to back with
// early ray termination.
#include "qf_common.h"
#include "qf_vertex_quant.h"
#include "vertex_baked_device.h"

namespace {

// what qf_frame_prune adds to a job (its parameters; the job struct has no room for them)
struct PruneTarget {
    float *tri_weight;
    int64_t n_tri;
    float valid_threshold;
    int64_t *counts;
    int32_t *bad_ids;
};

// The field over min(*n_device, cap) points of the job's samples, in the job's precision; order as qf_field_forward's.
int field_launch(const qf_frame_job &j, int64_t cap, const int64_t *n_device, const int32_t *order, void *stream)
{
    if (j.field_precision == QF_FIELD_FP32)
        return qf_field_forward(j.field, static_cast<const float *>(j.table), static_cast<const float *>(j.base_w),
                                static_cast<const float *>(j.head_ngp_w), static_cast<const qf_sg_head *>(j.head_sg),
                                j.xyz_c, j.dirs_c, cap, n_device, order, j.rgb_c, j.sigma_c, nullptr, nullptr, nullptr,
                                stream);
    auto fwd = j.field_precision == QF_FIELD_BF16 ? qf_field_forward_bf16 : qf_field_forward_f16;
    return fwd(j.field, static_cast<const uint16_t *>(j.table), static_cast<const uint16_t *>(j.base_w),
               static_cast<const uint16_t *>(j.head_ngp_w), static_cast<const qf_sg_head_bf16 *>(j.head_sg), j.xyz_c,
               j.dirs_c, cap, n_device, order, j.rgb_c, j.sigma_c, nullptr, stream);
}

// The frame's launch sequence; prune == nullptr: qf_frame_render.  samples_only: the job is validated as a whole, field
// and image included, but the sequence ends with the tile pack (qf_frame_render_front goes on from there).
int frame_sequence(qf_bvh *bvh, const qf_frame_job *job, const PruneTarget *prune, void *stream, bool samples_only = false)
{
    if (!bvh || !job || !job->camera) return QF_ERR_INVALID_ARGUMENT;
    const qf_frame_job &j = *job;
    const int32_t w = j.camera->width, h = j.camera->height;
    if (w < 1 || h < 1 || j.n_rays != (int64_t)w * h || j.max_hits < 1) return QF_ERR_INVALID_ARGUMENT;
    if (!j.rays_o || !j.rays_d || !j.hit_tri || !j.hit_t || !j.hit_count || !j.final_count || !j.tile_base || !j.total ||
        !j.dropped || !j.xyz_c || !j.dirs_c || !j.depth_c)
        return QF_ERR_INVALID_ARGUMENT;
    if (j.field_precision < QF_FIELD_FP32 || j.field_precision > QF_FIELD_FP16) return QF_ERR_INVALID_ARGUMENT;
    // pruning composites: a field, the samples' triangle ids and the per-triangle maxima are required; the image is not
    const bool image = !prune || j.out_packed || j.out_rgb || j.out_alpha || j.out_depth;
    if (prune && (!j.field || !j.tri_c || !prune->tri_weight || prune->n_tri < 0 || prune->n_tri > 0x7fffffff))
        return QF_ERR_INVALID_ARGUMENT;
    // The whole job is checked BEFORE the first launch: the entry points below repeat these tests, but by the
    // time qf_field_forward or qf_composite_tiles would refuse, four kernels have run, the handle's cull parity has
    // flipped and the pinned block has been written -- a C caller would get INVALID_ARGUMENT for a half-executed frame.
    if (j.field) {
        const qf_field_desc &f = *j.field;
        if (!j.rgb_c || !j.sigma_c || !j.table || !j.base_w) return QF_ERR_INVALID_ARGUMENT;
        // the frame composites colours: the head must produce them (qf_field_forward's own rules per head)
        if (f.head == QF_HEAD_NGP) {
            if (!j.head_ngp_w) return QF_ERR_INVALID_ARGUMENT;
        } else if (f.head == QF_HEAD_SG) {
            // six pointers in every precision (qf_sg_head / qf_sg_head_bf16 / qf_sg_head_f16): all must be set
            if (!j.head_sg) return QF_ERR_INVALID_ARGUMENT;
            if (j.field_precision == QF_FIELD_FP32) {
                const qf_sg_head *s = static_cast<const qf_sg_head *>(j.head_sg);
                if (!s->w1 || !s->b1 || !s->w2 || !s->b2 || !s->wout || !s->bout) return QF_ERR_INVALID_ARGUMENT;
            } else {
                const qf_sg_head_bf16 *s = static_cast<const qf_sg_head_bf16 *>(j.head_sg);
                if (!s->w1 || !s->b1 || !s->w2 || !s->b2 || !s->wout || !s->bout) return QF_ERR_INVALID_ARGUMENT;
            }
            if (f.n_lobes < 1 || f.n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
        } else {
            return QF_ERR_INVALID_ARGUMENT;       // QF_HEAD_NONE / QF_HEAD_SG_FEATURES give the compositor no rgb
        }
        for (int k = 0; k < 3; ++k)
            if (!(f.aabb[3 + k] > f.aabb[k])) return QF_ERR_INVALID_ARGUMENT;
        // ... and the compositor's (qf_composite_tiles): an image to write, a known background, its colour when custom
        if (image) {
            if (j.bg_mode < 0 || j.bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
            if (!j.out_packed && (!j.out_rgb || !j.out_alpha || !j.out_depth)) return QF_ERR_INVALID_ARGUMENT;
            if (j.bg_mode == QF_BG_CUSTOM && !j.bkgd) return QF_ERR_INVALID_ARGUMENT;
        }
    }
    const int64_t cap = j.n_rays * (int64_t)j.max_hits;
    int32_t *overflow = j.hit_count + j.n_rays;
    const int32_t cull = j.cull_chunks & 1;
    // The hit-bin route (qf_raster_intersect_tiles): the bins live in rgb_c and the tile masks and cursors in sigma_c until
    // the pack has read them; the field writes both only afterwards.
    const int64_t n_tiles = (int64_t)((w + 7) / 8) * ((h + 7) / 8);
    const int64_t bins_bytes = qf_hit_bins_bytes(w, h, j.max_hits);
    const bool use_bins = j.field && !cull && !(j.cull_chunks & QF_FRAME_PER_RAY_LISTS) && j.max_hits <= 32 &&
                          qf_bvh_num_triangles(bvh) < (1 << 26) && bins_bytes >= 0 &&
                          bins_bytes <= cap * 3 * (int64_t)sizeof(float) && n_tiles * 12 <= cap * (int64_t)sizeof(float) &&
                          reinterpret_cast<uintptr_t>(j.rgb_c) % 8 == 0 && reinterpret_cast<uintptr_t>(j.sigma_c) % 8 == 0;
    if (use_bins) {
        uint64_t *tile_mask = reinterpret_cast<uint64_t *>(j.sigma_c);
        int32_t *tile_cursor = reinterpret_cast<int32_t *>(tile_mask + n_tiles);
        int rc = qf_raster_intersect_tiles(bvh, j.camera, j.rays_o, j.rays_d, j.n_rays, j.max_hits, tile_cursor, tile_mask,
                                           j.rgb_c, bins_bytes, j.hit_count, overflow, overflow + 1, stream);
        if (rc != QF_OK) return rc;
        rc = qf_bvh_repair_overflow(bvh, j.rays_o, j.rays_d, j.n_rays, j.max_hits, w, j.hit_tri, j.hit_t, j.hit_count, nullptr,
                                    nullptr, overflow + 1, stream);
        if (rc != QF_OK) return rc;
        rc = qf_tile_offsets(j.hit_count, j.max_hits, w, h, j.tile_base, j.total, overflow, overflow + 1, j.host_block,
                             j.dropped, stream);
        if (rc != QF_OK) return rc;
        rc = qf_pack_tiles_bins(j.rays_o, j.rays_d, w, h, j.max_hits, j.hit_tri, j.hit_t, j.hit_count, j.tile_base, j.total,
                                j.xyz_c, j.dirs_c, j.depth_c, j.tri_c, j.min_separation, j.final_count, j.dropped, nullptr, 1,
                                tile_cursor, tile_mask, j.rgb_c, overflow + 1, stream);
        if (rc != QF_OK) return rc;
    } else {
        // 1. camera-coherent intersection (lists in arrival order), 2. exact K nearest for the pixels that overflowed
        int rc = qf_raster_intersect(bvh, j.camera, j.rays_o, j.rays_d, j.n_rays, j.max_hits, j.hit_tri, j.hit_t, j.hit_count,
                                     overflow, j.tri_c ? 0 : 2 /* no ids wanted: the pass skips their stores */, cull,
                                     overflow + 1, stream);
        if (rc != QF_OK) return rc;
        // (... and for EVERY pixel when the pass's ray check found that the rays are not this camera's pixel grid: the pass
        // wrote nothing then, and this launch is the intersection)
        rc = qf_bvh_repair_overflow(bvh, j.rays_o, j.rays_d, j.n_rays, j.max_hits, w, j.hit_tri, j.hit_t, j.hit_count, nullptr,
                                    nullptr, overflow + 1, stream);
        if (rc != QF_OK) return rc;
        // 3. tile bases + slot total (device; a copy on its way to the pinned block), 4. the tile pack with the re-origin rule
        rc = qf_tile_offsets(j.hit_count, j.max_hits, w, h, j.tile_base, j.total, overflow, overflow + 1, j.host_block, j.dropped,
                             stream);
        if (rc != QF_OK) return rc;
        rc = qf_pack_tiles(j.rays_o, j.rays_d, w, h, j.max_hits, j.hit_tri, j.hit_t, j.hit_count, j.tile_base, j.total, j.xyz_c,
                           j.dirs_c, j.depth_c, j.tri_c, nullptr, nullptr, j.min_separation, j.final_count, j.dropped, nullptr, 1,
                           stream);
        if (rc != QF_OK) return rc;
    }
    if (!j.field || samples_only) return QF_OK; // sampling only
    // 5. the field over min(*total, cap) points, in the job's precision, 6. the tile compositor
    int rc = field_launch(j, cap, j.total, nullptr, stream);
    if (rc != QF_OK) return rc;
    if (prune)
        return qf_composite_tiles_trimax(j.rgb_c, j.sigma_c, j.depth_c, j.delta_const, j.final_count, j.max_hits, j.tile_base, w,
                                         h, j.bg_mode, j.bkgd, j.out_rgb, j.out_alpha, j.out_depth, j.out_packed, j.tri_c,
                                         prune->tri_weight, prune->n_tri, prune->valid_threshold, prune->counts,
                                         prune->bad_ids, stream);
    return qf_composite_tiles(j.rgb_c, j.sigma_c, j.depth_c, j.delta_const, j.final_count, j.max_hits, j.tile_base, w, h,
                              j.bg_mode, j.bkgd, j.out_rgb, j.out_alpha, j.out_depth, nullptr, j.out_packed, stream);
}

}  // namespace

extern "C" int qf_frame_render(qf_bvh *bvh, const qf_frame_job *job, void *stream)
{
    return frame_sequence(bvh, job, nullptr, stream);
}

extern "C" int qf_frame_prune(qf_bvh *bvh, const qf_frame_job *job, float *tri_weight, int64_t n_tri, float valid_threshold,
                              int64_t *counts, int32_t *bad_ids, void *stream)
{
    const PruneTarget prune = {tri_weight, n_tri, valid_threshold, counts, bad_ids};
    return frame_sequence(bvh, job, &prune, stream);
}

extern "C" int qf_frame_render_baked(qf_bvh *bvh, const qf_frame_job *job, const qf_baked_shading *baked, float stop_tau,
                                     int32_t *shaded_count, void *stream)
{
    if (!bvh || !job || !job->camera || !baked) return QF_ERR_INVALID_ARGUMENT;
    const qf_frame_job &j = *job;
    // The whole job is checked before the first launch, as in frame_sequence (which checks the sampling half): no field
    // -- the colours come from the texture set --, the samples' triangle ids, then what qf_texture_composite_tiles tests.
    if (j.field || !j.tri_c) return QF_ERR_INVALID_ARGUMENT;
    if (!baked->records || !baked->triangle_records || baked->texture_size < 1) return QF_ERR_INVALID_ARGUMENT;
    if (baked->n_lobes < 1 || baked->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (j.bg_mode < 0 || j.bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!j.out_packed && (!j.out_rgb || !j.out_alpha || !j.out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (j.bg_mode == QF_BG_CUSTOM && !j.bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    int rc = frame_sequence(bvh, job, nullptr, stream);                      // intersection ... tile pack (per-ray lists)
    if (rc != QF_OK) return rc;
    return qf_texture_composite_tiles(baked->records, baked->texture_size, baked->n_lobes, baked->sigmoid_codec,
                                      baked->lambda_thres, baked->triangle_records, j.xyz_c, j.dirs_c, j.depth_c, j.tri_c,
                                      j.final_count, j.max_hits, j.tile_base, j.camera->width, j.camera->height, j.delta_const,
                                      j.bg_mode, j.bkgd, stop_tau, j.out_rgb, j.out_alpha, j.out_depth, j.out_packed,
                                      shaded_count, stream);
}

extern "C" int qf_frame_render_vertex_baked(qf_bvh *bvh, const qf_frame_job *job, const qf_vertex_baked_shading *shading,
                                            float stop_tau, int32_t *shaded_count, void *stream)
{
    if (!bvh || !job || !job->camera || !shading) return QF_ERR_INVALID_ARGUMENT;
    const qf_frame_job &j = *job;
    // The whole job is checked before the first launch, as in qf_frame_render_baked: no field -- the colours come from
    // the vertex table --, the samples' triangle ids, then what qf_vertex_composite_tiles tests.
    if (j.field || !j.tri_c) return QF_ERR_INVALID_ARGUMENT;
    if (!shading->table || reinterpret_cast<uintptr_t>(shading->table) % 16 != 0 || !shading->records ||
        shading->n_vertices < 1)
        return QF_ERR_INVALID_ARGUMENT;
    if (shading->n_lobes < 1 || shading->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (shading->stride != vertex_row_stride(shading->n_lobes)) return QF_ERR_INVALID_ARGUMENT;
    if (j.bg_mode < 0 || j.bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!j.out_packed && (!j.out_rgb || !j.out_alpha || !j.out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (j.bg_mode == QF_BG_CUSTOM && !j.bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    int rc = frame_sequence(bvh, job, nullptr, stream);                      // intersection ... tile pack (per-ray lists)
    if (rc != QF_OK) return rc;
    return qf_vertex_composite_tiles(shading->table, shading->stride, shading->n_lobes, shading->records, j.xyz_c, j.dirs_c,
                                     j.depth_c, j.tri_c, j.final_count, j.max_hits, j.tile_base, j.camera->width,
                                     j.camera->height, j.delta_const, j.bg_mode, j.bkgd, stop_tau, j.out_rgb, j.out_alpha,
                                     j.out_depth, j.out_packed, shaded_count, stream);
}

extern "C" int qf_frame_render_vertex_quant(qf_bvh *bvh, const qf_frame_job *job, const qf_vertex_quant_shading *shading,
                                            float stop_tau, int32_t *shaded_count, void *stream)
{
    if (!bvh || !job || !job->camera || !shading) return QF_ERR_INVALID_ARGUMENT;
    const qf_frame_job &j = *job;
    // The whole job is checked before the first launch, as in qf_frame_render_vertex_baked: no field -- the colours come
    // from the vertex records --, the samples' triangle ids, then what qf_vertex_quant_composite_tiles tests.
    if (j.field || !j.tri_c) return QF_ERR_INVALID_ARGUMENT;
    if (!shading->records || reinterpret_cast<uintptr_t>(shading->records) % 16 != 0 || !shading->tri_records ||
        shading->n_vertices < 1 || shading->n_vertices > 0x7fffffff)
        return QF_ERR_INVALID_ARGUMENT;
    if (shading->n_lobes < 1 || shading->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (j.bg_mode < 0 || j.bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!j.out_packed && (!j.out_rgb || !j.out_alpha || !j.out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (j.bg_mode == QF_BG_CUSTOM && !j.bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    int rc = frame_sequence(bvh, job, nullptr, stream);                      // intersection ... tile pack (per-ray lists)
    if (rc != QF_OK) return rc;
    return qf_vertex_quant_composite_tiles(shading->records, shading->n_vertices, shading->n_lobes, shading->sigmoid_codec,
                                           shading->lambda_thres, shading->tri_records, j.xyz_c, j.dirs_c, j.depth_c, j.tri_c,
                                           j.final_count, j.max_hits, j.tile_base, j.camera->width, j.camera->height,
                                           j.delta_const, j.bg_mode, j.bkgd, stop_tau, j.out_rgb, j.out_alpha, j.out_depth,
                                           j.out_packed, shaded_count, stream);
}

extern "C" int qf_frame_render_front(qf_bvh *bvh, const qf_frame_job *job, float stop_tau, const int32_t *rank_windows,
                                     int32_t n_windows, const qf_front_scratch *scratch, int32_t *shaded_count,
                                     int32_t *evaluated_count, void *stream)
{
    if (!bvh || !job || !job->camera || !scratch) return QF_ERR_INVALID_ARGUMENT;
    const qf_frame_job &j = *job;
    // The whole job, the schedule and stop_tau are checked before the first launch: what frame_sequence does not test
    // itself -- a field and an image are required here -- then the schedule, then the scratch.
    if (!j.field || j.max_hits < 1) return QF_ERR_INVALID_ARGUMENT;
    if ((int64_t)((job->camera->width + 7) / 8) * ((job->camera->height + 7) / 8) > QF_FRONT_MAX_TILES)
        return QF_ERR_INVALID_ARGUMENT;
    if (!j.out_packed && (!j.out_rgb || !j.out_alpha || !j.out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    if (!rank_windows || n_windows < 1 || n_windows > QF_FRONT_MAX_WINDOWS) return QF_ERR_INVALID_ARGUMENT;
    for (int i = 0; i < n_windows; ++i)
        if (rank_windows[i] <= (i ? rank_windows[i - 1] : 0)) return QF_ERR_INVALID_ARGUMENT;
    if (rank_windows[n_windows - 1] < j.max_hits) return QF_ERR_INVALID_ARGUMENT;
    if (!scratch->state || reinterpret_cast<uintptr_t>(scratch->state) % 16 != 0 || !scratch->win_count || !scratch->win_total ||
        !scratch->win_order)
        return QF_ERR_INVALID_ARGUMENT;
    int rc = frame_sequence(bvh, job, nullptr, stream, true);                // intersection ... tile pack, either route
    if (rc != QF_OK) return rc;
    const int32_t w = j.camera->width, h = j.camera->height;
    const int64_t cap = j.n_rays * (int64_t)j.max_hits;
    int32_t lo = 0, mid = 0;
    for (int i = 0; i < n_windows; ++i) {
        const int32_t hi = rank_windows[i];
        rc = qf_front_select(j.rgb_c, j.sigma_c, j.depth_c, j.delta_const, j.final_count, j.max_hits, j.tile_base, w, h, stop_tau,
                             lo, mid, hi, scratch->state, scratch->win_count, scratch->win_total, scratch->win_order, cap,
                             stream);
        if (rc != QF_OK) return rc;
        rc = field_launch(j, cap, scratch->win_total, scratch->win_order, stream);
        if (rc != QF_OK) return rc;
        lo = mid;
        mid = hi;
    }
    return qf_front_finish(j.rgb_c, j.sigma_c, j.depth_c, j.delta_const, j.final_count, j.max_hits, j.tile_base, w, h, stop_tau,
                           lo, mid, scratch->state, j.bg_mode, j.bkgd, j.out_rgb, j.out_alpha, j.out_depth, j.out_packed,
                           shaded_count, evaluated_count, stream);
}
