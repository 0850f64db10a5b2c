// The vertex-baked renderer (include/qf_vertex_baked.h): SG features kept at the mesh vertices,
// every quadrature point shaded from the barycentric blend of its triangle's three vertex rows -- the reference's
// render_image_finetune_baking_with_occgrid (utils.py:822-840) with the field evaluated once per vertex instead of three
// times per sample.  Three kernels: the per-face records, the point shader, and the tile compositor that shades inside
// its front-to-back walk with early ray termination (baked_frame.hip's walk and rule).  The arithmetic is
// vertex_baked_device.h's in all of them.
#include "qf_common.h"
#include "composite_device.h"
#include "vertex_baked_device.h"

#pragma clang fp contract(off)

namespace {

__global__ void vertex_records_kernel(const double *__restrict__ vertices, int64_t n_vertices, const int64_t *__restrict__ faces,
                                      int64_t n_faces, VertexTriRecord *__restrict__ records)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * blockDim.x) {
        int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
        if (ia < 0 || ia >= n_vertices || ib < 0 || ib >= n_vertices || ic < 0 || ic >= n_vertices)
            ia = ib = ic = 0;                      // both edges zero: 1 / det = 1 / 0, the face shades NaN
        VertexTriRecord r;
        triangle_record_geometry(vertices, ia, ib, ic, r);
        r.v[0] = (int32_t)ia; r.v[1] = (int32_t)ib; r.v[2] = (int32_t)ic;
        r.zero[0] = r.zero[1] = r.zero[2] = 0;
        records[f] = r;
    }
}

// One thread per sample: triangle record -> barycentrics -> blend (three rows, piece by piece) -> the outputs asked for.
// TriT: int64_t (the reference's index_tri) or int32_t (the tile pack's ids).
template <typename TriT>
__global__ __launch_bounds__(256) void vertex_shade_points_kernel(
    const float *__restrict__ table, int stride, int n_lobes, const VertexTriRecord *__restrict__ records,
    const float *__restrict__ points, const TriT *__restrict__ index_tri, const float *__restrict__ dirs, int64_t n,
    const int64_t *__restrict__ n_dev, float *__restrict__ features_out, float *__restrict__ rgb, float *__restrict__ sigma)
{
    if (n_dev) { const int64_t nd = *n_dev; n = nd < n ? (nd > 0 ? nd : 0) : n; }    // device-side count (render-only frame)
    const int n16 = vertex_row_pieces(n_lobes), width = vertex_row_width(n_lobes);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const VertexTriRecord tr = records[index_tri[i]];
        float b[3];
        vertex_barycentrics(tr, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], b);
        float blend[kVertexRowMax];
        vertex_blend(table, stride, n16, tr.v[0], tr.v[1], tr.v[2], b, blend);
        if (features_out) {
            float *o = features_out + i * width;
#pragma unroll
            for (int c = 0; c < kVertexRowMax; ++c)
                if (c < width) o[c] = blend[c];    // wave-uniform
        }
        if (rgb) {
            float c[3];
            vertex_blend_shade(blend, n_lobes, dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2], c);
            rgb[i * 3] = c[0]; rgb[i * 3 + 1] = c[1]; rgb[i * 3 + 2] = c[2];
            sigma[i] = vertex_blend_sigma(blend, n_lobes);
        }
    }
}

constexpr int kTileWaves = 4;         // tiles in flight per workgroup (no barrier: the waves run on their own)

// texture_composite_tiles_kernel's walk and rule (baked_frame.hip) with the vertex-baked shading.  A step is the chain
// slot (triangle id, position, depth: contiguous runs) -> triangle record (a 128-byte gather) -> three vertex rows
// (3 * n16 16-byte gathers) -> the arithmetic.  The first two links are software-pipelined: iteration k asks for the slot
// of rank k+2 and the triangle record of rank k+1 and then shades rank k.  The vertex rows are NOT fetched ahead: a rank
// of rows in flight would be 3 * 12 more 16-byte pieces (144 registers) per lane at 6 lobes, and the rows of a sample
// that fails the rule are never read.  The record of rank k is consumed (barycentrics and vertex ids: 6 registers) before the record of rank
// k+1 is asked for into the same registers.  Everything ahead of rank k is speculative, fetched for lanes that have not
// stopped at the time of the request; every speculative address comes from a valid slot (count > rank).
// The view direction is the same for all of a pixel's samples (the tile pack writes one normalised vector per lane to
// every slot of that lane): it is read once, at rank 0.
__global__ __launch_bounds__(64 * kTileWaves) void vertex_composite_tiles_kernel(
    const float *__restrict__ table, int stride, int n_lobes, const VertexTriRecord *__restrict__ tri_records,
    const float *__restrict__ xyz_c, const float *__restrict__ dirs_c, const float *__restrict__ depth_c,
    const int32_t *__restrict__ tri_c, const int32_t *__restrict__ hit_count, int max_hits,
    const int64_t *__restrict__ tile_base, int w, int h, int tiles_x, int n_tiles, float delta_const, int bg_mode,
    const float *__restrict__ bkgd, float stop_tau, float *__restrict__ out_rgb, float *__restrict__ out_alpha,
    float *__restrict__ out_depth, float *__restrict__ out_packed, int32_t *__restrict__ shaded_count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n16 = vertex_row_pieces(n_lobes);
    const bool never = stop_tau == INFINITY;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int tile = blockIdx.x * kTileWaves + wave; tile < n_tiles; tile += gridDim.x * kTileWaves) {   // wave-uniform
        int64_t ray = 0;
        int cnt = 0;
        const int inside = qf_tile_lane_ray(tile, lane, w, h, tiles_x, 0, &ray);
        if (inside) cnt = hit_count[ray] < max_hits ? hit_count[ray] : max_hits;
        RayAccum acc;
        int n_shaded = 0;
        const unsigned long long mask0 = __ballot(cnt > 0);
        if (mask0 != 0ull) {                           // wave-uniform
            int64_t base = tile_base[tile];            // first slot of the rank the slot stage asks for next
            bool alive = true;                         // no sample of this pixel has failed the rule yet
            // the slot of rank 0 and the view direction
            int tri_a = 0;
            float xa = 0.0f, ya = 0.0f, za = 0.0f, dep_a = 0.0f;          // slot stage: rank k+1 at the top of iteration k
            float dx = 0.0f, dy = 0.0f, dz = 0.0f;
            if (cnt > 0) {
                const int64_t pos = base + __popcll(mask0 & below);
                tri_a = tri_c[pos];
                xa = xyz_c[pos * 3]; ya = xyz_c[pos * 3 + 1]; za = xyz_c[pos * 3 + 2];
                dep_a = depth_c[pos];
                dx = dirs_c[pos * 3]; dy = dirs_c[pos * 3 + 1]; dz = dirs_c[pos * 3 + 2];
            }
            base += __popcll(mask0);
            float x0 = 0.0f, y0 = 0.0f, z0 = 0.0f, dep0 = 0.0f;           // position / depth of rank k
            VertexTriRecord tr = {};                                       // triangle record of rank k, then of rank k+1
            for (int k = -1;; ++k) {
                // anyone left to shade at rank k or behind it?  (wave-uniform exit: a tile whose pixels have all stopped
                // or run out leaves at once)
                if (k >= 0 && __ballot(cnt > k && alive) == 0ull) break;
                // 1. rank k: the rule; its record is here -> barycentrics and vertex ids
                bool shade = false;
                float b[3] = {0.0f, 0.0f, 0.0f};
                int v0 = 0, v1 = 0, v2 = 0;
                if (k >= 0 && cnt > k && alive) {
                    if (never || acc.cum <= stop_tau) {
                        shade = true;
                        vertex_barycentrics(tr, x0, y0, z0, b);
                        v0 = tr.v[0]; v1 = tr.v[1]; v2 = tr.v[2];
                    } else {
                        alive = false;
                    }
                }
                // 2. rank k+1: ask for its triangle record (the id arrived with the slot)
                if (cnt > k + 1 && alive) tr = tri_records[tri_a];
                // 3. rank k+2: ask for its slot
                const unsigned long long next = __ballot(cnt > k + 2);
                int tri_n = 0;
                float xn = 0.0f, yn = 0.0f, zn = 0.0f, dep_n = 0.0f;
                if (cnt > k + 2 && alive) {
                    const int64_t pos = base + __popcll(next & below);
                    tri_n = tri_c[pos];
                    xn = xyz_c[pos * 3]; yn = xyz_c[pos * 3 + 1]; zn = xyz_c[pos * 3 + 2];
                    dep_n = depth_c[pos];
                }
                base += __popcll(next);
                // 4. rank k: the rows, the blend, shade and composite
                if (shade) {
                    float blend[kVertexRowMax];
                    vertex_blend(table, stride, n16, v0, v1, v2, b, blend);
                    float c[3];
                    vertex_blend_shade(blend, n_lobes, dx, dy, dz, c);
                    const float tau = sample_tau(vertex_blend_sigma(blend, n_lobes), delta_const);
                    composite_step(acc, tau, sample_alpha(tau), c[0], c[1], c[2], dep0);
                    ++n_shaded;
                }
                // every stage moves up one rank
                x0 = xa; y0 = ya; z0 = za; dep0 = dep_a;
                tri_a = tri_n; xa = xn; ya = yn; za = zn; dep_a = dep_n;
            }
        }
        if (!inside) continue;
        float px[3];
        if (cnt > 0) {
            composite_blend(acc, bg_mode, bkgd, px);
        } else {                                       // fill_background_kernel's values
            px[0] = px[1] = px[2] = (bg_mode == QF_BG_BLACK || bg_mode == QF_BG_NONE) ? 0.0f : 1.0f;
        }
        if (shaded_count) shaded_count[ray] = n_shaded;
        if (out_packed) {              // [n, 5] = rgb | alpha | depth per pixel, as composite_tiles_kernel
            float *o = out_packed + ray * 5;
            o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; o[3] = acc.ca; o[4] = acc.cd;
            continue;
        }
        out_rgb[ray * 3 + 0] = px[0];
        out_rgb[ray * 3 + 1] = px[1];
        out_rgb[ray * 3 + 2] = px[2];
        out_alpha[ray] = acc.ca;
        out_depth[ray] = acc.cd;
    }
}

// table, stride and n_lobes as every entry point takes them
int check_table(const float *table, int32_t stride, int32_t n_lobes)
{
    if (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (stride != vertex_row_stride(n_lobes)) return QF_ERR_INVALID_ARGUMENT;
    return QF_OK;
}

}  // namespace

extern "C" int qf_vertex_records_pack(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                      void *records, void *stream)
{
    if (n_faces < 0 || n_vertices < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_faces == 0) return QF_OK;
    if (!vertices || !faces || !records || n_vertices < 1 || n_vertices > 0x7fffffff) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(vertex_records_kernel, n_faces, vertices, n_vertices, faces, n_faces,
                     static_cast<VertexTriRecord *>(records));
    return QF_OK;
}

extern "C" int qf_vertex_shade_points(const float *table, int32_t stride, int32_t n_lobes, const void *records,
                                      const float *points, const int64_t *index_tri, const int32_t *index_tri32,
                                      const float *dirs, int64_t n, const int64_t *n_device, float *features_out, float *rgb,
                                      float *sigma, void *stream)
{
    const int rc = check_table(table, stride, n_lobes);
    if (rc != QF_OK) return rc;
    if (!records || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if ((!rgb != !sigma) || (!rgb && !features_out) || (rgb && !dirs)) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!points || (!index_tri == !index_tri32)) return QF_ERR_INVALID_ARGUMENT;   // exactly one id array
    const VertexTriRecord *tr = static_cast<const VertexTriRecord *>(records);
    if (index_tri32) {
        QF_SIMPLE_LAUNCH(vertex_shade_points_kernel<int32_t>, n, table, (int)stride, (int)n_lobes, tr, points, index_tri32, dirs,
                         n, n_device, features_out, rgb, sigma);
    } else {
        QF_SIMPLE_LAUNCH(vertex_shade_points_kernel<int64_t>, n, table, (int)stride, (int)n_lobes, tr, points, index_tri, dirs,
                         n, n_device, features_out, rgb, sigma);
    }
    return QF_OK;
}

extern "C" int qf_vertex_composite_tiles(const float *table, int32_t stride, int32_t n_lobes, const void *records,
                                         const float *xyz_c, const float *dirs_c, const float *depth_c, const int32_t *tri_c,
                                         const int32_t *hit_count, int32_t max_hits, const int64_t *tile_base, int32_t width,
                                         int32_t height, float delta_const, int32_t bg_mode, const float *bkgd, float stop_tau,
                                         float *out_rgb, float *out_alpha, float *out_depth, float *out_packed,
                                         int32_t *shaded_count, void *stream)
{
    const int rc = check_table(table, stride, n_lobes);
    if (rc != QF_OK) return rc;
    if (!records) return QF_ERR_INVALID_ARGUMENT;
    if (width < 1 || height < 1 || max_hits < 1 || bg_mode < 0 || bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!xyz_c || !dirs_c || !depth_c || !tri_c || !hit_count || !tile_base) return QF_ERR_INVALID_ARGUMENT;
    if (!out_packed && (!out_rgb || !out_alpha || !out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (bg_mode == QF_BG_CUSTOM && !bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const int64_t n_tiles = (int64_t)tiles_x * tiles_y;
    if (n_tiles > (1 << 30)) return QF_ERR_INVALID_ARGUMENT;                   // the kernel's tile loop counts in int
    hipLaunchKernelGGL(vertex_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves)), dim3(64 * kTileWaves), 0,
                       qf_stream(stream), table, (int)stride, (int)n_lobes, static_cast<const VertexTriRecord *>(records), xyz_c,
                       dirs_c, depth_c, tri_c, hit_count, (int)max_hits, tile_base, (int)width, (int)height, tiles_x,
                       (int)n_tiles, delta_const, (int)bg_mode, bkgd, stop_tau, out_rgb, out_alpha, out_depth, out_packed,
                       shaded_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
