// The vertex-baked renderer (include/qf_vertex_baked.h): SG features kept at the mesh vertices,
// every quadrature point shaded from the barycentric blend of its triangle's three vertex rows -- the reference's
// render_image_finetune_baking_with_occgrid (utils.py:822-840) with the field evaluated once per vertex instead of three
// times per sample.  Three kernels: the per-face records, the point shader, and the tile compositor that shades inside
// its front-to-back walk with early ray termination (baked_frame.hip's walk and rule).  The arithmetic is
// vertex_baked_device.h's in all of them.
#include "qf_common.h"
#include "vertex_tiles_device.h"

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

constexpr int kTileWaves = kVertexTileWaves;     // no barrier: the waves run on their own

// The rows of the fp32 table for vertex_tiles_walk.
struct VertexTableRows {
    const float *__restrict__ table;
    int stride, n16;
    __device__ __forceinline__ void operator()(int v0, int v1, int v2, const float b[3], float (&blend)[kVertexRowMax]) const
    {
        vertex_blend(table, stride, n16, v0, v1, v2, b, blend);
    }
};

// The walk, pipeline and rule: vertex_tiles_walk (vertex_tiles_device.h), shared with vertex_quant.hip.
__global__ __launch_bounds__(64 * kTileWaves) void vertex_composite_tiles_kernel(
    const float *__restrict__ table, int stride, int n_lobes, const VertexTriRecord *__restrict__ tri_records,
    const float *__restrict__ xyz_c, const float *__restrict__ dirs_c, const float *__restrict__ depth_c,
    const int32_t *__restrict__ tri_c, const int32_t *__restrict__ hit_count, int max_hits,
    const int64_t *__restrict__ tile_base, int w, int h, int tiles_x, int n_tiles, float delta_const, int bg_mode,
    const float *__restrict__ bkgd, float stop_tau, float *__restrict__ out_rgb, float *__restrict__ out_alpha,
    float *__restrict__ out_depth, float *__restrict__ out_packed, int32_t *__restrict__ shaded_count)
{
    const VertexTableRows rows = {table, stride, vertex_row_pieces(n_lobes)};
    vertex_tiles_walk(rows, n_lobes, tri_records, xyz_c, dirs_c, depth_c, tri_c, hit_count, max_hits, tile_base, w, h, tiles_x,
                      n_tiles, delta_const, bg_mode, bkgd, stop_tau, out_rgb, out_alpha, out_depth, out_packed, shaded_count);
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
