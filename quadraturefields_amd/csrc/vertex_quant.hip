// The quantised vertex-baked renderer (include/qf_vertex_quant.h): the vertex table of
// vertex_baked.hip kept as one 64-byte uint8 texel record per vertex.  Three kernels: the decode to the fp32 table, the
// point shader, and the tile compositor (vertex_baked.hip's walk and rule).  Each fills the 7 KiB dequantiser tables in
// LDS once per workgroup and decodes by lookup; the arithmetic is vertex_quant_device.h's in all of them: decode first,
// then blend, so every output equals the fp32 kernels' on the decoded table bit for bit.
#include "qf_common.h"
#include "vertex_quant_device.h"
#include "vertex_tiles_device.h"

#pragma clang fp contract(off)

namespace {

// One thread per vertex: the record -> its row of the fp32 table, pad columns included (zero).
__global__ __launch_bounds__(256) void vertex_quant_decode_kernel(const uint8_t *__restrict__ records, int64_t n_vertices,
                                                                  int n_lobes, int sigmoid_codec, float lambda_thres,
                                                                  float *__restrict__ table, int stride)
{
    __shared__ DequantTables s_tab;
    dequant_tables_fill(s_tab, threadIdx.x, sigmoid_codec, lambda_thres);
    __syncthreads();
    const int n16 = texel_record_pieces(n_lobes);
    for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < n_vertices; v += (int64_t)gridDim.x * blockDim.x) {
        uint32_t w[kTexelRecord / 4];
        texel_record_load(records, v, n16, w);
        float row[kVertexRowMax];
        vertex_quant_decode_row(s_tab, w, n_lobes, row);
        float *o = table + v * stride;
#pragma unroll
        for (int c = 0; c < kVertexRowMax; ++c)
            if (c < stride) o[c] = row[c];         // wave-uniform
    }
}

// vertex_shade_points_kernel (vertex_baked.hip) with the blend read from three records.
template <typename TriT>
__global__ __launch_bounds__(256) void vertex_quant_shade_points_kernel(
    const uint8_t *__restrict__ records, int n_lobes, int sigmoid_codec, float lambda_thres,
    const VertexTriRecord *__restrict__ tri_records, const float *__restrict__ points, const TriT *__restrict__ index_tri,
    const float *__restrict__ dirs, int64_t n, const int64_t *__restrict__ n_dev, float *__restrict__ features_out,
    float *__restrict__ rgb, float *__restrict__ sigma)
{
    if (n_dev) { const int64_t nd = *n_dev; n = nd < n ? (nd > 0 ? nd : 0) : n; }    // device-side count (render-only frame)
    __shared__ DequantTables s_tab;
    dequant_tables_fill(s_tab, threadIdx.x, sigmoid_codec, lambda_thres);
    __syncthreads();
    const int n16 = texel_record_pieces(n_lobes), width = vertex_row_width(n_lobes);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const VertexTriRecord tr = tri_records[index_tri[i]];
        float b[3];
        vertex_barycentrics(tr, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], b);
        float blend[kVertexRowMax];
        vertex_quant_blend(s_tab, records, n16, n_lobes, tr.v[0], tr.v[1], tr.v[2], b, blend);
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

constexpr int kTileWaves = kVertexTileWaves;     // 256 threads, one per entry of the code tables

// The decoded rows of three 64-byte records for vertex_tiles_walk.
struct VertexQuantRows {
    const DequantTables &tab;
    const uint8_t *__restrict__ records;
    int n16, n_lobes;
    __device__ __forceinline__ void operator()(int v0, int v1, int v2, const float b[3], float (&blend)[kVertexRowMax]) const
    {
        vertex_quant_blend(tab, records, n16, n_lobes, v0, v1, v2, b, blend);
    }
};

// vertex_composite_tiles_kernel with the rows read from three 64-byte records: the table fill and its barrier come before
// the tile loop (texture_composite_tiles_kernel's place for them), then the ONE walk of vertex_tiles_device.h.  As for the
// fp32 table, the vertex records are NOT fetched a rank ahead; the pixels do not depend on that choice.
__global__ __launch_bounds__(64 * kTileWaves) void vertex_quant_composite_tiles_kernel(
    const uint8_t *__restrict__ records, int n_lobes, int sigmoid_codec, float lambda_thres,
    const VertexTriRecord *__restrict__ tri_records, const float *__restrict__ xyz_c, const float *__restrict__ dirs_c,
    const float *__restrict__ depth_c, const int32_t *__restrict__ tri_c, const int32_t *__restrict__ hit_count, int max_hits,
    const int64_t *__restrict__ tile_base, int w, int h, int tiles_x, int n_tiles, float delta_const, int bg_mode,
    const float *__restrict__ bkgd, float stop_tau, float *__restrict__ out_rgb, float *__restrict__ out_alpha,
    float *__restrict__ out_depth, float *__restrict__ out_packed, int32_t *__restrict__ shaded_count)
{
    __shared__ DequantTables s_tab;
    dequant_tables_fill(s_tab, threadIdx.x, sigmoid_codec, lambda_thres);
    __syncthreads();
    const VertexQuantRows rows = {s_tab, records, texel_record_pieces(n_lobes), n_lobes};
    vertex_tiles_walk(rows, n_lobes, tri_records, xyz_c, dirs_c, depth_c, tri_c, hit_count, max_hits, tile_base, w, h, tiles_x,
                      n_tiles, delta_const, bg_mode, bkgd, stop_tau, out_rgb, out_alpha, out_depth, out_packed, shaded_count);
}

// records, n_vertices and n_lobes as every entry point takes them
int check_records(const uint8_t *records, int64_t n_vertices, int32_t n_lobes)
{
    if (!records || reinterpret_cast<uintptr_t>(records) % 16 != 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_vertices < 1 || n_vertices > 0x7fffffff) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    return QF_OK;
}

}  // namespace

extern "C" int qf_vertex_quant_decode(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                                      float lambda_thres, float *table_out, int32_t stride, void *stream)
{
    const int rc = check_records(records, n_vertices, n_lobes);
    if (rc != QF_OK) return rc;
    if (!table_out || (stride != vertex_row_stride(n_lobes) && stride != vertex_row_width(n_lobes))) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(vertex_quant_decode_kernel, n_vertices, records, n_vertices, (int)n_lobes, (int)sigmoid_codec, lambda_thres,
                     table_out, (int)stride);
    return QF_OK;
}

extern "C" int qf_vertex_quant_shade_points(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                                            float lambda_thres, const void *tri_records, const float *points,
                                            const int64_t *index_tri, const int32_t *index_tri32, const float *dirs, int64_t n,
                                            const int64_t *n_device, float *features_out, float *rgb, float *sigma, void *stream)
{
    const int rc = check_records(records, n_vertices, n_lobes);
    if (rc != QF_OK) return rc;
    if (!tri_records || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if ((!rgb != !sigma) || (!rgb && !features_out) || (rgb && !dirs)) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!points || (!index_tri == !index_tri32)) return QF_ERR_INVALID_ARGUMENT;   // exactly one id array
    const VertexTriRecord *tr = static_cast<const VertexTriRecord *>(tri_records);
    if (index_tri32) {
        QF_SIMPLE_LAUNCH(vertex_quant_shade_points_kernel<int32_t>, n, records, (int)n_lobes, (int)sigmoid_codec, lambda_thres, tr,
                         points, index_tri32, dirs, n, n_device, features_out, rgb, sigma);
    } else {
        QF_SIMPLE_LAUNCH(vertex_quant_shade_points_kernel<int64_t>, n, records, (int)n_lobes, (int)sigmoid_codec, lambda_thres, tr,
                         points, index_tri, dirs, n, n_device, features_out, rgb, sigma);
    }
    return QF_OK;
}

extern "C" int qf_vertex_quant_composite_tiles(const uint8_t *records, int64_t n_vertices, int32_t n_lobes, int32_t sigmoid_codec,
                                               float lambda_thres, const void *tri_records, const float *xyz_c,
                                               const float *dirs_c, const float *depth_c, const int32_t *tri_c,
                                               const int32_t *hit_count, int32_t max_hits, const int64_t *tile_base,
                                               int32_t width, int32_t height, float delta_const, int32_t bg_mode,
                                               const float *bkgd, float stop_tau, float *out_rgb, float *out_alpha,
                                               float *out_depth, float *out_packed, int32_t *shaded_count, void *stream)
{
    const int rc = check_records(records, n_vertices, n_lobes);
    if (rc != QF_OK) return rc;
    if (!tri_records) return QF_ERR_INVALID_ARGUMENT;
    if (width < 1 || height < 1 || max_hits < 1 || bg_mode < 0 || bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!xyz_c || !dirs_c || !depth_c || !tri_c || !hit_count || !tile_base) return QF_ERR_INVALID_ARGUMENT;
    if (!out_packed && (!out_rgb || !out_alpha || !out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (bg_mode == QF_BG_CUSTOM && !bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const int64_t n_tiles = (int64_t)tiles_x * tiles_y;
    if (n_tiles > (1 << 30)) return QF_ERR_INVALID_ARGUMENT;                   // the kernel's tile loop counts in int
    hipLaunchKernelGGL(vertex_quant_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves)),
                       dim3(64 * kTileWaves), 0, qf_stream(stream), records, (int)n_lobes, (int)sigmoid_codec, lambda_thres,
                       static_cast<const VertexTriRecord *>(tri_records), xyz_c, dirs_c, depth_c, tri_c, hit_count, (int)max_hits,
                       tile_base, (int)width, (int)height, tiles_x, (int)n_tiles, delta_const, (int)bg_mode, bkgd, stop_tau,
                       out_rgb, out_alpha, out_depth, out_packed, shaded_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
