// Baked textures: per-triangle texel records and the nearest-texel lookup, the feature fetch from the reference's
// planes, the packed texel records and their decode / shade.
#include "exact_common.h"
#include "texture_device.h"

#pragma clang fp contract(off)

namespace {

// TexelRecord (the 128-byte record per triangle) and texel_from_record: texture_device.h.
__global__ void texel_records_kernel(const double *vertices, const int64_t *faces, const float *uv, int64_t n_faces,
                                     TexelRecord *records)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
        TexelRecord r;
        triangle_record_geometry(vertices, ia, ib, ic, r);
        r.uv[0] = uv[ia * 2]; r.uv[1] = uv[ia * 2 + 1];
        r.uv[2] = uv[ib * 2]; r.uv[3] = uv[ib * 2 + 1];
        r.uv[4] = uv[ic * 2]; r.uv[5] = uv[ic * 2 + 1];
        records[f] = r;
    }
}

__global__ void texel_indices_packed_kernel(const TexelRecord *__restrict__ records, const float *__restrict__ points,
                                            const int64_t *__restrict__ index_tri, int64_t n, int texture_size,
                                            int64_t *__restrict__ texel)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const TexelRecord r = records[index_tri[i]];
        int64_t q[2];
        texel_from_record(r, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], texture_size, q);
        texel[i * 2 + 0] = q[0];
        texel[i * 2 + 1] = q[1];
    }
}

struct TexArgs {
    const uint8_t *alpha, *diffuse;
    const uint8_t *colors[QF_MAX_LOBES];
    const uint8_t *lam[QF_MAX_LOBES];
    int size, n_lobes, sigmoid_codec;
    float lambda_thres;
};

// decode_color and the packed texel record (kTexelRecord bytes per texel): texture_device.h.

// Gathers a texel's bytes from the reference's planes into record order.
__device__ __forceinline__ void gather_record(const TexArgs &t, int64_t px, uint8_t *rec)
{
    rec[0] = t.alpha[px];
    rec[1] = t.diffuse[px * 3 + 0];
    rec[2] = t.diffuse[px * 3 + 1];
    rec[3] = t.diffuse[px * 3 + 2];
    for (int l = 0; l < t.n_lobes; ++l) {
        uint8_t *r = rec + 4 + 6 * l;
        r[0] = t.lam[l][px * 3 + 0];
        r[1] = t.lam[l][px * 3 + 1];
        r[2] = t.lam[l][px * 3 + 2];
        r[3] = t.colors[l][px * 3 + 0];
        r[4] = t.colors[l][px * 3 + 1];
        r[5] = t.colors[l][px * 3 + 2];
    }
}

__global__ void texture_pack_kernel(TexArgs t, uint8_t *records)
{
    const int64_t n = (int64_t)t.size * t.size;
    for (int64_t px = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; px < n; px += (int64_t)gridDim.x * blockDim.x) {
        union { uint8_t b[kTexelRecord]; uint4 q[kTexelRecord / 16]; } rec;
#pragma unroll
        for (int k = 0; k < kTexelRecord / 16; ++k) rec.q[k] = make_uint4(0u, 0u, 0u, 0u);
        gather_record(t, px, rec.b);
        uint4 *dst = reinterpret_cast<uint4 *>(records + px * kTexelRecord);
#pragma unroll
        for (int k = 0; k < kTexelRecord / 16; ++k) dst[k] = rec.q[k];
    }
}

// The shading kernel: a workgroup first fills the 256-entry dequantiser tables in LDS (DequantTables), then every sample
// is one record load and one decode by lookup (texel_record_load / texel_record_shade, texture_device.h: the record stays
// in registers, no scratch).
// kLookup: the texel is not read but looked up here, from the sample's position and triangle (texel_from_record): the
// frame path's fusion of qf_texel_indices_packed and this kernel (no int64 [n,2] texel array written and read back).
// TriT: int64_t (the reference's index_tri) or int32_t (the tile pack's ids).
template <bool kLookup, typename TriT>
__global__ __launch_bounds__(256) void texture_shade_packed_kernel(const uint8_t *__restrict__ records, int size, int n_lobes,
                                                                   int sigmoid_codec, float lambda_thres,
                                                                   const int64_t *__restrict__ texel,
                                                                   const float *__restrict__ dirs, int64_t n,
                                                                   float *__restrict__ rgb, float *__restrict__ sigma,
                                                                   const TexelRecord *__restrict__ tri_records,
                                                                   const float *__restrict__ points,
                                                                   const TriT *__restrict__ index_tri,
                                                                   const int64_t *__restrict__ n_dev)
{
    if (n_dev) { const int64_t nd = *n_dev; n = nd < n ? (nd > 0 ? nd : 0) : n; }    // device-side count (render-only frame)
    __shared__ DequantTables s_tab;
    dequant_tables_fill(s_tab, threadIdx.x, sigmoid_codec, lambda_thres);
    __syncthreads();
    const int n16 = texel_record_pieces(n_lobes);
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t px;
        if (kLookup) {
            const TexelRecord tr = tri_records[index_tri[i]];
            int64_t rc[2];
            texel_from_record(tr, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], size, rc);
            px = rc[0] * size + rc[1];
        } else {
            px = texel[i * 2] * size + texel[i * 2 + 1];
        }
        uint32_t w[kTexelRecord / 4];
        texel_record_load(records, px, n16, w);
        const float dx = dirs[i * 3], dy = dirs[i * 3 + 1], dz = dirs[i * 3 + 2];
        texel_record_shade(s_tab, w, n_lobes, dx, dy, dz, rgb + i * 3, sigma + i);
    }
}

// The feature fetch (get_features_from_texture_map) reads the reference's 2 + 2L separate planes: one texel's bytes
// are read plane by plane inside the unrolled lobe loop and each lobe is decoded and written at once (no per-lane
// feature array; round 2 kept float f[60] + a 64-byte record per lane in scratch: 256 B).
__device__ __forceinline__ void decode_lobe(const TexArgs &t, int l, int64_t px, float *o /* [7] */)
{
    const uint8_t lc = t.lam[l][px * 3 + 0], az8 = t.lam[l][px * 3 + 1], el8 = t.lam[l][px * 3 + 2];
    const float pi = 3.14159274101257324f;   // float32(np.pi)
    const float az = (float)(uint8_t)(az8 - 128) / 128.0f * pi;               // uint8 wrap (B-8), ngp.py:246
    const float el = (float)el8 / 256.0f * pi;                                // ngp.py:248
    const float se = sinf(el);
    o[0] = cosf(az) * se;
    o[1] = sinf(az) * se;
    o[2] = cosf(el);
    o[3] = expf((float)lc * t.lambda_thres / 255.0f - 2.5f);                  // ngp.py:261-262
    o[4] = decode_color(t.colors[l][px * 3 + 0], t.sigmoid_codec);
    o[5] = decode_color(t.colors[l][px * 3 + 1], t.sigmoid_codec);
    o[6] = decode_color(t.colors[l][px * 3 + 2], t.sigmoid_codec);
}

__global__ void texture_fetch_kernel(TexArgs t, const int64_t *texel, int64_t n, float *features)
{
    const int width = 3 + 7 * t.n_lobes + 1;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t px = texel[i * 2] * t.size + texel[i * 2 + 1];
        float *f = features + i * width;
        const float a = (float)t.alpha[px] / 255.0f;
        f[0] = decode_color(t.diffuse[px * 3 + 0], t.sigmoid_codec);
        f[1] = decode_color(t.diffuse[px * 3 + 1], t.sigmoid_codec);
        f[2] = decode_color(t.diffuse[px * 3 + 2], t.sigmoid_codec);
#pragma unroll
        for (int l = 0; l < QF_MAX_LOBES; ++l) {
            if (l < t.n_lobes) {
                float o[7];
                decode_lobe(t, l, px, o);
#pragma unroll
                for (int k = 0; k < 7; ++k) f[3 + 7 * l + k] = o[k];
            }
        }
        f[width - 1] = -logf(fmaxf(1.0f - a, 1e-6f)) / 0.005f;                // texture_utils.py:61-65 (B-9)
    }
}

int fill_tex_args(const qf_texture_set *tex, TexArgs *t)
{
    if (!tex || !tex->alpha || !tex->diffuse || tex->texture_size < 1) return QF_ERR_INVALID_ARGUMENT;
    if (tex->n_lobes < 1 || tex->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    t->alpha = tex->alpha;
    t->diffuse = tex->diffuse;
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        t->colors[l] = l < tex->n_lobes ? tex->colors[l] : nullptr;
        t->lam[l] = l < tex->n_lobes ? tex->lambda_axis[l] : nullptr;
        if (l < tex->n_lobes && (!t->colors[l] || !t->lam[l])) return QF_ERR_INVALID_ARGUMENT;
    }
    t->size = tex->texture_size;
    t->n_lobes = tex->n_lobes;
    t->sigmoid_codec = tex->sigmoid_codec;
    t->lambda_thres = tex->lambda_thres;
    return QF_OK;
}

}  // namespace

extern "C" int qf_texel_records_pack(const double *vertices, const int64_t *faces, const float *uv, int64_t n_faces,
                                     void *records, void *stream)
{
    if (n_faces < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_faces == 0) return QF_OK;
    if (!vertices || !faces || !uv || !records) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(texel_records_kernel, n_faces, vertices, faces, uv, n_faces, static_cast<TexelRecord *>(records));
    return QF_OK;
}

extern "C" int qf_texel_indices_packed(const void *records, const float *points, const int64_t *index_tri, int64_t n,
                                       int32_t texture_size, int64_t *texel, void *stream)
{
    if (n < 0 || texture_size < 1) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!records || !points || !index_tri || !texel) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(texel_indices_packed_kernel, n, static_cast<const TexelRecord *>(records), points, index_tri, n,
                     (int)texture_size, texel);
    return QF_OK;
}

extern "C" int qf_texture_fetch(const qf_texture_set *tex, const int64_t *texel, int64_t n, float *features, void *stream)
{
    TexArgs t;
    int rc = fill_tex_args(tex, &t);
    if (rc != QF_OK) return rc;
    if (n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!texel || !features) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(texture_fetch_kernel, n, t, texel, n, features);
    return QF_OK;
}

extern "C" int qf_texture_pack(const qf_texture_set *tex, uint8_t *records, void *stream)
{
    TexArgs t;
    int rc = fill_tex_args(tex, &t);
    if (rc != QF_OK) return rc;
    if (!records || 4 + 6 * t.n_lobes > kTexelRecord) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(texture_pack_kernel, (int64_t)t.size * t.size, t, records);
    return QF_OK;
}

extern "C" int qf_texture_shade_packed(const uint8_t *records, int32_t texture_size, int32_t n_lobes,
                                       int32_t sigmoid_codec, float lambda_thres, const int64_t *texel,
                                       const float *dirs, int64_t n, float *rgb, float *sigma, void *stream)
{
    if (!records || texture_size < 1 || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (n == 0) return QF_OK;
    if (!texel || !dirs || !rgb || !sigma) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH((texture_shade_packed_kernel<false, int64_t>), n, records, (int)texture_size, (int)n_lobes,
                     (int)sigmoid_codec, lambda_thres, texel, dirs, n, rgb, sigma, (const TexelRecord *)nullptr,
                     (const float *)nullptr, (const int64_t *)nullptr, (const int64_t *)nullptr);
    return QF_OK;
}

extern "C" int qf_texture_shade_points(const uint8_t *records, int32_t texture_size, int32_t n_lobes, int32_t sigmoid_codec,
                                       float lambda_thres, const void *triangle_records, const float *points,
                                       const int64_t *index_tri, const int32_t *index_tri32, const float *dirs, int64_t n,
                                       const int64_t *n_device, float *rgb, float *sigma, void *stream)
{
    if (!records || !triangle_records || texture_size < 1 || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (n == 0) return QF_OK;
    if (!points || (!index_tri == !index_tri32) || !dirs || !rgb || !sigma) return QF_ERR_INVALID_ARGUMENT;   // exactly one id array
    const TexelRecord *tr = static_cast<const TexelRecord *>(triangle_records);
    if (index_tri32) {
        QF_SIMPLE_LAUNCH((texture_shade_packed_kernel<true, int32_t>), n, records, (int)texture_size, (int)n_lobes,
                         (int)sigmoid_codec, lambda_thres, (const int64_t *)nullptr, dirs, n, rgb, sigma, tr, points,
                         index_tri32, n_device);
    } else {
        QF_SIMPLE_LAUNCH((texture_shade_packed_kernel<true, int64_t>), n, records, (int)texture_size, (int)n_lobes,
                         (int)sigmoid_codec, lambda_thres, (const int64_t *)nullptr, dirs, n, rgb, sigma, tr, points,
                         index_tri, n_device);
    }
    return QF_OK;
}
