// Baked textures: per-triangle texel records and the nearest-texel lookup, the feature fetch from the reference's
// planes, the packed texel records and their decode / shade.
#include "exact_common.h"

#pragma clang fp contract(off)

namespace {

// The nearest-texel lookup of utils.py:1055-1063: float64 Cramer barycentrics -> fp32 clamp / renormalise -> uv ->
// floor -> clip.  Everything that depends on the triangle alone is computed once per mesh into a 128-byte record per
// triangle -- corner a, edges e0 / e1, their three dot products and the reciprocal determinant (13 doubles), the three
// corners' uv (6 floats) -- so that a sample reads ONE line instead of following faces -> 3 vertices -> 3 uv, and
// evaluates two dot products instead of five and no division (texel_from_record).
struct TexelRecord {
    double ax, ay, az, e0x, e0y, e0z, e1x, e1y, e1z, d00, d01, d11, inv;
    float uv[6];                     // (u, v) of corners a, b, c
};
static_assert(sizeof(TexelRecord) == 128, "one 128-byte line per triangle");

__global__ void texel_records_kernel(const double *vertices, const int64_t *faces, const float *uv, int64_t n_faces,
                                     TexelRecord *records)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < n_faces; f += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = faces[f * 3], ib = faces[f * 3 + 1], ic = faces[f * 3 + 2];
        TexelRecord r;
        r.ax = vertices[ia * 3]; r.ay = vertices[ia * 3 + 1]; r.az = vertices[ia * 3 + 2];
        r.e0x = vertices[ib * 3] - r.ax; r.e0y = vertices[ib * 3 + 1] - r.ay; r.e0z = vertices[ib * 3 + 2] - r.az;
        r.e1x = vertices[ic * 3] - r.ax; r.e1y = vertices[ic * 3 + 1] - r.ay; r.e1z = vertices[ic * 3 + 2] - r.az;
        r.d00 = (r.e0x * r.e0x + r.e0y * r.e0y) + r.e0z * r.e0z;
        r.d01 = (r.e0x * r.e1x + r.e0y * r.e1y) + r.e0z * r.e1z;
        r.d11 = (r.e1x * r.e1x + r.e1y * r.e1y) + r.e1z * r.e1z;
        r.inv = 1.0 / (r.d00 * r.d11 - r.d01 * r.d01);
        r.uv[0] = uv[ia * 2]; r.uv[1] = uv[ia * 2 + 1];
        r.uv[2] = uv[ib * 2]; r.uv[3] = uv[ib * 2 + 1];
        r.uv[4] = uv[ic * 2]; r.uv[5] = uv[ic * 2 + 1];
        records[f] = r;
    }
}

__device__ __forceinline__ void texel_from_record(const TexelRecord &r, float px, float py, float pz, int texture_size,
                                                  int64_t out[2])
{
    const double wx = (double)px - r.ax, wy = (double)py - r.ay, wz = (double)pz - r.az;
    const double d02 = (r.e0x * wx + r.e0y * wy) + r.e0z * wz;
    const double d12 = (r.e1x * wx + r.e1y * wy) + r.e1z * wz;
    const double b2d = (r.d00 * d12 - r.d01 * d02) * r.inv;
    const double b1d = (r.d11 * d02 - r.d01 * d12) * r.inv;
    const double b0d = 1.0 - b1d - b2d;
    float b0 = fminf(fmaxf((float)b0d, 0.0f), 1.0f);
    float b1 = fminf(fmaxf((float)b1d, 0.0f), 1.0f);
    float b2 = fminf(fmaxf((float)b2d, 0.0f), 1.0f);
    const float s = (b0 + b1) + b2;
    b0 = b0 / s;
    b1 = b1 / s;
    b2 = b2 / s;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const float u = (r.uv[k] * b0 + r.uv[2 + k] * b1) + r.uv[4 + k] * b2;
        float fl = floorf(u);
        // torch: floor -> .long() -> clip(0, T-1); NaN (degenerate triangle) -> int64 min -> 0
        int64_t q = (fl != fl) ? 0 : (fl <= -9.2e18f ? INT64_MIN : (fl >= 9.2e18f ? INT64_MAX : (int64_t)fl));
        if (q < 0) q = 0;
        if (q > texture_size - 1) q = texture_size - 1;
        out[k] = q;
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

__device__ __forceinline__ float decode_color(uint8_t c, int sigmoid_codec)
{
    const float v = (float)c / 255.0f;
    if (sigmoid_codec) return logf(fminf(fmaxf(v / (1.0f - v), 1e-8f), 1e37f));   // ngp.py:277-278
    return v * 2.0f * 12.0f - 12.0f;                                              // ngp.py:280 (B-7)
}

// Device-resident texel record: the 4 + 6L quantised bytes of one texel, contiguous and padded to one 64-byte
// sector -- [alpha | diffuse rgb | (lambda, azimuth, elevation, colour rgb) * L].  The reference keeps 2 + 2L separate
// planes (the PNG set of texture_utils.py:67-124), i.e. 2 + 2L scattered sector reads per sample; a record is ONE.
constexpr int kTexelRecord = QF_TEXEL_RECORD_BYTES;

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

// Every quantity a record decodes to is a function of ONE uint8 code, so a workgroup first evaluates the reference's
// dequantisers (the same expressions as decode_color / decode_lobe, hence the same bits) for all 256 codes into LDS
// and then decodes by lookup: the 4L sin/cos, L exp and 3+3L colour decodes per sample become LDS reads.
// kLookup: the texel is not read but looked up here, from the sample's position and triangle (texel_from_record): the
// frame path's fusion of qf_texel_indices_packed and this kernel (no int64 [n,2] texel array written and read back).
// The record stays in REGISTERS: sixteen 32-bit words addressed with compile-time indices only -- the lobe loop is fully
// unrolled over QF_MAX_LOBES with a wave-uniform ``l < n_lobes`` guard, so ``word[(4 + 6 l + j) >> 2]`` is a constant
// register and the byte comes out with one shift + mask (v_bfe).  Round 2 indexed a byte array with the run-time lobe
// counter, which put the whole record in scratch: 80 B per lane written and read back per sample.
__device__ __forceinline__ uint32_t rec_byte(const uint32_t (&w)[kTexelRecord / 4], int idx)   // idx: compile-time
{
    return (w[idx >> 2] >> ((idx & 3) * 8)) & 0xffu;
}

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
    __shared__ float s_sigma[256], s_col[256], s_caz[256], s_saz[256], s_sel[256], s_cel[256], s_lam[256];
    {
        const int c = threadIdx.x;
        const float pi = 3.14159274101257324f;   // float32(np.pi)
        const float a = (float)c / 255.0f;
        s_sigma[c] = -logf(fmaxf(1.0f - a, 1e-6f)) / 0.005f;
        s_col[c] = decode_color((uint8_t)c, sigmoid_codec);
        const float az = (float)(uint8_t)(c - 128) / 128.0f * pi;
        const float el = (float)c / 256.0f * pi;
        s_caz[c] = cosf(az);
        s_saz[c] = sinf(az);
        s_sel[c] = sinf(el);
        s_cel[c] = cosf(el);
        s_lam[c] = expf((float)c * lambda_thres / 255.0f - 2.5f);
    }
    __syncthreads();
    const int n16 = (4 + 6 * n_lobes + 15) / 16;       // 16-byte pieces of the record that carry data
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
        const uint4 *src = reinterpret_cast<const uint4 *>(records + px * kTexelRecord);
        uint32_t w[kTexelRecord / 4];
#pragma unroll
        for (int k = 0; k < kTexelRecord / 16; ++k) {
            uint4 q = make_uint4(0u, 0u, 0u, 0u);
            if (k < n16) q = src[k];                   // wave-uniform
            w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
        }
        const float dx = dirs[i * 3], dy = dirs[i * 3 + 1], dz = dirs[i * 3 + 2];
        float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
        for (int l = 0; l < QF_MAX_LOBES; ++l) {
            if (l < n_lobes) {                         // wave-uniform; every index below is a compile-time constant
                const int o = 4 + 6 * l;
                const uint32_t c_lam = rec_byte(w, o), c_az = rec_byte(w, o + 1), c_el = rec_byte(w, o + 2);
                const float se = s_sel[c_el];
                const float x0 = s_caz[c_az] * se, x1 = s_saz[c_az] * se, x2 = s_cel[c_el];
                const float nrm = sqrtf((x0 * x0 + x1 * x1) + x2 * x2);
                const float dotp = ((x0 / nrm) * dx + (x1 / nrm) * dy) + (x2 / nrm) * dz;
                const float e = expf(fabsf(s_lam[c_lam]) * (dotp - 1.0f));
                r += s_col[rec_byte(w, o + 3)] * e;
                g += s_col[rec_byte(w, o + 4)] * e;
                b += s_col[rec_byte(w, o + 5)] * e;
            }
        }
        rgb[i * 3 + 0] = 1.0f / (1.0f + expf(-(s_col[rec_byte(w, 1)] + r)));
        rgb[i * 3 + 1] = 1.0f / (1.0f + expf(-(s_col[rec_byte(w, 2)] + g)));
        rgb[i * 3 + 2] = 1.0f / (1.0f + expf(-(s_col[rec_byte(w, 3)] + b)));
        sigma[i] = s_sigma[rec_byte(w, 0)];
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
