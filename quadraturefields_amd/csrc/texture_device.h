// Baked textures on the device: the per-triangle texel record and the nearest-texel lookup, the packed texel record,
// the 256-entry dequantiser tables and the decode + SG shading of one record -- shared by the shading kernels of
// texture.hip and the fused baked-frame kernel (baked_frame.hip): one definition, hence the same bits in both.
// Every function rounds each operation on its own (`#pragma clang fp contract(off)` inside the bodies, whatever the
// including translation unit is compiled with).
#pragma once
#include "qf_common.h"

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

// The 13 doubles every per-triangle record starts with (TexelRecord here, VertexTriRecord in vertex_baked_device.h): corner
// a, edges e0 / e1, their three dot products and the reciprocal determinant, from the float64 vertices ia, ib, ic.  One
// definition, hence the same bits in both record kinds.
template <class R>
__device__ __forceinline__ void triangle_record_geometry(const double *__restrict__ vertices, int64_t ia, int64_t ib,
                                                         int64_t ic, R &r)
{
#pragma clang fp contract(off)
    r.ax = vertices[ia * 3]; r.ay = vertices[ia * 3 + 1]; r.az = vertices[ia * 3 + 2];
    r.e0x = vertices[ib * 3] - r.ax; r.e0y = vertices[ib * 3 + 1] - r.ay; r.e0z = vertices[ib * 3 + 2] - r.az;
    r.e1x = vertices[ic * 3] - r.ax; r.e1y = vertices[ic * 3 + 1] - r.ay; r.e1z = vertices[ic * 3 + 2] - r.az;
    r.d00 = (r.e0x * r.e0x + r.e0y * r.e0y) + r.e0z * r.e0z;
    r.d01 = (r.e0x * r.e1x + r.e0y * r.e1y) + r.e0z * r.e1z;
    r.d11 = (r.e1x * r.e1x + r.e1y * r.e1y) + r.e1z * r.e1z;
    r.inv = 1.0 / (r.d00 * r.d11 - r.d01 * r.d01);
}

// The float64 Cramer barycentrics of a point in its triangle from the 13 doubles (trimesh's points_to_barycentric,
// method 'cramer'): b[0..2] for corners a, b, c.
template <class R>
__device__ __forceinline__ void barycentrics_from_record(const R &r, float px, float py, float pz, double b[3])
{
#pragma clang fp contract(off)
    const double wx = (double)px - r.ax, wy = (double)py - r.ay, wz = (double)pz - r.az;
    const double d02 = (r.e0x * wx + r.e0y * wy) + r.e0z * wz;
    const double d12 = (r.e1x * wx + r.e1y * wy) + r.e1z * wz;
    const double b2d = (r.d00 * d12 - r.d01 * d02) * r.inv;
    const double b1d = (r.d11 * d02 - r.d01 * d12) * r.inv;
    b[0] = 1.0 - b1d - b2d;
    b[1] = b1d;
    b[2] = b2d;
}

__device__ __forceinline__ void texel_from_record(const TexelRecord &r, float px, float py, float pz, int texture_size,
                                                  int64_t out[2])
{
#pragma clang fp contract(off)
    double bd[3];
    barycentrics_from_record(r, px, py, pz, bd);
    const double b0d = bd[0], b1d = bd[1], b2d = bd[2];
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

__device__ __forceinline__ float decode_color(uint8_t c, int sigmoid_codec)
{
#pragma clang fp contract(off)
    const float v = (float)c / 255.0f;
    if (sigmoid_codec) return logf(fminf(fmaxf(v / (1.0f - v), 1e-8f), 1e37f));   // ngp.py:277-278
    return v * 2.0f * 12.0f - 12.0f;                                              // ngp.py:280 (B-7)
}

// Device-resident texel record: the 4 + 6L quantised bytes of one texel, contiguous and padded to one 64-byte
// sector -- [alpha | diffuse rgb | (lambda, azimuth, elevation, colour rgb) * L].  The reference keeps 2 + 2L separate
// planes (the PNG set of texture_utils.py:67-124), i.e. 2 + 2L scattered sector reads per sample; a record is ONE.
constexpr int kTexelRecord = QF_TEXEL_RECORD_BYTES;

// Every quantity a record decodes to is a function of ONE uint8 code, so a workgroup first evaluates the reference's
// dequantisers (the same expressions as decode_color / decode_lobe, hence the same bits) for all 256 codes into LDS
// and then decodes by lookup: the 4L sin/cos, L exp and 3+3L colour decodes per sample become LDS reads.
struct DequantTables {
    float sigma[256], col[256], caz[256], saz[256], sel[256], cel[256], lam[256];
};

// Entry c of every table; thread c of a workgroup of (at least) 256 calls it, followed by a barrier.
__device__ __forceinline__ void dequant_tables_fill(DequantTables &t, int c, int sigmoid_codec, float lambda_thres)
{
#pragma clang fp contract(off)
    const float pi = 3.14159274101257324f;   // float32(np.pi)
    const float a = (float)c / 255.0f;
    t.sigma[c] = -logf(fmaxf(1.0f - a, 1e-6f)) / 0.005f;
    t.col[c] = decode_color((uint8_t)c, sigmoid_codec);
    const float az = (float)(uint8_t)(c - 128) / 128.0f * pi;
    const float el = (float)c / 256.0f * pi;
    t.caz[c] = cosf(az);
    t.saz[c] = sinf(az);
    t.sel[c] = sinf(el);
    t.cel[c] = cosf(el);
    t.lam[c] = expf((float)c * lambda_thres / 255.0f - 2.5f);
}

// The record stays in REGISTERS: sixteen 32-bit words addressed with compile-time indices only -- the lobe loop is fully
// unrolled over QF_MAX_LOBES with a wave-uniform ``l < n_lobes`` guard, so ``word[(4 + 6 l + j) >> 2]`` is a constant
// register and the byte comes out with one shift + mask (v_bfe).  Round 2 indexed a byte array with the run-time lobe
// counter, which put the whole record in scratch: 80 B per lane written and read back per sample.
__device__ __forceinline__ uint32_t rec_byte(const uint32_t (&w)[kTexelRecord / 4], int idx)   // idx: compile-time
{
    return (w[idx >> 2] >> ((idx & 3) * 8)) & 0xffu;
}

// 16-byte pieces of a record that carry data (wave-uniform)
__device__ __forceinline__ int texel_record_pieces(int n_lobes) { return (4 + 6 * n_lobes + 15) / 16; }

// Texel px's record -> w; the pieces past n16 are zero and not read.
__device__ __forceinline__ void texel_record_load(const uint8_t *__restrict__ records, int64_t px, int n16,
                                                  uint32_t (&w)[kTexelRecord / 4])
{
    const uint4 *src = reinterpret_cast<const uint4 *>(records + px * kTexelRecord);
#pragma unroll
    for (int k = 0; k < kTexelRecord / 16; ++k) {
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (k < n16) q = src[k];                   // wave-uniform
        w[4 * k] = q.x; w[4 * k + 1] = q.y; w[4 * k + 2] = q.z; w[4 * k + 3] = q.w;
    }
}

// Decode + SG shading of one record for the view direction (dx, dy, dz): sigmoid(diffuse + sum over lobes of
// colour * exp(|lambda| (axis . dir - 1))) -> rgb, and the density of the alpha code.
__device__ __forceinline__ void texel_record_shade(const DequantTables &t, const uint32_t (&w)[kTexelRecord / 4], int n_lobes,
                                                   float dx, float dy, float dz, float *__restrict__ rgb /* [3] */,
                                                   float *__restrict__ sigma)
{
#pragma clang fp contract(off)
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        if (l < n_lobes) {                         // wave-uniform; every index below is a compile-time constant
            const int o = 4 + 6 * l;
            const uint32_t c_lam = rec_byte(w, o), c_az = rec_byte(w, o + 1), c_el = rec_byte(w, o + 2);
            const float se = t.sel[c_el];
            const float x0 = t.caz[c_az] * se, x1 = t.saz[c_az] * se, x2 = t.cel[c_el];
            const float nrm = sqrtf((x0 * x0 + x1 * x1) + x2 * x2);
            const float dotp = ((x0 / nrm) * dx + (x1 / nrm) * dy) + (x2 / nrm) * dz;
            const float e = expf(fabsf(t.lam[c_lam]) * (dotp - 1.0f));
            r += t.col[rec_byte(w, o + 3)] * e;
            g += t.col[rec_byte(w, o + 4)] * e;
            b += t.col[rec_byte(w, o + 5)] * e;
        }
    }
    rgb[0] = 1.0f / (1.0f + expf(-(t.col[rec_byte(w, 1)] + r)));
    rgb[1] = 1.0f / (1.0f + expf(-(t.col[rec_byte(w, 2)] + g)));
    rgb[2] = 1.0f / (1.0f + expf(-(t.col[rec_byte(w, 3)] + b)));
    *sigma = t.sigma[rec_byte(w, 0)];
}

}  // namespace
