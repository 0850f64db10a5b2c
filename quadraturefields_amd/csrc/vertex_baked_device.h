// Vertex-baked SG features on the device: the per-triangle record with its three vertex ids, the
// unclamped fp32 barycentrics, the barycentric blend of three rows of the vertex table and the SG shading of the blend --
// shared by the kernels of vertex_baked.hip (the point shader and the fused tile compositor): one definition, hence the
// same bits in both.  Every function rounds each operation on its own (`#pragma clang fp contract(off)` inside the
// bodies, whatever the including translation unit is compiled with).
#pragma once
#include "qf_common.h"
#include "qf_vertex_baked.h"
#include "texture_device.h"

namespace {

// TexelRecord's 13 doubles (triangle_record_geometry, texture_device.h), the three vertex ids where TexelRecord keeps its
// uv, 12 zero bytes.
struct VertexTriRecord {
    double ax, ay, az, e0x, e0y, e0z, e1x, e1y, e1z, d00, d01, d11, inv;
    int32_t v[3];                    // rows of the vertex table: corners a, b, c
    int32_t zero[3];
};
static_assert(sizeof(VertexTriRecord) == QF_VERTEX_TRIANGLE_RECORD_BYTES, "one 128-byte line per triangle");

constexpr int kVertexRowMax = 16 * ((3 + 7 * QF_MAX_LOBES + 1 + 15) / 16);   // floats of the widest row: 64

// floats per row of the table for n_lobes: the width 3 + 7L + 1 rounded up to a 64-byte line
__host__ __device__ __forceinline__ int vertex_row_width(int n_lobes) { return 3 + 7 * n_lobes + 1; }
__host__ __device__ __forceinline__ int vertex_row_stride(int n_lobes) { return 16 * ((vertex_row_width(n_lobes) + 15) / 16); }
// 16-byte pieces of a row that carry data (wave-uniform)
__device__ __forceinline__ int vertex_row_pieces(int n_lobes) { return (vertex_row_width(n_lobes) + 3) / 4; }

// The reference's vertex route (utils.py:822-823): the float64 Cramer barycentrics cast to fp32, neither clamped nor
// renormalised; a degenerate triangle (1/det not finite) gives NaN.
__device__ __forceinline__ void vertex_barycentrics(const VertexTriRecord &r, float px, float py, float pz, float b[3])
{
    double bd[3];
    barycentrics_from_record(r, px, py, pz, bd);
    b[0] = (float)bd[0];
    b[1] = (float)bd[1];
    b[2] = (float)bd[2];
}

// One column of the blend: (f0 * b0 + f1 * b1) + f2 * b2, each operation rounded on its own.  The one definition every
// vertex route blends with (the fp32 table here, the quantised records of vertex_quant_device.h): the same bits in all.
__device__ __forceinline__ float vertex_blend_column(float f0, float f1, float f2, const float b[3])
{
#pragma clang fp contract(off)
    return (f0 * b[0] + f1 * b[1]) + f2 * b[2];
}

// blend[c] = (f0[c] * b0 + f1[c] * b1) + f2[c] * b2 for the columns of the n16 data-carrying 16-byte pieces, f_k = row v_k
// of the table; the columns past them are zero and not read.  The blend accumulates piece by piece: three 16-byte loads,
// four columns, next piece -- three whole rows are never live.  Every index of `blend` is a compile-time constant.
__device__ __forceinline__ void vertex_blend(const float *__restrict__ table, int stride, int n16, int v0, int v1, int v2,
                                             const float b[3], float (&blend)[kVertexRowMax])
{
#pragma clang fp contract(off)
    const float4 *r0 = reinterpret_cast<const float4 *>(table + (int64_t)v0 * stride);
    const float4 *r1 = reinterpret_cast<const float4 *>(table + (int64_t)v1 * stride);
    const float4 *r2 = reinterpret_cast<const float4 *>(table + (int64_t)v2 * stride);
#pragma unroll
    for (int k = 0; k < kVertexRowMax / 4; ++k) {
        float4 q = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (k < n16) {                             // wave-uniform
            const float4 f0 = r0[k], f1 = r1[k], f2 = r2[k];
            q.x = vertex_blend_column(f0.x, f1.x, f2.x, b);
            q.y = vertex_blend_column(f0.y, f1.y, f2.y, b);
            q.z = vertex_blend_column(f0.z, f1.z, f2.z, b);
            q.w = vertex_blend_column(f0.w, f1.w, f2.w, b);
        }
        blend[4 * k] = q.x; blend[4 * k + 1] = q.y; blend[4 * k + 2] = q.z; blend[4 * k + 3] = q.w;
    }
}

// The blended density: column 3 + 7L, picked with compile-time indices.
__device__ __forceinline__ float vertex_blend_sigma(const float (&blend)[kVertexRowMax], int n_lobes)
{
    float s = 0.0f;
#pragma unroll
    for (int l = 1; l <= QF_MAX_LOBES; ++l)
        if (l == n_lobes) s = blend[3 + 7 * l];    // wave-uniform
    return s;
}

// SG shading of a blend for the view direction (dx, dy, dz): sigmoid(diffuse + sum over lobes of
// colour * exp(|lambda| (axis / |axis| . dir - 1))), sg_features_to_rgb_kernel's formula (field_eval.hip).  The lobe loop
// is fully unrolled over QF_MAX_LOBES with a wave-uniform guard, so every register index is a compile-time constant.
__device__ __forceinline__ void vertex_blend_shade(const float (&blend)[kVertexRowMax], int n_lobes, float dx, float dy,
                                                   float dz, float rgb[3])
{
#pragma clang fp contract(off)
    float r = 0.0f, g = 0.0f, b = 0.0f;
#pragma unroll
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        if (l < n_lobes) {                         // wave-uniform
            const int o = 3 + 7 * l;
            const float x0 = blend[o], x1 = blend[o + 1], x2 = blend[o + 2];
            const float nrm = sqrtf((x0 * x0 + x1 * x1) + x2 * x2);
            const float dotp = ((x0 / nrm) * dx + (x1 / nrm) * dy) + (x2 / nrm) * dz;
            const float e = expf(fabsf(blend[o + 3]) * (dotp - 1.0f));
            r += blend[o + 4] * e;
            g += blend[o + 5] * e;
            b += blend[o + 6] * e;
        }
    }
    rgb[0] = 1.0f / (1.0f + expf(-(blend[0] + r)));
    rgb[1] = 1.0f / (1.0f + expf(-(blend[1] + g)));
    rgb[2] = 1.0f / (1.0f + expf(-(blend[2] + b)));
}

}  // namespace
