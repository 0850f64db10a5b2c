// The quantised vertex table on the device (include/qf_vertex_quant.h): one 64-byte texel record
// per vertex, decoded through the LDS code tables of texture_device.h and blended with vertex_baked_device.h's column
// expression -- shared by the kernels of vertex_quant.hip (decode, point shader, tile compositor): one definition, hence
// the same bits in all three, and the bits of the fp32 route on the decoded table.  Decode first, then blend; the codes
// are never blended.  Every function rounds each operation on its own.
#pragma once
#include "qf_vertex_quant.h"
#include "vertex_baked_device.h"

namespace {

// The seven decoded columns of lobe L of one record, (axis3, lambda, colour3): qf_texture_fetch's decode_lobe by lookup
// (the tables hold the same expressions per code).  L is a compile-time constant, so every record word is a register.
template <int L>
__device__ __forceinline__ void vertex_quant_lobe(const DequantTables &t, const uint32_t (&w)[kTexelRecord / 4], float o[7])
{
#pragma clang fp contract(off)
    constexpr int p = 4 + 6 * L;
    const uint32_t c_az = rec_byte(w, p + 1), c_el = rec_byte(w, p + 2);
    const float se = t.sel[c_el];
    o[0] = t.caz[c_az] * se;
    o[1] = t.saz[c_az] * se;
    o[2] = t.cel[c_el];
    o[3] = t.lam[rec_byte(w, p)];
    o[4] = t.col[rec_byte(w, p + 3)];
    o[5] = t.col[rec_byte(w, p + 4)];
    o[6] = t.col[rec_byte(w, p + 5)];
}

// Lobe L of the three records, decoded and blended straight into its seven columns: 21 decoded floats live at a time,
// never three decoded rows.
template <int L>
__device__ __forceinline__ void vertex_quant_blend_lobe(const DequantTables &t, const uint32_t (&w0)[kTexelRecord / 4],
                                                        const uint32_t (&w1)[kTexelRecord / 4],
                                                        const uint32_t (&w2)[kTexelRecord / 4], int n_lobes, const float b[3],
                                                        float sigma, float (&blend)[kVertexRowMax])
{
    if (L + 1 == n_lobes) blend[3 + 7 * (L + 1)] = sigma;    // wave-uniform: the density follows the last lobe
    if (L < n_lobes) {                             // wave-uniform
        float f0[7], f1[7], f2[7];
        vertex_quant_lobe<L>(t, w0, f0);
        vertex_quant_lobe<L>(t, w1, f1);
        vertex_quant_lobe<L>(t, w2, f2);
#pragma unroll
        for (int j = 0; j < 7; ++j) blend[3 + 7 * L + j] = vertex_blend_column(f0[j], f1[j], f2[j], b);
    }
}

// vertex_blend for the quantised table: the records of vertices v0, v1, v2 (n16 16-byte pieces each) -> the blend of their
// decoded rows; the columns past the width are zero.  Every index of `blend` and of the records is a compile-time
// constant.
__device__ __forceinline__ void vertex_quant_blend(const DequantTables &t, const uint8_t *__restrict__ records, int n16,
                                                   int n_lobes, int v0, int v1, int v2, const float b[3],
                                                   float (&blend)[kVertexRowMax])
{
    uint32_t w0[kTexelRecord / 4], w1[kTexelRecord / 4], w2[kTexelRecord / 4];
    texel_record_load(records, v0, n16, w0);
    texel_record_load(records, v1, n16, w1);
    texel_record_load(records, v2, n16, w2);
#pragma unroll
    for (int c = 0; c < kVertexRowMax; ++c) blend[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c)
        blend[c] = vertex_blend_column(t.col[rec_byte(w0, 1 + c)], t.col[rec_byte(w1, 1 + c)], t.col[rec_byte(w2, 1 + c)], b);
    const float s = vertex_blend_column(t.sigma[rec_byte(w0, 0)], t.sigma[rec_byte(w1, 0)], t.sigma[rec_byte(w2, 0)], b);
    static_assert(QF_MAX_LOBES == 8, "the lobe list below is written out");
    vertex_quant_blend_lobe<0>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<1>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<2>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<3>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<4>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<5>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<6>(t, w0, w1, w2, n_lobes, b, s, blend);
    vertex_quant_blend_lobe<7>(t, w0, w1, w2, n_lobes, b, s, blend);
}

// Lobe L of one record written to its seven columns of the row.
template <int L>
__device__ __forceinline__ void vertex_quant_row_lobe(const DequantTables &t, const uint32_t (&w)[kTexelRecord / 4], int n_lobes,
                                                      float sigma, float (&row)[kVertexRowMax])
{
    if (L + 1 == n_lobes) row[3 + 7 * (L + 1)] = sigma;      // wave-uniform: the density follows the last lobe
    if (L < n_lobes) {                             // wave-uniform
        float o[7];
        vertex_quant_lobe<L>(t, w, o);
#pragma unroll
        for (int j = 0; j < 7; ++j) row[3 + 7 * L + j] = o[j];
    }
}

// One record decoded to its row (what vertex_quant_blend blends three of); the columns past the width are zero.
__device__ __forceinline__ void vertex_quant_decode_row(const DequantTables &t, const uint32_t (&w)[kTexelRecord / 4], int n_lobes,
                                                        float (&row)[kVertexRowMax])
{
#pragma unroll
    for (int c = 0; c < kVertexRowMax; ++c) row[c] = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; ++c) row[c] = t.col[rec_byte(w, 1 + c)];
    const float s = t.sigma[rec_byte(w, 0)];
    static_assert(QF_MAX_LOBES == 8, "the lobe list below is written out");
    vertex_quant_row_lobe<0>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<1>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<2>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<3>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<4>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<5>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<6>(t, w, n_lobes, s, row);
    vertex_quant_row_lobe<7>(t, w, n_lobes, s, row);
}

}  // namespace
