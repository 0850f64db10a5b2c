// The fp32 matrix-core pieces shared by the fused field kernels and their training-side backward kernels
// (field_eval.hip, grid_extract.hip, mlp_train.hip, field_train.hip): the MFMA, the LDS weight images of the layers that
// more than one kernel computes, the layer idioms over them and the weight-gradient tiles of the training kernels.
//
// Every layer is computed transposed, H^T[neuron][point] = W . X^T, with v_mfma_f32_16x16x4_f32: W tiles are the A
// operand, one value per lane (i = lane & 15: row of the tile, kq = lane >> 4: k of the step), X^T the B operand.  The
// C/D layout puts D[4g+r][p] in register r of lane (g,p), which is the B operand of the next layer's k-step; the k
// order of each layer is permuted to match (hidden_col), and the permutation is folded into the weight image.
#pragma once
#include "field_common.h"

namespace {

__device__ __forceinline__ f32x4 mfma(float a, float b, f32x4 c)
{
    return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// Two image layouts.  Quad image: MFMAs m = 4q .. 4q+3 of a lane share one f32x4 (ds_read_b128) at img[q * 64 + lane];
// img_index is the float index of (m, lane).  Plain image: lds[m * 64 + lane] (ds_read_b32).
__device__ __forceinline__ int img_index(int m, int lane) { return ((((m >> 2) << 6) + lane) << 2) + (m & 3); }

// column of the head's first layer fed by register 4+r of lane quartet kq: [geo | 1] part of [SH16 | geo15 | 1]
__device__ __forceinline__ int geo_col(int o) { return o == 0 ? 31 : 15 + o; }

constexpr int kBaseMfma = 48;        // 32 (32->64) + 16 (64->16)
constexpr int kNgpHeadMfma = 112;    // 32 + 64 + 16
constexpr int kSgHiddenMfma = 80;    // 16 (16->64) + 64 (64->64); + 16 per output tile

// Weight value that lane `lane` must feed as A operand of MFMA number m (program order) of the base MLP followed by
// head HEAD: the image of field_kernel<HEAD>, and of the forward recomputation of the backward kernels (which stop
// before the SG output tiles).  One flat chain of tests on m: nesting it per network changes the staging code.
template <int HEAD>
__device__ __forceinline__ float field_image_weight(const float *base_w, const float *head_w, const qf_sg_head &sg,
                                                    int n_out, int m, int lane)
{
    const int i = lane & 15, kq = lane >> 4;
    if (m < 32) {                       // base 32 -> 64: s outer, mt inner
        const int s = m >> 2, mt = m & 3;
        const int col = 2 * (4 * (s >> 1) + kq) + (s & 1);
        return base_w[(16 * mt + i) * 32 + col];
    }
    if (m < kBaseMfma) {                // base 64 -> 16
        const int s = m - 32;
        return base_w[2048 + i * 64 + hidden_col(s, kq)];
    }
    m -= kBaseMfma;
    if (HEAD == QF_HEAD_NGP) {
        if (m < 32) {                   // [SH16 | geo15 | 1] -> 64
            const int s = m >> 2, mt = m & 3;
            int col;
            if (s < 4) col = 4 * kq + s;
            else col = geo_col(4 * kq + (s - 4));
            return head_w[(16 * mt + i) * 32 + col];
        }
        if (m < 96) {                   // 64 -> 64
            const int q = m - 32, s = q >> 2, mt = q & 3;
            return head_w[2048 + (16 * mt + i) * 64 + hidden_col(s, kq)];
        }
        const int s = m - 96;           // 64 -> 16 (3 used)
        return head_w[2048 + 4096 + i * 64 + hidden_col(s, kq)];
    }
    if (HEAD == QF_HEAD_SG || HEAD == QF_HEAD_SG_FEATURES) {
        if (m < 16) {                   // [geo15 | bias] -> 64 ; slot of the density carries b1
            const int s = m >> 2, mt = m & 3, row = 16 * mt + i;
            const int o = 4 * kq + s;
            return (o == 0) ? sg.b1[row] : sg.w1[row * 15 + (o - 1)];
        }
        if (m < kSgHiddenMfma) {
            const int q = m - 16, s = q >> 2, mt = q & 3;
            return sg.w2[(16 * mt + i) * 64 + hidden_col(s, kq)];
        }
        const int q = m - kSgHiddenMfma, mt = q >> 4, s = q & 15;   // output tiles: mt outer, s inner
        const int row = 16 * mt + i;
        return (row < n_out) ? sg.wout[row * 64 + hidden_col(s, kq)] : 0.0f;
    }
    return 0.0f;
}

// ---- layer idioms.  The accumulators carry the layer's bias (or zero) on entry.
__device__ __forceinline__ float k_input(const float *x, int s) { return x[s]; }
__device__ __forceinline__ float k_input(const f32x4 *x, int s) { return x[s >> 2][s & 3]; }   // a chained D layout

// Dense layer over MT row tiles and S k-steps, k-steps outer, row tiles inner.  Quad image, MT = 4: img -> the layer's
// first quad of this lane.
template <int S, class X>
__device__ __forceinline__ void dense_layer(const f32x4 *img, const X *x, f32x4 h[4])
{
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const f32x4 w4 = img[s * 64];
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) h[mt] = mfma(w4[mt], k_input(x, s), h[mt]);
    }
}

// The same over a plain image: wl -> the layer's first tile of this lane.
template <int MT, int S, class X>
__device__ __forceinline__ void dense_layer(const float *wl, const X *x, f32x4 h[MT])
{
#pragma unroll
    for (int s = 0; s < S; ++s)
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) h[mt] = mfma(wl[(MT * s + mt) * 64], k_input(x, s), h[mt]);
}

// One 16-row tile from a 4S-wide chained input, with the k-steps split over two accumulators (two dependent chains of
// half the length).  Quad image, S = 16.
__device__ __forceinline__ f32x4 row_tile_layer(const f32x4 *img, const f32x4 h[4], f32x4 oa)
{
    f32x4 ob = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const f32x4 w4 = img[q * 64];
        oa = mfma(w4[0], h[q][0], oa);
        ob = mfma(w4[1], h[q][1], ob);
        oa = mfma(w4[2], h[q][2], oa);
        ob = mfma(w4[3], h[q][3], ob);
    }
    return oa + ob;
}

template <int MT>
__device__ __forceinline__ void relu(f32x4 h[MT])
{
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) h[mt][r] = fmaxf(h[mt][r], 0.0f);
}

// backward of relu: dz where the forward output h is positive, else 0
template <int MT>
__device__ __forceinline__ void relu_mask(f32x4 dz[MT], const f32x4 h[MT])
{
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int r = 0; r < 4; ++r) dz[mt][r] = h[mt][r] > 0.0f ? dz[mt][r] : 0.0f;
}

// ---- weight-gradient tiles of the training-side kernels (mlp_train.hip, field_train.hip)
// D layout (lane (g,p): rows 4g..4g+3 of column p) -> A/B layout (lane (i,kq): row i, columns 4s+kq for s = 0..3),
// through a 16 x 17 float scratch private to the wave.
__device__ __forceinline__ f32x4 to_operand(const f32x4 d, volatile float *scratch, int lane)
{
    const int g = lane >> 4, p = lane & 15;
#pragma unroll
    for (int r = 0; r < 4; ++r) scratch[(4 * g + r) * 17 + p] = d[r];
    __builtin_amdgcn_wave_barrier();
    f32x4 o;
#pragma unroll
    for (int s = 0; s < 4; ++s) o[s] = scratch[p * 17 + 4 * s + g];   // row i = p, column 4s + kq, kq = g
    __builtin_amdgcn_wave_barrier();
    return o;
}

// acc += dz^T-tile x a^T-tile over the 16 points of the group (4 k-steps of 4 points)
__device__ __forceinline__ f32x4 outer_acc(const f32x4 dz_op, const f32x4 a_op, f32x4 acc)
{
#pragma unroll
    for (int s = 0; s < 4; ++s) acc = mfma(dz_op[s], a_op[s], acc);
    return acc;
}

}  // namespace
