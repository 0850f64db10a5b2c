// What the deformation-field kernels share (deform_kernel in field_eval.hip, grid_extract_kernel in grid_extract.hip,
// deform_mlp_backward_kernel in mlp_train.hip): table row types, the fp16 rounding of a blended feature pair and the
// LDS weight image of the decoder.
#pragma once
#include "field_common.h"

typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));

namespace {

// Table row types of deform_kernel.  fp32 (float2 rows) is the default; fp16 is the reference's own precision
// (field.py:157-171 builds the tcnn Encoding with dtype=torch.float16 and returns its output as fp16, while x01 and the
// BasicDecoder stay fp32): half2 rows (low half = feature 0, 4 B gathers) converted to fp32 exactly (v_cvt_f32_f16),
// blended in fp32 by level_blend, and the 8 blended features rounded ONCE to fp16, round-to-nearest-even (overflow to
// +-inf, as torch's .half()), before they enter the fp32 MLP and enc_out.  fp16 denormals are kept: the kernel
// descriptor's float_denorm_mode_16_64 is 3 (flush nothing), as for field_kernel_16.
struct DeformRowF32 {
    typedef float2 row;
    static constexpr bool kRoundF16 = false;
    static __device__ __forceinline__ float2 unpack(float2 r) { return r; }
};

struct DeformRowF16 {
    typedef uint32_t row;
    static constexpr bool kRoundF16 = true;
    static __device__ __forceinline__ float2 unpack(uint32_t raw)
    {
        const f16x2 h = __builtin_bit_cast(f16x2, raw);
        return make_float2((float)h.x, (float)h.y);
    }
};

// fp32 -> fp16 (RNE) -> fp32 of a feature pair: v_cvt_pk_f16_f32 + 2 x v_cvt_f32_f16
__device__ __forceinline__ void round_f16_pair(float *f0, float *f1)
{
    const f16x2 h = {(_Float16)*f0, (_Float16)*f1};
    *f0 = (float)h.x;
    *f1 = (float)h.y;
}

// LDS weight image (plain: A operand tiles, [tile][lane]) of the decoder cat[x01(3), grid(32)] -> H -> H -> 1 for hidden
// width H: S = H/4 k-steps over a hidden layer, MT = H/16 row tiles.  Forward: layer 1 (9 MT), layer 2 (S MT), lout (S);
// then grid_extract_kernel's backward of the scalar output: W2^T (S MT), W1[:, 0:3]^T (S).
template <int H>
struct DeformImage {
    static constexpr int MT = H / 16, S = H / 4;
    static constexpr int L1 = 0, L2 = 9 * MT, LO = L2 + S * MT, L2T = LO + S, L1X = L2T + S * MT, N = L1X + S;
};

// A operand of forward MFMA m < L2T for lane `lane`.  k-steps of layer 1: 0..7 grid features of the lane's level
// quartet, step 8: lane quartets 0..2 feed x01.{x,y,z}, quartet 3 feeds the constant 1 that carries b1.
template <int H>
__device__ __forceinline__ float deform_fwd_weight(const float *w1, const float *b1, const float *w2, const float *wout,
                                                   int m, int lane)
{
    typedef DeformImage<H> I;
    const int i = lane & 15, kq = lane >> 4;
    if (m < I::L2) {                       // cat[grid(32), x01 | 1] -> H: s outer (9), mt inner
        const int s = m / I::MT, mt = m % I::MT, row = 16 * mt + i;
        if (s < 8) return w1[row * 35 + 3 + 2 * (4 * (s >> 1) + kq) + (s & 1)];
        return kq < 3 ? w1[row * 35 + kq] : b1[row];
    }
    if (m < I::LO) {                       // H -> H
        const int q = m - I::L2, s = q / I::MT, mt = q % I::MT;
        return w2[(16 * mt + i) * H + hidden_col(s, kq)];
    }
    const int s = m - I::LO;               // H -> 1 (row 0 of a 16-row tile)
    return i == 0 ? wout[hidden_col(s, kq)] : 0.0f;
}

}  // namespace
