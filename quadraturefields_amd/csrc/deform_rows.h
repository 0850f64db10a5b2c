// Table row types of the deformation-field kernels (deform_kernel in field_eval.hip, grid_extract_kernel in
// grid_extract.hip) and the fp16 rounding of a blended feature pair.
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

}  // namespace
