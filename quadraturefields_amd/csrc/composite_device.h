// The per-ray compositing arithmetic of derive_properties as device functions, shared by the compositors of composite.hip
// and the fused baked-frame kernel (baked_frame.hip): one definition, hence the same bits wherever a ray is composited.
#pragma once
#include "qf_common.h"

namespace {

// The per-ray arithmetic of derive_properties with every rounding fixed, so that the chunked kernel, its long-ray tail
// and the tile kernel give the same bits whatever the optimiser does around them: tau = sigma * delta;
// w = exp(-cum) * (1 - exp(-tau)); cum += tau; the sums accumulate with one fma each.  (`#pragma clang fp contract(off)`
// inside the bodies: HIP's __fmul_rn / __fadd_rn are plain operators, which the default -ffp-contract=fast may still
// fuse with their neighbours after inlining; the fmas that are wanted are written as __builtin_fmaf.)
struct RayAccum {
    float cum = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f, cd = 0.0f, ca = 0.0f;
};

__device__ __forceinline__ float sample_tau(float sigma, float delta)
{
#pragma clang fp contract(off)
    return sigma * delta;
}

__device__ __forceinline__ float sample_alpha(float tau)
{
#pragma clang fp contract(off)
    return 1.0f - expf(-tau);
}

__device__ __forceinline__ float composite_step(RayAccum &a, float tau, float alpha, float r, float g, float b, float dep)
{
#pragma clang fp contract(off)
    const float w = expf(-a.cum) * alpha;
    a.cum = a.cum + tau;
    a.cr = __builtin_fmaf(w, r, a.cr);
    a.cg = __builtin_fmaf(w, g, a.cg);
    a.cb = __builtin_fmaf(w, b, a.cb);
    a.cd = __builtin_fmaf(w, dep, a.cd);
    a.ca = a.ca + w;
    return w;
}

__device__ __forceinline__ void composite_blend(const RayAccum &a, int bg_mode, const float *bkgd, float out[3])
{
#pragma clang fp contract(off)
    const float c[3] = {a.cr, a.cg, a.cb};
    const float rest = 1.0f - a.ca;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        if (bg_mode == QF_BG_WHITE) out[i] = __builtin_fmaf(a.ca, c[i], rest);      // (1 - a) + a * sum(w c): the double-alpha quirk (B-1)
        else if (bg_mode == QF_BG_BLACK) out[i] = a.ca * c[i];
        else if (bg_mode == QF_BG_NONE) out[i] = c[i];     // the plain sums (nerfacc's accumulate_along_rays): no blend, no quirk
        else {
            const float back = rest * bkgd[i];
            out[i] = __builtin_fmaf(a.ca, c[i], back);
        }
    }
}

}  // namespace
