// The marching rule shared by grid_march.hip (whole rays) and volumetric.hip (capped rounds): the clipped box range of a
// ray and the occupancy of a sample midpoint.  One rule, stated once; every operation individually rounded so the oracle
// (oracle/occgrid.py) reproduces counts exactly.
#pragma once
#include "exact_common.h"

#pragma clang fp contract(off)

namespace {

struct MarchArgs {
    float lo[3], hi[3];
    int res[3];
    float near_plane, far_plane, step;
};

__device__ __forceinline__ bool march_range(const MarchArgs &m, const float *o, const float *d, float t_near_ray,
                                            float t_far_ray, float *t0, float *t1)
{
    float tn = -INFINITY, tf = INFINITY;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float inv = safe_inv(d[k]);
        const float a = (m.lo[k] - o[k]) * inv, b = (m.hi[k] - o[k]) * inv;
        tn = fmaxf(tn, fminf(a, b));
        tf = fminf(tf, fmaxf(a, b));
    }
    *t0 = fmaxf(tn, t_near_ray);
    *t1 = fminf(tf, t_far_ray);
    return tn <= tf && *t0 < *t1;
}

__device__ __forceinline__ bool march_occupied(const MarchArgs &m, const uint8_t *binaries, const float *o,
                                               const float *d, float tm)
{
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float p = o[k] + d[k] * tm;
        const float u = (p - m.lo[k]) / (m.hi[k] - m.lo[k]) * (float)m.res[k];
        const float f = floorf(u);
        if (!(f >= 0.0f && f < (float)m.res[k])) return false;
        c[k] = (int)f;
    }
    return binaries[((int64_t)c[0] * m.res[1] + c[1]) * m.res[2] + c[2]] != 0;
}

inline int fill_march_args(const float *aabb, const int32_t *res, float near_plane, float far_plane, float step, MarchArgs *m)
{
    if (!aabb || !res || !(step > 0.0f) || !(far_plane > near_plane)) return QF_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k) {
        m->lo[k] = aabb[k];
        m->hi[k] = aabb[3 + k];
        m->res[k] = res[k];
        if (!(aabb[3 + k] > aabb[k]) || res[k] < 1) return QF_ERR_INVALID_ARGUMENT;
        // bound the per-ray step count so the march loop always terminates quickly
        if ((aabb[3 + k] - aabb[k]) / step > 1.0e7f) return QF_ERR_UNSUPPORTED;
    }
    m->near_plane = near_plane;
    m->far_plane = far_plane;
    m->step = step;
    return QF_OK;
}

}  // namespace
