// Occupancy-grid ray marching (nerfacc 0.5.3 OccGridEstimator.sampling -> traverse_grids, one
// level, cone_angle = 0).  nerfacc walks the cells with a DDA but keeps the step phase through empty cells, so its
// samples are [t0 + k dt, t0 + (k+1) dt] with t0 the clipped aabb entry, kept iff the sample's MIDPOINT lies before
// the aabb exit and in an occupied cell.  That rule is evaluated directly here (one byte of grid per step, the
// 2 MiB grid is L2 resident), with every operation individually rounded so the oracle reproduces counts exactly.
#include "grid_march_common.h"

#pragma clang fp contract(off)

namespace {

// count != nullptr: pass 1 (count per ray); else pass 2 (write at offsets)
__global__ void grid_march_kernel(MarchArgs m, const uint8_t *binaries, const float *rays_o, const float *rays_d,
                                  const float *t_min, const float *t_max, int64_t n_rays, int32_t *count,
                                  const int64_t *offsets, float *t_starts, float *t_ends, int64_t *ray_indices)
{
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rays; r += (int64_t)gridDim.x * blockDim.x) {
        const float o[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
        const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
        const float near_r = t_min ? fmaxf(m.near_plane, t_min[r]) : m.near_plane;
        const float far_r = t_max ? fminf(m.far_plane, t_max[r]) : m.far_plane;
        float t0, t1;
        int n = 0;
        int64_t w = count ? 0 : offsets[r];
        if (march_range(m, o, d, near_r, far_r, &t0, &t1)) {
            for (int k = 0; k < (1 << 22); ++k) {      // hard cap: a degenerate ray can never spin
                const float ts = t0 + (float)k * m.step;
                const float te = t0 + (float)(k + 1) * m.step;
                const float tm = (ts + te) * 0.5f;
                if (!(tm < t1)) break;
                if (!march_occupied(m, binaries, o, d, tm)) continue;
                if (!count) { t_starts[w] = ts; t_ends[w] = te; ray_indices[w] = r; ++w; }
                ++n;
            }
        }
        if (count) count[r] = n;
    }
}

}  // namespace

extern "C" int qf_grid_march_count(const float *aabb, const int32_t *resolution, const uint8_t *binaries,
                                   const float *rays_o, const float *rays_d, const float *t_min, const float *t_max,
                                   int64_t n_rays, float near_plane, float far_plane, float step, int32_t *count,
                                   void *stream)
{
    MarchArgs m;
    int rc = fill_march_args(aabb, resolution, near_plane, far_plane, step, &m);
    if (rc != QF_OK) return rc;
    if (n_rays < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays == 0) return QF_OK;
    if (!binaries || !rays_o || !rays_d || !count) return QF_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(grid_march_kernel, dim3(qf_grid_1d(n_rays, 64, 64)), dim3(64), 0, qf_stream(stream), m, binaries,
                       rays_o, rays_d, t_min, t_max, n_rays, count, (const int64_t *)nullptr, (float *)nullptr,
                       (float *)nullptr, (int64_t *)nullptr);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_grid_march_write(const float *aabb, const int32_t *resolution, const uint8_t *binaries,
                                   const float *rays_o, const float *rays_d, const float *t_min, const float *t_max,
                                   int64_t n_rays, float near_plane, float far_plane, float step, const int64_t *offsets,
                                   float *t_starts, float *t_ends, int64_t *ray_indices, void *stream)
{
    MarchArgs m;
    int rc = fill_march_args(aabb, resolution, near_plane, far_plane, step, &m);
    if (rc != QF_OK) return rc;
    if (n_rays < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays == 0) return QF_OK;
    if (!binaries || !rays_o || !rays_d || !offsets) return QF_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(grid_march_kernel, dim3(qf_grid_1d(n_rays, 64, 64)), dim3(64), 0, qf_stream(stream), m, binaries,
                       rays_o, rays_d, t_min, t_max, n_rays, (int32_t *)nullptr, offsets, t_starts, t_ends, ray_indices);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
