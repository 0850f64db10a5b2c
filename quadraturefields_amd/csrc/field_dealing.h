// How the fused field kernels (field_kernel, deform_kernel, field_kernel_16, grid_extract_kernel) share out their
// 16-point groups: the host's workgroup count and each wave's run of groups.  Pure integer arithmetic, host and device,
// so that a host test can enumerate which wave visits which group.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define QF_DEAL_FN __host__ __device__ __forceinline__
#else
#define QF_DEAL_FN inline
#endif

// Groups grp = begin, begin + stride, ... < end belong to one wave.
struct QfGroupRange {
    int64_t begin, end, stride;
};

// Workgroups of a launch over n_groups groups.  ONE workgroup per CU: the kernels are bound by the fabric's
// sector-request rate, not by latency hiding (measured on the bench frame with 8-wave workgroups, 4 / 6 / 8 / 10 / 12 /
// 16 waves per CU -> 2.17 / 1.54 / 1.39 / 1.60 / 1.52 / 1.53 ms: fewer points in flight per XCD = a smaller L2 working
// set; below 8 waves the gathers no longer cover the latency).  From 64 workgroups on, a multiple of 8, which is what
// selects the XCD-contiguous route of qf_group_range.
QF_DEAL_FN int64_t qf_field_blocks(int64_t n_groups, int waves_per_block, int cu_count)
{
    int64_t blocks = (n_groups + waves_per_block - 1) / waves_per_block;
    if (blocks > cu_count) blocks = cu_count;
    if (blocks >= 64) blocks &= ~(int64_t)7;
    return blocks;
}

// The groups of wave `wave` of workgroup `block` in a grid of `grid` workgroups of waves_per_block waves.
// Workgroups are dealt round-robin to the 8 XCDs, each with its own L2.  When the grid is a multiple of 8, every XCD
// gets one CONTIGUOUS eighth of the (spatially coherent) processing order instead of every eighth chunk of it: an L2
// then only sees the table rows of its own slab of the scene, which is what lets the mid-resolution levels stay
// resident.  Any other grid: the waves stride over all groups.
QF_DEAL_FN QfGroupRange qf_group_range(int64_t n_groups, uint32_t grid, uint32_t block, int wave, int waves_per_block)
{
    QfGroupRange r;
    if ((grid & 7) == 0) {
        const int64_t per_xcd = (n_groups + 7) >> 3;
        r.begin = (int64_t)(block & 7) * per_xcd;
        r.end = r.begin + per_xcd < n_groups ? r.begin + per_xcd : n_groups;
        r.begin += (int64_t)(block >> 3) * waves_per_block + wave;
        r.stride = (int64_t)(grid >> 3) * waves_per_block;
    } else {
        r.begin = (int64_t)block * waves_per_block + wave;
        r.end = n_groups;
        r.stride = (int64_t)grid * waves_per_block;
    }
    return r;
}

// A point count that lives in device memory (a render-only frame's sample count is data dependent, qf_tile_offsets'
// total: no host wait between the tile pack and the field kernel), clamped to the capacity n of the arrays.
QF_DEAL_FN int64_t qf_clamp_count(int64_t n_dev, int64_t n) { return n_dev < n ? (n_dev > 0 ? n_dev : 0) : n; }
