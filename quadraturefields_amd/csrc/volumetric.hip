// Test-time volumetric renderer with early ray termination (examples/utils.py:176-350 of the reference,
// render_image_with_occgrid_test).  The frame is rendered in ROUNDS: every ray that is still
// alive marches at most n_samples = clamp(n_rays / n_alive, 1, 64) kept samples onward from its own near plane, the field
// is evaluated on exactly those, and one launch composites them onto the per-ray state and decides who stays alive.
//
//   march_round_kernel<false>   count per ray + termination plane            (qf_grid_march_round_count)
//   (the caller's inclusive scan of the counts)
//   march_round_kernel<true>    t_starts / t_ends / ray_indices and the xyz / dirs rows the field reads
//                                                                            (qf_grid_march_round_write)
//   (the field)
//   volumetric_accumulate_kernel  per-ray update, next n_alive, sample totals (qf_volumetric_accumulate)
//
// The marching rule is grid_march.hip's (grid_march_common.h), so a round's samples are bit-exact against the numpy
// restatement.  n_samples never crosses the host: every kernel derives it from the device-side n_alive of the previous
// round, state[parity]; the accumulate launch counts the survivors into state[1 - parity], which the count launch of the
// same round has zeroed.  Kernel boundaries order all of it, there is no hand-off inside a launch.
#include "grid_march_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kRoundCap = 64;          // the reference's cap on samples per ray and round

__device__ __forceinline__ int round_quota(const int64_t *state, int parity, int64_t n_rays)
{
    const int64_t alive = state[parity];
    if (alive <= 0) return 1;
    const int64_t q = n_rays / alive;
    return (int)(q < 1 ? 1 : (q > kRoundCap ? kRoundCap : q));
}

// kWrite = false: count[r] and term[r] of every ray; kWrite = true: the samples, at csum[r] - count[r]
template <bool kWrite>
__global__ __launch_bounds__(64) void march_round_kernel(MarchArgs m, const uint8_t *__restrict__ binaries,
                                                         const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                         const float *__restrict__ near, const uint8_t *__restrict__ alive,
                                                         int64_t n_rays, int64_t *state, int parity, int32_t *count,
                                                         float *term, const int64_t *__restrict__ csum, int64_t capacity,
                                                         float *t_starts, float *t_ends, int64_t *ray_indices, float *xyz,
                                                         float *dirs)
{
    const int quota = round_quota(state, parity, n_rays);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (kWrite) {
            state[QF_VOLUMETRIC_ROUND_SAMPLES] = csum[n_rays - 1];
        } else {
            state[1 - parity] = 0;                         // the survivors of this round are counted into it
            state[QF_VOLUMETRIC_ROUND_QUOTA] = quota;
        }
    }
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n_rays; r += (int64_t)gridDim.x * blockDim.x) {
        if (!alive[r]) {                                   // a dead ray emits nothing; its near plane stays
            if (!kWrite) count[r] = 0;
            continue;
        }
        const int want = kWrite ? count[r] : quota;
        if (kWrite && want == 0) continue;
        const float o[3] = {rays_o[r * 3], rays_o[r * 3 + 1], rays_o[r * 3 + 2]};
        const float d[3] = {rays_d[r * 3], rays_d[r * 3 + 1], rays_d[r * 3 + 2]};
        float t0, t1, last_end = 0.0f;
        int n = 0;
        int64_t w = kWrite ? csum[r] - want : 0;
        if (march_range(m, o, d, near[r], m.far_plane, &t0, &t1)) {
            for (int k = 0; k < (1 << 22); ++k) {          // hard cap: a degenerate ray can never spin
                const float ts = t0 + (float)k * m.step;
                const float te = t0 + (float)(k + 1) * m.step;
                const float tm = (ts + te) * 0.5f;
                if (!(tm < t1)) break;
                if (!march_occupied(m, binaries, o, d, tm)) continue;
                if (kWrite && w >= 0 && w < capacity) {    // capacity: a state block that disagrees with `alive` cannot overrun
                    t_starts[w] = ts;
                    t_ends[w] = te;
                    ray_indices[w] = r;
                    const float s = ts + te;
#pragma unroll
                    for (int c = 0; c < 3; ++c) {
                        xyz[w * 3 + c] = o[c] + (d[c] * s) / 2.0f;
                        dirs[w * 3 + c] = d[c];
                    }
                }
                ++w;
                last_end = te;
                if (++n == want) break;
            }
        }
        if (!kWrite) {
            count[r] = n;
            term[r] = n == quota ? last_end : t1;          // out of box: the clipped exit
        }
    }
}

// One lane per ray, walking the ray's packed run of the round.  alpha and T as render_from_density_kernel computes them
// (composite.hip), T scaled by the prefix transmittance 1 - opacity[ray]; the alpha filter drops contributions, never
// attenuation.  One atomic per wave and counter.
__global__ __launch_bounds__(256) void volumetric_accumulate_kernel(
    const float *__restrict__ t_starts, const float *__restrict__ t_ends, const float *__restrict__ sigmas,
    const float *__restrict__ rgbs, const int32_t *__restrict__ count, const int64_t *__restrict__ csum,
    const float *__restrict__ term, int64_t n_rays, int64_t capacity, float alpha_thre, float opc_thre, int64_t *state,
    int parity, float *rgb, float *opacity, float *depth, float *near, uint8_t *alive)
{
    const int quota = round_quota(state, parity, n_rays);
    const int lane = threadIdx.x & 63;
    // block-uniform trip count: the ballot below sees whole waves
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n_rays; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = base + threadIdx.x;
        bool live = false;
        int kept = 0;
        if (r < n_rays && alive[r]) {
            const int cnt = count[r];
            const int64_t b = csum[r] - cnt;
            float ca = opacity[r];
            const float prefix = 1.0f - ca;
            float cum = 0.0f, cr = 0.0f, cg = 0.0f, cb = 0.0f, cd = 0.0f, cw = 0.0f;
            if (b >= 0 && b + cnt <= capacity) {
                for (int64_t j = b; j < b + cnt; ++j) {
                    const float ts = t_starts[j], te = t_ends[j];
                    const float sdt = sigmas[j] * (te - ts);
                    const float al = 1.0f - expf(-sdt);
                    const float T = prefix * expf(-cum);
                    const float w = T * al;
                    cum += sdt;
                    if (alpha_thre > 0.0f && al < alpha_thre) continue;
                    cr += w * rgbs[j * 3 + 0];
                    cg += w * rgbs[j * 3 + 1];
                    cb += w * rgbs[j * 3 + 2];
                    cd += w * ((ts + te) / 2.0f);
                    cw += w;
                    ++kept;
                }
            }
            ca += cw;
            rgb[r * 3 + 0] += cr;
            rgb[r * 3 + 1] += cg;
            rgb[r * 3 + 2] += cb;
            depth[r] += cd;
            opacity[r] = ca;
            near[r] = term[r];
            live = ca <= opc_thre && cnt == quota;
            alive[r] = live ? 1 : 0;
        }
        const unsigned long long mask = __ballot(live);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) kept += __shfl_xor(kept, off, 64);
        if (lane == 0) {
            if (mask) atomicAdd(reinterpret_cast<unsigned long long *>(state + (1 - parity)), (unsigned long long)__popcll(mask));
            if (kept) atomicAdd(reinterpret_cast<unsigned long long *>(state + QF_VOLUMETRIC_TOTAL_SAMPLES), (unsigned long long)kept);
        }
    }
}

__global__ __launch_bounds__(256) void mark_visited_kernel(const float *__restrict__ p01, int64_t n, int M, uint8_t *mask,
                                                           int64_t *out_of_range)
{
    const float s = (float)(M - 1);
    const int lane = threadIdx.x & 63;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += (int64_t)gridDim.x * blockDim.x) {
        const int64_t i = base + threadIdx.x;
        bool outside = false;
        if (i < n) {
            const float p[3] = {p01[i * 3], p01[i * 3 + 1], p01[i * 3 + 2]};
            outside = !(p[0] >= 0.0f && p[0] <= 1.0f && p[1] >= 0.0f && p[1] <= 1.0f && p[2] >= 0.0f && p[2] <= 1.0f);
            if (!outside) {
                int64_t lo = 0, hi = 0;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const float u = p[c] * s;              // in [0, M - 1]: both cells exist
                    const int f = min((int)floorf(u), M - 1), g = min((int)ceilf(u), M - 1);
                    lo = lo * M + f;
                    hi = hi * M + g;
                }
                mask[lo] = 1;
                mask[hi] = 1;
            }
        }
        const unsigned long long bad = __ballot(outside);
        if (lane == 0 && bad && out_of_range)
            atomicAdd(reinterpret_cast<unsigned long long *>(out_of_range), (unsigned long long)__popcll(bad));
    }
}

int check_round(const float *aabb, const int32_t *resolution, float near_plane, float far_plane, float step, int64_t n_rays,
                int32_t parity, const void *const *required, int n_required, MarchArgs *m)
{
    const int rc = fill_march_args(aabb, resolution, near_plane, far_plane, step, m);
    if (rc != QF_OK) return rc;
    if (n_rays < 1 || n_rays >= 0x7fffffff || (parity != 0 && parity != 1)) return QF_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < n_required; ++k)
        if (!required[k]) return QF_ERR_INVALID_ARGUMENT;
    return QF_OK;
}

}  // namespace

extern "C" int qf_grid_march_round_count(const float *aabb, const int32_t *resolution, const uint8_t *binaries,
                                         const float *rays_o, const float *rays_d, const float *near,
                                         const uint8_t *alive, int64_t n_rays, float near_plane, float far_plane,
                                         float step, int64_t *state, int32_t parity, int32_t *count, float *term,
                                         void *stream)
{
    MarchArgs m;
    const void *required[] = {binaries, rays_o, rays_d, near, alive, state, count, term};
    const int rc = check_round(aabb, resolution, near_plane, far_plane, step, n_rays, parity, required, 8, &m);
    if (rc != QF_OK) return rc;
    hipLaunchKernelGGL(march_round_kernel<false>, dim3(qf_grid_1d(n_rays, 64, 64)), dim3(64), 0, qf_stream(stream), m,
                       binaries, rays_o, rays_d, near, alive, n_rays, state, (int)parity, count, term,
                       (const int64_t *)nullptr, (int64_t)0, (float *)nullptr, (float *)nullptr, (int64_t *)nullptr,
                       (float *)nullptr, (float *)nullptr);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_grid_march_round_write(const float *aabb, const int32_t *resolution, const uint8_t *binaries,
                                         const float *rays_o, const float *rays_d, const float *near,
                                         const uint8_t *alive, int64_t n_rays, float near_plane, float far_plane,
                                         float step, int64_t *state, int32_t parity, const int32_t *count,
                                         const int64_t *csum, int64_t capacity, float *t_starts, float *t_ends,
                                         int64_t *ray_indices, float *xyz, float *dirs, void *stream)
{
    MarchArgs m;
    const void *required[] = {binaries, rays_o, rays_d, near, alive, state, count, csum, t_starts, t_ends, ray_indices,
                              xyz, dirs};
    const int rc = check_round(aabb, resolution, near_plane, far_plane, step, n_rays, parity, required, 13, &m);
    if (rc != QF_OK) return rc;
    if (capacity < 1) return QF_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(march_round_kernel<true>, dim3(qf_grid_1d(n_rays, 64, 64)), dim3(64), 0, qf_stream(stream), m,
                       binaries, rays_o, rays_d, near, alive, n_rays, state, (int)parity, const_cast<int32_t *>(count),
                       (float *)nullptr, csum, capacity, t_starts, t_ends, ray_indices, xyz, dirs);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_volumetric_accumulate(const float *t_starts, const float *t_ends, const float *sigmas,
                                        const float *rgbs, const int32_t *count, const int64_t *csum, const float *term,
                                        int64_t n_rays, int64_t capacity, float alpha_thre, double early_stop_eps,
                                        int64_t *state, int32_t parity, float *rgb, float *opacity, float *depth,
                                        float *near, uint8_t *alive, void *stream)
{
    if (n_rays < 1 || n_rays >= 0x7fffffff || capacity < 1 || (parity != 0 && parity != 1)) return QF_ERR_INVALID_ARGUMENT;
    if (!(alpha_thre >= 0.0f) || !(early_stop_eps >= 0.0 && early_stop_eps <= 1.0)) return QF_ERR_INVALID_ARGUMENT;
    if (!t_starts || !t_ends || !sigmas || !rgbs || !count || !csum || !term || !state || !rgb || !opacity || !depth ||
        !near || !alive)
        return QF_ERR_INVALID_ARGUMENT;
    const float opc_thre = (float)(1.0 - early_stop_eps);       // the reference's double, compared in fp32
    QF_SIMPLE_LAUNCH(volumetric_accumulate_kernel, n_rays, t_starts, t_ends, sigmas, rgbs, count, csum, term, n_rays,
                     capacity, alpha_thre, opc_thre, state, (int)parity, rgb, opacity, depth, near, alive);
    return QF_OK;
}

extern "C" int qf_mark_visited_cells(const float *p01, int64_t n, int32_t m, uint8_t *mask, int64_t *out_of_range,
                                     void *stream)
{
    if (n < 0 || m < 1 || m > 1024) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!p01 || !mask) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(mark_visited_kernel, n, p01, n, (int)m, mask, out_of_range);
    return QF_OK;
}
