// Distortion loss of packed ray samples and its gradient in ONE launch: for a ray with
// samples i = 0..c-1 in stored order, weights w, positions m, lengths d,
//     L_ray = sum_i sum_{j<i} 2 w_i w_j (m_i - m_j) + (1/3) sum_i w_i^2 d_i,       loss = (sum_rays L_ray) / n_rays,
//     dloss/dw_k = [ 2 ( m_k (P_k - S_k) + (SM_k - PM_k) ) + (2/3) w_k d_k ] / n_rays
// with P / PM the exclusive prefix sums of w / w m along the ray and S / SM the exclusive suffix sums.  The sum is
// ORDERED (no absolute value): it is the Mip-NeRF-360 loss exactly when m is nondecreasing along the ray.
//
// Mapping: a fixed grid of waves strides over batches of kDlBatch consecutive rays.  A wave finds the first sample of
// its batch with a 64-ary search of the sorted ray ids (every lane probes one position, a ballot narrows the range 64
// times per step), then each ray's end with the same search in a window behind its start -- the next ray starts where
// this one ended.  A ray is swept in 64-sample chunks with a carried prefix: one sweep for the totals (skipped when the
// ray is one chunk: the totals are the scan's last lane), one for the scans, the loss terms and the gradient stores.
// All loads and stores are coalesced.  Scans, totals and the loss are fp64 (m P - PM cancels in fp32); the gradient is
// rounded once, at its store.  The loss is reduced in a fixed order: one partial per workgroup in the workspace, summed
// by the workgroup that draws the last ticket (an integer atomic; it puts the ticket back to 0).
#include "qf_common.h"

namespace {

constexpr int kDlThreads = 256;
constexpr int kDlWaves = kDlThreads / 64;
constexpr int kDlBatch = 4;               // consecutive rays per wave turn: one full search per batch
constexpr int64_t kDlWindow = 4096;       // the end of a ray is searched in this many samples behind its start first
constexpr int kDlMaxBlocks = 2048;        // partials of the workspace: (QF_DISTORTION_WORKSPACE_BYTES - 16) / 8

static_assert(16 + kDlMaxBlocks * 8 == QF_DISTORTION_WORKSPACE_BYTES, "workspace layout");

// first index in [lo, hi) whose id is >= key (hi if none); ids nondecreasing; wave-uniform arguments and result
__device__ __forceinline__ int64_t wave_lower_bound(const int64_t *__restrict__ ids, int64_t lo, int64_t hi, int64_t key,
                                                    int lane)
{
    while (lo < hi) {
        const int64_t step = (hi - lo + 63) >> 6;
        const int64_t idx = lo + (int64_t)lane * step;
        const bool below = idx < hi && ids[idx] < key;
        const int c = __popcll(__ballot(below));          // the probes are monotone: lanes 0..c-1 are below
        if (c == 0) return lo;
        const int64_t nhi = lo + (int64_t)c * step;
        lo = lo + (int64_t)(c - 1) * step + 1;
        hi = nhi < hi ? nhi : hi;
    }
    return lo;
}

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// one ray [start, end), end > start: returns this lane's share of L_ray, stores the gradient entries
__device__ __forceinline__ double ray_sweep(const float *__restrict__ w, const float *__restrict__ m,
                                            const float *__restrict__ interval, float interval_const, int64_t start,
                                            int64_t end, double inv_n, float *__restrict__ grad_w, int lane)
{
    const bool single = end - start <= 64;
    double tw = 0.0, twm = 0.0;
    if (!single) {
        for (int64_t i = start + lane; i < end; i += 64) {
            const double wi = (double)w[i];
            tw += wi;
            twm += wi * (double)m[i];
        }
        tw = wave_sum(tw);
        twm = wave_sum(twm);
    }
    double cp = 0.0, cpm = 0.0, loss = 0.0;
    for (int64_t c0 = start; c0 < end; c0 += 64) {
        const int64_t i = c0 + lane;
        const bool on = i < end;
        const double wi = on ? (double)w[i] : 0.0;
        const double mi = on ? (double)m[i] : 0.0;
        const double di = on ? (double)(interval ? interval[i] : interval_const) : 0.0;
        const double wm = wi * mi;
        double iw = wi, iwm = wm;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const double a = __shfl_up(iw, off, 64), b = __shfl_up(iwm, off, 64);
            if (lane >= off) { iw += a; iwm += b; }
        }
        const double cw = __shfl(iw, 63, 64), cwm = __shfl(iwm, 63, 64);
        if (single) { tw = cw; twm = cwm; }
        const double p = cp + (iw - wi), pm = cpm + (iwm - wm);
        const double s = tw - p - wi, sm = twm - pm - wm;
        loss += 2.0 * wi * (mi * p - pm) + (1.0 / 3.0) * wi * wi * di;
        if (grad_w && on) grad_w[i] = (float)((2.0 * (mi * (p - s) + (sm - pm)) + (2.0 / 3.0) * wi * di) * inv_n);
        cp += cw;
        cpm += cwm;
    }
    return loss;
}

__global__ __launch_bounds__(kDlThreads) void distortion_kernel(const float *__restrict__ w, const float *__restrict__ m,
                                                                const float *__restrict__ interval, float interval_const,
                                                                const int64_t *__restrict__ ray_id, int64_t uniform_count,
                                                                int64_t n, int64_t n_rays_arg, float *__restrict__ loss_out,
                                                                float *__restrict__ grad_w,
                                                                unsigned long long *__restrict__ partial,
                                                                unsigned int *__restrict__ ticket)
{
    __shared__ double s_part[kDlThreads];
    __shared__ int s_last;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // the rays that hold samples end at ray_id[n-1]; a larger n_rays only changes the scale
    const int64_t n_have = ray_id ? ray_id[n - 1] + 1 : n / uniform_count;
    const int64_t n_scale = n_rays_arg > 0 ? n_rays_arg : n_have;
    const double inv_n = n_scale > 0 ? 1.0 / (double)n_scale : 0.0;
    const int64_t n_waves = (int64_t)gridDim.x * kDlWaves;
    double acc = 0.0;
    for (int64_t r0 = ((int64_t)blockIdx.x * kDlWaves + wave) * kDlBatch; r0 < n_have; r0 += n_waves * kDlBatch) {
        int64_t start = ray_id ? wave_lower_bound(ray_id, 0, n, r0, lane) : r0 * uniform_count;
        if (start >= n) break;                 // every later ray is empty too
        for (int b = 0; b < kDlBatch && r0 + b < n_have && start < n; ++b) {
            int64_t end = start + uniform_count;
            if (ray_id) {
                const int64_t hi = start + kDlWindow < n ? start + kDlWindow : n;
                end = wave_lower_bound(ray_id, start, hi, r0 + b + 1, lane);
                if (end == hi && hi < n) end = wave_lower_bound(ray_id, hi, n, r0 + b + 1, lane);
            }
            if (end > start) acc += ray_sweep(w, m, interval, interval_const, start, end, inv_n, grad_w, lane);
            start = end;
        }
    }
    acc = wave_sum(acc);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int q = 0; q < kDlWaves; ++q) s += s_part[q];
        __hip_atomic_store(&partial[blockIdx.x], (unsigned long long)__double_as_longlong(s), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        s_last = atomicAdd(ticket, 1u) == gridDim.x - 1u;
    }
    __syncthreads();
    if (!s_last) return;
    __threadfence();
    double s = 0.0;
    for (unsigned i = threadIdx.x; i < gridDim.x; i += kDlThreads)
        s += __longlong_as_double((long long)__hip_atomic_load(&partial[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    s_part[threadIdx.x] = s;
    __syncthreads();
    for (int half = kDlThreads / 2; half > 0; half >>= 1) {
        if ((int)threadIdx.x < half) s_part[threadIdx.x] += s_part[threadIdx.x + half];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        *loss_out = (float)(s_part[0] * inv_n);
        __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
    }
}

}  // namespace

extern "C" int qf_distortion_loss(const float *w, const float *m, const float *interval, float interval_const,
                                  const int64_t *ray_id, int64_t uniform_count, int64_t n, int64_t n_rays, float *loss_out,
                                  float *grad_w, void *workspace, void *stream)
{
    if (n < 0 || n_rays < 0 || !loss_out || !workspace) return QF_ERR_INVALID_ARGUMENT;
    if ((ray_id != nullptr) == (uniform_count > 0) && n > 0) return QF_ERR_INVALID_ARGUMENT;      // exactly one of the two
    if (!ray_id && n > 0 && (uniform_count <= 0 || n % uniform_count != 0)) return QF_ERR_INVALID_ARGUMENT;
    if (n > 0 && (!w || !m)) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    if (n == 0) {
        QF_HIP_TRY(hipMemsetAsync(loss_out, 0, sizeof(float), st));
        return QF_OK;
    }
    int64_t blocks = qf_div_up(n, kDlThreads);
    if (blocks > kDlMaxBlocks) blocks = kDlMaxBlocks;
    unsigned int *ticket = reinterpret_cast<unsigned int *>(workspace);
    unsigned long long *partial = reinterpret_cast<unsigned long long *>(reinterpret_cast<char *>(workspace) + 16);
    hipLaunchKernelGGL(distortion_kernel, dim3((unsigned)blocks), dim3(kDlThreads), 0, st, w, m, interval, interval_const,
                       ray_id, ray_id ? (int64_t)0 : uniform_count, n, n_rays, loss_out, grad_w, partial, ticket);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
