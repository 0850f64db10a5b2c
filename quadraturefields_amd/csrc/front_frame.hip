// The field-evaluated frame, front to back with early ray termination.  The batched field kernel
// cannot decide per sample whether a pixel still sees anything, so the frame is evaluated in RANK WINDOWS: window j covers
// the ranks [b_{j-1}, b_j) of every pixel, and only the pixels that still see something at rank b_{j-1} have their
// samples of that window evaluated.  Per window the kernels below
//   1. composite the previous window's samples into a per-pixel RayAccum that lives in a [n_rays] state array between
//      the launches, apply the rule at rank b_{j-1} and count the live samples of window j per tile and per group of
//      16 tiles (front_accumulate_kernel<false>),
//   2. write the window list in (tile, rank, pixel) order (front_write_kernel): the slots of the live samples, which the
//      field kernel takes as its `order` argument, so that its outputs land in place in rgb_c / sigma_c.  The layout is
//      deterministic -- counts, their scan, a write -- and the scan rides in this launch: a workgroup sums the group counts
//      in front of it and scans its own tiles' counts.  The window's sample total is left in a device int64 -- the field
//      launch's n_device.
// After the last window's field launch front_accumulate_kernel<true> composites that window, blends and writes the image.
// No launch count or grid size depends on data and nothing waits for the host.
//
// The rule is baked_frame.hip's: the rank-k sample of a pixel (k < count) contributes iff the optical depth accumulated
// before it satisfies cum <= stop_tau, cum being the fp32 value composite_step keeps; a pixel that has stopped stays
// stopped; stop_tau = +inf never stops.  The compositor applies it PER SAMPLE, whatever the windows are: a sample that was
// evaluated but lies behind the stop adds nothing, so the pixels do not depend on the schedule.  A pixel is selected for
// window j by the same test on the same state the compositor will see at rank b_{j-1}, so every sample the compositor
// reads has been evaluated.  One wave per 8x8 tile, lane = pixel; source slots are located with ballots over count > k
// (they depend on the counts alone), positions in the window list with ballots over live && count > k.
#include "qf_common.h"
#include "composite_device.h"

namespace {

constexpr int kTileWaves = 16;             // tiles per workgroup: a GROUP of tiles, the unit of the window list's layout
constexpr int kMaxGroups = QF_FRONT_MAX_TILES / kTileWaves;
constexpr uint32_t kLive = 1u << 30;       // state word 7: selected for the window being evaluated
constexpr uint32_t kStopped = 1u << 29;    //               a sample of the pixel has failed the rule
constexpr uint32_t kCountMask = (1u << 29) - 1u;

// state: two float4 per ray = cum cr cg cb | cd ca shaded(int) flags+evaluated(int)
__device__ __forceinline__ void state_load(const float4 *__restrict__ state, int64_t ray, RayAccum &a, int &shaded,
                                           int &evaluated, bool &stopped)
{
    const float4 s0 = state[ray * 2], s1 = state[ray * 2 + 1];
    a.cum = s0.x; a.cr = s0.y; a.cg = s0.z; a.cb = s0.w;
    a.cd = s1.x; a.ca = s1.y;
    shaded = __float_as_int(s1.z);
    const uint32_t f = __float_as_uint(s1.w);
    evaluated = (int)(f & kCountMask);
    stopped = (f & kStopped) != 0u;
}

__device__ __forceinline__ void state_store(float4 *__restrict__ state, int64_t ray, const RayAccum &a, int shaded,
                                            int evaluated, bool stopped, bool live)
{
    const uint32_t f = (uint32_t)evaluated | (stopped ? kStopped : 0u) | (live ? kLive : 0u);
    state[ray * 2] = make_float4(a.cum, a.cr, a.cg, a.cb);
    state[ray * 2 + 1] = make_float4(a.cd, a.ca, __int_as_float(shaded), __uint_as_float(f));
}

// first slot of rank `rank` in the tile whose rank-0 run starts at `base`: the runs of the ranks below it are as long as
// the ballots over count > k say (wave-uniform)
__device__ __forceinline__ int64_t skip_ranks(int64_t base, int cnt, int rank)
{
    for (int k = 0; k < rank; ++k) {
        const unsigned long long m = __ballot(cnt > k);
        if (m == 0ull) break;
        base += __popcll(m);
    }
    return base;
}

// Composites the ranks [lo, mid) of every pixel on top of its state (first: there is none yet), then
//   FINISH = false: selects the pixels that enter the window [mid, hi), counts the samples in it per tile (win_count) and
//                   per workgroup (group_count) and stores the state;
//   FINISH = true : blends, writes the image and the two counts (composite_tiles_kernel's epilogue).
// composite_tiles_kernel's walk: the loads of step k+1 are issued before the arithmetic of step k; they are asked for the
// lanes that had not stopped by then, what contributes is decided by the rule alone.
template <bool FINISH>
__global__ __launch_bounds__(64 * kTileWaves) void front_accumulate_kernel(
    const float *__restrict__ rgb_c, const float *__restrict__ sigma_c, const float *__restrict__ depth_c, float delta_const,
    const int32_t *__restrict__ hit_count, int max_hits, const int64_t *__restrict__ tile_base, int w, int h, int tiles_x,
    int n_tiles, float stop_tau, int first, int lo, int mid, int hi, float4 *__restrict__ state,
    int32_t *__restrict__ win_count, int32_t *__restrict__ group_count, int bg_mode, const float *__restrict__ bkgd, float *__restrict__ out_rgb,
    float *__restrict__ out_alpha, float *__restrict__ out_depth, float *__restrict__ out_packed,
    int32_t *__restrict__ shaded_count, int32_t *__restrict__ evaluated_count)
{
    const int lane = threadIdx.x & 63, tile = blockIdx.x * kTileWaves + (threadIdx.x >> 6);
    // a wave beyond the last tile has no pixel inside the image: it loads and stores nothing, but it stays for the select's
    // barrier
    if (FINISH && tile >= n_tiles) return;            // wave-uniform
    int64_t ray = 0;
    int cnt = 0;
    const int inside = tile < n_tiles && qf_tile_lane_ray(tile, lane, w, h, tiles_x, 0, &ray);
    if (inside) cnt = hit_count[ray] < max_hits ? hit_count[ray] : max_hits;
    RayAccum acc;
    int shaded = 0, evaluated = 0;
    bool stopped = false;
    if (!first && inside) state_load(state, ray, acc, shaded, evaluated, stopped);
    const bool never = stop_tau == INFINITY;
    const unsigned long long below = (1ull << lane) - 1ull;
    unsigned long long mask = lo < mid ? __ballot(cnt > lo) : 0ull;
    if (mask != 0ull) {                               // wave-uniform
        int64_t base = skip_ranks(tile_base[tile], cnt, lo);
        int64_t pos = base + __popcll(mask & below);
        float sg = 0.0f, r = 0.0f, g = 0.0f, b = 0.0f, dep = 0.0f;
        if (cnt > lo && !stopped) { sg = sigma_c[pos]; r = rgb_c[pos * 3]; g = rgb_c[pos * 3 + 1]; b = rgb_c[pos * 3 + 2]; dep = depth_c[pos]; }
        for (int k = lo; mask != 0ull; ++k) {
            base += __popcll(mask);
            const unsigned long long next = k + 1 < mid ? __ballot(cnt > k + 1) : 0ull;
            pos = base + __popcll(next & below);
            float nsg = 0.0f, nr = 0.0f, ng = 0.0f, nb = 0.0f, ndep = 0.0f;
            if (k + 1 < mid && cnt > k + 1 && !stopped) {
                nsg = sigma_c[pos]; nr = rgb_c[pos * 3]; ng = rgb_c[pos * 3 + 1]; nb = rgb_c[pos * 3 + 2]; ndep = depth_c[pos];
            }
            if (cnt > k && !stopped) {
                if (never || acc.cum <= stop_tau) {
                    const float tau = sample_tau(sg, delta_const);
                    composite_step(acc, tau, sample_alpha(tau), r, g, b, dep);
                    ++shaded;
                } else {
                    stopped = true;
                }
            }
            mask = next; sg = nsg; r = nr; g = ng; b = nb; dep = ndep;
        }
    }
    if (!FINISH) {
        // the rule at rank mid, on the state the compositor will find there
        const bool live = cnt > mid && !stopped && (never || acc.cum <= stop_tau);
        if (cnt > mid && !live) stopped = true;
        if (live) evaluated = cnt < hi ? cnt : hi;
        __shared__ int s_live[kTileWaves];
        int n_live = 0;
        for (int k = mid; k < hi; ++k) {
            const unsigned long long m = __ballot(live && cnt > k);
            if (m == 0ull) break;
            n_live += __popcll(m);
        }
        if (lane == 0) {
            s_live[threadIdx.x >> 6] = n_live;
            if (tile < n_tiles) win_count[tile] = n_live;
        }
        if (inside) state_store(state, ray, acc, shaded, evaluated, stopped, live);
        __syncthreads();                               // the only barrier: every wave of the workgroup reaches it
        if (threadIdx.x == 0) {
            int sum = 0;
#pragma unroll
            for (int q = 0; q < kTileWaves; ++q) sum += s_live[q];
            group_count[blockIdx.x] = sum;
        }
        return;
    }
    if (!inside) return;
    float px[3];
    if (cnt > 0) {
        composite_blend(acc, bg_mode, bkgd, px);
    } else {                                           // fill_background_kernel's values
        px[0] = px[1] = px[2] = (bg_mode == QF_BG_BLACK || bg_mode == QF_BG_NONE) ? 0.0f : 1.0f;
    }
    if (shaded_count) shaded_count[ray] = shaded;
    if (evaluated_count) evaluated_count[ray] = evaluated;
    if (out_packed) {                  // [n, 5] = rgb | alpha | depth per pixel, as composite_tiles_kernel
        float *o = out_packed + ray * 5;
        o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; o[3] = acc.ca; o[4] = acc.cd;
        return;
    }
    out_rgb[ray * 3 + 0] = px[0];
    out_rgb[ray * 3 + 1] = px[1];
    out_rgb[ray * 3 + 2] = px[2];
    out_alpha[ray] = acc.ca;
    out_depth[ray] = acc.cd;
}

// The window list: order[...] = slot, for the samples of the ranks [mid, hi) of the live pixels, in (tile, rank, pixel)
// order.  A workgroup finds its own place in the list: the samples of the groups in front of it (group_count, summed by
// the whole workgroup), then those of its tiles in front of each tile (a 16-lane scan of the group's tile counts) -- the
// scan over the tiles without a launch of its own (a one-workgroup scan kernel between the two launches took 9.4 us per
// window on an 800 x 800 frame).  The last workgroup leaves the window's total in *win_total.  The cost of the first step
// grows with the square of the group count, which is why the entry points stop at kMaxGroups.
// capacity = the slots of the frame's arrays: nothing outside [0, capacity) is written or named.
__global__ __launch_bounds__(64 * kTileWaves) void front_write_kernel(
    const int32_t *__restrict__ hit_count, int max_hits, const int64_t *__restrict__ tile_base, int w, int h, int tiles_x,
    int n_tiles, int mid, int hi, const float4 *__restrict__ state, const int32_t *__restrict__ win_count,
    const int32_t *__restrict__ group_count, int64_t *__restrict__ win_total, int32_t *__restrict__ order, int64_t capacity)
{
    __shared__ int64_t s_part[kTileWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, group = blockIdx.x;
    const int tile = group * kTileWaves + wave;
    int64_t before = 0;
    for (int g = threadIdx.x; g < group; g += 64 * kTileWaves) before += group_count[g];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if (lane == 0) s_part[wave] = before;
    __syncthreads();                                   // the only barrier: every wave of the workgroup reaches it
    int64_t dst = 0;
#pragma unroll
    for (int q = 0; q < kTileWaves; ++q) dst += s_part[q];
    const int c = (lane < kTileWaves && group * kTileWaves + lane < n_tiles) ? win_count[group * kTileWaves + lane] : 0;
    int incl = c;
#pragma unroll
    for (int off = 1; off < kTileWaves; off <<= 1) {
        const int o = __shfl_up(incl, off, 64);
        if (lane >= off) incl += o;
    }
    const int all = __shfl(incl, kTileWaves - 1, 64);
    if (group == (int)gridDim.x - 1 && threadIdx.x == 0) *win_total = dst + all;
    dst += __shfl(incl - c, wave, 64);
    if (tile >= n_tiles) return;                      // wave-uniform
    int64_t ray = 0;
    int cnt = 0;
    bool live = false;
    if (qf_tile_lane_ray(tile, lane, w, h, tiles_x, 0, &ray)) {
        cnt = hit_count[ray] < max_hits ? hit_count[ray] : max_hits;
        live = (__float_as_uint(state[ray * 2 + 1].w) & kLive) != 0u;
    }
    if (__ballot(live) == 0ull) return;               // wave-uniform: the tile has nothing in this window
    const unsigned long long below = (1ull << lane) - 1ull;
    int64_t base = skip_ranks(tile_base[tile], cnt, mid);
    for (int k = mid; k < hi; ++k) {
        const unsigned long long has = __ballot(cnt > k), go = __ballot(live && cnt > k);
        if (go == 0ull) break;
        if (live && cnt > k) {
            const int64_t d = dst + __popcll(go & below), p = base + __popcll(has & below);
            if (d >= 0 && d < capacity && p >= 0 && p < capacity) order[d] = (int32_t)p;
        }
        base += __popcll(has);
        dst += __popcll(go);
    }
}

bool front_frame_ok(const float *rgb_c, const float *sigma_c, const float *depth_c, const int32_t *hit_count, int32_t max_hits,
                    const int64_t *tile_base, int32_t width, int32_t height, float stop_tau, const float *state)
{
    if (width < 1 || height < 1 || max_hits < 1 || (int64_t)width * height >= 0x7fffffff) return false;
    if ((int64_t)((width + 7) / 8) * ((height + 7) / 8) > QF_FRONT_MAX_TILES) return false;
    if (!rgb_c || !sigma_c || !depth_c || !hit_count || !tile_base || !state) return false;
    if (reinterpret_cast<uintptr_t>(state) % 16 != 0) return false;
    return stop_tau >= 0.0f;                           // NaN or negative: refused
}

}  // namespace

extern "C" int qf_front_select(const float *rgb_c, const float *sigma_c, const float *depth_c, float delta_const,
                               const int32_t *hit_count, int32_t max_hits, const int64_t *tile_base, int32_t width,
                               int32_t height, float stop_tau, int32_t rank_lo, int32_t rank_mid, int32_t rank_hi, float *state,
                               int32_t *win_count, int64_t *win_total, int32_t *win_order, int64_t capacity, void *stream)
{
    if (!front_frame_ok(rgb_c, sigma_c, depth_c, hit_count, max_hits, tile_base, width, height, stop_tau, state))
        return QF_ERR_INVALID_ARGUMENT;
    if (rank_lo < 0 || rank_lo > rank_mid || rank_mid >= rank_hi || (rank_mid == 0) != (rank_lo == rank_mid))
        return QF_ERR_INVALID_ARGUMENT;
    if (!win_count || !win_total || !win_order || capacity < 0 || capacity > 0x7fffffff) return QF_ERR_INVALID_ARGUMENT;
    const int tiles_x = (width + 7) / 8, n_tiles = tiles_x * ((height + 7) / 8);
    const int n_groups = (int)qf_div_up(n_tiles, kTileWaves);
    static_assert(kMaxGroups * kTileWaves == QF_FRONT_MAX_TILES, "whole groups");
    const dim3 grid((unsigned)n_groups), block(64 * kTileWaves);
    int32_t *group_count = win_count + n_tiles;
    hipStream_t st = qf_stream(stream);
    hipLaunchKernelGGL(front_accumulate_kernel<false>, grid, block, 0, st, rgb_c, sigma_c, depth_c, delta_const, hit_count,
                       (int)max_hits, tile_base, (int)width, (int)height, tiles_x, n_tiles, stop_tau, rank_mid == 0 ? 1 : 0,
                       (int)rank_lo, (int)rank_mid, (int)rank_hi, reinterpret_cast<float4 *>(state), win_count, group_count,
                       0, (const float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr, (float *)nullptr,
                       (int32_t *)nullptr, (int32_t *)nullptr);
    hipLaunchKernelGGL(front_write_kernel, grid, block, 0, st, hit_count, (int)max_hits, tile_base, (int)width, (int)height,
                       tiles_x, n_tiles, (int)rank_mid, (int)rank_hi, reinterpret_cast<const float4 *>(state), win_count,
                       group_count, win_total, win_order, capacity);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_front_finish(const float *rgb_c, const float *sigma_c, const float *depth_c, float delta_const,
                               const int32_t *hit_count, int32_t max_hits, const int64_t *tile_base, int32_t width,
                               int32_t height, float stop_tau, int32_t rank_lo, int32_t rank_hi, float *state, int32_t bg_mode,
                               const float *bkgd, float *out_rgb, float *out_alpha, float *out_depth, float *out_packed,
                               int32_t *shaded_count, int32_t *evaluated_count, void *stream)
{
    if (!front_frame_ok(rgb_c, sigma_c, depth_c, hit_count, max_hits, tile_base, width, height, stop_tau, state))
        return QF_ERR_INVALID_ARGUMENT;
    if (rank_lo < 0 || rank_lo >= rank_hi || bg_mode < 0 || bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!out_packed && (!out_rgb || !out_alpha || !out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (bg_mode == QF_BG_CUSTOM && !bkgd) return QF_ERR_INVALID_ARGUMENT;
    const int tiles_x = (width + 7) / 8, n_tiles = tiles_x * ((height + 7) / 8);
    hipLaunchKernelGGL(front_accumulate_kernel<true>, dim3((unsigned)qf_div_up(n_tiles, kTileWaves)), dim3(64 * kTileWaves), 0,
                       qf_stream(stream), rgb_c, sigma_c, depth_c, delta_const, hit_count, (int)max_hits, tile_base, (int)width,
                       (int)height, tiles_x, n_tiles, stop_tau, 0 /* the select launch of this window wrote the state */,
                       (int)rank_lo, (int)rank_hi, (int)rank_hi,
                       reinterpret_cast<float4 *>(state), (int32_t *)nullptr, (int32_t *)nullptr, (int)bg_mode, bkgd, out_rgb, out_alpha, out_depth,
                       out_packed, shaded_count, evaluated_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
