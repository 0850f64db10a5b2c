// The tail of the reference's evaluation loops (train_finetune.py:620-667) on the device: INTER_AREA down-sample by an
// integer factor, MSE / PSNR, SSIM as torchmetrics' StructuralSimilarityIndexMeasure(data_range=1) computes it, the depth
// maximum, and the three uint8 images the scripts write.  Nothing here waits for the device: a frame's four numbers land
// in one slot of a device-resident table that the caller reads once, after the last frame.
//
//   1. frame_score_tile_kernel<F>: a workgroup owns a 32x16 tile of SSIM windows of ONE colour channel.  It box-averages
//      the (32+10) x (16+10) patch of the full-resolution render straight into LDS (the frame is never written back at full
//      resolution) next to the same patch of the ground truth, runs the 11-tap row pass into LDS and the column pass into
//      registers -- the five window moments in fp64, so E[x^2] - mu^2 does not cancel -- and reduces its SSIM sum, its
//      squared-error sum and its depth maximum in the wave and across the four waves.  A pixel's squared error (and its
//      down-sampled value, and its depth) belongs to the one tile that owns it, not to the tiles that hold it as halo.
//   2. frame_score_finalize_kernel: ONE workgroup adds the per-workgroup partial sums in a fixed order in fp64 and writes
//      the record (mse, psnr, ssim, depth_max).  No floating-point atomics anywhere: two calls on the same inputs give the
//      same bits whatever the scheduling.
//   3. frame_images_u8_kernel: rgb8, err8 and depth8 in one launch; depth_max is read from the record on the device.
#include <math.h>

#include "qf_common.h"

namespace {

constexpr int kFmThreads = 256;
constexpr int kFmTaps = 11, kFmHalo = kFmTaps - 1;
constexpr int kFmTileW = 32, kFmTileH = 16;                                  // SSIM windows per workgroup
constexpr int kFmPatchW = kFmTileW + kFmHalo, kFmPatchH = kFmTileH + kFmHalo;  // pixels they read
constexpr int kFmRows = kFmTileH / (kFmThreads / kFmTileW);                  // windows per thread in the column pass
constexpr int kFmPartial = 3;                                                // doubles per workgroup in the scratch array
static_assert(kFmTileW == 32 && kFmRows * (kFmThreads / kFmTileW) == kFmTileH, "thread -> window mapping");

struct FmWeights {
    double g[kFmTaps];
};

// f x f block summed in fp32 in row-major order, multiplied once by 1/f^2 (exact for f = 1, 2, 4)
template <int F>
__device__ __forceinline__ float box_average(const float *__restrict__ src, int64_t row_stride, int stride)
{
    float s = src[0];
#pragma unroll
    for (int dy = 0; dy < F; ++dy)
#pragma unroll
        for (int dx = 0; dx < F; ++dx)
            if (dy | dx) s += src[dy * row_stride + dx * stride];
    return F == 1 ? s : s * (1.0f / (float)(F * F));
}

// sum (or maximum) over the workgroup in a fixed order: butterfly in the wave, then the waves in index order
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double *s_wave)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double o = __shfl_xor(v, off, 64);
        v = MAX ? fmax(v, o) : v + o;
    }
    if ((threadIdx.x & 63) == 0) s_wave[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = s_wave[0];
    for (int w = 1; w < kFmThreads / 64; ++w) r = MAX ? fmax(r, s_wave[w]) : r + s_wave[w];
    __syncthreads();
    return r;
}

template <int F>
__global__ __launch_bounds__(kFmThreads) void frame_score_tile_kernel(const float *__restrict__ rgb, const float *__restrict__ depth,
                                                                      const float *__restrict__ pixels, int H, int W, FmWeights wts,
                                                                      float *__restrict__ rgb_small, float *__restrict__ depth_small,
                                                                      float *__restrict__ ssim_map, double *__restrict__ partial)
{
    __shared__ float s_p[kFmPatchH * kFmPatchW], s_t[kFmPatchH * kFmPatchW];
    __shared__ double s_row[5][kFmPatchH][kFmTileW];
    __shared__ double s_wave[kFmThreads / 64];
    const int c = blockIdx.z, x0 = blockIdx.x * kFmTileW, y0 = blockIdx.y * kFmTileH;
    // the pixels this tile owns: its 32x16 corner, and the halo too where no tile follows
    const int own_w = blockIdx.x + 1 == gridDim.x ? kFmPatchW : kFmTileW;
    const int own_h = blockIdx.y + 1 == gridDim.y ? kFmPatchH : kFmTileH;
    const int64_t fw = (int64_t)W * F;
    double se = 0.0, dmax = -INFINITY;
    for (int i = threadIdx.x; i < kFmPatchH * kFmPatchW; i += kFmThreads) {
        const int ly = i / kFmPatchW, lx = i - ly * kFmPatchW;
        const int y = y0 + ly, x = x0 + lx;
        float p = 0.0f, t = 0.0f;
        if (y < H && x < W) {
            p = box_average<F>(rgb + ((int64_t)y * F * fw + (int64_t)x * F) * 3 + c, fw * 3, 3);
            t = pixels[((int64_t)y * W + x) * 3 + c];
            if (lx < own_w && ly < own_h) {
                if (rgb_small) rgb_small[((int64_t)y * W + x) * 3 + c] = p;
                const double d = (double)p - (double)t;
                se += d * d;
                if (c == 0 && depth) {
                    const float dv = box_average<F>(depth + (int64_t)y * F * fw + (int64_t)x * F, fw, 1);
                    if (depth_small) depth_small[(int64_t)y * W + x] = dv;
                    dmax = fmax(dmax, (double)dv);
                }
            }
        }
        s_p[i] = p;
        s_t[i] = t;
    }
    __syncthreads();
    const double *g = wts.g;
    // row pass: mu_p, mu_t, E[p^2], E[t^2], E[pt] along x for every patch row
    for (int i = threadIdx.x; i < kFmPatchH * kFmTileW; i += kFmThreads) {
        const int ly = i / kFmTileW, ox = i - ly * kFmTileW;
        const float *pp = s_p + ly * kFmPatchW + ox, *tp = s_t + ly * kFmPatchW + ox;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, a4 = 0.0;
#pragma unroll
        for (int k = 0; k < kFmTaps; ++k) {
            const double p = (double)pp[k], t = (double)tp[k];
            a0 = fma(g[k], p, a0);
            a1 = fma(g[k], t, a1);
            a2 = fma(g[k], p * p, a2);
            a3 = fma(g[k], t * t, a3);
            a4 = fma(g[k], p * t, a4);
        }
        s_row[0][ly][ox] = a0;
        s_row[1][ly][ox] = a1;
        s_row[2][ly][ox] = a2;
        s_row[3][ly][ox] = a3;
        s_row[4][ly][ox] = a4;
    }
    __syncthreads();
    // column pass: thread (ox, grp) owns kFmRows consecutive windows of one column and slides down their rows
    const int ox = threadIdx.x & (kFmTileW - 1), r0 = (threadIdx.x / kFmTileW) * kFmRows;
    double acc[kFmRows][5];
#pragma unroll
    for (int j = 0; j < kFmRows; ++j)
#pragma unroll
        for (int q = 0; q < 5; ++q) acc[j][q] = 0.0;
#pragma unroll
    for (int r = 0; r < kFmRows + kFmHalo; ++r) {
        double v[5];
#pragma unroll
        for (int q = 0; q < 5; ++q) v[q] = s_row[q][r0 + r][ox];
#pragma unroll
        for (int j = 0; j < kFmRows; ++j) {
            const int k = r - j;
            if (k >= 0 && k < kFmTaps) {
#pragma unroll
                for (int q = 0; q < 5; ++q) acc[j][q] = fma(g[k], v[q], acc[j][q]);
            }
        }
    }
    const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
    double ss = 0.0;
#pragma unroll
    for (int j = 0; j < kFmRows; ++j) {
        const int oy = y0 + r0 + j, gx = x0 + ox;
        if (oy < H - kFmHalo && gx < W - kFmHalo) {
            const double mp = acc[j][0], mt = acc[j][1];
            const double spp = acc[j][2] - mp * mp, stt = acc[j][3] - mt * mt, spt = acc[j][4] - mp * mt;
            const double s = ((2.0 * mp * mt + c1) * (2.0 * spt + c2)) / ((mp * mp + mt * mt + c1) * (spp + stt + c2));
            // the frame's SSIM is the mean of the values AS RETURNED in the fp32 map, whether or not the map is asked for
            const float sf = (float)s;
            if (ssim_map) ssim_map[((int64_t)oy * (W - kFmHalo) + gx) * 3 + c] = sf;
            ss += (double)sf;
        }
    }
    ss = block_reduce<false>(ss, s_wave);
    se = block_reduce<false>(se, s_wave);
    dmax = block_reduce<true>(dmax, s_wave);
    if (threadIdx.x == 0) {
        double *out = partial + ((int64_t)(blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * kFmPartial;
        out[0] = ss;
        out[1] = se;
        out[2] = dmax;
    }
}

// every thread adds a contiguous run of the partial sums in index order, then the fixed-order workgroup reduction
__global__ __launch_bounds__(kFmThreads) void frame_score_finalize_kernel(const double *__restrict__ partial, int n_blocks,
                                                                          double n_ssim, double n_mse, int has_depth,
                                                                          double *__restrict__ record)
{
    __shared__ double s_wave[kFmThreads / 64];
    const int per = (n_blocks + kFmThreads - 1) / kFmThreads;
    const int i0 = threadIdx.x * per, i1 = i0 + per < n_blocks ? i0 + per : n_blocks;
    double ss = 0.0, se = 0.0, dmax = -INFINITY;
    for (int i = i0; i < i1; ++i) {
        ss += partial[(int64_t)i * kFmPartial];
        se += partial[(int64_t)i * kFmPartial + 1];
        dmax = fmax(dmax, partial[(int64_t)i * kFmPartial + 2]);
    }
    ss = block_reduce<false>(ss, s_wave);
    se = block_reduce<false>(se, s_wave);
    dmax = block_reduce<true>(dmax, s_wave);
    if (threadIdx.x == 0) {
        const double mse = se / n_mse;
        record[0] = mse;
        record[1] = mse == 0.0 ? INFINITY : -10.0 * log10(mse);
        record[2] = ss / n_ssim;
        record[3] = has_depth ? dmax : 0.0;
    }
}

// uint8 by truncation, as numpy's astype(np.uint8) does; every value is one multiply (or one correctly rounded divide and
// one multiply) away from its input, so the bytes equal the torch expressions on the same inputs
__device__ __forceinline__ uint8_t to_u8(float v) { return (uint8_t)(int32_t)v; }
__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

__global__ __launch_bounds__(256) void frame_images_u8_kernel(const float *__restrict__ rgb_small, const float *__restrict__ pixels,
                                                              const float *__restrict__ depth_small, const double *__restrict__ record,
                                                              int64_t n_pixels, uint8_t *__restrict__ rgb8, uint8_t *__restrict__ err8,
                                                              uint8_t *__restrict__ depth8)
{
    const float depth_max = depth_small ? (float)record[3] : 0.0f;
    const int64_t step = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < 3 * n_pixels; i += step) {
        const float v = clamp01(rgb_small[i]);
        if (rgb8) rgb8[i] = to_u8(v * 255.0f);
        if (err8) err8[i] = to_u8(clamp01(fabsf(v - pixels[i])) * 255.0f);
        // a frame without a hit has depth_max 0: a zero image instead of the reference's division by zero
        if (depth8 && i < n_pixels) depth8[i] = depth_max > 0.0f ? to_u8(depth_small[i] / depth_max * 255.0f) : (uint8_t)0;
    }
}

int64_t fm_blocks(int32_t height, int32_t width)
{
    return qf_div_up(width - kFmHalo, kFmTileW) * qf_div_up(height - kFmHalo, kFmTileH) * 3;
}

}  // namespace

extern "C" int64_t qf_frame_score_scratch_bytes(int32_t height, int32_t width)
{
    if (height < kFmTaps || width < kFmTaps || (int64_t)height * width >= 0x7fffffff / 48) return -1;
    return fm_blocks(height, width) * kFmPartial * (int64_t)sizeof(double);
}

extern "C" int qf_frame_score(const float *rgb, int32_t rgb_height, int32_t rgb_width, const float *depth, const float *pixels,
                              int32_t height, int32_t width, int32_t factor, float *rgb_small, float *depth_small,
                              float *ssim_map, double *table, int64_t slot, int64_t capacity, void *scratch,
                              int64_t scratch_bytes, void *stream)
{
    if (factor < 1 || factor > 4) return QF_ERR_INVALID_ARGUMENT;
    const int64_t need = qf_frame_score_scratch_bytes(height, width);
    if (need < 0 || (int64_t)rgb_height != (int64_t)factor * height || (int64_t)rgb_width != (int64_t)factor * width)
        return QF_ERR_INVALID_ARGUMENT;
    if (!rgb || !pixels || !table || !scratch || scratch_bytes < need) return QF_ERR_INVALID_ARGUMENT;
    if (slot < 0 || slot >= capacity || (depth_small && !depth)) return QF_ERR_INVALID_ARGUMENT;
    // torchmetrics' _gaussian(11, 1.5): exp(-(d / sigma)^2 / 2) normalised to sum 1 -- in fp64.  Built in fp32, as
    // torchmetrics builds them for fp32 images, the weights add up to 1 + 4e-8 in the fp64 moments, and that alone moves
    // sigma^2 = E[x^2] - mu^2 of a flat window by 1e-8 against c2 = 9e-4: 8e-6 in the SSIM of constant images (measured).
    FmWeights wts;
    double sum = 0.0;
    for (int k = 0; k < kFmTaps; ++k) {
        const double d = (double)(k - kFmTaps / 2) / 1.5;
        wts.g[k] = exp(-(d * d) / 2.0);
        sum += wts.g[k];
    }
    for (int k = 0; k < kFmTaps; ++k) wts.g[k] /= sum;
    const dim3 grid((unsigned)qf_div_up(width - kFmHalo, kFmTileW), (unsigned)qf_div_up(height - kFmHalo, kFmTileH), 3);
    double *partial = reinterpret_cast<double *>(scratch);
    hipStream_t st = qf_stream(stream);
#define QF_FM_LAUNCH(F)                                                                                                      \
    hipLaunchKernelGGL(frame_score_tile_kernel<F>, grid, dim3(kFmThreads), 0, st, rgb, depth, pixels, (int)height, (int)width, \
                       wts, rgb_small, depth_small, ssim_map, partial)
    switch (factor) {
    case 1: QF_FM_LAUNCH(1); break;
    case 2: QF_FM_LAUNCH(2); break;
    case 3: QF_FM_LAUNCH(3); break;
    default: QF_FM_LAUNCH(4); break;
    }
#undef QF_FM_LAUNCH
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(frame_score_finalize_kernel, dim3(1), dim3(kFmThreads), 0, st, partial, (int)fm_blocks(height, width),
                       3.0 * (double)(height - kFmHalo) * (double)(width - kFmHalo), 3.0 * (double)height * (double)width,
                       depth ? 1 : 0, table + slot * 4);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_frame_images_u8(const float *rgb_small, const float *pixels, const float *depth_small, const double *record,
                                  int32_t height, int32_t width, uint8_t *rgb8, uint8_t *err8, uint8_t *depth8, void *stream)
{
    if (height < 1 || width < 1 || !rgb_small || (err8 && !pixels) || (depth8 && (!depth_small || !record)))
        return QF_ERR_INVALID_ARGUMENT;
    if (!rgb8 && !err8 && !depth8) return QF_OK;
    const int64_t n_pixels = (int64_t)height * width;
    QF_SIMPLE_LAUNCH(frame_images_u8_kernel, 3 * n_pixels, rgb_small, pixels, depth8 ? depth_small : (const float *)nullptr, record,
                     n_pixels, rgb8, err8, depth8);
    return QF_OK;
}
