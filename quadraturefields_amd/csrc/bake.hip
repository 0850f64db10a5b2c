// Stage 6c, the bake of the SG field into the uint8 texture set (bake_texture_images_shelly.py:270-294), as a fixed
// launch sequence per band of rows of the texel-position map V [T, T, 3]:
//
//   1. qf_bake_compact_texels: the valid texels of the band -- (x + y) + z != 0 in fp32, in that order: numpy's
//      V.sum(-1) == 0, so (1, 1e8, -1e8) and (1, -1, 0) are EMPTY; the reference's quirk is restated, not repaired -- as
//      flat indices r * T + c in ascending order, their positions as contiguous [n, 3] rows (what the field kernels take,
//      no gather), the count as a device int64 and the band's part of the bool mask.  Deterministic: a count launch (one
//      int per workgroup), then an emit launch in which a workgroup adds the counts of the workgroups before it, a wave
//      the counts of the waves before it and a lane the set bits below it in the wave's ballot.  No atomic anywhere.
//   2. (the two field launches of the caller, bounded by the device count)
//   3. qf_bake_encode_texels: the codecs of FeatureCompression.compress (texture_utils.py:67-98, ngp.py:239-273) on one
//      feature row per texel, written into the 2 + 2L planes at that texel.  Every operation is ONE fp32 operation rounded
//      on its own (this file is compiled with -ffp-contract=off), python scalars rounded to fp32 first, in the reference's
//      order; uint8 conversion truncates toward zero and wraps mod 256 (an azimuth of exactly 256 becomes 0; the decoder
//      treats 0 and 255 as neighbours).  NaN features or densities are the caller's problem: their codes are unspecified.
#include <math.h>

#include "qf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kBakeThreads = 256;
constexpr int kBakeWaves = kBakeThreads / 64;
constexpr int kBakeWaveIters = 8;                                   // runs of 64 consecutive texels per wave
constexpr int kBakeWaveTexels = 64 * kBakeWaveIters;
constexpr int kBakeBlockTexels = kBakeWaves * kBakeWaveTexels;       // 2048 consecutive texels per workgroup

__device__ __forceinline__ bool texel_valid(const float *__restrict__ v, int64_t px, float *x, float *y, float *z)
{
    *x = v[px * 3];
    *y = v[px * 3 + 1];
    *z = v[px * 3 + 2];
    return ((*x + *y) + *z) != 0.0f;
}

// counts[b] = valid texels among the band's texels [b * 2048, (b + 1) * 2048)
__global__ __launch_bounds__(kBakeThreads) void bake_count_kernel(const float *__restrict__ v, int64_t first, int n,
                                                                  int32_t *__restrict__ counts)
{
    __shared__ int s_wave[kBakeWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int begin = blockIdx.x * kBakeBlockTexels + wave * kBakeWaveTexels;
    int cnt = 0;
#pragma unroll
    for (int it = 0; it < kBakeWaveIters; ++it) {
        const int i = begin + it * 64 + lane;
        float x, y, z;
        const bool ok = i < n && texel_valid(v, first + i, &x, &y, &z);
        cnt += __popcll(__ballot(ok));
    }
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) {
        int total = 0;
        for (int w = 0; w < kBakeWaves; ++w) total += s_wave[w];
        counts[blockIdx.x] = total;
    }
}

__global__ __launch_bounds__(kBakeThreads) void bake_emit_kernel(const float *__restrict__ v, int64_t first, int n,
                                                                 const int32_t *__restrict__ counts,
                                                                 int32_t *__restrict__ texel, float *__restrict__ positions,
                                                                 int64_t *__restrict__ count, uint8_t *__restrict__ mask)
{
    __shared__ int s_part[kBakeWaves];
    __shared__ int s_wave[kBakeWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    // workgroups before this one (a band has at most 2^28 / 2048 of them; in practice about a thousand)
    int before = 0;
    for (int b = threadIdx.x; b < (int)blockIdx.x; b += kBakeThreads) before += counts[b];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) before += __shfl_xor(before, off, 64);
    if (lane == 0) s_part[wave] = before;

    const int begin = blockIdx.x * kBakeBlockTexels + wave * kBakeWaveTexels;
    unsigned long long ballots[kBakeWaveIters];
    float x[kBakeWaveIters], y[kBakeWaveIters], z[kBakeWaveIters];
    int cnt = 0;
#pragma unroll
    for (int it = 0; it < kBakeWaveIters; ++it) {
        const int i = begin + it * 64 + lane;
        x[it] = y[it] = z[it] = 0.0f;
        const bool ok = i < n && texel_valid(v, first + i, &x[it], &y[it], &z[it]);
        if (mask && i < n) mask[first + i] = ok ? 1 : 0;
        ballots[it] = __ballot(ok);
        cnt += __popcll(ballots[it]);
    }
    if (lane == 0) s_wave[wave] = cnt;
    __syncthreads();
    int block_base = 0, own = 0, earlier_waves = 0;
    for (int w = 0; w < kBakeWaves; ++w) {
        block_base += s_part[w];
        if (w < wave) earlier_waves += s_wave[w];
        own += s_wave[w];
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *count = (int64_t)block_base + own;
    int base = block_base + earlier_waves;
    const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
    for (int it = 0; it < kBakeWaveIters; ++it) {
        if ((ballots[it] >> lane) & 1ull) {
            const int64_t o = (int64_t)base + __popcll(ballots[it] & below);
            texel[o] = (int32_t)(first + begin + it * 64 + lane);
            positions[o * 3] = x[it];
            positions[o * 3 + 1] = y[it];
            positions[o * 3 + 2] = z[it];
        }
        base += __popcll(ballots[it]);
    }
}

struct BakePlanes {
    uint8_t *alpha, *diffuse;
    uint8_t *colors[QF_MAX_LOBES];
    uint8_t *lam[QF_MAX_LOBES];
    int64_t texels;                          // T * T
    int n_lobes, sigmoid_codec;
    float lambda_thres;
};

// float -> uint8 as the reference's .to(torch.uint8): toward zero, then mod 256
__device__ __forceinline__ uint8_t u8(float f) { return (uint8_t)((int)f & 0xff); }

__device__ __forceinline__ uint8_t encode_color(float c, int sigmoid_codec)
{
    float q;
    if (sigmoid_codec) q = 1.0f / (1.0f + expf(-c));                                    // ngp.py:265-266
    else q = (fminf(fmaxf(c, -12.0f), 12.0f) + 12.0f) / 2.0f / 12.0f;                    // ngp.py:268 (B-7)
    return u8(q * 255.0f);
}

__global__ __launch_bounds__(kBakeThreads) void bake_encode_kernel(BakePlanes t, const float *__restrict__ features,
                                                                   int width, const float *__restrict__ sigma,
                                                                   const int32_t *__restrict__ texel, int64_t cap,
                                                                   const int64_t *__restrict__ n_dev)
{
    const int64_t nd = *n_dev;
    const int64_t n = nd < cap ? (nd > 0 ? nd : 0) : cap;
    const float pi = 3.14159274101257324f;   // float32(np.pi)
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t px = texel[i];
        if (px < 0 || px >= t.texels) continue;                                          // a list that is not this set's
        const float *f = features + i * width;
        const float a = 1.0f - expf(-sigma[i] * 0.005f);                                // texture_utils.py:51-55
        t.alpha[px] = u8(fminf(fmaxf(a * 255.0f, 0.0f), 255.0f));
        t.diffuse[px * 3 + 0] = encode_color(f[0], t.sigmoid_codec);
        t.diffuse[px * 3 + 1] = encode_color(f[1], t.sigmoid_codec);
        t.diffuse[px * 3 + 2] = encode_color(f[2], t.sigmoid_codec);
#pragma unroll
        for (int l = 0; l < QF_MAX_LOBES; ++l) {
            if (l < t.n_lobes) {                                                        // wave-uniform
                const float *o = f + 3 + 7 * l;
                const float ax = o[0], ay = o[1], az = o[2];
                const float d = sqrtf((ax * ax + ay * ay) + az * az) + 1e-6f;           // ngp.py:240
                const float vx = ax / d, vy = ay / d, vz = az / d;
                const float lg = logf(fmaxf(fabsf(o[3]), 1e-5f));                        // ngp.py:255
                const float lc = fminf(fmaxf((lg + 2.5f) / t.lambda_thres, 0.0f), 1.0f);
                uint8_t *lam = t.lam[l] + px * 3, *col = t.colors[l] + px * 3;
                lam[0] = u8(255.0f * lc);
                lam[1] = u8(atan2f(vy, vx) * 128.0f / pi + 128.0f);                     // ngp.py:241
                lam[2] = u8(acosf(vz) * 256.0f / pi);                                    // ngp.py:242
                col[0] = encode_color(o[4], t.sigmoid_codec);
                col[1] = encode_color(o[5], t.sigmoid_codec);
                col[2] = encode_color(o[6], t.sigmoid_codec);
            }
        }
    }
}

constexpr int kBakeMaxSide = 16384;          // T * T < 2^31: a flat texel index is an int32

}  // namespace

extern "C" int64_t qf_bake_compact_workspace_bytes(int64_t n_texels)
{
    if (n_texels < 1 || n_texels > (int64_t)kBakeMaxSide * kBakeMaxSide) return -1;
    return qf_div_up(n_texels, kBakeBlockTexels) * (int64_t)sizeof(int32_t);
}

extern "C" int qf_bake_compact_texels(const float *v, int32_t texture_size, int32_t row_begin, int32_t rows, int32_t *texel,
                                      float *positions, int64_t *count, uint8_t *mask, void *workspace,
                                      int64_t workspace_bytes, void *stream)
{
    if (texture_size < 1 || texture_size > kBakeMaxSide || row_begin < 0 || rows < 1 ||
        (int64_t)row_begin + rows > texture_size)
        return QF_ERR_INVALID_ARGUMENT;
    if (!v || !texel || !positions || !count || !workspace) return QF_ERR_INVALID_ARGUMENT;
    const int64_t n = (int64_t)rows * texture_size;
    if (workspace_bytes < qf_bake_compact_workspace_bytes(n)) return QF_ERR_INVALID_ARGUMENT;
    const int blocks = (int)qf_div_up(n, kBakeBlockTexels);
    const int64_t first = (int64_t)row_begin * texture_size;
    int32_t *counts = static_cast<int32_t *>(workspace);
    hipLaunchKernelGGL(bake_count_kernel, dim3(blocks), dim3(kBakeThreads), 0, qf_stream(stream), v, first, (int)n, counts);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(bake_emit_kernel, dim3(blocks), dim3(kBakeThreads), 0, qf_stream(stream), v, first, (int)n,
                       (const int32_t *)counts, texel, positions, count, mask);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_bake_encode_texels(const qf_texture_set *tex, const float *features, int32_t feature_width,
                                     const float *sigma, const int32_t *texel, int64_t capacity, const int64_t *n_device,
                                     void *stream)
{
    if (!tex || !tex->alpha || !tex->diffuse || tex->texture_size < 1 || tex->texture_size > kBakeMaxSide)
        return QF_ERR_INVALID_ARGUMENT;
    if (tex->n_lobes < 1 || tex->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (feature_width != 3 + 7 * tex->n_lobes + 1 || capacity < 0 ||
        capacity > (int64_t)tex->texture_size * tex->texture_size)
        return QF_ERR_INVALID_ARGUMENT;
    BakePlanes t;
    t.alpha = const_cast<uint8_t *>(tex->alpha);
    t.diffuse = const_cast<uint8_t *>(tex->diffuse);
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        t.colors[l] = l < tex->n_lobes ? const_cast<uint8_t *>(tex->colors[l]) : nullptr;
        t.lam[l] = l < tex->n_lobes ? const_cast<uint8_t *>(tex->lambda_axis[l]) : nullptr;
        if (l < tex->n_lobes && (!t.colors[l] || !t.lam[l])) return QF_ERR_INVALID_ARGUMENT;
    }
    t.texels = (int64_t)tex->texture_size * tex->texture_size;
    t.n_lobes = tex->n_lobes;
    t.sigmoid_codec = tex->sigmoid_codec;
    t.lambda_thres = tex->lambda_thres;
    if (capacity == 0) return QF_OK;
    if (!features || !sigma || !texel || !n_device) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(bake_encode_kernel, capacity, t, features, (int)feature_width, sigma, texel, capacity, n_device);
    return QF_OK;
}
