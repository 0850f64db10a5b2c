// Fused field evaluation for gfx950: multi-resolution hash-grid gather + tiny MLPs on the
// fp32 matrix cores + SH / spherical-Gaussian head, one launch per batch of quadrature points.
//
// Replaces: tcnn GridEncoding + FullyFusedMLP + SphericalHarmonics behind
// NGPRadianceField.forward (examples/radiance_fields/ngp.py:757-809) and the BasicDecoder + SG
// mixture behind NGPRadianceFieldSGNew.forward / features (ngp.py:371-470).
//
// Mapping (DESIGN.md "field kernel"):
//   * a wave handles 16 points per pass; lane l = (p = l & 15, g = l >> 4): point p of the group,
//     level quartet g.  Lane (g,p) gathers levels {g, 4+g, 8+g, 12+g} of point p: 4 levels x 8
//     corners x float2 = 32 independent 8-byte loads in flight per lane.
//   * every layer is computed transposed, H^T[neuron][point] = W . X^T, with
//     v_mfma_f32_16x16x4_f32 (exact fp32, = fmaf chain).  W tiles are the A operand (staged once
//     per workgroup into LDS, already in per-lane operand order), X^T is the B operand.  The
//     16x16x4 C/D layout puts D[4g+r][p] in register r of lane (g,p), i.e. each lane ends up with
//     four neurons of ITS OWN point -- exactly the B operand of the next layer's k-step, so
//     activations never leave registers between layers (no LDS, no shuffles).  The k order of each
//     layer is permuted to match; the permutation is folded into the LDS weight image.
//   * workgroup = 8 waves, persistent: grid = CUs, waves stride over the 16-point groups of their XCD's share.
#include "mlp_tiles.h"
#include "deform_rows.h"

namespace {

constexpr int kBlock = 512;          // 8 waves

struct FieldArgs {
    GridArgs grid;
    float aabb_lo[3];
    float aabb_hi[3];
    const float2 *table;
    const float *base_w;
    const float *head_w;   // NGP head
    qf_sg_head sg;         // SG head
    const float *xyz;
    const float *dirs;
    int64_t n;
    const int64_t *n_dev;  // optional: the point count lives in device memory (min(*n_dev, n) points are processed)
    float *rgb;
    float *sigma;
    float *geo;
    float *features;
    float *raw16;       // optional [n,16]: raw base-MLP outputs (tcnn NetworkWithInputEncoding.forward)
    float *enc_out;     // optional [n,32]: the hash-grid encoding, kept for the training step's backward
    const int32_t *order;   // optional [n]: point processed at slot i
    int32_t n_lobes;
    int32_t n_out;      // 3 + 7L
    int32_t nt_out;     // ceil(n_out / 16)
};

template <int HEAD>
__device__ float weight_for(const FieldArgs &a, int m, int lane)
{
    return field_image_weight<HEAD>(a.base_w, a.head_w, a.sg, a.n_out, m, lane);
}

template <int HEAD>
__device__ __forceinline__ int n_mfma(const FieldArgs &a)
{
    if (HEAD == QF_HEAD_NGP) return kBaseMfma + kNgpHeadMfma;
    if (HEAD == QF_HEAD_SG || HEAD == QF_HEAD_SG_FEATURES) return kBaseMfma + kSgHiddenMfma + 16 * a.nt_out;
    return kBaseMfma;
}

// ENC: also write the hash-grid encoding (training forward).  A template parameter, not a run-time test: with the branch
// in the inference kernel it ran 1.5-2 % slower (1.335-1.357 ms against 1.313-1.330 on the bench frame).
template <int HEAD, bool ENC>
__global__ __launch_bounds__(kBlock, 4) void field_kernel(const FieldArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int g = lane >> 4, p = lane & 15;

    // ---- stage the A-operand images (and SG biases) into LDS, once per workgroup
    const int total = n_mfma<HEAD>(a) * 64;
    for (int e = tid; e < total; e += kBlock) {
        const int m = e >> 6, l = e & 63;
        lds[img_index(m, l)] = weight_for<HEAD>(a, m, l);
    }
    float *bias_lds = lds + total;      // [b2 (64) | bout (64, zero padded)]
    if (HEAD == QF_HEAD_SG || HEAD == QF_HEAD_SG_FEATURES) {
        if (tid < 64) bias_lds[tid] = a.sg.b2[tid];
        else if (tid < 128) bias_lds[tid] = (tid - 64 < a.n_out) ? a.sg.bout[tid - 64] : 0.0f;
    }
    // level table behind the biases
    uint32_t *lvl_lds = reinterpret_cast<uint32_t *>(bias_lds + 128);
    stage_level_table(lvl_lds, a.grid, tid);
    __syncthreads();
    const f32x4 *img_base = reinterpret_cast<const f32x4 *>(lds);   // img_base[(m>>2)*64 + lane]

    // which groups this wave takes: field_dealing.h.  With a.n_dev, a.n is the capacity of the arrays
    const int64_t n_pts = a.n_dev ? qf_clamp_count(*a.n_dev, a.n) : a.n;
    const QfGroupRange deal = qf_group_range((n_pts + 15) >> 4, gridDim.x, blockIdx.x, tid >> 6, kBlock / 64);

    for (int64_t grp = deal.begin; grp < deal.end; grp += deal.stride) {
        const int64_t pt_raw = grp * 16 + p;
        const bool valid = pt_raw < n_pts;
        int64_t pt = valid ? pt_raw : n_pts - 1;
        if (a.order) pt = a.order[pt];   // processing permutation (spatially coherent groups); results unchanged

        const float X = a.xyz[pt * 3 + 0], Y = a.xyz[pt * 3 + 1], Z = a.xyz[pt * 3 + 2];
        // (x - lo) / (hi - lo), ngp.py:761-763
        const float x01 = (X - a.aabb_lo[0]) / (a.aabb_hi[0] - a.aabb_lo[0]);
        const float y01 = (Y - a.aabb_lo[1]) / (a.aabb_hi[1] - a.aabb_lo[1]);
        const float z01 = (Z - a.aabb_lo[2]) / (a.aabb_hi[2] - a.aabb_lo[2]);
        const bool selector = x01 > 0.0f && x01 < 1.0f && y01 > 0.0f && y01 < 1.0f && z01 > 0.0f && z01 < 1.0f;

        // ---- hash grid: issue all 32 gathers, then blend
        // LDS contents are loop-invariant; opaque offsets keep the compiler from hoisting the level table and
        // all 160 weight operand registers out of the point loop
        int loff = lane, goff = g * 8;
        asm volatile("" : "+v"(loff), "+v"(goff));
        const f32x4 *img = img_base + loff;

        float frac[4][3];
        float2 val[4][8];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t idx[8];
            level_indices(load_level(lvl_lds, j, goff), x01, y01, z01, idx, frac[j]);
#pragma unroll
            for (int c = 0; c < 8; ++c) val[j][c] = a.table[idx[c]];
        }
        float feat[8];
#pragma unroll
        for (int j = 0; j < 4; ++j) level_blend(val[j], frac[j], &feat[2 * j], &feat[2 * j + 1]);
        if (ENC && valid) {                // training: the backward reads this instead of gathering the table again
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float2 *>(a.enc_out + pt * 32 + 2 * (4 * j + g)) = make_float2(feat[2 * j], feat[2 * j + 1]);
        }

        // ---- base MLP 32 -> 64 (ReLU) -> 16
        const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
        f32x4 h[4] = {zero, zero, zero, zero};
        dense_layer<8>(img, feat, h);
        relu<4>(h);
        const f32x4 base_out = row_tile_layer(img + 8 * 64, h, zero);    // lane (g,p): outputs 4g .. 4g+3 of point p

        // density = exp(raw - 1) * selector, ngp.py:772-775 (B-5, B-6)
        const float density = selector ? expf(base_out[0] - 1.0f) : 0.0f;
        if (g == 0 && valid && a.sigma) a.sigma[pt] = density;
        if (a.raw16 && valid) *reinterpret_cast<f32x4 *>(a.raw16 + pt * 16 + 4 * g) = base_out;
        if (a.geo && valid) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int o = 4 * g + r;
                if (o > 0) a.geo[pt * 15 + (o - 1)] = base_out[r];
            }
        }

        if (HEAD == QF_HEAD_NGP) {
            const float dx = a.dirs[pt * 3 + 0], dy = a.dirs[pt * 3 + 1], dz = a.dirs[pt * 3 + 2];
            // ngp.py:784 feeds (d+1)/2; tcnn maps back 2u-1 (A.3)
            const float ux = ((dx + 1.0f) / 2.0f) * 2.0f - 1.0f;
            const float uy = ((dy + 1.0f) / 2.0f) * 2.0f - 1.0f;
            const float uz = ((dz + 1.0f) / 2.0f) * 2.0f - 1.0f;
            float in[8];
            sh4_quartet(g, ux, uy, uz, in);
#pragma unroll
            for (int r = 0; r < 4; ++r) in[4 + r] = base_out[r];
            if (g == 0) in[4] = 1.0f;      // the density slot carries the constant-1 pad input
            f32x4 h1[4] = {zero, zero, zero, zero}, h2[4] = {zero, zero, zero, zero};
            dense_layer<8>(img + 12 * 64, in, h1);
            relu<4>(h1);
            dense_layer<16>(img + 20 * 64, h1, h2);
            relu<4>(h2);
            const f32x4 c = row_tile_layer(img + 36 * 64, h2, zero);
            if (g == 0 && valid) {
                a.rgb[pt * 3 + 0] = sigmoidf(c[0]);
                a.rgb[pt * 3 + 1] = sigmoidf(c[1]);
                a.rgb[pt * 3 + 2] = sigmoidf(c[2]);
            }
        }

        if (HEAD == QF_HEAD_SG || HEAD == QF_HEAD_SG_FEATURES) {
            float in[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) in[r] = base_out[r];
            if (g == 0) in[0] = 1.0f;      // bias slot
            f32x4 h1[4] = {zero, zero, zero, zero};
            dense_layer<4>(img + 12 * 64, in, h1);
            relu<4>(h1);
            f32x4 h2[4];
            const f32x4 *b2v = reinterpret_cast<const f32x4 *>(bias_lds);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) h2[mt] = b2v[4 * mt + g];
            dense_layer<16>(img + 16 * 64, h1, h2);
            relu<4>(h2);
            // output tiles: lane (g,p) register r of tile mt = head output 16mt + 4g + r
            f32x4 out[4];
            const f32x4 *bov = reinterpret_cast<const f32x4 *>(bias_lds + 64);
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                out[mt] = zero;
                if (mt < a.nt_out) out[mt] = row_tile_layer(img + (32 + 4 * mt) * 64, h2, bov[4 * mt + g]);
            }
            if (HEAD == QF_HEAD_SG_FEATURES) {
                if (valid) {
                    const int64_t row = pt * (int64_t)(a.n_out + 1);
#pragma unroll
                    for (int mt = 0; mt < 4; ++mt)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int o = 16 * mt + 4 * g + r;
                            if (o < a.n_out) a.features[row + o] = out[mt][r];
                        }
                    if (g == 0) a.features[row + a.n_out] = density;
                }
            } else {
                const float dx = a.dirs[pt * 3 + 0], dy = a.dirs[pt * 3 + 1], dz = a.dirs[pt * 3 + 2];
                // gather each head output from the lane quartet that holds it (compile-time slot)
                auto fetch = [&](int o) -> float {
                    return __shfl(out[o >> 4][o & 3], p + 16 * ((o >> 2) & 3), 64);
                };
                float acc_r = 0.0f, acc_g = 0.0f, acc_b = 0.0f;
#pragma unroll
                for (int l = 0; l < QF_MAX_LOBES; ++l) {
                    if (l < a.n_lobes) {
                        const int o = 3 + 7 * l;
                        const float ax = fetch(o), ay = fetch(o + 1), az = fetch(o + 2);
                        const float lam = fabsf(fetch(o + 3));
                        const float cr = fetch(o + 4), cg = fetch(o + 5), cb = fetch(o + 6);
                        const float nrm = sqrtf(ax * ax + ay * ay + az * az);
                        const float dotp = (ax / nrm) * dx + (ay / nrm) * dy + (az / nrm) * dz;
                        const float e = expf(lam * (dotp - 1.0f));
                        acc_r += cr * e;
                        acc_g += cg * e;
                        acc_b += cb * e;
                    }
                }
                const float d0 = fetch(0), d1 = fetch(1), d2 = fetch(2);
                if (g == 0 && valid) {
                    a.rgb[pt * 3 + 0] = sigmoidf(d0 + acc_r);
                    a.rgb[pt * 3 + 1] = sigmoidf(d1 + acc_g);
                    a.rgb[pt * 3 + 2] = sigmoidf(d2 + acc_b);
                }
            }
        }
    }
}

// Plain grid encode (tcnn.Encoding.forward): one thread per (point, level).
__global__ void grid_encode_kernel(GridArgs ga, const float2 *table, const float *x01, int64_t n, float *out)
{
    const int64_t total = n * QF_MAX_LEVELS;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < total;
         e += (int64_t)gridDim.x * blockDim.x) {
        const int64_t pt = e >> 4;
        const int level = (int)(e & 15);
        LevelConst lc;
        lc.offset = ga.offset[level];
        lc.rows = ga.rows[level];
        lc.res = ga.res[level];
        lc.scale = ga.scale[level];
        lc.hashed = (ga.hashed_mask >> level) & 1u;
        uint32_t idx[8];
        float frac[3];
        float2 val[8];
        level_indices(lc, x01[pt * 3], x01[pt * 3 + 1], x01[pt * 3 + 2], idx, frac);
#pragma unroll
        for (int c = 0; c < 8; ++c) val[c] = table[idx[c]];
        float f0, f1;
        level_blend(val, frac, &f0, &f1);
        out[pt * 32 + 2 * level] = f0;
        out[pt * 32 + 2 * level + 1] = f1;
    }
}

__global__ void sg_features_to_rgb_kernel(const float *features, int64_t stride, const float *dirs,
                                          int64_t n, int n_lobes, float *rgb)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (int64_t)gridDim.x * blockDim.x) {
        const float *f = features + i * stride;
        const float dx = dirs[i * 3], dy = dirs[i * 3 + 1], dz = dirs[i * 3 + 2];
        float r = 0.0f, g = 0.0f, b = 0.0f;
        for (int l = 0; l < n_lobes; ++l) {
            const float *x = f + 3 + 7 * l;
            const float nrm = sqrtf(x[0] * x[0] + x[1] * x[1] + x[2] * x[2]);
            const float dotp = (x[0] / nrm) * dx + (x[1] / nrm) * dy + (x[2] / nrm) * dz;
            const float e = expf(fabsf(x[3]) * (dotp - 1.0f));
            r += x[4] * e;
            g += x[5] * e;
            b += x[6] * e;
        }
        rgb[i * 3 + 0] = sigmoidf(f[0] + r);
        rgb[i * 3 + 1] = sigmoidf(f[1] + g);
        rgb[i * 3 + 2] = sigmoidf(f[2] + b);
    }
}

// Deformation field (examples/field.py:186-203): cat[x01(3), grid(32)] -> 32 -> 32 -> 1, ReLU, biases.
// Same wave mapping as field_kernel; the weight image is deform_rows.h's.
struct DeformArgs {
    GridArgs grid;
    const void *table;      // [rows] of the kernel's row type (DeformRowF32 / DeformRowF16)
    float scale;
    const float *w1, *b1, *w2, *b2, *wout, *bout;
    const float *xyz;
    const int32_t *order;
    int64_t n;
    const int64_t *n_dev;   // see FieldArgs
    float *out;
    float *enc_out;     // optional [n,32], see FieldArgs
};

constexpr int kDeformMfma = DeformImage<32>::L2T;   // 18 + 16 + 8: the forward part of the image

template <class R>
__global__ __launch_bounds__(kBlock, 4) void deform_kernel(const DeformArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, p = lane & 15;
    // image: plain [m][lane] floats (ds_read_b32); + b2[32] + bout[1]
    for (int e = tid; e < kDeformMfma * 64; e += kBlock) lds[e] = deform_fwd_weight<32>(a.w1, a.b1, a.w2, a.wout, e >> 6, e & 63);
    float *bias = lds + kDeformMfma * 64;
    if (tid < 32) bias[tid] = a.b2[tid];
    if (tid == 32) bias[32] = a.bout[0];
    // the level table lives in LDS next to the weights (stage_level_table; round 2 kept four LevelConst per lane in
    // registers for the whole point loop: 128 VGPRs + 6 spilled, 28 B/lane of scratch)
    uint32_t *lvl_lds = reinterpret_cast<uint32_t *>(bias + 64);
    stage_level_table(lvl_lds, a.grid, tid);
    __syncthreads();

    // which groups this wave takes: field_dealing.h
    const int64_t n_pts = a.n_dev ? qf_clamp_count(*a.n_dev, a.n) : a.n;
    const QfGroupRange deal = qf_group_range((n_pts + 15) >> 4, gridDim.x, blockIdx.x, tid >> 6, kBlock / 64);
    for (int64_t grp = deal.begin; grp < deal.end; grp += deal.stride) {
        const int64_t pt_raw = grp * 16 + p;
        const bool valid = pt_raw < n_pts;
        int64_t pt = valid ? pt_raw : n_pts - 1;
        if (a.order) pt = a.order[pt];
        // (x - (-s)) / (s - (-s)), field.py:195
        const float x01 = (a.xyz[pt * 3 + 0] + a.scale) / (a.scale + a.scale);
        const float y01 = (a.xyz[pt * 3 + 1] + a.scale) / (a.scale + a.scale);
        const float z01 = (a.xyz[pt * 3 + 2] + a.scale) / (a.scale + a.scale);
        float in[9];
        float frac[4][3];
        float2 val[4][8];
        // LDS contents are loop-invariant; opaque offsets keep the compiler from hoisting the level table and the
        // weight operands out of the point loop
        int loff = lane, goff = g * 8;
        asm volatile("" : "+v"(loff), "+v"(goff));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t idx[8];
            level_indices(load_level(lvl_lds, j, goff), x01, y01, z01, idx, frac[j]);
#pragma unroll
            for (int c = 0; c < 8; ++c) val[j][c] = R::unpack(static_cast<const typename R::row *>(a.table)[idx[c]]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            level_blend(val[j], frac[j], &in[2 * j], &in[2 * j + 1]);
            if (R::kRoundF16) round_f16_pair(&in[2 * j], &in[2 * j + 1]);   // the fp16 Encoding output
        }
        if (a.enc_out && valid) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                *reinterpret_cast<float2 *>(a.enc_out + pt * 32 + 2 * (4 * j + g)) = make_float2(in[2 * j], in[2 * j + 1]);
        }
        const float *wl = lds + loff;
        in[8] = g == 0 ? x01 : (g == 1 ? y01 : (g == 2 ? z01 : 1.0f));
        typedef DeformImage<32> I;
        f32x4 h1[2] = {(f32x4){0.f, 0.f, 0.f, 0.f}, (f32x4){0.f, 0.f, 0.f, 0.f}};
        dense_layer<2, 9>(wl + I::L1 * 64, in, h1);
        relu<2>(h1);
        f32x4 h2[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) h2[mt][r] = bias[16 * mt + 4 * g + r];
        dense_layer<2, 8>(wl + I::L2 * 64, h1, h2);
        relu<2>(h2);
        f32x4 oa = (f32x4){0.f, 0.f, 0.f, 0.f}, ob = oa;
#pragma unroll
        for (int s = 0; s < 8; s += 2) {
            oa = mfma(wl[(I::LO + s) * 64], h2[s >> 2][s & 3], oa);
            ob = mfma(wl[(I::LO + s + 1) * 64], h2[(s + 1) >> 2][(s + 1) & 3], ob);
        }
        if (g == 0 && valid) a.out[pt] = (oa[0] + ob[0]) + bias[32];
    }
}

template <int HEAD>
int launch_field(const FieldArgs &a, hipStream_t st)
{
    int n_m = kBaseMfma;
    if (HEAD == QF_HEAD_NGP) n_m += kNgpHeadMfma;
    if (HEAD == QF_HEAD_SG || HEAD == QF_HEAD_SG_FEATURES) n_m += kSgHiddenMfma + 16 * a.nt_out;
    const size_t lds_bytes = (size_t)(n_m * 64 + 128 + 8 * QF_MAX_LEVELS) * sizeof(float);
    const int64_t blocks = qf_field_blocks((a.n + 15) / 16, kBlock / 64, qf_cu_count_cached());
    if (a.enc_out)
        hipLaunchKernelGGL((field_kernel<HEAD, true>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    else
        hipLaunchKernelGGL((field_kernel<HEAD, false>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

}  // namespace

extern "C" int qf_grid_encode(const qf_grid_desc *desc, const float *table, const float *x01,
                              int64_t n, float *out, void *stream)
{
    if (!desc || !table || n < 0 || (n > 0 && (!x01 || !out))) return QF_ERR_INVALID_ARGUMENT;
    GridArgs ga;
    int rc = fill_grid_args(desc, &ga);
    if (rc != QF_OK) return rc;
    if (n == 0) return QF_OK;
    hipLaunchKernelGGL(grid_encode_kernel, dim3(qf_grid_1d(n * 16, 256)), dim3(256), 0, qf_stream(stream), ga,
                       reinterpret_cast<const float2 *>(table), x01, n, out);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_field_forward(const qf_field_desc *desc, const float *table, const float *base_w,
                                const float *head_ngp_w, const qf_sg_head *head_sg, const float *xyz,
                                const float *dirs, int64_t n, const int64_t *n_device, const int32_t *order, float *rgb,
                                float *sigma, float *geo, float *features, float *enc_out, void *stream)
{
    if (!desc || !table || !base_w || n < 0 || n > 0x7fffffff) return QF_ERR_INVALID_ARGUMENT;
    FieldArgs a = {};
    a.enc_out = enc_out;
    int rc = fill_grid_args(&desc->grid, &a.grid);
    if (rc != QF_OK) return rc;
    for (int k = 0; k < 3; ++k) {
        a.aabb_lo[k] = desc->aabb[k];
        a.aabb_hi[k] = desc->aabb[3 + k];
        if (!(desc->aabb[3 + k] > desc->aabb[k])) return QF_ERR_INVALID_ARGUMENT;
    }
    a.table = reinterpret_cast<const float2 *>(table);
    a.base_w = base_w;
    a.xyz = xyz;
    a.dirs = dirs;
    a.n = n;
    a.n_dev = n_device;
    a.rgb = rgb;
    a.sigma = sigma;
    a.geo = geo;
    a.features = features;
    a.order = order;
    if (n == 0) return QF_OK;
    if (!xyz) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    switch (desc->head) {
    case QF_HEAD_NONE:
        if (!sigma && !geo) return QF_ERR_INVALID_ARGUMENT;
        return launch_field<QF_HEAD_NONE>(a, st);
    case QF_HEAD_NGP:
        if (!head_ngp_w || !dirs || !rgb) return QF_ERR_INVALID_ARGUMENT;
        a.head_w = head_ngp_w;
        return launch_field<QF_HEAD_NGP>(a, st);
    case QF_HEAD_SG:
    case QF_HEAD_SG_FEATURES:
        if (!head_sg || !head_sg->w1 || !head_sg->b1 || !head_sg->w2 || !head_sg->b2 || !head_sg->wout ||
            !head_sg->bout)
            return QF_ERR_INVALID_ARGUMENT;
        if (desc->n_lobes < 1 || desc->n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
        a.sg = *head_sg;
        a.n_lobes = desc->n_lobes;
        a.n_out = 3 + 7 * desc->n_lobes;
        a.nt_out = (a.n_out + 15) / 16;
        if (desc->head == QF_HEAD_SG) {
            if (!dirs || !rgb) return QF_ERR_INVALID_ARGUMENT;
            return launch_field<QF_HEAD_SG>(a, st);
        }
        if (!features) return QF_ERR_INVALID_ARGUMENT;
        return launch_field<QF_HEAD_SG_FEATURES>(a, st);
    default:
        return QF_ERR_INVALID_ARGUMENT;
    }
}

extern "C" int qf_sg_features_to_rgb(const float *features, int64_t feat_stride, const float *dirs, int64_t n,
                                     int32_t n_lobes, float *rgb, void *stream)
{
    if (n < 0 || n_lobes < 1 || n_lobes > QF_MAX_LOBES || feat_stride < 3 + 7 * n_lobes) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!features || !dirs || !rgb) return QF_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(sg_features_to_rgb_kernel, dim3(qf_grid_1d(n, 256)), dim3(256), 0, qf_stream(stream),
                       features, feat_stride, dirs, n, (int)n_lobes, rgb);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

namespace {

// the argument handling and launch of both deformation entry points (same rules for both row types)
template <class R>
int deform_forward(const qf_grid_desc *grid, const void *table, float scale, int32_t hidden, const float *w1,
                   const float *b1, const float *w2, const float *b2, const float *wout, const float *bout,
                   const float *xyz, int64_t n, const int64_t *n_device, const int32_t *order, float *out,
                   float *enc_out, void *stream)
{
    if (!grid || !table || n < 0 || !(scale > 0.0f)) return QF_ERR_INVALID_ARGUMENT;
    if (hidden != 32) return QF_ERR_UNSUPPORTED;
    if (!w1 || !b1 || !w2 || !b2 || !wout || !bout) return QF_ERR_INVALID_ARGUMENT;
    DeformArgs a = {};
    int rc = fill_grid_args(grid, &a.grid);
    if (rc != QF_OK) return rc;
    if (n == 0) return QF_OK;
    if (!xyz || !out) return QF_ERR_INVALID_ARGUMENT;
    a.table = table;
    a.scale = scale;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.wout = wout; a.bout = bout;
    a.xyz = xyz;
    a.order = order;
    a.n = n;
    a.n_dev = n_device;
    a.out = out;
    a.enc_out = enc_out;
    const size_t lds_bytes = (size_t)(kDeformMfma * 64 + 64 + 8 * QF_MAX_LEVELS) * sizeof(float);
    const int64_t blocks = qf_field_blocks((n + 15) / 16, kBlock / 64, qf_cu_count_cached());
    hipLaunchKernelGGL(deform_kernel<R>, dim3((unsigned)blocks), dim3(kBlock), lds_bytes, qf_stream(stream), a);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

}  // namespace

extern "C" int qf_deform_field_forward(const qf_grid_desc *grid, const float *table, float scale, int32_t hidden,
                                       const float *w1, const float *b1, const float *w2, const float *b2,
                                       const float *wout, const float *bout, const float *xyz, int64_t n,
                                       const int64_t *n_device, const int32_t *order, float *out, float *enc_out,
                                       void *stream)
{
    return deform_forward<DeformRowF32>(grid, table, scale, hidden, w1, b1, w2, b2, wout, bout, xyz, n, n_device,
                                        order, out, enc_out, stream);
}

extern "C" int qf_deform_field_forward_f16(const qf_grid_desc *grid, const uint16_t *table, float scale,
                                           int32_t hidden, const float *w1, const float *b1, const float *w2,
                                           const float *b2, const float *wout, const float *bout, const float *xyz,
                                           int64_t n, const int64_t *n_device, const int32_t *order, float *out,
                                           float *enc_out, void *stream)
{
    return deform_forward<DeformRowF16>(grid, table, scale, hidden, w1, b1, w2, b2, wout, bout, xyz, n, n_device,
                                        order, out, enc_out, stream);
}

extern "C" int qf_grid_mlp_forward(const qf_grid_desc *grid, const float *table, const float *base_w, const float *x01,
                                   int64_t n, float *out16, void *stream)
{
    if (!grid || !table || !base_w || n < 0) return QF_ERR_INVALID_ARGUMENT;
    FieldArgs a = {};
    int rc = fill_grid_args(grid, &a.grid);
    if (rc != QF_OK) return rc;
    if (n == 0) return QF_OK;
    if (!x01 || !out16) return QF_ERR_INVALID_ARGUMENT;
    for (int k = 0; k < 3; ++k) { a.aabb_lo[k] = 0.0f; a.aabb_hi[k] = 1.0f; }   // (x - 0) / (1 - 0) == x exactly
    a.table = reinterpret_cast<const float2 *>(table);
    a.base_w = base_w;
    a.xyz = x01;
    a.n = n;
    a.raw16 = out16;
    return launch_field<QF_HEAD_NONE>(a, qf_stream(stream));
}
