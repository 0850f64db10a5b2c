// Stage 2's training step in one launch: the quadrature loss of the scalar Field and every gradient
// it needs, for gfx950.
//
// Replaces what torch autograd does for train_field.py:297-372 over field.py:206-259: Field(x) with
// autograd.grad(create_graph=True), compute_field_loss = mean | max(w, w_rev) - |grad f . d/|d|| |, and the double
// backward through the decoder.  With back_prop=False the encoder sees x01.detach() (field.py:196-199), so grad f
// reaches x only through the three x01 columns of the first layer and the hash features enter only through the
// pre-activations: the table's gradient is the first-order scatter of a per-point d_enc [n,32], which stays
// qf_grid_encode_backward's work.
//
// Mapping: grid_extract_kernel's point list (grid_extract.hip).  A wave takes 16 points per pass, lane l = (p = l & 15,
// g = l >> 4): point p, level quartet g; the wave gathers its own table rows (no [n,32] encoding is read), the decoder
// cat[x01, grid] -> 16 -> 16 -> 1 (ELU) and the backward of its scalar output run on v_mfma_f32_16x16x4_f32 with the
// D-layout accumulator of one layer as the B operand of the next.  The loss's backward is the same chain once more:
//   v   = -sign(r) sign(p) d^ upstream / (2 s n)        dL / d(W1[:, 0:3]^T delta1)
//   q1  = W1[:, 0:3] v            e1 = q1 phi'(z1)      q2 = W2 e1
//   y2  = q2 wout phi''(z2)                             dL/dz2
//   y1  = q1 c1 phi''(z1) + (W2^T y2) phi'(z1)          dL/dz1
//   d_enc = W1[:, 3:35]^T y1
// and the weight gradients are sums over points of outer products of these, accumulated on the matrix cores through the
// per-wave 16 x 17 LDS transpose of mlp_tiles.h: 864 parameters = 6 tiles (W2: delta2 e1^T + y2 a1^T; b2: y2; wout:
// q2 phi'(z2); W1 grid columns: 2 tiles of y1 h^T; W1 x01 columns and b1: y1 [x01 | 1]^T + delta1 v^T), 24 accumulator
// registers per lane for the whole launch.  At the end the eight waves of a workgroup add their tiles in LDS and the
// workgroup adds the sums to the gradient vectors with atomics.  The loss is summed in fp64: per lane, per wave, per
// workgroup into the workspace, and a one-wave launch adds the workgroups' partials in index order -- bit-identical
// run to run.
#include "mlp_tiles.h"
#include "deform_rows.h"

namespace {

constexpr int kBlock = 512;               // 8 waves, one workgroup per CU (qf_field_blocks)
constexpr int kWaves = kBlock / 64;
constexpr int kMaxBlocks = QF_FIELD_LOSS_WORKSPACE_BYTES / 8;

typedef DeformImage<16> I;
constexpr int kW1X = I::N;                // W1[:, 0:3] as the A operand of q1 = W1[:, 0:3] v (one k-step)
constexpr int kW1T = kW1X + 1;            // W1[:, 3:35]^T: 4 k-steps outer, 2 row tiles inner
constexpr int kTiles = kW1T + 8;
constexpr int kAccTiles = 6;              // W2, b2, wout, W1 grid columns (2), W1 x01 columns | b1
constexpr int kLdsFloats = kTiles * 64 + 128 + 8 * QF_MAX_LEVELS + kWaves * 16 * 17;

static_assert(kAccTiles * 256 <= kTiles * 64, "the workgroup's tile sums reuse the weight image");
static_assert(kAccTiles * 64 <= kBlock, "one thread per (tile, lane) at the flush");

struct FieldTrainArgs {
    GridArgs grid;
    const float2 *table;
    float scale;
    float inv_2sn;                        // 1 / (2 s n)
    const float *w1, *b1, *w2, *b2, *wout, *bout;
    const float *xyz, *dirs, *weights, *weights_rev;
    int64_t n;
    const float *upstream;
    float *value, *grad, *d_enc;
    float *g_w1, *g_b1, *g_w2, *g_b2, *g_wout;
    double *partial;                      // one per workgroup, or NULL (no loss wanted)
};

__device__ float weight_for(const FieldTrainArgs &a, int m, int lane)
{
    if (m < I::L2T) return deform_fwd_weight<16>(a.w1, a.b1, a.w2, a.wout, m, lane);
    const int i = lane & 15, kq = lane >> 4;
    if (m < I::L1X) return a.w2[hidden_col(m - I::L2T, kq) * 16 + i];                      // W2^T
    if (m < I::N) return i < 3 ? a.w1[hidden_col(m - I::L1X, kq) * 35 + i] : 0.0f;         // W1[:, 0:3]^T
    if (m == kW1X) return kq < 3 ? a.w1[i * 35 + kq] : 0.0f;
    const int q = m - kW1T, s = q >> 1, mt = q & 1;
    return a.w1[hidden_col(s, kq) * 35 + 3 + 16 * mt + i];
}

// torch.nn.ELU() (alpha 1) from the pre-activation, with its first derivative (elu_backward from the input: exp(z)
// where z <= 0).  The second derivative equals the first where z <= 0 and is 0 above: elu2 takes it from the output,
// which is positive exactly where z is.
__device__ __forceinline__ float elu_fwd(float z, float *d)
{
    if (z > 0.0f) { *d = 1.0f; return z; }
    *d = expf(z);
    return expm1f(z);
}
__device__ __forceinline__ float elu2(float act, float d) { return act > 0.0f ? 0.0f : d; }

__device__ __forceinline__ float sign0(float x) { return x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : 0.0f); }   // torch's sgn: 0 at 0

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// LOSS false: value and gradient only (inference).
template <bool LOSS>
__global__ __launch_bounds__(kBlock) void field_train_kernel(const FieldTrainArgs a)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];
    __shared__ double s_part[kWaves];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, p = lane & 15;
    constexpr int n_img = LOSS ? kTiles : I::N;
    for (int e = tid; e < n_img * 64; e += kBlock) lds[e] = weight_for(a, e >> 6, e & 63);
    float *bias = lds + kTiles * 64;        // b2 [0, 16), bout [32], wout [64, 80)
    if (tid < 16) { bias[tid] = a.b2[tid]; bias[64 + tid] = a.wout[tid]; }
    if (tid == 32) bias[32] = a.bout[0];
    uint32_t *lvl_lds = reinterpret_cast<uint32_t *>(bias + 128);
    stage_level_table(lvl_lds, a.grid, tid);
    volatile float *scratch = bias + 128 + 8 * QF_MAX_LEVELS + wave * (16 * 17);
    __syncthreads();

    const f32x4 zero = (f32x4){0.f, 0.f, 0.f, 0.f};
    const f32x4 ones_op = p == 0 ? (f32x4){1.f, 1.f, 1.f, 1.f} : zero;
    f32x4 aW2 = zero, ab2 = zero, awo = zero, aW1f[2] = {zero, zero}, aW1x = zero;
    double loss_acc = 0.0;
    const bool want_grads = LOSS && a.g_w1 != nullptr;
    const bool want_back = LOSS && (want_grads || a.d_enc != nullptr);
    const float up = (LOSS && a.upstream) ? a.upstream[0] : 1.0f;

    const int64_t n_groups = (a.n + 15) >> 4;
    const QfGroupRange deal = qf_group_range(n_groups, gridDim.x, blockIdx.x, wave, kWaves);
    const float two_s = a.scale + a.scale;
    for (int64_t grp = deal.begin; grp < deal.end; grp += deal.stride) {
        const int64_t pt_raw = grp * 16 + p;
        const bool valid = pt_raw < a.n;
        const int64_t pt = valid ? pt_raw : a.n - 1;
        const float x = a.xyz[pt * 3 + 0], y = a.xyz[pt * 3 + 1], z = a.xyz[pt * 3 + 2];
        // (x - (-s)) / (s - (-s)), field.py:195
        const float x01 = (x + a.scale) / two_s, y01 = (y + a.scale) / two_s, z01 = (z + a.scale) / two_s;
        float in[9];
        float frac[4][3];
        float2 val[4][8];
        int loff = lane, goff = g * 8;
        asm volatile("" : "+v"(loff), "+v"(goff));
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            uint32_t idx[8];
            level_indices(load_level(lvl_lds, j, goff), x01, y01, z01, idx, frac[j]);
#pragma unroll
            for (int c = 0; c < 8; ++c) val[j][c] = a.table[idx[c]];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) level_blend(val[j], frac[j], &in[2 * j], &in[2 * j + 1]);
        const float *wl = lds + loff;
        in[8] = g == 0 ? x01 : (g == 1 ? y01 : (g == 2 ? z01 : 1.0f));

        // ---------------------------------------------------------------- forward, as grid_extract_kernel
        f32x4 a1[1] = {zero}, d1, a2[1], d2;
        dense_layer<1, 9>(wl + I::L1 * 64, in, a1);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d;
            a1[0][r] = elu_fwd(a1[0][r], &d);
            d1[r] = d;
            a2[0][r] = bias[4 * g + r];
        }
        dense_layer<1, 4>(wl + I::L2 * 64, a1, a2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float d;
            a2[0][r] = elu_fwd(a2[0][r], &d);
            d2[r] = d;
        }
        f32x4 oa = zero, ob = zero;
        oa = mfma(wl[(I::LO + 0) * 64], a2[0][0], oa);
        ob = mfma(wl[(I::LO + 1) * 64], a2[0][1], ob);
        oa = mfma(wl[(I::LO + 2) * 64], a2[0][2], oa);
        ob = mfma(wl[(I::LO + 3) * 64], a2[0][3], ob);
        const float f = (oa[0] + ob[0]) + bias[32];            // lanes g = 0

        // ---------------------------------------------------------------- backward of the scalar output
        f32x4 wo, delta2[1], c1[1] = {zero}, delta1;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            wo[r] = bias[64 + 4 * g + r];
            delta2[0][r] = d2[r] * wo[r];
        }
        dense_layer<1, 4>(wl + I::L2T * 64, delta2, c1);
#pragma unroll
        for (int r = 0; r < 4; ++r) delta1[r] = d1[r] * c1[0][r];
        f32x4 ga = zero, gb = zero;
        ga = mfma(wl[(I::L1X + 0) * 64], delta1[0], ga);
        gb = mfma(wl[(I::L1X + 1) * 64], delta1[1], gb);
        ga = mfma(wl[(I::L1X + 2) * 64], delta1[2], ga);
        gb = mfma(wl[(I::L1X + 3) * 64], delta1[3], gb);
        // d/dx = d/dx01 / (xyz_max - xyz_min): lanes g = 0
        const float gx0 = (ga[0] + gb[0]) / two_s, gy0 = (ga[1] + gb[1]) / two_s, gz0 = (ga[2] + gb[2]) / two_s;
        if (g == 0 && valid) {
            if (a.value) a.value[pt] = f;
            if (a.grad) {
                a.grad[pt * 3 + 0] = gx0;
                a.grad[pt * 3 + 1] = gy0;
                a.grad[pt * 3 + 2] = gz0;
            }
        }
        if (!LOSS) continue;

        // ---------------------------------------------------------------- the loss (field.py:253-259), on every lane
        const float gx = __shfl(gx0, p, 64), gy = __shfl(gy0, p, 64), gz = __shfl(gz0, p, 64);
        const float dx = a.dirs[pt * 3 + 0], dy = a.dirs[pt * 3 + 1], dz = a.dirs[pt * 3 + 2];
        const float nrm = sqrtf(dx * dx + dy * dy + dz * dz);
        const float ux = dx / nrm, uy = dy / nrm, uz = dz / nrm;
        const float proj = gx * ux + gy * uy + gz * uz;
        const float res = fmaxf(a.weights[pt], a.weights_rev[pt]) - fabsf(proj);
        if (g == 0 && valid) loss_acc += (double)fabsf(res);
        if (!want_back) continue;
        const float coef = valid ? -sign0(res) * sign0(proj) * a.inv_2sn * up : 0.0f;
        const float vB = g == 0 ? coef * ux : (g == 1 ? coef * uy : (g == 2 ? coef * uz : 0.0f));

        // ---------------------------------------------------------------- backward of the loss through the decoder
        f32x4 q1 = mfma(wl[kW1X * 64], vB, zero);
        f32x4 e1[1], q2[1] = {zero}, gw, y2[1], t1[1] = {zero}, y1;
#pragma unroll
        for (int r = 0; r < 4; ++r) e1[0][r] = q1[r] * d1[r];
        dense_layer<1, 4>(wl + I::L2 * 64, e1, q2);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            gw[r] = q2[0][r] * d2[r];
            y2[0][r] = q2[0][r] * wo[r] * elu2(a2[0][r], d2[r]);
        }
        dense_layer<1, 4>(wl + I::L2T * 64, y2, t1);
#pragma unroll
        for (int r = 0; r < 4; ++r) y1[r] = q1[r] * c1[0][r] * elu2(a1[0][r], d1[r]) + t1[0][r] * d1[r];
        if (a.d_enc) {
            f32x4 de[2] = {zero, zero};
#pragma unroll
            for (int s = 0; s < 4; ++s) {
                de[0] = mfma(wl[(kW1T + 2 * s + 0) * 64], y1[s], de[0]);
                de[1] = mfma(wl[(kW1T + 2 * s + 1) * 64], y1[s], de[1]);
            }
            if (valid) {
                *reinterpret_cast<f32x4 *>(a.d_enc + pt * 32 + 4 * g) = de[0];
                *reinterpret_cast<f32x4 *>(a.d_enc + pt * 32 + 16 + 4 * g) = de[1];
            }
        }
        if (!want_grads) continue;

        // ---------------------------------------------------------------- weight / bias gradients
        {
            const f32x4 tY2 = to_operand(y2[0], scratch, lane);
            aW2 = outer_acc(to_operand(delta2[0], scratch, lane), to_operand(e1[0], scratch, lane), aW2);
            aW2 = outer_acc(tY2, to_operand(a1[0], scratch, lane), aW2);
            ab2 = outer_acc(tY2, ones_op, ab2);
            awo = outer_acc(to_operand(gw, scratch, lane), ones_op, awo);
            const f32x4 tY1 = to_operand(y1, scratch, lane);
            aW1f[0] = outer_acc(tY1, to_operand((f32x4){in[0], in[1], in[2], in[3]}, scratch, lane), aW1f[0]);
            aW1f[1] = outer_acc(tY1, to_operand((f32x4){in[4], in[5], in[6], in[7]}, scratch, lane), aW1f[1]);
            aW1x = outer_acc(tY1, to_operand((f32x4){in[8], 0.f, 0.f, 0.f}, scratch, lane), aW1x);
            aW1x = outer_acc(to_operand(delta1, scratch, lane), to_operand((f32x4){vB, 0.f, 0.f, 0.f}, scratch, lane), aW1x);
        }
    }
    if (!LOSS) return;

    // ---- the loss: lane -> wave -> workgroup, each in a fixed order
    if (a.partial) {
        const double w = wave_sum(loss_acc);
        if (lane == 0) s_part[wave] = w;
    }
    __syncthreads();                        // also: every wave is done with the weight image
    if (a.partial && tid == 0) {
        double s = 0.0;
        for (int q = 0; q < kWaves; ++q) s += s_part[q];
        a.partial[blockIdx.x] = s;
    }
    if (!want_grads) return;

    // ---- the workgroup's tiles: summed in LDS (tile t, lane l, register r at (64 t + l) * 4 + r), then one atomic per
    // parameter.  Lane (g,p) register r = d[row 4g + r][column p of the tile's operand].
    float *red = lds;
    for (int e = tid; e < kAccTiles * 256; e += kBlock) red[e] = 0.0f;
    __syncthreads();
    const f32x4 tiles[kAccTiles] = {aW2, ab2, awo, aW1f[0], aW1f[1], aW1x};
#pragma unroll
    for (int t = 0; t < kAccTiles; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) atomicAdd(&red[(64 * t + lane) * 4 + r], tiles[t][r]);
    __syncthreads();
    if (tid >= kAccTiles * 64) return;
    const int t = wave;                     // tile of this thread, its lane is `lane`
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 4 * g + r;
        const float v = red[(64 * t + lane) * 4 + r];
        if (t == 0) {
            atomicAdd(a.g_w2 + row * 16 + p, v);
        } else if (t == 1) {
            if (p == 0) atomicAdd(a.g_b2 + row, v);
        } else if (t == 2) {
            if (p == 0) atomicAdd(a.g_wout + row, v);
        } else if (t < 5) {
            const int s = 4 * (t - 3) + (p & 3);
            atomicAdd(a.g_w1 + row * 35 + 3 + 2 * (4 * (s >> 1) + (p >> 2)) + (s & 1), v);
        } else if ((p & 3) == 0) {
            if (p < 12) atomicAdd(a.g_w1 + row * 35 + (p >> 2), v);
            else atomicAdd(a.g_b1 + row, v);
        }
    }
}

// loss = (sum of the workgroups' partials, lanes striding over them, then the wave's butterfly) / n
__global__ __launch_bounds__(64) void field_loss_finish_kernel(const double *partial, int blocks, int64_t n, double *loss)
{
    double s = 0.0;
    for (int i = threadIdx.x; i < blocks; i += 64) s += partial[i];
    s = wave_sum(s);
    if (threadIdx.x == 0) *loss = s / (double)n;
}

}  // namespace

extern "C" int qf_field_quadrature_loss(const qf_grid_desc *grid, const float *table, float scale, int32_t hidden,
                                        int32_t activation, const float *w1, const float *b1, const float *w2,
                                        const float *b2, const float *wout, const float *bout, const float *xyz,
                                        const float *dirs, const float *weights, const float *weights_rev, int64_t n,
                                        const float *upstream, double *loss, float *value, float *grad, float *d_enc,
                                        float *g_w1, float *g_b1, float *g_w2, float *g_b2, float *g_wout,
                                        void *workspace, int64_t workspace_bytes, void *stream)
{
    if (!grid || !table || !(scale > 0.0f) || !(scale <= 3.0e38f) || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (hidden != 16 || activation != QF_ACT_ELU) return QF_ERR_UNSUPPORTED;
    if (!w1 || !b1 || !w2 || !b2 || !wout || !bout) return QF_ERR_INVALID_ARGUMENT;
    const int n_grads = (g_w1 != nullptr) + (g_b1 != nullptr) + (g_w2 != nullptr) + (g_b2 != nullptr) + (g_wout != nullptr);
    if (n_grads != 0 && n_grads != 5) return QF_ERR_INVALID_ARGUMENT;
    const bool with_loss = loss || d_enc || n_grads;
    if (!with_loss && upstream) return QF_ERR_INVALID_ARGUMENT;
    if (loss && (!workspace || workspace_bytes < 8)) return QF_ERR_INVALID_ARGUMENT;
    FieldTrainArgs a = {};
    int rc = fill_grid_args(grid, &a.grid);
    if (rc != QF_OK) return rc;
    hipStream_t st = qf_stream(stream);
    if (n == 0) {                          // torch's mean of an empty tensor
        if (loss) {
            QF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(loss), 0, 1, st));
            QF_HIP_TRY(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(reinterpret_cast<char *>(loss) + 4), 0x7ff80000, 1, st));
        }
        return QF_OK;
    }
    if (!xyz || (with_loss && (!dirs || !weights || !weights_rev))) return QF_ERR_INVALID_ARGUMENT;
    const int64_t n_groups = (n + 15) / 16;
    int64_t blocks = qf_field_blocks(n_groups, kWaves, qf_cu_count_cached());
    if (loss) {
        int64_t room = workspace_bytes / 8;
        if (room > kMaxBlocks) room = kMaxBlocks;
        if (blocks > room) blocks = qf_field_blocks(n_groups, kWaves, (int)room);
    }
    a.table = reinterpret_cast<const float2 *>(table);
    a.scale = scale;
    a.inv_2sn = (float)(1.0 / (2.0 * (double)scale * (double)n));
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.wout = wout; a.bout = bout;
    a.xyz = xyz; a.dirs = dirs; a.weights = weights; a.weights_rev = weights_rev;
    a.n = n;
    a.upstream = upstream;
    a.value = value; a.grad = grad; a.d_enc = d_enc;
    a.g_w1 = g_w1; a.g_b1 = g_b1; a.g_w2 = g_w2; a.g_b2 = g_b2; a.g_wout = g_wout;
    a.partial = loss ? reinterpret_cast<double *>(workspace) : nullptr;
    const size_t lds_bytes = (size_t)kLdsFloats * sizeof(float);
    if (with_loss)
        hipLaunchKernelGGL(field_train_kernel<true>, dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    else
        hipLaunchKernelGGL(field_train_kernel<false>, dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    QF_LAUNCH_CHECK();
    if (loss) {
        hipLaunchKernelGGL(field_loss_finish_kernel, dim3(1), dim3(64), 0, st, a.partial, (int)blocks, n, loss);
        QF_LAUNCH_CHECK();
    }
    return QF_OK;
}
