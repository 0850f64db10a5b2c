// The quadrature field's value and spatial-gradient norm on a lattice, average-pooled, for gfx950.
//
// Replaces field_utils.extract_grid (examples/field_utils.py:276-318): the Field (examples/field.py:130-238) sampled on
// a (2n)^3 lattice through torch autograd, |d field / dx| clipped to [0, 65504], both grids 2x2x2 average-pooled on the
// CPU.  Here one launch evaluates the field AND its input gradient per point and pools in registers.
//
// Mapping: deform_kernel's (field_eval.hip).  A wave takes 16 points per pass, lane l = (p = l & 15, g = l >> 4):
// point p, level quartet g; weights and level table in LDS; the decoder on v_mfma_f32_16x16x4_f32 with activations
// chained in registers.  The decoder's backward for the scalar output runs on the same matrix cores in the same
// layout: dz2 = wout * act'(z2) is already the B operand of a W2^T tile, da1 lands where z1 lives, and one W1[:, 0:3]^T
// tile sequence gives d out / d x01 in registers 0..2 of lanes g = 0.  With back_prop=False (the reference's stage-2
// field) the encoder sees x01.detach() (field.py:196-199): the gradient flows through the three x01 columns only.
//
// Lattice source: a 16-point group is a 2 x 2 x 4 brick of lattice points (x, y, z), so at the finest level (256
// cells across against 2048 lattice points) a group's corners are mostly the same 8 rows.  Groups are ordered
// (z tile of 16 bricks, y brick, x brick, z brick in the tile): 16 consecutive groups fill 128 B of value output and
// the waves of an XCD sweep x at fixed (y, z), the table's contiguous axis.  Pool 2: the brick holds two voxels
// (lanes with the same p>>1 & 1); lane e of a voxel's 8 is fetched with a cross-lane read and summed in torch's CPU
// AvgPool3d order (dx outer, dz inner, from 0, then / 8).
#include "mlp_tiles.h"
#include "deform_rows.h"

namespace {

constexpr int kBlock = 512;   // 8 waves, one workgroup per CU (qf_field_blocks)
constexpr int kTileZ = 16;    // z bricks per tile of the lattice walk

enum GxSource { GX_LIST = 0, GX_LATTICE_1 = 1, GX_LATTICE_2 = 2 };

struct GridExtractArgs {
    GridArgs grid;
    const void *table;
    float scale;
    const float *w1, *b1, *w2, *b2, *wout, *bout;
    // point list
    const float *xyz;
    int64_t n_points;
    const int64_t *n_dev;
    // lattice
    const float *axis;
    int32_t n;          // output cells per axis
    int32_t lat;        // lattice points per axis = n * pool
    int32_t x_begin, x_count;
    int32_t nbx, nby, nbz;
    int64_t n_groups;
    float *value;
    uint16_t *grad;     // fp16 bits, or NULL
};

// A operand of MFMA m of DeformImage<H>: the forward part, then the backward of the scalar output
template <int H>
__device__ float weight_for(const GridExtractArgs &a, int m, int lane)
{
    typedef DeformImage<H> I;
    if (m < I::L2T) return deform_fwd_weight<H>(a.w1, a.b1, a.w2, a.wout, m, lane);
    const int i = lane & 15, kq = lane >> 4;
    if (m < I::L1X) {                      // backward of layer 2: W2^T
        const int q = m - I::L2T, s = q / I::MT, mt = q % I::MT;
        return a.w2[hidden_col(s, kq) * H + 16 * mt + i];
    }
    const int s = m - I::L1X;              // backward of layer 1 to the x01 columns: rows 0..2 of W1^T
    return i < 3 ? a.w1[hidden_col(s, kq) * 35 + i] : 0.0f;
}

// activation and its derivative from the pre-activation: ReLU (threshold_backward: 1 where the output is > 0) or
// torch.nn.ELU() (alpha 1: expm1 below 0; elu_backward from the input: exp(z) where z <= 0)
template <int ACT>
__device__ __forceinline__ float act_fwd(float z, float *d)
{
    if (ACT == QF_ACT_ELU) {
        if (z > 0.0f) { *d = 1.0f; return z; }
        *d = expf(z);
        return expm1f(z);
    }
    *d = z > 0.0f ? 1.0f : 0.0f;
    return fmaxf(z, 0.0f);
}

template <class R, int ACT, int H, int SRC>
__global__ __launch_bounds__(kBlock) void grid_extract_kernel(const GridExtractArgs a)
{
    typedef DeformImage<H> I;
    constexpr int MT = I::MT, S = I::S;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int tid = threadIdx.x, lane = tid & 63, g = lane >> 4, p = lane & 15;
    for (int e = tid; e < I::N * 64; e += kBlock) lds[e] = weight_for<H>(a, e >> 6, e & 63);
    float *bias = lds + I::N * 64;          // b2 [0, H), bout [32], wout [64, 64 + H)
    if (tid < H) { bias[tid] = a.b2[tid]; bias[64 + tid] = a.wout[tid]; }
    if (tid == 32) bias[32] = a.bout[0];
    uint32_t *lvl_lds = reinterpret_cast<uint32_t *>(bias + 128);
    stage_level_table(lvl_lds, a.grid, tid);
    __syncthreads();

    int64_t n_groups;
    int64_t n_pts = 0;
    if (SRC == GX_LIST) {
        n_pts = a.n_dev ? qf_clamp_count(*a.n_dev, a.n_points) : a.n_points;
        n_groups = (n_pts + 15) >> 4;
    } else {
        n_groups = a.n_groups;
    }
    // which groups this wave takes: field_dealing.h
    const QfGroupRange deal = qf_group_range(n_groups, gridDim.x, blockIdx.x, tid >> 6, kBlock / 64);
    const float two_s = a.scale + a.scale;
    for (int64_t grp = deal.begin; grp < deal.end; grp += deal.stride) {
        bool valid;
        int64_t out_idx;
        float x, y, z;
        if (SRC == GX_LIST) {
            const int64_t pt_raw = grp * 16 + p;
            valid = pt_raw < n_pts;
            out_idx = valid ? pt_raw : n_pts - 1;
            x = a.xyz[out_idx * 3 + 0];
            y = a.xyz[out_idx * 3 + 1];
            z = a.xyz[out_idx * 3 + 2];
        } else {
            const int64_t bz_in = grp % kTileZ, r = grp / kTileZ;
            const int64_t r2 = r / a.nbx, bx = r - r2 * a.nbx, tz = r2 / a.nby, by = r2 - tz * a.nby;
            const int64_t bz = tz * kTileZ + bz_in;
            const int64_t xl0 = (int64_t)a.x_begin * (SRC == GX_LATTICE_2 ? 2 : 1);
            const int64_t xl1 = xl0 + (int64_t)a.x_count * (SRC == GX_LATTICE_2 ? 2 : 1);
            int64_t X = xl0 + 2 * bx + (p >> 3), Y = 2 * by + ((p >> 2) & 1), Z = 4 * bz + (p & 3);
            valid = bz < a.nbz && X < xl1 && Y < a.lat && Z < a.lat;
            if (X >= xl1) X = xl1 - 1;
            if (Y >= a.lat) Y = a.lat - 1;
            if (Z >= a.lat) Z = a.lat - 1;
            if (SRC == GX_LATTICE_2)     // voxel of this lane's lattice point (written by lanes p = 0 and 2)
                out_idx = ((X >> 1) - a.x_begin) * a.n * (int64_t)a.n + (Y >> 1) * (int64_t)a.n + (Z >> 1);
            else
                out_idx = (X - a.x_begin) * a.n * (int64_t)a.n + Y * (int64_t)a.n + Z;
            x = a.axis[X];
            y = a.axis[Y];
            z = a.axis[Z];
        }
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
            for (int c = 0; c < 8; ++c) val[j][c] = R::unpack(static_cast<const typename R::row *>(a.table)[idx[c]]);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            level_blend(val[j], frac[j], &in[2 * j], &in[2 * j + 1]);
            if (R::kRoundF16) round_f16_pair(&in[2 * j], &in[2 * j + 1]);   // the fp16 Encoding output
        }
        const float *wl = lds + loff;
        in[8] = g == 0 ? x01 : (g == 1 ? y01 : (g == 2 ? z01 : 1.0f));
        // forward
        f32x4 h1[MT], d1[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) h1[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        dense_layer<MT, 9>(wl + I::L1 * 64, in, h1);
        f32x4 h2[MT], d2[MT];
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float d;
                h1[mt][r] = act_fwd<ACT>(h1[mt][r], &d);
                d1[mt][r] = d;
                h2[mt][r] = bias[16 * mt + 4 * g + r];
            }
        }
        dense_layer<MT, S>(wl + I::L2 * 64, h1, h2);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float d;
                h2[mt][r] = act_fwd<ACT>(h2[mt][r], &d);
                d2[mt][r] = d;
            }
        // (the two split-accumulator row tiles of this kernel stay written out: as a shared template the ELU list
        // instantiations allocate their scalar registers differently)
        f32x4 oa = (f32x4){0.f, 0.f, 0.f, 0.f}, ob = oa;
#pragma unroll
        for (int s = 0; s < S; s += 2) {
            oa = mfma(wl[(I::LO + s) * 64], h2[s >> 2][s & 3], oa);
            ob = mfma(wl[(I::LO + s + 1) * 64], h2[(s + 1) >> 2][(s + 1) & 3], ob);
        }
        const float v = (oa[0] + ob[0]) + bias[32];        // lanes g = 0
        float gn = 0.0f;
        if (a.grad) {
            // backward of the scalar output: dz2 = wout * act'(z2) (the B operand of W2^T), dz1 = (W2^T dz2) * act'(z1)
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) d2[mt][r] *= bias[64 + 16 * mt + 4 * g + r];
            f32x4 da1[MT];
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) da1[mt] = (f32x4){0.f, 0.f, 0.f, 0.f};
            dense_layer<MT, S>(wl + I::L2T * 64, d2, da1);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int r = 0; r < 4; ++r) d1[mt][r] *= da1[mt][r];
            f32x4 ga = (f32x4){0.f, 0.f, 0.f, 0.f}, gb = ga;
#pragma unroll
            for (int s = 0; s < S; s += 2) {
                ga = mfma(wl[(I::L1X + s) * 64], d1[s >> 2][s & 3], ga);
                gb = mfma(wl[(I::L1X + s + 1) * 64], d1[(s + 1) >> 2][(s + 1) & 3], gb);
            }
            // d/dx = d/dx01 / (xyz_max - xyz_min) (field.py:195 under autograd), then |.|, clipped to [0, 65504]
            const float gx = (ga[0] + gb[0]) / two_s, gy = (ga[1] + gb[1]) / two_s, gz = (ga[2] + gb[2]) / two_s;
            gn = sqrtf(gx * gx + gy * gy + gz * gz);
            gn = gn > 65504.0f ? 65504.0f : gn;               // a NaN stays NaN, as torch.clip
        }
        if (SRC == GX_LATTICE_2) {
            // voxel (p >> 1) & 1 of the brick; its e-th value (dx, dy, dz) = (e >> 2, e >> 1 & 1, e & 1) sits on lane
            // 8 dx + 4 dy + 2 voxel + dz.  torch's CPU AvgPool3d: sum from 0 in that order, then / 8.
            const int vox = (p >> 1) & 1;
            float sv = 0.0f, sg = 0.0f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int src = ((e >> 2) << 3) | (((e >> 1) & 1) << 2) | (vox << 1) | (e & 1);
                sv += __shfl(v, src, 64);
                if (a.grad) sg += __shfl(gn, src, 64);
            }
            if (g == 0 && (p == 0 || p == 2) && valid) {
                a.value[out_idx] = sv / 8.0f;
                if (a.grad) a.grad[out_idx] = __builtin_bit_cast(uint16_t, (_Float16)(sg / 8.0f));
            }
        } else if (g == 0 && valid) {
            a.value[out_idx] = v;
            if (a.grad) a.grad[out_idx] = __builtin_bit_cast(uint16_t, (_Float16)gn);
        }
    }
}

template <class R, int ACT, int H>
int launch_extract(const GridExtractArgs &a, int src, int64_t n_groups, hipStream_t st)
{
    const size_t lds_bytes = (size_t)(DeformImage<H>::N * 64 + 128 + 8 * QF_MAX_LEVELS) * sizeof(float);
    const int64_t blocks = qf_field_blocks(n_groups, kBlock / 64, qf_cu_count_cached());
    if (src == GX_LIST)
        hipLaunchKernelGGL((grid_extract_kernel<R, ACT, H, GX_LIST>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    else if (src == GX_LATTICE_1)
        hipLaunchKernelGGL((grid_extract_kernel<R, ACT, H, GX_LATTICE_1>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    else
        hipLaunchKernelGGL((grid_extract_kernel<R, ACT, H, GX_LATTICE_2>), dim3((unsigned)blocks), dim3(kBlock), lds_bytes, st, a);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

template <class R>
int grid_extract(const qf_grid_desc *grid, const void *table, float scale, int32_t hidden, int32_t activation,
                 const float *w1, const float *b1, const float *w2, const float *b2, const float *wout,
                 const float *bout, const float *axis, int32_t n, int32_t x_begin, int32_t x_count, int32_t pool,
                 const float *xyz, int64_t n_points, const int64_t *n_device, float *value, uint16_t *grad_norm,
                 void *stream)
{
    if (!grid || !table || !(scale > 0.0f) || !(scale <= 3.0e38f)) return QF_ERR_INVALID_ARGUMENT;
    if (hidden != 16 && hidden != 32) return QF_ERR_UNSUPPORTED;
    if (activation != QF_ACT_RELU && activation != QF_ACT_ELU) return QF_ERR_UNSUPPORTED;
    if (!w1 || !b1 || !w2 || !b2 || !wout || !bout) return QF_ERR_INVALID_ARGUMENT;
    GridExtractArgs a = {};
    int rc = fill_grid_args(grid, &a.grid);
    if (rc != QF_OK) return rc;
    int src;
    int64_t n_groups;
    if (axis) {            // lattice source: no point list
        if (xyz || n_points != 0 || n_device) return QF_ERR_INVALID_ARGUMENT;
        if (pool != 1 && pool != 2) return QF_ERR_UNSUPPORTED;
        if (n < 1 || (int64_t)n * pool > 16384) return QF_ERR_INVALID_ARGUMENT;
        if (x_begin < 0 || x_count < 0 || (int64_t)x_begin + x_count > n) return QF_ERR_INVALID_ARGUMENT;
        src = pool == 2 ? GX_LATTICE_2 : GX_LATTICE_1;
        a.axis = axis;
        a.n = n;
        a.lat = n * pool;
        a.x_begin = x_begin;
        a.x_count = x_count;
        a.nbx = (int32_t)qf_div_up((int64_t)x_count * pool, 2);
        a.nby = (int32_t)qf_div_up(a.lat, 2);
        a.nbz = (int32_t)qf_div_up(a.lat, 4);
        a.n_groups = n_groups = qf_div_up(a.nbz, kTileZ) * kTileZ * (int64_t)a.nby * a.nbx;
    } else {               // point list: no lattice
        if (n != 0 || x_begin != 0 || x_count != 0 || pool != 1 || n_points < 0) return QF_ERR_INVALID_ARGUMENT;
        src = GX_LIST;
        a.xyz = xyz;
        a.n_points = n_points;
        a.n_dev = n_device;
        n_groups = (n_points + 15) / 16;
    }
    if (n_groups == 0) return QF_OK;
    if (!value || (src == GX_LIST && !xyz)) return QF_ERR_INVALID_ARGUMENT;
    a.table = table;
    a.scale = scale;
    a.w1 = w1; a.b1 = b1; a.w2 = w2; a.b2 = b2; a.wout = wout; a.bout = bout;
    a.value = value;
    a.grad = grad_norm;
    hipStream_t st = qf_stream(stream);
    if (activation == QF_ACT_RELU)
        return hidden == 16 ? launch_extract<R, QF_ACT_RELU, 16>(a, src, n_groups, st)
                            : launch_extract<R, QF_ACT_RELU, 32>(a, src, n_groups, st);
    return hidden == 16 ? launch_extract<R, QF_ACT_ELU, 16>(a, src, n_groups, st)
                        : launch_extract<R, QF_ACT_ELU, 32>(a, src, n_groups, st);
}

}  // namespace

extern "C" int qf_field_grid_extract(const qf_grid_desc *grid, const float *table, float scale, int32_t hidden,
                                     int32_t activation, const float *w1, const float *b1, const float *w2,
                                     const float *b2, const float *wout, const float *bout, const float *axis,
                                     int32_t n, int32_t x_begin, int32_t x_count, int32_t pool, const float *xyz,
                                     int64_t n_points, const int64_t *n_device, float *value, uint16_t *grad_norm,
                                     void *stream)
{
    return grid_extract<DeformRowF32>(grid, table, scale, hidden, activation, w1, b1, w2, b2, wout, bout, axis, n,
                                      x_begin, x_count, pool, xyz, n_points, n_device, value, grad_norm, stream);
}

extern "C" int qf_field_grid_extract_f16(const qf_grid_desc *grid, const uint16_t *table, float scale,
                                         int32_t hidden, int32_t activation, const float *w1, const float *b1,
                                         const float *w2, const float *b2, const float *wout, const float *bout,
                                         const float *axis, int32_t n, int32_t x_begin, int32_t x_count, int32_t pool,
                                         const float *xyz, int64_t n_points, const int64_t *n_device, float *value,
                                         uint16_t *grad_norm, void *stream)
{
    return grid_extract<DeformRowF16>(grid, table, scale, hidden, activation, w1, b1, w2, b2, wout, bout, axis, n,
                                      x_begin, x_count, pool, xyz, n_points, n_device, value, grad_norm, stream);
}
