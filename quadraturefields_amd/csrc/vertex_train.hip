// Training through the vertex table (include/qf_vertex_train.h): the backward of
// qf_vertex_shade_points, from dL/d rgb and dL/d sigma per sample to dL/d table.  One kernel in two phases per 256
// samples of a workgroup.  Phase A, a lane per sample: the forward is recomputed with the forward's own device functions
// (vertex_baked_device.h: the blend differentiated is the forward's bit for bit, nothing of size [n, W] crosses from the
// forward), the SG mixture is differentiated on the blend and the row dL/d blend goes to LDS.  Phase B, a lane per COLUMN:
// for every active sample of the wave in turn the lanes c < W add d_blend[c] * b_k to row v_k of the gradient, k = 0, 1,
// 2 -- one float-atomic wave instruction per (sample, vertex) that covers W contiguous floats of one row, the shape
// the memory side takes at full rate, where a lane per sample would put 64 lanes into 64 rows.
#include "qf_common.h"
#include "qf_vertex_train.h"
#include "vertex_baked_device.h"

#pragma clang fp contract(off)

namespace {

constexpr int kTrainThreads = 256;

// LDS floats per sample: the row width made odd, so that the 64 lanes of phase A, each writing column c of its own row,
// fall into different banks (11 / 19 / 47 / 61 for 1 / 2 / 6 / 8 lobes)
__host__ __device__ __forceinline__ int vertex_train_pitch(int n_lobes) { return vertex_row_width(n_lobes) | 1; }

// dL/d blend of one sample from dL/d rgb, written to its LDS row: sg_features_to_rgb_backward_kernel's formula
// (mlp_train.hip) on the blend.  d|lambda| is 0 at lambda = 0, as torch.abs; the axis gradient is projected orthogonally to
// the unit axis and divided by the norm.  The density column (W - 1) is the caller's.
// Two quantities of that formula are differences of nearly equal numbers whenever the view direction lies close to a
// lobe's axis: t = a_hat . d - 1 and the projection d - a_hat (a_hat . d).  In fp32 their rounding (6e-8 of an O(1) term)
// is the whole error of the lambda and axis gradients, which are themselves small there -- a few 1e-4 of the entry where
// the blend's own rounding accounts for 1e-5.  They are formed in fp64 from the fp32 blend (about 25 fp64 operations per
// lobe, against 3 W atomic adds per sample) and rounded once.  The sigmoid's derivative s (1 - s) is taken as
// u / (1 + u)^2 with u = exp(-|x|), which does not cancel for a saturated colour.  Every index of `blend` is a
// compile-time constant.
__device__ __forceinline__ void vertex_blend_shade_backward(const float (&blend)[kVertexRowMax], int n_lobes, float dx, float dy,
                                                            float dz, const float d_rgb[3], float *__restrict__ row)
{
    float e[QF_MAX_LOBES], t[QF_MAX_LOBES], cx[QF_MAX_LOBES], cy[QF_MAX_LOBES], cz[QF_MAX_LOBES];
    float pre[3] = {blend[0], blend[1], blend[2]};
#pragma unroll
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        if (l < n_lobes) {                         // wave-uniform
            const int o = 3 + 7 * l;
            const double x0 = blend[o], x1 = blend[o + 1], x2 = blend[o + 2];
            const double inv = 1.0 / sqrt((x0 * x0 + x1 * x1) + x2 * x2);
            const double ax = x0 * inv, ay = x1 * inv, az = x2 * inv;
            const double proj = (ax * dx + ay * dy) + az * dz;
            t[l] = (float)(proj - 1.0);
            cx[l] = (float)((dx - ax * proj) * inv);      // (I - a_hat a_hat^T) d / |a|
            cy[l] = (float)((dy - ay * proj) * inv);
            cz[l] = (float)((dz - az * proj) * inv);
            e[l] = expf(fabsf(blend[o + 3]) * t[l]);
            pre[0] += blend[o + 4] * e[l];
            pre[1] += blend[o + 5] * e[l];
            pre[2] += blend[o + 6] * e[l];
        }
    }
    float g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float u = expf(-fabsf(pre[k]));
        g[k] = d_rgb[k] * (u / ((1.0f + u) * (1.0f + u)));
        row[k] = g[k];
    }
#pragma unroll
    for (int l = 0; l < QF_MAX_LOBES; ++l) {
        if (l < n_lobes) {                         // wave-uniform
            const int o = 3 + 7 * l;
            const float lam = blend[o + 3];
            const float dE = (g[0] * blend[o + 4] + g[1] * blend[o + 5]) + g[2] * blend[o + 6];
            const float dEe = dE * e[l];
            const float dt = dEe * fabsf(lam);     // d(a_hat . d)
            row[o] = dt * cx[l];
            row[o + 1] = dt * cy[l];
            row[o + 2] = dt * cz[l];
            row[o + 3] = dEe * t[l] * (lam > 0.0f ? 1.0f : (lam < 0.0f ? -1.0f : 0.0f));
            row[o + 4] = g[0] * e[l];
            row[o + 5] = g[1] * e[l];
            row[o + 6] = g[2] * e[l];
        }
    }
}

// TriT: int64_t or int32_t, as vertex_shade_points_kernel.  Every thread of a workgroup makes the same number of trips
// (the barriers sit in the loop).  A sample contributes iff it lies below min(*n_dev, n), its record's 1 / det is finite
// (a degenerate face, or one qf_vertex_records_pack gave the ids 0, 0, 0: the forward's NaN never reaches row 0) and its
// three vertex ids lie in [0, n_vertices) -- the rows of any other sample are neither read nor written.
template <typename TriT>
__global__ __launch_bounds__(kTrainThreads) void vertex_shade_points_backward_kernel(
    const float *__restrict__ table, int stride, int n_lobes, const VertexTriRecord *__restrict__ records, int n_vertices,
    const float *__restrict__ points, const TriT *__restrict__ index_tri, const float *__restrict__ dirs, int64_t n,
    const int64_t *__restrict__ n_dev, const float *__restrict__ d_rgb, const float *__restrict__ d_sigma,
    float *__restrict__ grad_table)
{
    extern __shared__ float d_blend[];             // [kTrainThreads][pitch]
    if (n_dev) { const int64_t nd = *n_dev; n = nd < n ? (nd > 0 ? nd : 0) : n; }
    const int n16 = vertex_row_pieces(n_lobes), width = vertex_row_width(n_lobes), pitch = vertex_train_pitch(n_lobes);
    const int columns = d_sigma ? width : width - 1;       // a frozen density column gets no atomics
    const int lane = threadIdx.x & 63, wave_first = threadIdx.x & ~63;
    for (int64_t first = (int64_t)blockIdx.x * kTrainThreads; first < n; first += (int64_t)gridDim.x * kTrainThreads) {
        // phase A: a lane per sample
        const int64_t i = first + threadIdx.x;
        bool active = false;
        float b[3] = {0.0f, 0.0f, 0.0f};
        int v0 = 0, v1 = 0, v2 = 0;
        if (i < n) {
            const VertexTriRecord tr = records[index_tri[i]];
            v0 = tr.v[0]; v1 = tr.v[1]; v2 = tr.v[2];
            active = isfinite(tr.inv) && (unsigned)v0 < (unsigned)n_vertices && (unsigned)v1 < (unsigned)n_vertices &&
                     (unsigned)v2 < (unsigned)n_vertices;
            if (active) {
                vertex_barycentrics(tr, points[i * 3], points[i * 3 + 1], points[i * 3 + 2], b);
                float blend[kVertexRowMax];
                vertex_blend(table, stride, n16, v0, v1, v2, b, blend);
                const float g[3] = {d_rgb[i * 3], d_rgb[i * 3 + 1], d_rgb[i * 3 + 2]};
                float *row = d_blend + (int)threadIdx.x * pitch;
                vertex_blend_shade_backward(blend, n_lobes, dirs[i * 3], dirs[i * 3 + 1], dirs[i * 3 + 2], g, row);
                row[width - 1] = d_sigma ? d_sigma[i] : 0.0f;
            }
        }
        __syncthreads();
        // phase B: a lane per column; the wave's own 64 samples, one after the other
        unsigned long long todo = __ballot(active);
        while (todo != 0ull) {                     // wave-uniform
            const int s = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
            todo &= todo - 1ull;
            const int u0 = __builtin_amdgcn_readlane(v0, s), u1 = __builtin_amdgcn_readlane(v1, s),
                      u2 = __builtin_amdgcn_readlane(v2, s);
            const float c0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b[0]), s));
            const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b[1]), s));
            const float c2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(b[2]), s));
            if (lane < columns) {
                const float d = d_blend[(wave_first + s) * pitch + lane];
                atomicAdd(grad_table + (int64_t)u0 * stride + lane, d * c0);
                atomicAdd(grad_table + (int64_t)u1 * stride + lane, d * c1);
                atomicAdd(grad_table + (int64_t)u2 * stride + lane, d * c2);
            }
        }
        __syncthreads();                           // the rows are rewritten by the next trip
    }
}

}  // namespace

extern "C" int qf_vertex_shade_points_backward(const float *table, int32_t stride, int32_t n_lobes, const void *records,
                                               int64_t n_vertices, const float *points, const int64_t *index_tri,
                                               const int32_t *index_tri32, const float *dirs, int64_t n,
                                               const int64_t *n_device, const float *d_rgb, const float *d_sigma,
                                               float *grad_table, void *stream)
{
    if (!table || reinterpret_cast<uintptr_t>(table) % 16 != 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (stride != vertex_row_stride(n_lobes)) return QF_ERR_INVALID_ARGUMENT;
    if (!records || n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!points || !dirs || (!index_tri == !index_tri32)) return QF_ERR_INVALID_ARGUMENT;      // exactly one id array
    if (!d_rgb || !grad_table || reinterpret_cast<uintptr_t>(grad_table) % 16 != 0) return QF_ERR_INVALID_ARGUMENT;
    if (n_vertices < 1 || n_vertices > 0x7fffffff) return QF_ERR_INVALID_ARGUMENT;
    const VertexTriRecord *tr = static_cast<const VertexTriRecord *>(records);
    const size_t lds_bytes = (size_t)kTrainThreads * vertex_train_pitch(n_lobes) * sizeof(float);      // at most 62 464
    const dim3 grid(qf_grid_1d(n, kTrainThreads)), block(kTrainThreads);
    if (index_tri32) {
        hipLaunchKernelGGL(vertex_shade_points_backward_kernel<int32_t>, grid, block, lds_bytes, qf_stream(stream), table,
                           (int)stride, (int)n_lobes, tr, (int)n_vertices, points, index_tri32, dirs, n, n_device, d_rgb, d_sigma,
                           grad_table);
    } else {
        hipLaunchKernelGGL(vertex_shade_points_backward_kernel<int64_t>, grid, block, lds_bytes, qf_stream(stream), table,
                           (int)stride, (int)n_lobes, tr, (int)n_vertices, points, index_tri, dirs, n, n_device, d_rgb, d_sigma,
                           grad_table);
    }
    QF_LAUNCH_CHECK();
    return QF_OK;
}
