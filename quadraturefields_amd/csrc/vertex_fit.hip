// The vertex table fitted to a field over the surface (include/qf_vertex_fit.h; the rule is DESIGN.md section 3.9i,
// restated in numpy in tests/vertex_fit_reference.py).  Every floating-point operation is fp64 and rounded on its own
// (the file is built with -ffp-contract=off); no floating-point atomic is used: every sum is a gather in a stated order.
//
// Lanes run over columns: thread t of a [rows, C] launch has row t / C and column t % C, so the lanes of a wave read and
// write contiguous runs of the dense [V,C] fp64 vectors and of the table rows.
//
// Passes of qf_vertex_fit_assemble (one stream, no host wait):
//   validity  per sample, per target entry and per prior entry: the three tallies of rule 1; one thread then sets the
//             flag that every later kernel of both entry points reads on the device;
//   keys      per corner 3 f + i of a face that is not skipped: vertex << 32 | corner, so that rocPRIM's radix sort
//             leaves every vertex's corners in ascending (f, i); start / end of every vertex's run (the idiom of
//             mesh_decimate.hip, with the corner in the low word in place of the face);
//   gram      per face: its sample run by two binary searches of the non-decreasing face ids, then M_f and m_f over it;
//   vertex    per vertex: d_v, a_v, inv_v and lambda * d_v over its corner run;
//   rhs       per (vertex, column): B and the clamp bounds over the sample runs of its corners' faces.
// qf_vertex_fit_solve: init, then per step the operator (a gather over the corner runs), two dot products (a leaf kernel
// over 256 vertices by 16 columns in LDS and one workgroup that adds the block sums in order and derives the step's
// scalar) and two fused vector updates; then the two stats, the clamp and the fp32 table.
#include "mesh_device.h"
#include "qf_vertex_fit.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <cmath>

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr uint64_t kNone = ~uint64_t(0);        // the key of a corner of a skipped face: sorts behind every vertex
constexpr int kLeaf = 256;                      // vertices per leaf of a dot product (rule 6)
constexpr int kDotCols = 16;                    // columns per workgroup of the leaf kernel: 256 x 16 doubles of LDS
constexpr int kTile = 64;                       // block sums per column staged in LDS by the sequential pass
constexpr int kMaxCols = QF_VERTEX_FIT_MAX_COLUMNS;

struct Info {
    unsigned long long bad_sample_faces, unsorted, nonfinite, skipped_faces, skipped_samples, inactive, clamped;
    double lambda;
    int32_t refused;                    // 1: rule 1 refuses the input (written by verdict_kernel)
};

struct Workspace {
    Info *info;
    uint64_t *key_a, *key_b;            // [3F] corner keys, unsorted and sorted
    int32_t *cstart, *cend;             // [V] a vertex's run in key_b
    int32_t *run;                       // [F,2] a face's sample run
    double *face_m;                     // [F,3] m_f
    double *inv, *ld;                   // [V] inv_v and lambda * d_v
    float *lo, *hi;                     // [V,C] clamp bounds (they are fp32 values of the input)
    double *Z, *R, *P, *Q;              // [V,C]
    double *partial;                    // [ceil(V / 256), C] block sums of a dot product
    double *rho, *alpha, *beta;         // [64] per column
    void *temp;                         // rocPRIM's scratch
    size_t temp_bytes;
    int64_t bytes;
};

// Scratch set aside for rocPRIM's sort of the 3 F corner keys.  Its own size query needs a device for all but the smallest
// inputs, and the workspace size is a host computation that must not: the sort keeps one more buffer of keys and, per
// workgroup of a few thousand keys, a 256-bin histogram, so two buffers of keys and 4 MiB over is well above what it
// asks for; assemble checks the real figure against this before its first launch.
size_t temp_bytes_for(int64_t F) { return (size_t)(2 * 3 * F) * sizeof(uint64_t) + (size_t(4) << 20); }

Workspace carve(void *base, int64_t V, int64_t F, int64_t C, size_t temp)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.key_a = c.take<uint64_t>(3 * F);
    w.key_b = c.take<uint64_t>(3 * F);
    w.cstart = c.take<int32_t>(V);
    w.cend = c.take<int32_t>(V);
    w.run = c.take<int32_t>(2 * F);
    w.face_m = c.take<double>(3 * F);
    w.inv = c.take<double>(V);
    w.ld = c.take<double>(V);
    w.lo = c.take<float>(V * C);
    w.hi = c.take<float>(V * C);
    w.Z = c.take<double>(V * C);
    w.R = c.take<double>(V * C);
    w.P = c.take<double>(V * C);
    w.Q = c.take<double>(V * C);
    w.partial = c.take<double>(qf_div_up(V, kLeaf) * C);
    w.rho = c.take<double>(kMaxCols);
    w.alpha = c.take<double>(kMaxCols);
    w.beta = c.take<double>(kMaxCols);
    w.temp = c.take<char>((int64_t)temp);
    w.temp_bytes = temp;
    w.bytes = c.off;
    return w;
}

struct Job {
    const int64_t *f;
    const int64_t *sface;
    const double *bary;
    const float *y, *x0;
    int64_t F, V, N, ys, xs;
    int C;
};

__device__ __forceinline__ bool finite_bits(uint64_t w) { return (w & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

// fp32 bit patterns as unsigned keys in the order of the values, -0.0 below +0.0
__device__ __forceinline__ uint32_t order_key(float x)
{
    const uint32_t b = __float_as_uint(x);
    return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float order_value(uint32_t k)
{
    return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xffffffffu));
}

__device__ __forceinline__ bool face_ok(const int64_t *t, int64_t V)
{
    return t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V && t[0] != t[1] && t[1] != t[2] &&
           t[0] != t[2];
}

// ---------------------------------------------------------------------------------------------------------------- assemble

__global__ __launch_bounds__(kBlock) void validity_samples_kernel(Job J, Workspace ws)
{
    const int64_t s = gtid();
    int bad = 0, unsorted = 0, nonfinite = 0;
    if (s < J.N) {
        const int64_t face = J.sface[s];
        bad = face < 0 || face >= J.F;
        unsorted = s > 0 && face < J.sface[s - 1];
        const uint64_t *w = reinterpret_cast<const uint64_t *>(J.bary) + 3 * s;
        nonfinite = !finite_bits(w[0]) + !finite_bits(w[1]) + !finite_bits(w[2]);
    }
    tally(&ws.info->bad_sample_faces, bad);
    tally(&ws.info->unsorted, unsorted);
    tally(&ws.info->nonfinite, nonfinite);
}

// the first C columns of `rows` rows, `stride` floats apart
__global__ __launch_bounds__(kBlock) void validity_rows_kernel(const float *__restrict__ p, int64_t rows, int C,
                                                               int64_t stride, Workspace ws)
{
    const int64_t t = gtid();
    int nonfinite = 0;
    if (t < rows * C) {
        const int64_t r = t / C;
        const int c = (int)(t - r * C);
        nonfinite = (__float_as_uint(p[r * stride + c]) & 0x7f800000u) == 0x7f800000u;
    }
    tally(&ws.info->nonfinite, nonfinite);
}

__global__ void verdict_kernel(Workspace ws, double lambda)
{
    Info &I = *ws.info;
    I.refused = I.bad_sample_faces != 0 || I.unsorted != 0 || I.nonfinite != 0;
    I.lambda = lambda;
}

// Corner 3 f + i -> vertex << 32 | corner for a face that takes part, else kNone.
__global__ __launch_bounds__(kBlock) void corner_key_kernel(Job J, Workspace ws)
{
    const int64_t i = gtid();
    int skipped = 0;
    if (i < 3 * J.F) {
        const int64_t f = i / 3, k = i - 3 * f;
        const int64_t *t = J.f + 3 * f;
        const bool ok = face_ok(t, J.V);
        skipped = !ok && k == 0;
        ws.key_a[i] = ok ? ((uint64_t)t[k] << 32 | (uint64_t)i) : kNone;
    }
    tally(&ws.info->skipped_faces, skipped);
}

// start / end of every vertex's run in the sorted keys (rows of vertices without a corner stay at the memset's 0, 0).
__global__ __launch_bounds__(kBlock) void range_kernel(const uint64_t *keys, int64_t n, int32_t *start, int32_t *end)
{
    const int64_t j = gtid();
    if (j >= n) return;
    const uint64_t key = keys[j];
    if (key == kNone) return;
    const uint64_t v = key >> 32;
    if (j == 0 || (keys[j - 1] >> 32) != v) start[v] = (int32_t)j;
    if (j == n - 1 || keys[j + 1] == kNone || (keys[j + 1] >> 32) != v) end[v] = (int32_t)(j + 1);
}

// the first s with sface[s] >= f
__device__ __forceinline__ int64_t lower_bound(const int64_t *sface, int64_t n, int64_t f)
{
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (sface[mid] < f) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

__global__ __launch_bounds__(kBlock) void gram_kernel(Job J, Workspace ws, double *__restrict__ gram)
{
    if (ws.info->refused) return;       // the same for every thread of the grid
    const int64_t f = gtid();
    if (f >= J.F) return;
    const int64_t s0 = lower_bound(J.sface, J.N, f), s1 = lower_bound(J.sface, J.N, f + 1);
    if (!face_ok(J.f + 3 * f, J.V)) {
        if (s1 > s0) atomicAdd(&ws.info->skipped_samples, (unsigned long long)(s1 - s0));
        ws.run[2 * f] = 0;
        ws.run[2 * f + 1] = 0;
        return;                         // its gram stays at the memset's zeros; no corner key names it
    }
    double m0 = 0.0, m1 = 0.0, m2 = 0.0, g00 = 0.0, g01 = 0.0, g02 = 0.0, g11 = 0.0, g12 = 0.0, g22 = 0.0;
    for (int64_t s = s0; s < s1; ++s) {
        const double b0 = J.bary[3 * s], b1 = J.bary[3 * s + 1], b2 = J.bary[3 * s + 2];
        m0 += b0;
        m1 += b1;
        m2 += b2;
        g00 += b0 * b0;
        g01 += b0 * b1;
        g02 += b0 * b2;
        g11 += b1 * b1;
        g12 += b1 * b2;
        g22 += b2 * b2;
    }
    ws.run[2 * f] = (int32_t)s0;
    ws.run[2 * f + 1] = (int32_t)s1;
    ws.face_m[3 * f] = m0;
    ws.face_m[3 * f + 1] = m1;
    ws.face_m[3 * f + 2] = m2;
    double *g = gram + 9 * f;
    g[0] = g00, g[1] = g01, g[2] = g02;
    g[3] = g01, g[4] = g11, g[5] = g12;
    g[6] = g02, g[7] = g12, g[8] = g22;
}

__global__ __launch_bounds__(kBlock) void vertex_kernel(Job J, Workspace ws, const double *__restrict__ gram,
                                                        double *__restrict__ mass)
{
    if (ws.info->refused) return;
    const int64_t v = gtid();
    int inactive = 0;
    if (v < J.V) {
        double d = 0.0, a = 0.0;
        for (int32_t j = ws.cstart[v]; j < ws.cend[v]; ++j) {
            const int64_t corner = (int64_t)(ws.key_b[j] & 0xffffffffu);
            const int64_t f = corner / 3, i = corner - 3 * f;
            d += ws.face_m[corner];
            a += gram[9 * f + 4 * i];
        }
        const double ld = ws.info->lambda * d;
        a = a + ld;
        mass[v] = d;
        ws.ld[v] = ld;
        ws.inv[v] = a > 0.0 ? 1.0 / a : 0.0;
        inactive = d == 0.0;
    }
    tally(&ws.info->inactive, inactive);
}

__global__ __launch_bounds__(kBlock) void rhs_kernel(Job J, Workspace ws, double *__restrict__ rhs)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    if (t >= J.V * J.C) return;
    const int64_t v = t / J.C;
    const int c = (int)(t - v * J.C);
    uint32_t lo = order_key(J.x0[v * J.xs + c]), hi = lo;
    double B = 0.0;
    for (int32_t j = ws.cstart[v]; j < ws.cend[v]; ++j) {
        const int64_t corner = (int64_t)(ws.key_b[j] & 0xffffffffu);
        const int64_t f = corner / 3, i = corner - 3 * f;
        const int64_t *tri = J.f + 3 * f;
        const double x0 = (double)J.x0[tri[0] * J.xs + c], x1 = (double)J.x0[tri[1] * J.xs + c],
                     x2 = (double)J.x0[tri[2] * J.xs + c];
        double g = 0.0;
        for (int64_t s = ws.run[2 * f]; s < ws.run[2 * f + 1]; ++s) {
            const double *b = J.bary + 3 * s;
            const float y = J.y[s * J.ys + c];
            const double e = (double)y - ((b[0] * x0 + b[1] * x1) + b[2] * x2);
            g += b[i] * e;
            const uint32_t k = order_key(y);
            lo = k < lo ? k : lo;
            hi = k > hi ? k : hi;
        }
        B += g;
    }
    rhs[t] = B;
    ws.lo[t] = order_value(lo);
    ws.hi[t] = order_value(hi);
}

__global__ void counts_kernel(Workspace ws, int64_t *counts)
{
    const Info &I = *ws.info;
    counts[0] = (int64_t)I.bad_sample_faces;
    counts[1] = (int64_t)I.unsorted;
    counts[2] = (int64_t)I.nonfinite;
    counts[3] = I.refused ? 0 : (int64_t)I.skipped_faces;
    counts[4] = I.refused ? 0 : (int64_t)I.skipped_samples;
    counts[5] = I.refused ? 0 : (int64_t)I.inactive;
    counts[6] = I.refused ? 0 : (int64_t)I.clamped;
    counts[7] = I.refused;
}

// ------------------------------------------------------------------------------------------------------------------- solve

// Z = 0, R = B, P = S = inv * R
__global__ __launch_bounds__(kBlock) void init_kernel(Workspace ws, const double *__restrict__ rhs, int64_t V, int C)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    if (t >= V * C) return;
    const double r = rhs[t];
    ws.Z[t] = 0.0;
    ws.R[t] = r;
    ws.P[t] = ws.inv[t / C] * r;
}

// Q = A P (rule 5): a gather over the vertex's corner run
__global__ __launch_bounds__(kBlock) void operator_kernel(Workspace ws, const int64_t *__restrict__ faces,
                                                          const double *__restrict__ gram, int64_t V, int C)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    if (t >= V * C) return;
    const int64_t v = t / C;
    const int c = (int)(t - v * C);
    const double *P = ws.P;
    double acc = 0.0;
    for (int32_t j = ws.cstart[v]; j < ws.cend[v]; ++j) {
        const int64_t corner = (int64_t)(ws.key_b[j] & 0xffffffffu);
        const int64_t f = corner / 3;
        const int64_t *tri = faces + 3 * f;
        const double *g = gram + 3 * corner;            // row i of M_f: 9 f + 3 i
        acc += (g[0] * P[tri[0] * C + c] + g[1] * P[tri[1] * C + c]) + g[2] * P[tri[2] * C + c];
    }
    ws.Q[t] = acc + ws.ld[v] * P[t];
}

// The leaves of rule 6: the products of 256 vertices by 16 columns in LDS, the stride-halving tree, one block sum per
// column.  kMode 0: x * y;  1: x * (inv * x);  2: x * x.
template <int kMode>
__global__ __launch_bounds__(kBlock) void dot_leaf_kernel(Workspace ws, const double *__restrict__ x,
                                                          const double *__restrict__ y, int64_t V, int C)
{
    __shared__ double s_t[kLeaf * kDotCols];
    if (ws.info->refused) return;
    const int cl = threadIdx.x & (kDotCols - 1), r0 = threadIdx.x / kDotCols;
    const int c = blockIdx.y * kDotCols + cl;
    const int64_t v0 = (int64_t)blockIdx.x * kLeaf;
    for (int row = r0; row < kLeaf; row += kBlock / kDotCols) {
        const int64_t v = v0 + row;
        double p = 0.0;
        if (v < V && c < C) {
            const double xv = x[v * C + c];
            p = kMode == 0 ? xv * y[v * C + c] : kMode == 1 ? xv * (ws.inv[v] * xv) : xv * xv;
        }
        s_t[row * kDotCols + cl] = p;
    }
    __syncthreads();
    for (int s = kLeaf / 2; s >= 1; s >>= 1) {          // entry (i, cl) sits at i * 16 + cl: i + s is s * 16 further on
        for (int idx = threadIdx.x; idx < s * kDotCols; idx += kBlock) s_t[idx] = s_t[idx] + s_t[idx + s * kDotCols];
        __syncthreads();
    }
    if (threadIdx.x < kDotCols && c < C) ws.partial[(int64_t)blockIdx.x * C + c] = s_t[threadIdx.x];
}

// The block sums added in ascending block order (one workgroup; lane c owns column c; the sums go through LDS, 64 blocks
// at a time, so that their loads are coalesced and in flight together), and what the step derives from the sum.
// kKind 0: rho = sum;  1: alpha = sum > 0 ? rho / sum : 0;  2: beta = rho > 0 ? sum / rho : 0, rho = sum;
// 3, 4: stats[2 c + kKind - 3] = sqrt(sum).
template <int kKind>
__global__ __launch_bounds__(kBlock) void dot_final_kernel(Workspace ws, int64_t n_blocks, int C, double *__restrict__ stats)
{
    __shared__ double s_t[kTile * kMaxCols];
    if (ws.info->refused) return;
    double sum = 0.0;
    for (int64_t base = 0; base < n_blocks; base += kTile) {
        const int rows = n_blocks - base < kTile ? (int)(n_blocks - base) : kTile;
        for (int idx = threadIdx.x; idx < rows * C; idx += kBlock) s_t[idx] = ws.partial[base * C + idx];
        __syncthreads();
        if ((int)threadIdx.x < C)
            for (int r = 0; r < rows; ++r) sum += s_t[r * C + threadIdx.x];
        __syncthreads();
    }
    const int c = threadIdx.x;
    if (c >= C) return;
    if (kKind == 0) {
        ws.rho[c] = sum;
    } else if (kKind == 1) {
        ws.alpha[c] = sum > 0.0 ? ws.rho[c] / sum : 0.0;
    } else if (kKind == 2) {
        const double rho = ws.rho[c];
        ws.beta[c] = rho > 0.0 ? sum / rho : 0.0;
        ws.rho[c] = sum;
    } else {
        stats[2 * c + (kKind - 3)] = sqrt(sum);
    }
}

// Z = Z + alpha P, R = R - alpha Q
__global__ __launch_bounds__(kBlock) void update_zr_kernel(Workspace ws, int64_t V, int C)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    if (t >= V * C) return;
    const double a = ws.alpha[t % C];
    ws.Z[t] = ws.Z[t] + a * ws.P[t];
    ws.R[t] = ws.R[t] - a * ws.Q[t];
}

// P = inv R + beta P
__global__ __launch_bounds__(kBlock) void update_p_kernel(Workspace ws, int64_t V, int C)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    if (t >= V * C) return;
    const int64_t v = t / C;
    const double s = ws.inv[v] * ws.R[t];
    ws.P[t] = s + ws.beta[t - v * C] * ws.P[t];
}

// rules 8 and 9
__global__ __launch_bounds__(kBlock) void finish_kernel(Workspace ws, const float *__restrict__ x0, int64_t xs,
                                                        const double *__restrict__ mass, uint64_t mask, int64_t V, int C,
                                                        float *__restrict__ out, int64_t os)
{
    if (ws.info->refused) return;
    const int64_t t = gtid();
    int moved = 0;
    if (t < V * C) {
        const int64_t v = t / C;
        const int c = (int)(t - v * C);
        const float prior = x0[v * xs + c];
        float result = prior;                           // an inactive vertex keeps the bits of its prior row
        if (mass[v] != 0.0) {
            double X = (double)prior + ws.Z[t];
            if ((mask >> c) & 1) {
                const double lo = (double)ws.lo[t], hi = (double)ws.hi[t];
                if (X < lo) {
                    X = lo;
                    moved = 1;
                } else if (X > hi) {
                    X = hi;
                    moved = 1;
                }
            }
            result = (float)X;
        }
        out[v * os + c] = result;
    }
    tally(&ws.info->clamped, moved);
}

bool sizes_ok(int64_t V, int64_t F, int64_t N, int64_t C)
{
    return V >= 1 && V < kMaxCount && F >= 0 && 3 * F < kMaxCount && N >= 0 && N < kMaxCount && C >= 1 && C <= kMaxCols;
}

}  // namespace

extern "C" int64_t qf_vertex_fit_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_samples, int64_t n_columns)
{
    if (!sizes_ok(n_vertices, n_faces, n_samples, n_columns)) return -1;
    return carve(nullptr, n_vertices, n_faces, n_columns, temp_bytes_for(n_faces)).bytes;
}

extern "C" int qf_vertex_fit_assemble(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *sample_face,
                                      const double *sample_bary, int64_t n_samples, const float *targets, int64_t y_stride,
                                      const float *prior, int64_t x0_stride, int64_t n_columns, double prior_weight,
                                      double *face_gram, double *vertex_mass, double *rhs, void *workspace,
                                      int64_t workspace_bytes, int64_t *counts, void *stream)
{
    const int64_t V = n_vertices, F = n_faces, N = n_samples, C = n_columns;
    if (!sizes_ok(V, F, N, C) || y_stride < C || x0_stride < C || !(prior_weight >= 0.0) || std::isinf(prior_weight))
        return QF_ERR_INVALID_ARGUMENT;
    if ((F > 0 && (!faces || !face_gram)) || (N > 0 && (!sample_face || !sample_bary || !targets)) || !prior ||
        !vertex_mass || !rhs || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    Workspace ws = carve(workspace, V, F, C, temp_bytes_for(F));
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    if (F > 0) {
        size_t tb = 0;
        QF_HIP_TRY(rocprim::radix_sort_keys(nullptr, tb, ws.key_a, ws.key_b, (size_t)(3 * F), 0, 64, s));
        if (tb > ws.temp_bytes) return QF_ERR_UNSUPPORTED;
    }
    const Job J{faces, sample_face, sample_bary, targets, prior, F, V, N, y_stride, x0_stride, (int)C};

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ws.cstart, 0, sizeof(int32_t) * V, s));
    QF_HIP_TRY(hipMemsetAsync(ws.cend, 0, sizeof(int32_t) * V, s));
    QF_HIP_TRY(hipMemsetAsync(vertex_mass, 0, sizeof(double) * V, s));
    QF_HIP_TRY(hipMemsetAsync(rhs, 0, sizeof(double) * V * C, s));
    if (F > 0) QF_HIP_TRY(hipMemsetAsync(face_gram, 0, sizeof(double) * 9 * F, s));
    QF_MESH_LAUNCH(validity_samples_kernel, N, J, ws);
    QF_MESH_LAUNCH(validity_rows_kernel, N * C, targets, N, (int)C, y_stride, ws);
    QF_MESH_LAUNCH(validity_rows_kernel, V * C, prior, V, (int)C, x0_stride, ws);
    hipLaunchKernelGGL(verdict_kernel, dim3(1), dim3(1), 0, s, ws, prior_weight);
    QF_LAUNCH_CHECK();
    if (F > 0) {
        QF_MESH_LAUNCH(corner_key_kernel, 3 * F, J, ws);
        size_t tb = ws.temp_bytes;
        QF_HIP_TRY(rocprim::radix_sort_keys(ws.temp, tb, ws.key_a, ws.key_b, (size_t)(3 * F), 0, 64, s));
        QF_MESH_LAUNCH(range_kernel, 3 * F, ws.key_b, 3 * F, ws.cstart, ws.cend);
        QF_MESH_LAUNCH(gram_kernel, F, J, ws, face_gram);
    }
    QF_MESH_LAUNCH(vertex_kernel, V, J, ws, face_gram, vertex_mass);
    QF_MESH_LAUNCH(rhs_kernel, V * C, J, ws, rhs);
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_vertex_fit_solve(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const float *prior,
                                   int64_t x0_stride, int64_t n_columns, const double *face_gram, const double *vertex_mass,
                                   const double *rhs, int64_t iterations, uint64_t clamp_mask, void *workspace,
                                   int64_t workspace_bytes, float *out, int64_t out_stride, double *stats, int64_t *counts,
                                   void *stream)
{
    const int64_t V = n_vertices, F = n_faces, C = n_columns;
    if (!sizes_ok(V, F, 0, C) || x0_stride < C || out_stride < C || iterations < 0 || iterations >= kMaxCount)
        return QF_ERR_INVALID_ARGUMENT;
    if ((F > 0 && (!faces || !face_gram)) || !prior || !vertex_mass || !rhs || !workspace || !out || !stats || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    Workspace ws = carve(workspace, V, F, C, temp_bytes_for(F));
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const int64_t n = V * C, n_blocks = qf_div_up(V, kLeaf);
    const dim3 leaf_grid((unsigned)n_blocks, (unsigned)qf_div_up(C, kDotCols));
    const int Ci = (int)C;

#define QF_FIT_DOT(mode, kind, x, y)                                                                            \
    do {                                                                                                        \
        hipLaunchKernelGGL(dot_leaf_kernel<mode>, leaf_grid, dim3(kBlock), 0, s, ws, x, y, V, Ci);              \
        QF_LAUNCH_CHECK();                                                                                      \
        hipLaunchKernelGGL(dot_final_kernel<kind>, dim3(1), dim3(kBlock), 0, s, ws, n_blocks, Ci, stats);       \
        QF_LAUNCH_CHECK();                                                                                      \
    } while (0)

    QF_HIP_TRY(hipMemsetAsync(&ws.info->clamped, 0, sizeof(unsigned long long), s));
    QF_HIP_TRY(hipMemsetAsync(stats, 0, sizeof(double) * 2 * C, s));
    QF_MESH_LAUNCH(init_kernel, n, ws, rhs, V, Ci);
    QF_FIT_DOT(1, 0, ws.R, (const double *)nullptr);
    for (int64_t k = 0; k < iterations; ++k) {
        QF_MESH_LAUNCH(operator_kernel, n, ws, faces, face_gram, V, Ci);
        QF_FIT_DOT(0, 1, ws.P, ws.Q);
        QF_MESH_LAUNCH(update_zr_kernel, n, ws, V, Ci);
        QF_FIT_DOT(1, 2, ws.R, (const double *)nullptr);
        QF_MESH_LAUNCH(update_p_kernel, n, ws, V, Ci);
    }
    QF_FIT_DOT(2, 3, rhs, (const double *)nullptr);
    QF_FIT_DOT(2, 4, ws.R, (const double *)nullptr);
    QF_MESH_LAUNCH(finish_kernel, n, ws, prior, x0_stride, vertex_mass, clamp_mask, V, Ci, out, out_stride);
    hipLaunchKernelGGL(counts_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
#undef QF_FIT_DOT
    return QF_OK;
}
