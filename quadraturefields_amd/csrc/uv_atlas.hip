// Per-triangle UV atlas of a triangle mesh: every face gets its own staircase of texels, packed on shelves with no
// waste.  It stands where the reference runs the ScanNet segmentator and xatlas (examples/generate_uv_xatlas_old.py);
// the baked path looks textures up by nearest texel, so chart seams cost nothing.  The rules (DESIGN.md section 3.12;
// restated in numpy in tests/uv_atlas_reference.py), with S the atlas side, N the largest leg and delta = 1/16:
//   measure   face (a, b, c): u = b - a, w = c - a, n = u x w, len = sqrt((n0 n0 + n1 n1) + n2 n2), l = sqrt(len): the
//             leg of the right isosceles triangle of the face's area;
//   class     q = floor(rho l); k = N if q >= N, q if q > 0, else 0.  A class-k chart is the staircase dr + dc <= k of
//             (k+1)(k+2)/2 texels; two of them, one rotated by 180 degrees, tile a block of k+1 rows by k+2 columns;
//   order     stable sort by (N - k) << 30 | morton30(g), g the centroid ((a + b) + c) / 3 quantised per axis to
//             min(1023, floor((g - lo) / (hi - lo) * 1024)) over the bounding box of all vertices (0 if hi == lo);
//   place     face j of its class run: block j >> 1, half j & 1; P_k = (S-1) / (k+2) blocks per shelf of k+1 rows;
//             class k starts at row Y_k = sum over k' > k of shelves_k' (k'+1); the last row and column stay empty;
//   corners   in texels, then one division by S; lower half (r0+d, c0+d), (r0+k+1-2d, c0+d), (r0+d, c0+k+1-2d); upper
//             half (r0+k+1-d, c0+k+2-d), (r0+2d, c0+k+2-d), (r0+k+1-d, c0+1+2d); the right angle goes to the face
//             vertex opposite the longest edge (ties: the lowest corner), the others follow in cyclic order.
//
// Passes (one stream, no host wait inside a call):
//   measure   min / max / validity reduction -> one thread for the box and the checks -> one lane per face: l, the
//             longest edge, the Morton code; counts[3];
//   probe     class histogram (LDS bins, one integer atomic per bin and workgroup) -> one wave lays the shelves out
//             (classes on lanes, wave scan); result[4];
//   emit      probe at the final rho -> keys -> stable radix sort of (key, face) -> rank of every face -> one lane
//             per face places it; vertices and UVs leave as flat, contiguous stores.
// Every value is a function of the rules: the only atomics add integers.  The file is compiled with
// -ffp-contract=off: every product and sum is rounded on its own.
#pragma clang fp contract(off)

#include <cmath>

#include <rocprim/device/device_radix_sort.hpp>

#include "mesh_device.h"

namespace {

constexpr int kRedBlocks = 512;
constexpr int kClasses = 64;                    // max_leg <= 63
constexpr int kKeyBits = 36;                    // 6 bits of class above 30 bits of Morton code
constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr int32_t kMaxSide = 16384;
constexpr double kDelta = 0.0625;

struct Info {
    double lo[3], hi[3];
    int32_t valid;                              // written by measure: finite vertices, face indices in range
    int32_t fits;                               // written by every probe
};

struct Workspace {
    Info *info;
    double *red;                                // [kRedBlocks][6] per-block min xyz, max xyz over finite vertices
    int64_t *red_bad;                           // [kRedBlocks][2] non-finite vertices, out-of-range faces
    double *ell;                                // [F]
    uint32_t *morton;                           // [F]
    uint8_t *apex;                              // [F] corner opposite the longest edge
    uint32_t *hist;                             // [kClasses]
    int64_t *first_row;                         // [kClasses] Y_k
    int32_t *start;                             // [kClasses] first sorted position of class k
    uint64_t *key_a, *key_b;                    // [F]
    int32_t *fid_a, *fid_b;                     // [F]
    int32_t *rank;                              // [F] sorted position of face f
    void *temp;
    size_t temp_bytes;
    int64_t bytes;
};

size_t temp_bytes_for(int64_t F, hipStream_t s)
{
    size_t b = 0;
    if (rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, (size_t)F, 0, kKeyBits, s) != hipSuccess)
        return 0;
    return b > 0 ? b : 1;
}

Workspace carve(void *base, int64_t F, size_t temp)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.red = c.take<double>(6 * kRedBlocks);
    w.red_bad = c.take<int64_t>(2 * kRedBlocks);
    w.ell = c.take<double>(F);
    w.morton = c.take<uint32_t>(F);
    w.apex = c.take<uint8_t>(F);
    w.hist = c.take<uint32_t>(kClasses);
    w.first_row = c.take<int64_t>(kClasses);
    w.start = c.take<int32_t>(kClasses);
    w.key_a = c.take<uint64_t>(F);
    w.key_b = c.take<uint64_t>(F);
    w.fid_a = c.take<int32_t>(F);
    w.fid_b = c.take<int32_t>(F);
    w.rank = c.take<int32_t>(F);
    w.temp = c.take<char>((int64_t)temp);
    w.temp_bytes = temp;
    w.bytes = c.off;
    return w;
}

struct Mesh {
    const double *v;
    const int64_t *f;
    int64_t V, F;
};

// Per block: min / max of the finite vertices, the count of non-finite vertices and of faces with an index outside
// [0, V).  Min and max do not depend on order; the counts are integers.
__global__ __launch_bounds__(kBlock) void reduce_kernel(Mesh M, Workspace ws)
{
    __shared__ double lds[6][kBlock];
    __shared__ int64_t ldb[2][kBlock];
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int64_t bad_v = 0, bad_f = 0;
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t i = gtid(); i < M.V; i += stride) {
        const double x[3] = {M.v[3 * i], M.v[3 * i + 1], M.v[3 * i + 2]};
        if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) {
            ++bad_v;
            continue;
        }
        for (int k = 0; k < 3; ++k) {
            mn[k] = fmin(mn[k], x[k]);
            mx[k] = fmax(mx[k], x[k]);
        }
    }
    for (int64_t i = gtid(); i < M.F; i += stride) {
        const int64_t a = M.f[3 * i], b = M.f[3 * i + 1], c = M.f[3 * i + 2];
        bad_f += (a < 0 || a >= M.V || b < 0 || b >= M.V || c < 0 || c >= M.V);
    }
    const int t = threadIdx.x;
    for (int k = 0; k < 3; ++k) {
        lds[k][t] = mn[k];
        lds[3 + k][t] = mx[k];
    }
    ldb[0][t] = bad_v;
    ldb[1][t] = bad_f;
    __syncthreads();
    for (int o = kBlock / 2; o > 0; o >>= 1) {
        if (t < o) {
            for (int k = 0; k < 3; ++k) {
                lds[k][t] = fmin(lds[k][t], lds[k][t + o]);
                lds[3 + k][t] = fmax(lds[3 + k][t], lds[3 + k][t + o]);
            }
            ldb[0][t] += ldb[0][t + o];
            ldb[1][t] += ldb[1][t + o];
        }
        __syncthreads();
    }
    if (t == 0) {
        for (int k = 0; k < 6; ++k) ws.red[6 * blockIdx.x + k] = lds[k][0];
        ws.red_bad[2 * blockIdx.x] = ldb[0][0];
        ws.red_bad[2 * blockIdx.x + 1] = ldb[1][0];
    }
}

// One thread: the bounding box, the validity flag and counts[0..1]; counts[2] zeroed.
__global__ void finalize_kernel(Workspace ws, int64_t *counts)
{
    double mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    int64_t bad_v = 0, bad_f = 0;
    for (int b = 0; b < kRedBlocks; ++b) {
        for (int k = 0; k < 3; ++k) {
            mn[k] = fmin(mn[k], ws.red[6 * b + k]);
            mx[k] = fmax(mx[k], ws.red[6 * b + 3 + k]);
        }
        bad_v += ws.red_bad[2 * b];
        bad_f += ws.red_bad[2 * b + 1];
    }
    for (int k = 0; k < 3; ++k) {
        ws.info->lo[k] = mn[k];
        ws.info->hi[k] = mx[k];
    }
    ws.info->valid = (bad_v == 0 && bad_f == 0) ? 1 : 0;
    ws.info->fits = 0;
    counts[0] = bad_v;
    counts[1] = bad_f;
    counts[2] = 0;
}

__device__ __forceinline__ uint32_t spread3(uint32_t x)          // bit i of a 10-bit value -> bit 3 i
{
    x &= 0x3ffu;
    x = (x | (x << 16)) & 0x030000ffu;
    x = (x | (x << 8)) & 0x0300f00fu;
    x = (x | (x << 4)) & 0x030c30c3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

__device__ __forceinline__ uint32_t quantise(double g, double lo, double hi)
{
    if (hi == lo) return 0;
    const double t = (g - lo) / (hi - lo) * 1024.0;
    return t >= 1023.0 ? 1023u : (t > 0.0 ? (uint32_t)floor(t) : 0u);      // a NaN lands on 0
}

__device__ __forceinline__ double dot3(double x, double y, double z) { return (x * x + y * y) + z * z; }

// One lane per face.  The block's 3 * kBlock indices are loaded as one contiguous run and handed out through LDS.
__global__ __launch_bounds__(kBlock) void measure_kernel(Mesh M, Workspace ws, int64_t *counts)
{
    __shared__ int64_t idx[3 * kBlock];
    if (!ws.info->valid) return;                 // uniform: the indices may not be trusted
    const int64_t base = (int64_t)blockIdx.x * kBlock;
    for (int i = threadIdx.x; i < 3 * kBlock; i += kBlock) {
        const int64_t g = 3 * base + i;
        idx[i] = g < 3 * M.F ? M.f[g] : 0;
    }
    __syncthreads();
    const int64_t f = base + threadIdx.x;
    bool positive = false;
    if (f < M.F) {
        const double *a = M.v + 3 * idx[3 * threadIdx.x], *b = M.v + 3 * idx[3 * threadIdx.x + 1],
                     *c = M.v + 3 * idx[3 * threadIdx.x + 2];
        const double a0 = a[0], a1 = a[1], a2 = a[2], b0 = b[0], b1 = b[1], b2 = b[2], c0 = c[0], c1 = c[1], c2 = c[2];
        const double u0 = b0 - a0, u1 = b1 - a1, u2 = b2 - a2;
        const double w0 = c0 - a0, w1 = c1 - a1, w2 = c2 - a2;
        const double n0 = u1 * w2 - u2 * w1;
        const double n1 = u2 * w0 - u0 * w2;
        const double n2 = u0 * w1 - u1 * w0;
        const double ell = sqrt(sqrt(dot3(n0, n1, n2)));
        // squared lengths of the edges opposite corners 0, 1, 2
        const double e0 = dot3(c0 - b0, c1 - b1, c2 - b2), e1 = dot3(a0 - c0, a1 - c1, a2 - c2), e2 = dot3(u0, u1, u2);
        int apex = e1 > e0 ? 1 : 0;
        if (e2 > (apex ? e1 : e0)) apex = 2;
        const Info &I = *ws.info;
        const uint32_t qx = quantise(((a0 + b0) + c0) / 3.0, I.lo[0], I.hi[0]);
        const uint32_t qy = quantise(((a1 + b1) + c1) / 3.0, I.lo[1], I.hi[1]);
        const uint32_t qz = quantise(((a2 + b2) + c2) / 3.0, I.lo[2], I.hi[2]);
        ws.ell[f] = ell;
        ws.apex[f] = (uint8_t)apex;
        ws.morton[f] = spread3(qx) << 2 | spread3(qy) << 1 | spread3(qz);
        positive = ell > 0.0;
    }
    const unsigned long long m = __ballot(positive);
    if ((threadIdx.x & 63) == 0 && m)             // counts[2]: faces with l > 0, one integer atomic per wave
        atomicAdd(reinterpret_cast<unsigned long long *>(counts + 2), (unsigned long long)__popcll(m));
}

__device__ __forceinline__ int class_of(double rho, double ell, int N)
{
    const double q = floor(rho * ell);
    return q >= (double)N ? N : (q > 0.0 ? (int)q : 0);                   // a NaN lands on 0
}

__global__ __launch_bounds__(kBlock) void histogram_kernel(int64_t F, double rho, int N, Workspace ws)
{
    __shared__ uint32_t bins[kClasses];
    if (!ws.info->valid) return;                 // uniform: measure wrote no l; the histogram stays zero
    if (threadIdx.x < kClasses) bins[threadIdx.x] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t f = gtid(); f < F; f += stride) atomicAdd(&bins[class_of(rho, ws.ell[f], N)], 1u);
    __syncthreads();
    if (threadIdx.x < kClasses && bins[threadIdx.x]) atomicAdd(&ws.hist[threadIdx.x], bins[threadIdx.x]);
}

__device__ __forceinline__ int64_t wave_inclusive_scan(int64_t x, int lane)
{
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t y = __shfl_up((long long)x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}

// One wave.  Lane i holds class k = 63 - i, so that a prefix over lower lanes is a sum over taller classes.
// result[4] = rows_used, texels_used, faces of class N, fits; class_counts [N + 1] may be NULL.  After a refused
// measure the histogram is empty: everything is zero and fits is 0.
__global__ __launch_bounds__(64) void layout_kernel(int32_t S, int N, Workspace ws, int64_t *result,
                                                    int64_t *class_counts)
{
    const int lane = threadIdx.x, k = kClasses - 1 - lane;
    const int64_t cnt = k <= N ? (int64_t)ws.hist[k] : 0;
    const int64_t per_shelf = k <= N ? (S - 1) / (k + 2) : 1;            // >= 1: S >= N + 3
    const int64_t blocks = (cnt + 1) >> 1;
    const int64_t rows = (blocks + per_shelf - 1) / per_shelf * (k + 1);
    const int64_t texels = cnt * ((int64_t)(k + 1) * (k + 2) / 2);
    const int64_t rows_in = wave_inclusive_scan(rows, lane);
    const int64_t cnt_in = wave_inclusive_scan(cnt, lane);
    const int64_t tex_in = wave_inclusive_scan(texels, lane);
    ws.first_row[k] = rows_in - rows;
    ws.start[k] = (int32_t)(cnt_in - cnt);
    if (class_counts && k <= N) class_counts[k] = cnt;
    if (k == N) result[2] = cnt;
    if (lane == kClasses - 1) {
        const int fits = ws.info->valid && rows_in <= (int64_t)S - 1;
        result[0] = rows_in;
        result[1] = tex_in;
        result[3] = fits;
        ws.info->fits = fits;
    }
}

__global__ __launch_bounds__(kBlock) void key_kernel(int64_t F, double rho, int N, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= F) return;
    if (!ws.info->valid) {                       // measure wrote neither l nor the codes
        ws.key_a[f] = 0;
        ws.fid_a[f] = (int32_t)f;
        return;
    }
    const int k = class_of(rho, ws.ell[f], N);
    ws.key_a[f] = (uint64_t)(N - k) << 30 | ws.morton[f];
    ws.fid_a[f] = (int32_t)f;
}

__global__ __launch_bounds__(kBlock) void rank_kernel(int64_t F, Workspace ws)
{
    const int64_t j = gtid();
    if (j < F) ws.rank[ws.fid_b[j]] = (int32_t)j;
}

struct Out {
    double *vertices;           // [3F, 3]
    double *uv;                 // [3F, 2]
    int32_t *face_class;        // [F]
    int32_t *face_origin;       // [F, 2]
    uint8_t *face_half;         // [F]
};

// One lane per face places it; then the block's 9 * kBlock vertex coordinates and 6 * kBlock UV coordinates are
// written as flat runs, consecutive lanes on consecutive doubles.
__global__ __launch_bounds__(kBlock) void emit_kernel(Mesh M, double rho, int N, int32_t S, Workspace ws, Out out)
{
    __shared__ int64_t first_row[kClasses];
    __shared__ int32_t start[kClasses];
    __shared__ int32_t r0s[kBlock], c0s[kBlock], shape[kBlock];          // shape: k | half << 8 | apex << 16
    if (!ws.info->valid || !ws.info->fits) return;                        // uniform
    const int t = threadIdx.x;
    if (t < kClasses) {
        first_row[t] = ws.first_row[t];
        start[t] = ws.start[t];
    }
    __syncthreads();
    const int64_t base = (int64_t)blockIdx.x * kBlock, f = base + t;
    if (f < M.F) {
        const int k = class_of(rho, ws.ell[f], N);
        const int32_t j = ws.rank[f] - start[k];
        const int32_t block = j >> 1, half = j & 1, per_shelf = (S - 1) / (k + 2);
        const int32_t r0 = (int32_t)(first_row[k] + (int64_t)(block / per_shelf) * (k + 1));
        const int32_t c0 = (block % per_shelf) * (k + 2);
        r0s[t] = r0;
        c0s[t] = c0;
        shape[t] = k | half << 8 | (int32_t)ws.apex[f] << 16;
        out.face_class[f] = k;
        out.face_origin[2 * f] = r0;
        out.face_origin[2 * f + 1] = c0;
        out.face_half[f] = (uint8_t)half;
    }
    __syncthreads();
    for (int i = t; i < 9 * kBlock; i += kBlock) {
        const int fl = i / 9, c = i - 9 * fl;
        if (base + fl >= M.F) break;
        const int64_t v = M.f[3 * (base + fl) + c / 3];
        out.vertices[9 * base + i] = M.v[3 * v + c % 3];
    }
    const double side = (double)S;
    for (int i = t; i < 6 * kBlock; i += kBlock) {
        const int fl = i / 6, c = i - 6 * fl;
        if (base + fl >= M.F) break;
        const int sh = shape[fl], k = sh & 0xff, half = (sh >> 8) & 1, apex = sh >> 16;
        const int corner = c >> 1, col = c & 1;
        const int p = (corner - apex + 3) % 3;                            // the apex gets p0, the next corner p1
        const double o = col ? (double)c0s[fl] : (double)r0s[fl];
        double x;                                                         // every sum below is exact
        if (half == 0) {
            x = (p == (col ? 2 : 1)) ? (o + (double)(k + 1)) - 2.0 * kDelta : o + kDelta;
        } else if (col == 0) {
            x = p == 1 ? o + 2.0 * kDelta : (o + (double)(k + 1)) - kDelta;
        } else {
            x = p == 2 ? (o + 1.0) + 2.0 * kDelta : (o + (double)(k + 2)) - kDelta;
        }
        out.uv[6 * base + i] = x / side;
    }
}

bool faces_ok(int64_t F) { return F >= 1 && 3 * F < kMaxCount; }

bool shape_ok(int32_t max_leg, int32_t S) { return max_leg >= 0 && max_leg < kClasses && S >= max_leg + 3 && S <= kMaxSide; }

int probe(int64_t F, double rho, int N, int32_t S, const Workspace &ws, int64_t *result, int64_t *class_counts,
          hipStream_t s)
{
    QF_HIP_TRY(hipMemsetAsync(ws.hist, 0, 4 * kClasses, s));
    hipLaunchKernelGGL(histogram_kernel, dim3(qf_grid_1d(F, kBlock)), dim3(kBlock), 0, s, F, rho, N, ws);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(layout_kernel, dim3(1), dim3(64), 0, s, S, N, ws, result, class_counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

}  // namespace

extern "C" int64_t qf_uv_atlas_workspace_bytes(int64_t n_faces)
{
    if (!faces_ok(n_faces)) return -1;
    const size_t temp = temp_bytes_for(n_faces, nullptr);
    if (temp == 0) return -1;
    return carve(nullptr, n_faces, temp).bytes;
}

extern "C" int qf_uv_atlas_measure(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                   void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream)
{
    if (!faces_ok(n_faces) || n_vertices < 1 || n_vertices >= kMaxCount || !vertices || !faces || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(n_faces, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, n_faces, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const Mesh M = {vertices, faces, n_vertices, n_faces};
    hipLaunchKernelGGL(reduce_kernel, dim3(kRedBlocks), dim3(kBlock), 0, s, M, ws);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
    QF_MESH_LAUNCH(measure_kernel, n_faces, M, ws, counts);
    return QF_OK;
}

extern "C" int qf_uv_atlas_probe(int64_t n_faces, double texels_per_unit, int32_t max_leg, int32_t texture_size,
                                 void *workspace, int64_t workspace_bytes, int64_t *result, void *stream)
{
    if (!faces_ok(n_faces) || !shape_ok(max_leg, texture_size) || !(texels_per_unit >= 0.0) ||
        !std::isfinite(texels_per_unit) || !workspace || !result)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    // the sort scratch is the last region of the carve and a probe does not touch it: no size query per probe
    Workspace ws = carve(workspace, n_faces, 1);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    return probe(n_faces, texels_per_unit, max_leg, texture_size, ws, result, nullptr, s);
}

extern "C" int qf_uv_atlas_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                double texels_per_unit, int32_t max_leg, int32_t texture_size, void *workspace,
                                int64_t workspace_bytes, double *out_vertices, double *out_uv, int32_t *face_class,
                                int32_t *face_origin, uint8_t *face_half, int64_t *class_counts, int64_t *result,
                                void *stream)
{
    if (!faces_ok(n_faces) || n_vertices < 1 || n_vertices >= kMaxCount || !shape_ok(max_leg, texture_size) ||
        !(texels_per_unit >= 0.0) || !std::isfinite(texels_per_unit) || !vertices || !faces || !workspace ||
        !out_vertices || !out_uv || !face_class || !face_origin || !face_half || !class_counts || !result)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(n_faces, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, n_faces, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const int64_t F = n_faces;
    const int status = probe(F, texels_per_unit, max_leg, texture_size, ws, result, class_counts, s);
    if (status != QF_OK) return status;
    QF_MESH_LAUNCH(key_kernel, F, F, texels_per_unit, (int)max_leg, ws);
    size_t tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.key_a, ws.key_b, ws.fid_a, ws.fid_b, (size_t)F, 0, kKeyBits, s));
    QF_MESH_LAUNCH(rank_kernel, F, F, ws);
    const Mesh M = {vertices, faces, n_vertices, F};
    const Out out = {out_vertices, out_uv, face_class, face_origin, face_half};
    QF_MESH_LAUNCH(emit_kernel, F, M, texels_per_unit, (int)max_leg, texture_size, ws, out);
    return QF_OK;
}
