// Texel-position map of a UV-mapped mesh (the fill step of the reference's UV stage,
// examples/parameterization_utils.py:97-153): V[r, c] = the 3-D point of the mesh that texel (r, c) of an H x W atlas
// stands for.  The rules:
//   1. s = clip(uv * (H, W), 0, (H-1, W-1)) in fp64, integer corners q = trunc(s); uv[:,0] is the row.
//   2. face f covers the texels of q[f]'s bounding box that pass the even-odd test of texel_inside();
//   3. owner(p) = the largest f covering p (faces drawn in index order, a later one overwrites); tri_size[f] counts
//      f's cover whoever owns it;
//   4. every edge a->b is sampled at numpy's linspace(0, 1, 100) on the unrounded s; line_owner(p) = the largest f one
//      of whose samples lands on p;
//   5. an owned texel gets the fp64 barycentric blend of its owner's vertices, an unowned one the centroid of
//      line_owner(p), or of face F-1 (untouched = last face) / 0 (untouched = zero) when no edge reached it.
// Every rule is a maximum over face indices or a per-texel function, so the map does not depend on launch order:
// it is bit-identical run to run.
//
// Passes (all on one stream, no host wait):
//   face_setup   per face: q, its bounding box area (int64), 1/denominator of the barycentric solve, fp32 centroid;
//   scan         inclusive scan of the areas -> the candidate-texel index space of the cover pass;
//   cover (a)    one lane per candidate texel: atomicMax on owner; tri_size by one atomic per face run of a wave;
//   edges (b)    one lane per (face, edge): atomicMax on line_owner when the sampled texel changes and is unowned;
//   resolve (c)  one lane per 4 texels: fp64 blend, fp32 out, staged through LDS into 16-byte stores.
// The file is compiled with -ffp-contract=off: rules 4 and 5 are products and sums rounded one by one.
#pragma clang fp contract(off)

#include "qf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kScanItems = 4;                        // elements per thread of the block scan
constexpr int kScanTile = kBlock * kScanItems;
constexpr int kResolveTexels = 4;                    // texels per lane of the resolve pass (12 floats = 3 x 16 B)

struct Workspace {
    int32_t *owner, *line_owner;
    int4 *qrec;          // [F][2]: (q0r, q0c, q1r, q1c), (q2r, q2c, bbox row min, bbox col min)
    int64_t *cum;        // [F] inclusive scan of the bounding-box areas
    int64_t *block_sum;  // [ceil(F / kScanTile)]
    double *inv_den;     // [F] 1 / (d00 d11 - d01^2), 0 for a degenerate face
    float4 *centroid;    // [F] fp32 centroid (w unused)
    int64_t bytes;
};

Workspace carve(void *base, int64_t hw, int64_t F)
{
    Workspace w;
    const int64_t nb = qf_div_up(F, kScanTile);
    QfCarver c{base};
    w.owner = c.take<int32_t>(hw);
    w.line_owner = c.take<int32_t>(hw);
    w.qrec = c.take<int4>(2 * F);
    w.cum = c.take<int64_t>(F);
    w.block_sum = c.take<int64_t>(nb);
    w.inv_den = c.take<double>(F);
    w.centroid = c.take<float4>(F);
    w.bytes = c.off;
    return w;
}

// Rule 2, the even-odd test of point (x, y) = (column, row) against the triangle with integer corners (xs, ys), edges
// j -> i in corner order.  Corners and edge points are inside: a corner, a point strictly inside a horizontal edge at
// height y, or a point ON a straddling edge returns inside; otherwise a straddling edge (half-open in y) whose crossing
// l = (x_j - x_i)(y - y_i)/(y_j - y_i) + x_i lies right of x toggles the parity.  The corners are integers below
// 2^14, so the comparisons with l are exact in int64 cross-multiplication (and equal fp64's).
__device__ __forceinline__ bool texel_inside(int x, int y, const int xs[3], const int ys[3])
{
    bool in = false;
    for (int i = 0, j = 2; i < 3; j = i++) {
        const int xi = xs[i], yi = ys[i], xj = xs[j], yj = ys[j];
        if (x == xi && y == yi) return true;
        if (yi == yj && yi == y && ((xi < x && x < xj) || (xj < x && x < xi))) return true;
        if ((yi > y) != (yj > y)) {
            const int64_t den = yj - yi;                                   // nonzero: the edge straddles y
            const int64_t num = (int64_t)(xj - xi) * (y - yi) - (int64_t)(x - xi) * den;   // (l - x) * den
            if (num == 0) return true;
            if ((num > 0) == (den > 0)) in = !in;                          // x < l
        }
    }
    return in;
}

__device__ __forceinline__ double scaled(double u, int n)
{
    const double s = u * (double)n;
    return fmin(fmax(s, 0.0), (double)(n - 1));                            // numpy clip; NaN is refused by the wrapper
}

// Per face: integer corners, bounding box area, barycentric denominator, fp32 centroid.
__global__ void face_setup_kernel(const double *__restrict__ verts, const int64_t *__restrict__ faces,
                                  const double *__restrict__ uv, int64_t F, int H, int W, Workspace ws)
{
    for (int64_t f = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; f < F; f += (int64_t)gridDim.x * blockDim.x) {
        int qr[3], qc[3];
        double v[3][3];
        for (int k = 0; k < 3; ++k) {
            const int64_t vi = faces[3 * f + k];
            qr[k] = (int)scaled(uv[2 * vi + 0], H);
            qc[k] = (int)scaled(uv[2 * vi + 1], W);
            for (int d = 0; d < 3; ++d) v[k][d] = verts[3 * vi + d];
        }
        const int r0 = min(qr[0], min(qr[1], qr[2])), r1 = max(qr[0], max(qr[1], qr[2]));
        const int c0 = min(qc[0], min(qc[1], qc[2])), c1 = max(qc[0], max(qc[1], qc[2]));
        ws.qrec[2 * f + 0] = make_int4(qr[0], qc[0], qr[1], qc[1]);
        ws.qrec[2 * f + 1] = make_int4(qr[2], qc[2], r0, c0);
        ws.cum[f] = (int64_t)(r1 - r0 + 1) * (c1 - c0 + 1);
        // rule 5's denominator: e0 = q1 - q0, e1 = q2 - q0; the dot products are exact (integers below 2^29)
        const double e0r = qr[1] - qr[0], e0c = qc[1] - qc[0], e1r = qr[2] - qr[0], e1c = qc[2] - qc[0];
        const double d00 = e0r * e0r + e0c * e0c, d01 = e0r * e1r + e0c * e1c, d11 = e1r * e1r + e1c * e1c;
        const double den = d00 * d11 - d01 * d01;
        ws.inv_den[f] = den == 0.0 ? 0.0 : 1.0 / den;
        ws.centroid[f] = make_float4((float)((v[0][0] + v[1][0] + v[2][0]) / 3.0),
                                     (float)((v[0][1] + v[1][1] + v[2][1]) / 3.0),
                                     (float)((v[0][2] + v[1][2] + v[2][2]) / 3.0), 0.0f);
    }
}

// Inclusive scan of x[0, n) in place, tile by tile (kScanTile elements per block); tile totals into block_sum.
__global__ __launch_bounds__(kBlock) void scan_tiles_kernel(int64_t *x, int64_t n, int64_t *block_sum)
{
    __shared__ int64_t part[kBlock];
    const int64_t base = (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
    int64_t v[kScanItems], run = 0;
    for (int k = 0; k < kScanItems; ++k) {
        v[k] = base + k < n ? x[base + k] : 0;
        run += v[k];
        v[k] = run;
    }
    part[threadIdx.x] = run;
    __syncthreads();
    for (int off = 1; off < kBlock; off <<= 1) {                           // Hillis-Steele over the thread totals
        const int64_t add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
        __syncthreads();
        part[threadIdx.x] += add;
        __syncthreads();
    }
    const int64_t before = threadIdx.x ? part[threadIdx.x - 1] : 0;
    for (int k = 0; k < kScanItems; ++k)
        if (base + k < n) x[base + k] = v[k] + before;
    if (threadIdx.x == kBlock - 1) block_sum[blockIdx.x] = part[kBlock - 1];
}

// Exclusive scan of the tile totals by one block, kBlock at a time (there are F / 1024 of them).
__global__ __launch_bounds__(kBlock) void scan_block_sums_kernel(int64_t *block_sum, int64_t nb)
{
    __shared__ int64_t part[kBlock];
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < nb; b0 += kBlock) {
        const int64_t i = b0 + threadIdx.x;
        const int64_t own = i < nb ? block_sum[i] : 0;
        part[threadIdx.x] = own;
        __syncthreads();
        for (int off = 1; off < kBlock; off <<= 1) {
            const int64_t add = threadIdx.x >= (unsigned)off ? part[threadIdx.x - off] : 0;
            __syncthreads();
            part[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < nb) block_sum[i] = carry + part[threadIdx.x] - own;
        const int64_t total = part[kBlock - 1];
        __syncthreads();
        carry += total;
    }
}

__global__ void scan_add_kernel(int64_t *x, int64_t n, const int64_t *block_sum)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        x[i] += block_sum[i / kScanTile];
}

// First face in [lo, hi] whose inclusive area sum exceeds t (the face of candidate t); hi must qualify.
__device__ __forceinline__ int64_t face_of(const int64_t *__restrict__ cum, int64_t t, int64_t lo, int64_t hi)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (cum[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}

// (a) Cover.  The candidate texels of all faces form one index space [0, cum[F-1]); each wave walks one contiguous
// segment of it 64 candidates at a time, so a face of 10^4 texels is spread over many waves and a wave of small faces
// handles many faces.  The faces of a 64-candidate chunk lie within 64 of the chunk's first face (every area is >= 1),
// so after one full search per segment each lane searches a window of 65 faces.
__global__ __launch_bounds__(kBlock) void cover_kernel(const int4 *__restrict__ qrec, const int64_t *__restrict__ cum,
                                                       int64_t F, int W, int32_t *__restrict__ owner,
                                                       int64_t *__restrict__ tri_size)
{
    const int lane = threadIdx.x & 63;
    const int64_t total = cum[F - 1];
    const int64_t n_waves = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t wave = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const int64_t seg = ((total + n_waves - 1) / n_waves + 63) / 64 * 64;
    const int64_t t_begin = wave * seg, t_end = min(total, t_begin + seg);
    if (t_begin >= t_end) return;
    int64_t f0 = face_of(cum, t_begin, 0, F - 1);
    for (int64_t chunk = t_begin; chunk < t_end; chunk += 64) {
        const int64_t t = chunk + lane;
        const bool valid = t < t_end;
        int64_t f = F;                                                     // sentinel of an idle lane
        bool inside = false;
        if (valid) {
            f = face_of(cum, t, f0, min(f0 + 64, F - 1));
            const int4 a = qrec[2 * f], b = qrec[2 * f + 1];
            const int xs[3] = {a.y, a.w, b.y}, ys[3] = {a.x, a.z, b.x};
            const int r1 = max(a.x, max(a.z, b.x)), c1 = max(a.y, max(a.w, b.y));
            const int64_t k = t - (f ? cum[f - 1] : 0);
            const int bw = c1 - b.w + 1;
            // 0 <= k < area holds by construction; checked anyway, so that no texel outside f's box is ever written
            if (k >= 0 && k < (int64_t)(r1 - b.z + 1) * bw) {
                const int r = b.z + (int)k / bw, c = b.w + (int)k % bw;
                inside = texel_inside(c, r, xs, ys);
                if (inside) atomicMax(owner + (int64_t)r * W + c, (int)f);
            }
        }
        // tri_size: the lanes of one face are one contiguous run (f ascends with the lane); the run's first lane adds
        // the run's count of inside lanes.
        const int64_t f_prev = __shfl_up(f, 1);
        const bool start = valid && (lane == 0 || f_prev != f);
        const uint64_t starts = __ballot(start), ins = __ballot(inside);
        if (start) {
            const uint64_t later = lane == 63 ? 0 : starts & (~uint64_t(0) << (lane + 1));
            const uint64_t run = (later ? (uint64_t(1) << __builtin_ctzll(later)) - 1 : ~uint64_t(0)) &
                                 (~uint64_t(0) << lane);
            const int n = __popcll(ins & run);
            if (n) atomicAdd(reinterpret_cast<unsigned long long *>(tri_size + f), (unsigned long long)n);
        }
        f0 = __shfl(f, 63);                                                // face of chunk + 63 (the loop ends if idle)
    }
}

// (b) Edges.  One lane per (face, edge a -> b): 100 samples of numpy's linspace(0, 1, 100) on the unrounded scaled
// corners; consecutive samples repeat texels, so a texel is looked at only when it changes, and only texels left
// unowned by (a) take part (only those read line_owner in (c)).
__global__ void edges_kernel(const int64_t *__restrict__ faces, const double *__restrict__ uv, int64_t F, int H, int W,
                             const int32_t *__restrict__ owner, int32_t *__restrict__ line_owner)
{
    const double step = 1.0 / 99.0;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < 3 * F; g += (int64_t)gridDim.x * blockDim.x) {
        const int64_t f = g / 3;
        const int e = (int)(g - 3 * f);
        const int64_t ia = faces[3 * f + e], ib = faces[3 * f + (e == 2 ? 0 : e + 1)];
        const double ar = scaled(uv[2 * ia], H), ac = scaled(uv[2 * ia + 1], W);
        const double br = scaled(uv[2 * ib], H), bc = scaled(uv[2 * ib + 1], W);
        int64_t last = -1;
        for (int k = 0; k < 100; ++k) {
            const double w = k == 99 ? 1.0 : (double)k * step, u = 1.0 - w;
            const int r = min((int)(br * w + ar * u), H - 1), c = min((int)(bc * w + ac * u), W - 1);
            const int64_t p = (int64_t)r * W + c;
            if (p == last) continue;
            last = p;
            if (owner[p] < 0) atomicMax(line_owner + p, (int)f);
        }
    }
}

// (c) Resolve.  One lane per kResolveTexels consecutive texels; a wave's 768 output floats are staged in LDS and leave
// as three 1 KiB rows of 16-byte stores.  No division here (face_setup_kernel did them), so the fp64 blend is plain
// multiplies and adds: the ISA of this kernel has no v_fma_f64.
__global__ __launch_bounds__(kBlock) void resolve_kernel(const double *__restrict__ verts,
                                                         const int64_t *__restrict__ faces,
                                                         const int4 *__restrict__ qrec, const double *__restrict__ inv_den,
                                                         const float4 *__restrict__ centroid,
                                                         const int32_t *__restrict__ owner,
                                                         const int32_t *__restrict__ line_owner, int64_t F, int H,
                                                         int W, int32_t untouched_zero, float *__restrict__ out)
{
    constexpr int kWaveFloats = 64 * kResolveTexels * 3;
    __shared__ float stage[kBlock / 64][kWaveFloats];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int64_t hw = (int64_t)H * W, n_floats = 3 * hw;
    const bool aligned = (reinterpret_cast<uintptr_t>(out) & 15) == 0;
    const int64_t wave_stride = (int64_t)gridDim.x * kBlock * kResolveTexels;
    for (int64_t wbase = ((int64_t)blockIdx.x * kBlock + wv * 64) * kResolveTexels; wbase < hw; wbase += wave_stride) {
        for (int j = 0; j < kResolveTexels; ++j) {
            const int64_t p = wbase + lane * kResolveTexels + j;
            float x = 0.0f, y = 0.0f, z = 0.0f;
            if (p < hw) {
                const int o = owner[p];
                if (o >= 0 && inv_den[o] != 0.0) {
                    const int r = (int)p / W, c = (int)p - r * W;         // p < H W < 2^31
                    const int4 a = qrec[2 * o], b = qrec[2 * o + 1];
                    const double e0r = a.z - a.x, e0c = a.w - a.y, e1r = b.x - a.x, e1c = b.y - a.y;
                    const double wr = r - a.x, wc = c - a.y;
                    const double d00 = e0r * e0r + e0c * e0c, d01 = e0r * e1r + e0c * e1c;
                    const double d02 = e0r * wr + e0c * wc, d11 = e1r * e1r + e1c * e1c, d12 = e1r * wr + e1c * wc;
                    const double inv = inv_den[o];
                    const double b2 = (d00 * d12 - d01 * d02) * inv;
                    const double b1 = (d11 * d02 - d01 * d12) * inv;
                    const double b0 = (1.0 - b1) - b2;
                    const double *v0 = verts + 3 * faces[3 * (int64_t)o], *v1 = verts + 3 * faces[3 * (int64_t)o + 1],
                                 *v2 = verts + 3 * faces[3 * (int64_t)o + 2];
                    x = (float)((b0 * v0[0] + b1 * v1[0]) + b2 * v2[0]);
                    y = (float)((b0 * v0[1] + b1 * v1[1]) + b2 * v2[1]);
                    z = (float)((b0 * v0[2] + b1 * v1[2]) + b2 * v2[2]);
                } else {
                    int g = o;                                             // a degenerate owner: its centroid
                    if (g < 0) g = line_owner[p];
                    if (g < 0 && !untouched_zero) g = (int)(F - 1);
                    if (g >= 0) {
                        const float4 m = centroid[g];
                        x = m.x;
                        y = m.y;
                        z = m.z;
                    }
                }
            }
            float *s = &stage[wv][(lane * kResolveTexels + j) * 3];
            s[0] = x;
            s[1] = y;
            s[2] = z;
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        const int64_t f0 = 3 * wbase;
        if (aligned && f0 + kWaveFloats <= n_floats) {
            float4 *dst = reinterpret_cast<float4 *>(out + f0);
            const float4 *src = reinterpret_cast<const float4 *>(stage[wv]);
            for (int k = 0; k < kWaveFloats / 256; ++k) dst[k * 64 + lane] = src[k * 64 + lane];
        } else {
            for (int k = lane; k < kWaveFloats; k += 64)
                if (f0 + k < n_floats) out[f0 + k] = stage[wv][k];
        }
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
}

}  // namespace

extern "C" int64_t qf_texel_positions_workspace_bytes(int64_t n_faces, int32_t height, int32_t width)
{
    if (n_faces < 1 || height < 1 || width < 1 || height > 16384 || width > 16384 ||
        (int64_t)height * width >= (int64_t(1) << 31))
        return -1;
    return carve(nullptr, (int64_t)height * width, n_faces).bytes;
}

extern "C" int qf_texel_positions(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                  const double *uv, int32_t height, int32_t width, int32_t untouched, float *out,
                                  int64_t *tri_size, void *workspace, int64_t workspace_bytes, void *stream)
{
    const int64_t need = qf_texel_positions_workspace_bytes(n_faces, height, width);
    if (need < 0 || n_vertices < 1 || (untouched != QF_UNTOUCHED_LAST_FACE && untouched != QF_UNTOUCHED_ZERO))
        return QF_ERR_INVALID_ARGUMENT;
    if (!vertices || !faces || !uv || !out || !tri_size || !workspace || workspace_bytes < need)
        return QF_ERR_INVALID_ARGUMENT;
    const int64_t hw = (int64_t)height * width, F = n_faces;
    const Workspace ws = carve(workspace, hw, F);
    hipStream_t s = qf_stream(stream);
    QF_HIP_TRY(hipMemsetAsync(ws.owner, 0xff, 4 * hw, s));                 // -1: no face yet
    QF_HIP_TRY(hipMemsetAsync(ws.line_owner, 0xff, 4 * hw, s));
    QF_HIP_TRY(hipMemsetAsync(tri_size, 0, 8 * F, s));
    hipLaunchKernelGGL(face_setup_kernel, dim3(qf_grid_1d(F, kBlock)), dim3(kBlock), 0, s, vertices, faces, uv, F,
                       (int)height, (int)width, ws);
    QF_LAUNCH_CHECK();
    const int64_t nb = qf_div_up(F, kScanTile);
    hipLaunchKernelGGL(scan_tiles_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, ws.cum, F, ws.block_sum);
    QF_LAUNCH_CHECK();
    if (nb > 1) {
        hipLaunchKernelGGL(scan_block_sums_kernel, dim3(1), dim3(kBlock), 0, s, ws.block_sum, nb);
        QF_LAUNCH_CHECK();
        hipLaunchKernelGGL(scan_add_kernel, dim3(qf_grid_1d(F, kBlock)), dim3(kBlock), 0, s, ws.cum, F,
                           ws.block_sum);
        QF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(cover_kernel, dim3(qf_cu_count_cached() * 8), dim3(kBlock), 0, s, ws.qrec, ws.cum, F,
                       (int)width, ws.owner, tri_size);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(edges_kernel, dim3(qf_grid_1d(3 * F, kBlock)), dim3(kBlock), 0, s, faces, uv, F, (int)height,
                       (int)width, ws.owner, ws.line_owner);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(resolve_kernel, dim3(qf_grid_1d(qf_div_up(hw, kResolveTexels), kBlock)), dim3(kBlock), 0, s,
                       vertices, faces, ws.qrec, ws.inv_den, ws.centroid, ws.owner, ws.line_owner, F, (int)height,
                       (int)width, untouched, out);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
