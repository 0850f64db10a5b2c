// Points drawn by area from a mesh's surface on the device (include/qf_mesh_sample.h; the rule is DESIGN.md section
// 3.9h, restated in numpy in tests/mesh_sample_reference.py).  Every floating-point operation is fp64 and rounded on its
// own (the file is built with -ffp-contract=off); no floating-point atomic is used.
//
// Passes of qf_mesh_sample_prepare (one stream, no host wait):
//   vertices  per vertex: the non-finite tally;
//   measure   per face: the index, weight and measure tallies of rule 1, m_f of rule 2, and the maximum of rule 3: the
//             bit pattern of a non-negative double orders as the double does, so a wave reduction and one integer
//             atomicMax per wave give the exact maximum whatever the arrival order;
//   quantise  per face: q_f of rule 3 (0 for every face when the mesh is refused or M == 0) and the q == 0 tally;
//   scan      rocPRIM's inclusive scan over the uint64 q: an integer sum, the same whatever the scan's shape;
//   finalize  counts[6], and the flag and the total S that emit reads.
// qf_mesh_sample_emit is one launch, a lane per sample: three hashes, a binary search of S for rule 6 (t is
// non-decreasing in i, so neighbouring lanes walk the same top of the search and end in neighbouring places), three
// vertex gathers, rules 7 and 8.  The [N,3] rows go through LDS so that every store instruction of a wave writes 512
// contiguous bytes.  Every tally is an integer sum (a wave reduction and one atomic per wave).
#include "mesh_device.h"
#include "qf_mesh_sample.h"

#include <rocprim/device/device_scan.hpp>

#include <cmath>

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;

struct Info {
    unsigned long long n_nonfinite_vertices, n_invalid_faces, n_bad_weights, n_nonfinite_measures, n_zero;
    unsigned long long max_bits;        // the bit pattern of M
    unsigned long long total;           // S, written by finalize
    int32_t ready;                      // 1: emit may sample (the mesh is valid and M > 0), written by finalize
};

struct Workspace {
    Info *info;
    double *measure;        // [F] m_f
    uint64_t *q;            // [F] q_f
    uint64_t *cum;          // [F] S_f
    void *temp;             // rocPRIM's scratch
    size_t temp_bytes;
    int64_t bytes;
};

// Scratch set aside for rocPRIM's scan.  Its own size query needs a device, and the workspace size is a host computation
// that must not: the scan keeps a few words per workgroup of at least 256 items, so a byte per face and 64 KiB over is
// more than ten times what it asks for; prepare checks the real figure against this before its first launch.
size_t temp_bytes_for(int64_t F) { return (size_t)F + 65536; }

Workspace carve(void *base, int64_t F, size_t temp)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.measure = c.take<double>(F);
    w.q = c.take<uint64_t>(F);
    w.cum = c.take<uint64_t>(F);
    w.temp = c.take<char>((int64_t)temp);
    w.temp_bytes = temp;
    w.bytes = c.off;
    return w;
}

struct Job {
    const double *v;
    const int64_t *f;
    const double *weight;   // NULL: every weight is 1
    int64_t V, F;
};

__device__ __forceinline__ bool finite_bits(uint64_t w) { return (w & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

__device__ __forceinline__ bool refused(const Info &I)
{
    return I.n_nonfinite_vertices != 0 || I.n_invalid_faces != 0 || I.n_bad_weights != 0 || I.n_nonfinite_measures != 0;
}

__global__ __launch_bounds__(kBlock) void vertices_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    int bad = 0;
    if (v < J.V) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(J.v) + 3 * v;
        bad = !(finite_bits(w[0]) && finite_bits(w[1]) && finite_bits(w[2]));
    }
    tally(&ws.info->n_nonfinite_vertices, bad);
}

__global__ __launch_bounds__(kBlock) void measure_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int invalid = 0, bad_weight = 0, nonfinite = 0;
    unsigned long long bits = 0;
    if (f < J.F) {
        const int64_t ia = J.f[3 * f], ib = J.f[3 * f + 1], ic = J.f[3 * f + 2];
        invalid = ia < 0 || ia >= J.V || ib < 0 || ib >= J.V || ic < 0 || ic >= J.V;
        double wf = 1.0;
        if (J.weight) {
            wf = J.weight[f];
            bad_weight = !(wf >= 0.0) || !finite_bits((uint64_t)__double_as_longlong(wf));
        }
        double m = 0.0;
        if (!invalid && ia != ib && ib != ic && ic != ia) {
            const double *a = J.v + 3 * ia, *b = J.v + 3 * ib, *c = J.v + 3 * ic;
            const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
            const double w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
            const double n0 = u1 * w2 - u2 * w1;
            const double n1 = u2 * w0 - u0 * w2;
            const double n2 = u0 * w1 - u1 * w0;
            const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
            m = J.weight ? len * wf : len;
        }
        nonfinite = !invalid && !finite_bits((uint64_t)__double_as_longlong(m));
        ws.measure[f] = m;
        // only a finite, positive measure enters the maximum: anything else either refuses the mesh or is a zero
        if (!nonfinite && m > 0.0) bits = (unsigned long long)__double_as_longlong(m);
    }
    tally(&ws.info->n_invalid_faces, invalid);
    tally(&ws.info->n_bad_weights, bad_weight);
    tally(&ws.info->n_nonfinite_measures, nonfinite);
    tally_max(&ws.info->max_bits, bits);
}

__global__ __launch_bounds__(kBlock) void quantise_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    const Info &I = *ws.info;
    const bool live = !refused(I) && I.max_bits != 0;
    int zero = 0;
    if (f < J.F) {
        uint64_t q = 0;
        if (live) {
            const double M = __longlong_as_double((long long)I.max_bits);
            q = (uint64_t)floor(ws.measure[f] / M * 4294967296.0);
            zero = q == 0;
        }
        ws.q[f] = q;
    }
    tally(&ws.info->n_zero, zero);
}

__global__ void finalize_kernel(Job J, Workspace ws, int64_t *counts)
{
    Info &I = *ws.info;
    const bool ok = !refused(I);
    const bool live = ok && I.max_bits != 0;
    counts[0] = (int64_t)I.n_nonfinite_vertices;
    counts[1] = (int64_t)I.n_invalid_faces;
    counts[2] = (int64_t)I.n_bad_weights;
    counts[3] = (int64_t)I.n_nonfinite_measures;
    counts[4] = live ? (int64_t)I.n_zero : 0;
    counts[5] = ok && !live ? 1 : 0;
    I.total = live ? ws.cum[J.F - 1] : 0;
    I.ready = live ? 1 : 0;
}

// splitmix64's finaliser
__device__ __forceinline__ uint64_t fin(uint64_t s)
{
    s ^= s >> 30;
    s *= 0xBF58476D1CE4E5B9ull;
    s ^= s >> 27;
    s *= 0x94D049BB133111EBull;
    s ^= s >> 31;
    return s;
}

__global__ __launch_bounds__(kBlock) void emit_kernel(Job J, Workspace ws, int64_t N, uint64_t seed,
                                                      double *__restrict__ points, int64_t *__restrict__ face,
                                                      double *__restrict__ bary)
{
    __shared__ double s_point[3 * kBlock], s_bary[3 * kBlock];
    if (!ws.info->ready) return;        // the same for every thread of the grid
    const uint64_t S = ws.info->total;
    const int64_t i = gtid();
    if (i < N) {
        const uint64_t golden = 0x9E3779B97F4A7C15ull;
        const uint64_t h0 = fin(seed + (3 * (uint64_t)i + 1) * golden);
        const uint64_t h1 = fin(seed + (3 * (uint64_t)i + 2) * golden);
        const uint64_t h2 = fin(seed + (3 * (uint64_t)i + 3) * golden);
        const double xi = (double)(h0 >> 11) * 0x1p-53;
        const double u = ((double)i + xi) / (double)N;
        uint64_t t = (uint64_t)floor(u * (double)S);
        t = t < S - 1 ? t : S - 1;
        // the smallest f with S_f > t; S_{F-1} = S > t, so there is one
        int64_t lo = 0, hi = J.F - 1;
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (ws.cum[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        double r1 = (double)(h1 >> 11) * 0x1p-53, r2 = (double)(h2 >> 11) * 0x1p-53;
        if (r1 + r2 > 1.0) {
            r1 = 1.0 - r1;
            r2 = 1.0 - r2;
        }
        const double d = (1.0 - r1) - r2;
        const double b0 = d > 0.0 ? d : 0.0;
        const double *a = J.v + 3 * J.f[3 * lo], *b = J.v + 3 * J.f[3 * lo + 1], *c = J.v + 3 * J.f[3 * lo + 2];
        face[i] = lo;
        double *sp = s_point + 3 * threadIdx.x, *sb = s_bary + 3 * threadIdx.x;
#pragma unroll
        for (int k = 0; k < 3; ++k) sp[k] = (a[k] * b0 + b[k] * r1) + c[k] * r2;
        sb[0] = b0;
        sb[1] = r1;
        sb[2] = r2;
    }
    __syncthreads();
    const int64_t base = 3 * (int64_t)blockIdx.x * kBlock, end = 3 * N;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int j = k * kBlock + threadIdx.x;
        if (base + j < end) {
            points[base + j] = s_point[j];
            bary[base + j] = s_bary[j];
        }
    }
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && V < kMaxCount && F >= 1 && 3 * F < kMaxCount; }

}  // namespace

extern "C" int64_t qf_mesh_sample_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!sizes_ok(n_vertices, n_faces)) return -1;
    return carve(nullptr, n_faces, temp_bytes_for(n_faces)).bytes;
}

extern "C" int qf_mesh_sample_prepare(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                      const double *face_weight, void *workspace, int64_t workspace_bytes,
                                      int64_t *counts, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces) || !vertices || !faces || !workspace || !counts) return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = n_vertices, F = n_faces;
    Workspace ws = carve(workspace, F, temp_bytes_for(F));
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    size_t tb = 0;
    QF_HIP_TRY(rocprim::inclusive_scan(nullptr, tb, ws.q, ws.cum, (size_t)F, rocprim::plus<uint64_t>(), s));
    if (tb > ws.temp_bytes) return QF_ERR_UNSUPPORTED;
    const Job J{vertices, faces, face_weight, V, F};

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_MESH_LAUNCH(vertices_kernel, V, J, ws);
    QF_MESH_LAUNCH(measure_kernel, F, J, ws);
    QF_MESH_LAUNCH(quantise_kernel, F, J, ws);
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::inclusive_scan(ws.temp, tb, ws.q, ws.cum, (size_t)F, rocprim::plus<uint64_t>(), s));
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, J, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_sample_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                   void *workspace, int64_t workspace_bytes, int64_t n_samples, uint64_t seed,
                                   double *points, int64_t *face, double *bary, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces) || !vertices || !faces || !workspace) return QF_ERR_INVALID_ARGUMENT;
    const int64_t N = n_samples;
    if (N < 0 || N >= kMaxCount || (N > 0 && (!points || !face || !bary))) return QF_ERR_INVALID_ARGUMENT;
    Workspace ws = carve(workspace, n_faces, temp_bytes_for(n_faces));
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    if (N == 0) return QF_OK;
    const Job J{vertices, faces, nullptr, n_vertices, n_faces};
    hipLaunchKernelGGL(emit_kernel, dim3(blocks(N)), dim3(kBlock), 0, qf_stream(stream), J, ws, N, seed, points, face, bary);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
