// Mesh decimation: rounds of independent quadric edge collapses (the rules are stated in
// include/qf_mesh_decimate.h and restated in numpy in tests/mesh_decimate_reference.py).  Per round the caller numbers the
// edges (mesh_subdivide.hip), calls select and apply here, compacts (mesh_compact.hip) and gathers here.
//
// Passes of select (one stream, no host wait):
//   face keys (v << 32 | f per corner of a face without two equal indices) -> radix sort -> the run of every vertex: the
//   CSR of faces, rows ascending;  edge keys (a << 32 | b and b << 32 | a) -> radix sort -> runs: the CSR of neighbours,
//   rows ascending;  uses (integer atomicAdd per half-edge) -> locks -> one thread per edge: point, cost, legality, key,
//   integer atomicMin into m1 of both ends -> m2 per vertex over its row -> selected edges keyed by their cost bits, the
//   others by all ones -> stable radix sort of (key, e) -> the first max_take that are not all ones are taken.
// Every valence loop walks a CSR row; no kernel keeps a per-thread list.  Every floating-point value is computed by one
// thread in a stated order, so results do not depend on the launch shape; the atomics are integer min, add and flags.
// The file is compiled with -ffp-contract=off: every product and sum is rounded on its own.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "mesh_device.h"
#include "qf_mesh_decimate.h"
#include "qf_mesh_decimate_open.h"

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr uint64_t kNone = ~uint64_t(0);        // above every key: keys fit 63 bits
constexpr double kTau = 1e-6;

struct Info {
    unsigned long long candidates, legal, selected, locked, invalid, nonfinite;
};

struct Workspace {
    Info *info;
    int64_t *fstart, *fend;     // [V] run of each vertex in fkey_b
    int64_t *nstart, *nend;     // [V] run of each vertex in nkey_b
    uint64_t *m1, *m2;          // [V]
    int32_t *remap;             // [V] the kept end of a removed vertex, else -1
    uint8_t *locked;            // [V]
    uint64_t *fkey_a, *fkey_b;  // [3F] vertex << 32 | face, then sorted
    double *plane;              // [4F] (quadrics only)
    uint64_t *nkey_a, *nkey_b;  // [2E] vertex << 32 | neighbour, then sorted
    int32_t *uses;              // [E]
    uint64_t *key;              // [E] the key of a legal candidate, else kNone
    uint64_t *skey_a, *skey_b;  // [E] cost bits of a legal candidate, then of a selected edge; sorted
    int32_t *sval_a, *sval_b;   // [E] edge ids; sorted
    void *temp;
    size_t temp_bytes;
    int64_t bytes;
};

bool sizes_ok(int64_t V, int64_t F, int64_t E)
{
    return V >= 1 && V < kMaxCount && F >= 0 && 3 * F < kMaxCount && E >= 0 && E < kMaxCount;
}

// rocPRIM scratch for the largest of the three sorts (host query, no launch).
size_t temp_bytes_for(int64_t F, int64_t E, hipStream_t s)
{
    size_t need = 1, b = 0;
    if (rocprim::radix_sort_keys(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)(3 * F > 0 ? 3 * F : 1), 0, 64,
                                 s) != hipSuccess)
        return 0;
    need = b > need ? b : need;
    if (rocprim::radix_sort_keys(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (size_t)(2 * E > 0 ? 2 * E : 1), 0, 64,
                                 s) != hipSuccess)
        return 0;
    need = b > need ? b : need;
    if (rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, (size_t)(E > 0 ? E : 1), 0, 64, s) != hipSuccess)
        return 0;
    need = b > need ? b : need;
    return need;
}

Workspace carve(void *base, int64_t V, int64_t F, int64_t E, size_t temp)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.fstart = c.take<int64_t>(V);
    w.fend = c.take<int64_t>(V);
    w.nstart = c.take<int64_t>(V);
    w.nend = c.take<int64_t>(V);
    w.m1 = c.take<uint64_t>(V);
    w.m2 = c.take<uint64_t>(V);
    w.remap = c.take<int32_t>(V);
    w.locked = c.take<uint8_t>(V);
    w.fkey_a = c.take<uint64_t>(3 * F);
    w.fkey_b = c.take<uint64_t>(3 * F);
    w.plane = c.take<double>(4 * F);
    w.nkey_a = c.take<uint64_t>(2 * E);
    w.nkey_b = c.take<uint64_t>(2 * E);
    w.uses = c.take<int32_t>(E);
    w.key = c.take<uint64_t>(E);
    w.skey_a = c.take<uint64_t>(E);
    w.skey_b = c.take<uint64_t>(E);
    w.sval_a = c.take<int32_t>(E);
    w.sval_b = c.take<int32_t>(E);
    w.temp = c.take<char>((int64_t)temp);
    w.temp_bytes = temp;
    w.bytes = c.off;
    return w;
}

struct Mesh {
    const double *p;
    const int64_t *f;
    const int64_t *edges;
    const int64_t *face_edges;
    const double *Q;
    int64_t V, F, E;
};

__device__ __forceinline__ bool face_ok(const int64_t *t, int64_t V)
{
    return t[0] >= 0 && t[0] < V && t[1] >= 0 && t[1] < V && t[2] >= 0 && t[2] < V;
}

// Corner 3f + k -> vertex << 32 | face for a face with three distinct indices in range, else kNone.
__global__ __launch_bounds__(kBlock) void face_key_kernel(Mesh M, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= 3 * M.F) return;
    const int64_t f = i / 3, k = i - 3 * f;
    const int64_t *t = M.f + 3 * f;
    uint64_t key = kNone;
    if (!face_ok(t, M.V)) {
        if (k == 0) atomicAdd(&ws.info->invalid, 1ull);
    } else if (t[0] != t[1] && t[1] != t[2] && t[0] != t[2]) {
        key = (uint64_t)t[k] << 32 | (uint64_t)f;
    }
    ws.fkey_a[i] = key;
}

// The two directed copies of edge e, or kNone for an edge that is not 0 <= a < b < V.
__global__ __launch_bounds__(kBlock) void edge_key_kernel(Mesh M, Workspace ws)
{
    const int64_t e = gtid();
    if (e >= M.E) return;
    const int64_t a = M.edges[2 * e], b = M.edges[2 * e + 1];
    const bool ok = a >= 0 && a < b && b < M.V;
    if (!ok) atomicAdd(&ws.info->invalid, 1ull);
    ws.nkey_a[2 * e] = ok ? ((uint64_t)a << 32 | (uint64_t)b) : kNone;
    ws.nkey_a[2 * e + 1] = ok ? ((uint64_t)b << 32 | (uint64_t)a) : kNone;
}

// start / end of every vertex's run in sorted keys (rows of vertices without a key stay at the memset's 0, 0).
__global__ __launch_bounds__(kBlock) void range_kernel(const uint64_t *keys, int64_t n, int64_t *start, int64_t *end)
{
    const int64_t j = gtid();
    if (j >= n) return;
    const uint64_t key = keys[j];
    if (key == kNone) return;
    const uint64_t v = key >> 32;
    if (j == 0 || (keys[j - 1] >> 32) != v) start[v] = j;
    if (j == n - 1 || keys[j + 1] == kNone || (keys[j + 1] >> 32) != v) end[v] = j + 1;
}

__device__ __forceinline__ void cross_of(const double *p0, const double *p1, const double *p2, double &n0, double &n1,
                                         double &n2)
{
    const double u0 = p1[0] - p0[0], u1 = p1[1] - p0[1], u2 = p1[2] - p0[2];
    const double w0 = p2[0] - p0[0], w1 = p2[1] - p0[1], w2 = p2[2] - p0[2];
    n0 = u1 * w2 - u2 * w1;
    n1 = u2 * w0 - u0 * w2;
    n2 = u0 * w1 - u1 * w0;
}

__global__ __launch_bounds__(kBlock) void plane_kernel(Mesh M, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= M.F) return;
    const int64_t *t = M.f + 3 * f;
    double n0 = 0.0, n1 = 0.0, n2 = 0.0, d = 0.0;
    if (face_ok(t, M.V)) {
        const double *a = M.p + 3 * t[0];
        cross_of(a, M.p + 3 * t[1], M.p + 3 * t[2], n0, n1, n2);
        const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
        if (len == 0.0) {
            n0 = n1 = n2 = 0.0;
        } else {
            n0 = n0 / len;
            n1 = n1 / len;
            n2 = n2 / len;
            d = -((n0 * a[0] + n1 * a[1]) + n2 * a[2]);
        }
    }
    double *p = ws.plane + 4 * f;
    p[0] = n0;
    p[1] = n1;
    p[2] = n2;
    p[3] = d;
}

__global__ __launch_bounds__(kBlock) void quadric_kernel(Mesh M, Workspace ws, double *out)
{
    const int64_t v = gtid();
    if (v >= M.V) return;
    const double *x = M.p + 3 * v;
    if (!(isfinite(x[0]) && isfinite(x[1]) && isfinite(x[2]))) atomicAdd(&ws.info->nonfinite, 1ull);
    double q0 = 0.0, q1 = 0.0, q2 = 0.0, q3 = 0.0, q4 = 0.0, q5 = 0.0, q6 = 0.0, q7 = 0.0, q8 = 0.0, q9 = 0.0;
    for (int64_t j = ws.fstart[v], je = ws.fend[v]; j < je; ++j) {
        const double *p = ws.plane + 4 * (int64_t)(ws.fkey_b[j] & 0xffffffffu);
        const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
        q0 = q0 + p0 * p0;
        q1 = q1 + p0 * p1;
        q2 = q2 + p0 * p2;
        q3 = q3 + p0 * p3;
        q4 = q4 + p1 * p1;
        q5 = q5 + p1 * p2;
        q6 = q6 + p1 * p3;
        q7 = q7 + p2 * p2;
        q8 = q8 + p2 * p3;
        q9 = q9 + p3 * p3;
    }
    double *o = out + 10 * v;
    o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4;
    o[5] = q5; o[6] = q6; o[7] = q7; o[8] = q8; o[9] = q9;
}

__global__ void quadric_counts_kernel(Workspace ws, int64_t *counts)
{
    counts[0] = (int64_t)ws.info->nonfinite;
    counts[1] = (int64_t)ws.info->invalid;
}

__global__ __launch_bounds__(kBlock) void uses_kernel(Mesh M, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= 3 * M.F) return;
    const int64_t e = M.face_edges[i];
    if (e >= 0 && e < M.E) atomicAdd(&ws.uses[e], 1);
    else if (e != -1) atomicAdd(&ws.info->invalid, 1ull);
}

__global__ __launch_bounds__(kBlock) void lock_init_kernel(int64_t V, const uint8_t *vertex_lock, Workspace ws)
{
    const int64_t v = gtid();
    if (v >= V) return;
    ws.locked[v] = (vertex_lock && vertex_lock[v]) ? 1 : 0;
}

// Both ends of a boundary or non-manifold edge (every writer stores the same 1).
__global__ __launch_bounds__(kBlock) void lock_edge_kernel(Mesh M, Workspace ws)
{
    const int64_t e = gtid();
    if (e >= M.E || ws.nkey_a[2 * e] == kNone || ws.uses[e] == 2) return;
    ws.locked[M.edges[2 * e]] = 1;
    ws.locked[M.edges[2 * e + 1]] = 1;
}

__global__ __launch_bounds__(kBlock) void lock_count_kernel(int64_t V, Workspace ws)
{
    const int64_t v = gtid();
    if (v < V && ws.locked[v]) atomicAdd(&ws.info->locked, 1ull);
}

// Qe = Q[a] + Q[b] per component.
__device__ __forceinline__ void edge_quadric(const double *Q, int64_t a, int64_t b, double *qe)
{
    const double *qa = Q + 10 * a, *qb = Q + 10 * b;
#pragma unroll
    for (int k = 0; k < 10; ++k) qe[k] = qa[k] + qb[k];
}

// Step 3's point for edge (a, b): the minimiser of Qe where it is well conditioned and near the edge, else the midpoint.
__device__ __forceinline__ void optimal_point(const double *p, const double *qe, int64_t a, int64_t b, double &z0, double &z1,
                                              double &z2)
{
    const double *pa = p + 3 * a, *pb = p + 3 * b;
    const double pa0 = pa[0], pa1 = pa[1], pa2 = pa[2], pb0 = pb[0], pb1 = pb[1], pb2 = pb[2];
    const double m0 = (pa0 + pb0) * 0.5, m1 = (pa1 + pb1) * 0.5, m2 = (pa2 + pb2) * 0.5;
    const double a00 = qe[0], a01 = qe[1], a02 = qe[2], a11 = qe[4], a12 = qe[5], a22 = qe[7];
    const double b0 = -qe[3], b1 = -qe[6], b2 = -qe[8];
    const double r0 = b0 - ((a00 * m0 + a01 * m1) + a02 * m2);
    const double r1 = b1 - ((a01 * m0 + a11 * m1) + a12 * m2);
    const double r2 = b2 - ((a02 * m0 + a12 * m1) + a22 * m2);
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a12 * a02 - a01 * a22;
    const double c02 = a01 * a12 - a11 * a02;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double t3 = ((a00 + a11) + a22) / 3.0;
    z0 = m0;
    z1 = m1;
    z2 = m2;
    if (det > kTau * ((t3 * t3) * t3)) {
        const double y0 = m0 + ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        const double y1 = m1 + ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        const double y2 = m2 + ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        const double L = fmax(fmax(fabs(pa0 - pb0), fabs(pa1 - pb1)), fabs(pa2 - pb2));
        const bool in = y0 >= fmin(pa0, pb0) - L && y0 <= fmax(pa0, pb0) + L && y1 >= fmin(pa1, pb1) - L &&
                        y1 <= fmax(pa1, pb1) + L && y2 >= fmin(pa2, pb2) - L && y2 <= fmax(pa2, pb2) + L;
        if (in) {
            z0 = y0;
            z1 = y1;
            z2 = y2;
        }
    }
}

// The cost of Qe at z, clamped at zero.
__device__ __forceinline__ double point_cost(const double *qe, double z0, double z1, double z2)
{
    const double s0 = ((qe[0] * z0 + qe[1] * z1) + qe[2] * z2) + qe[3];
    const double s1 = ((qe[1] * z0 + qe[4] * z1) + qe[5] * z2) + qe[6];
    const double s2 = ((qe[2] * z0 + qe[5] * z1) + qe[7] * z2) + qe[8];
    const double s3 = ((qe[3] * z0 + qe[6] * z1) + qe[8] * z2) + qe[9];
    const double c = ((s0 * z0 + s1 * z1) + s2 * z2) + s3;
    return c > 0.0 ? c : 0.0;
}

// Step 3: Qe, the point z and the cost of edge (a, b).  With pin >= 0 (collapse mode, an edge from an interior vertex to
// the border vertex `pin`) z is the position of `pin`, bit for bit.
__device__ __forceinline__ void collapse_point(const double *p, const double *Q, int64_t a, int64_t b, int64_t pin, double *qe,
                                               double &z0, double &z1, double &z2, double &cost)
{
    edge_quadric(Q, a, b, qe);
    if (pin >= 0) {
        z0 = p[3 * pin];
        z1 = p[3 * pin + 1];
        z2 = p[3 * pin + 2];
    } else {
        optimal_point(p, qe, a, b, z0, z1, z2);
    }
    cost = point_cost(qe, z0, z1, z2);
}

// (L3) for face t, in which v appears once: the normal before and after v moves to z.
__device__ __forceinline__ bool keeps_side(const double *p, const int64_t *t, int64_t v, double z0, double z1, double z2)
{
    const double *p0 = p + 3 * t[0], *p1 = p + 3 * t[1], *p2 = p + 3 * t[2];
    double n0, n1, n2, k0, k1, k2;
    cross_of(p0, p1, p2, n0, n1, n2);
    const bool m0 = t[0] == v, m1 = t[1] == v, m2 = t[2] == v;
    const double a0 = m0 ? z0 : p0[0], a1 = m0 ? z1 : p0[1], a2 = m0 ? z2 : p0[2];
    const double b0 = m1 ? z0 : p1[0], b1 = m1 ? z1 : p1[1], b2 = m1 ? z2 : p1[2];
    const double c0 = m2 ? z0 : p2[0], c1 = m2 ? z1 : p2[1], c2 = m2 ? z2 : p2[2];
    const double u0 = b0 - a0, u1 = b1 - a1, u2 = b2 - a2;
    const double w0 = c0 - a0, w1 = c1 - a1, w2 = c2 - a2;
    k0 = u1 * w2 - u2 * w1;
    k1 = u2 * w0 - u0 * w2;
    k2 = u0 * w1 - u1 * w0;
    return (n0 * k0 + n1 * k1) + n2 * k2 > 0.0;
}

// The other two vertices of face t at v, as (low, high).
__device__ __forceinline__ void other_pair(const int64_t *t, int64_t v, int64_t &lo, int64_t &hi)
{
    const int64_t x = t[0] == v ? t[1] : t[0];
    const int64_t y = t[2] == v ? t[1] : t[2];
    lo = x < y ? x : y;
    hi = x < y ? y : x;
}

__device__ __forceinline__ uint64_t mix(uint64_t x, uint64_t round)
{
    uint64_t s = x + (round + 1) * 0x9E3779B97F4A7C15ull;
    s ^= s >> 30;
    s *= 0xBF58476D1CE4E5B9ull;
    s ^= s >> 27;
    s *= 0x94D049BB133111EBull;
    s ^= s >> 31;
    return s;
}

// Step 4 for edge e = (a, b) collapsing to z.
__device__ __forceinline__ bool collapse_legal(const Mesh &M, const Workspace &ws, int64_t e, int64_t a, int64_t b, double z0,
                                               double z1, double z2)
{
    // (L1) rows are ascending and hold no vertex twice
    int common = 0;
    {
        int64_t i = ws.nstart[a], j = ws.nstart[b];
        const int64_t ie = ws.nend[a], je = ws.nend[b];
        while (i < ie && j < je) {
            const uint32_t x = (uint32_t)ws.nkey_b[i], y = (uint32_t)ws.nkey_b[j];
            common += x == y;
            i += x <= y;
            j += y <= x;
        }
    }
    if (common != ws.uses[e]) return false;
    // (L2) and (L3) over the faces of a without b, then (L3) over those of b without a
    const int64_t bs = ws.fstart[b], be = ws.fend[b];
    for (int64_t i = ws.fstart[a], ie = ws.fend[a]; i < ie; ++i) {
        const int64_t *t = M.f + 3 * (int64_t)(ws.fkey_b[i] & 0xffffffffu);
        if (t[0] == b || t[1] == b || t[2] == b) continue;
        if (!keeps_side(M.p, t, a, z0, z1, z2)) return false;
        int64_t lo, hi;
        other_pair(t, a, lo, hi);
        for (int64_t j = bs; j < be; ++j) {
            const int64_t *u = M.f + 3 * (int64_t)(ws.fkey_b[j] & 0xffffffffu);
            if (u[0] == a || u[1] == a || u[2] == a) continue;
            int64_t lo2, hi2;
            other_pair(u, b, lo2, hi2);
            if (lo == lo2 && hi == hi2) return false;
        }
    }
    for (int64_t j = bs; j < be; ++j) {
        const int64_t *u = M.f + 3 * (int64_t)(ws.fkey_b[j] & 0xffffffffu);
        if (u[0] == a || u[1] == a || u[2] == a) continue;
        if (!keeps_side(M.p, u, b, z0, z1, z2)) return false;
    }
    return true;
}

// Steps 3 to 5 and m1, one thread per edge.
__global__ __launch_bounds__(kBlock) void candidate_kernel(Mesh M, Workspace ws, double max_cost, uint64_t round)
{
    const int64_t e = gtid();
    if (e >= M.E) return;
    ws.key[e] = kNone;
    ws.skey_a[e] = kNone;
    if (ws.nkey_a[2 * e] == kNone) return;
    const int64_t a = M.edges[2 * e], b = M.edges[2 * e + 1];
    if (ws.locked[a] || ws.locked[b]) return;
    double qe[10], z0, z1, z2, cost;
    collapse_point(M.p, M.Q, a, b, -1, qe, z0, z1, z2, cost);
    if (cost > max_cost) return;
    atomicAdd(&ws.info->candidates, 1ull);

    if (!collapse_legal(M, ws, e, a, b, z0, z1, z2)) return;
    atomicAdd(&ws.info->legal, 1ull);
    const uint64_t bits = (uint64_t)__double_as_longlong(cost);
    const uint64_t key = (bits >> 52) << 52 | (mix((uint64_t)a << 32 | (uint64_t)b, round) & 0x1FFFFFull) << 31 | (uint64_t)e;
    ws.key[e] = key;
    ws.skey_a[e] = bits;
    atomicMin((unsigned long long *)&ws.m1[a], (unsigned long long)key);
    atomicMin((unsigned long long *)&ws.m1[b], (unsigned long long)key);
}

__global__ __launch_bounds__(kBlock) void min2_kernel(int64_t V, Workspace ws)
{
    const int64_t v = gtid();
    if (v >= V) return;
    uint64_t m = ws.m1[v];
    for (int64_t i = ws.nstart[v], ie = ws.nend[v]; i < ie; ++i) {
        const uint64_t x = ws.m1[(uint32_t)ws.nkey_b[i]];
        m = x < m ? x : m;
    }
    ws.m2[v] = m;
}

// Step 6: the sort key of a selected edge is its cost bits, of any other edge all ones.
__global__ __launch_bounds__(kBlock) void select_kernel(Mesh M, Workspace ws)
{
    const int64_t e = gtid();
    if (e >= M.E) return;
    const uint64_t key = ws.key[e];
    bool sel = key != kNone;
    if (sel) sel = key == ws.m2[M.edges[2 * e]] && key == ws.m2[M.edges[2 * e + 1]];
    if (sel) atomicAdd(&ws.info->selected, 1ull);
    else ws.skey_a[e] = kNone;
    ws.sval_a[e] = (int32_t)e;
}

__global__ void collapse_counts_kernel(Workspace ws, int64_t max_take, int64_t *counts)
{
    const int64_t sel = (int64_t)ws.info->selected;
    counts[0] = (int64_t)ws.info->candidates;
    counts[1] = (int64_t)ws.info->legal;
    counts[2] = sel;
    counts[3] = sel < max_take ? sel : max_take;
    counts[4] = (int64_t)ws.info->locked;
    counts[5] = (int64_t)ws.info->invalid;
}

// Step 8 for the i-th edge of the sorted selection.  The ends of two taken edges neither coincide nor neighbour, so no
// thread reads what another writes.
__global__ __launch_bounds__(kBlock) void apply_kernel(double *p, double *Q, const int64_t *edges, int64_t n, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= n || ws.skey_b[i] == kNone) return;
    const int64_t e = ws.sval_b[i];
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    double qe[10], z0, z1, z2, cost;
    collapse_point(p, Q, a, b, -1, qe, z0, z1, z2, cost);
    p[3 * a] = z0;
    p[3 * a + 1] = z1;
    p[3 * a + 2] = z2;
    double *qa = Q + 10 * a;
#pragma unroll
    for (int k = 0; k < 10; ++k) qa[k] = qe[k];
    ws.remap[b] = (int32_t)a;
}

__global__ __launch_bounds__(kBlock) void remap_kernel(int64_t *idx, int64_t n, int64_t V, const int32_t *remap)
{
    const int64_t i = gtid();
    if (i >= n) return;
    const int64_t v = idx[i];
    if (v < 0 || v >= V) return;
    const int32_t r = remap[v];
    if (r >= 0) idx[i] = r;
}

// ---- boundary = collapse (include/qf_mesh_decimate_open.h) ---------------------------------------------------------------
// The same passes with three changes: vertex classes in place of the boundary lock (integer atomicAdd of a vertex's boundary
// edges, a flag for non-manifold ones), a candidate pass that knows the three edge kinds, and a budget that is a prefix of
// the sorted selection by summed uses (a device-wide exclusive scan).  Round 0 adds the boundary planes to Q: the boundary
// edges of a vertex are a CSR row of vertex << 32 | edge keys, so they are summed in ascending edge index by one thread.
constexpr uint8_t kInterior = 0, kBorder = 1, kLocked = 2;

struct OpenInfo {
    unsigned long long taken, boundary_taken, border, planes;
};

struct Open {
    OpenInfo *info;
    int32_t *nb;        // [V] boundary edges at the vertex
    uint8_t *bad;       // [V] an edge at the vertex has uses other than 1 or 2
    uint8_t *cls;       // [V]
    uint8_t *iso;       // [E] the edge belongs to a face whose three edges are boundary edges
    int32_t *weight;    // [E] faces the i-th edge of the sorted selection removes, 0 behind the selection
    int32_t *before;    // [E] exclusive scan of weight
    double *eplane;     // [4E] constraint plane of a boundary edge, else zero
    void *temp;
    size_t temp_bytes;
    int64_t bytes;
};

size_t scan_bytes_for(int64_t E, hipStream_t s)
{
    size_t b = 0;
    if (rocprim::exclusive_scan(nullptr, b, (int32_t *)nullptr, (int32_t *)nullptr, (int32_t)0, (size_t)(E > 0 ? E : 1),
                                rocprim::plus<int32_t>(), s) != hipSuccess)
        return 0;
    return b > 0 ? b : 1;
}

// The collapse-mode arrays lie behind the lock-mode workspace.
Open carve_open(void *base, int64_t first, int64_t V, int64_t E, size_t temp)
{
    Open o;
    QfCarver c{base, qf_align_up(first)};
    o.info = c.take<OpenInfo>(1);
    o.nb = c.take<int32_t>(V);
    o.bad = c.take<uint8_t>(V);
    o.cls = c.take<uint8_t>(V);
    o.iso = c.take<uint8_t>(E);
    o.weight = c.take<int32_t>(E);
    o.before = c.take<int32_t>(E);
    o.eplane = c.take<double>(4 * E);
    o.temp = c.take<char>((int64_t)temp);
    o.temp_bytes = temp;
    o.bytes = c.off;
    return o;
}

__device__ __forceinline__ bool edge_ok(const int64_t *edges, int64_t e, int64_t V)
{
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    return a >= 0 && a < b && b < V;
}

// One thread per half-edge: the constraint plane of a boundary edge from its one face.
__global__ __launch_bounds__(kBlock) void boundary_plane_kernel(Mesh M, Workspace ws, Open ox)
{
    const int64_t i = gtid();
    if (i >= 3 * M.F) return;
    const int64_t e = M.face_edges[i];
    if (e < 0 || e >= M.E || ws.uses[e] != 1 || !edge_ok(M.edges, e, M.V)) return;
    const int64_t *t = M.f + 3 * (i / 3);
    if (!face_ok(t, M.V) || t[0] == t[1] || t[1] == t[2] || t[0] == t[2]) return;
    const double *p0 = M.p + 3 * t[0];
    double n0, n1, n2;
    cross_of(p0, M.p + 3 * t[1], M.p + 3 * t[2], n0, n1, n2);
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    if (len == 0.0) return;
    n0 = n0 / len;
    n1 = n1 / len;
    n2 = n2 / len;
    if (n0 == 0.0 && n1 == 0.0 && n2 == 0.0) return;
    const double *pa = M.p + 3 * M.edges[2 * e], *pb = M.p + 3 * M.edges[2 * e + 1];
    const double d0 = pb[0] - pa[0], d1 = pb[1] - pa[1], d2 = pb[2] - pa[2];
    double m0 = d1 * n2 - d2 * n1;
    double m1 = d2 * n0 - d0 * n2;
    double m2 = d0 * n1 - d1 * n0;
    const double ml = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
    if (ml == 0.0) return;
    m0 = m0 / ml;
    m1 = m1 / ml;
    m2 = m2 / ml;
    double *o = ox.eplane + 4 * e;
    o[0] = m0;
    o[1] = m1;
    o[2] = m2;
    o[3] = -((m0 * pa[0] + m1 * pa[1]) + m2 * pa[2]);
    atomicAdd(&ox.info->planes, 1ull);
}

// vertex << 32 | edge for both ends of a boundary edge, else kNone.
__global__ __launch_bounds__(kBlock) void boundary_key_kernel(Mesh M, Workspace ws)
{
    const int64_t e = gtid();
    if (e >= M.E) return;
    const bool ok = edge_ok(M.edges, e, M.V);
    if (!ok) atomicAdd(&ws.info->invalid, 1ull);
    const bool on = ok && ws.uses[e] == 1;
    ws.nkey_a[2 * e] = on ? ((uint64_t)M.edges[2 * e] << 32 | (uint64_t)e) : kNone;
    ws.nkey_a[2 * e + 1] = on ? ((uint64_t)M.edges[2 * e + 1] << 32 | (uint64_t)e) : kNone;
}

// Q[v] += weight * (m, d)(m, d)^T over the boundary edges of v in ascending edge index.
__global__ __launch_bounds__(kBlock) void boundary_sum_kernel(int64_t V, Workspace ws, Open ox, double weight, double *Q)
{
    const int64_t v = gtid();
    if (v >= V) return;
    const int64_t js = ws.nstart[v], je = ws.nend[v];
    if (js >= je) return;
    double *o = Q + 10 * v;
    double q0 = o[0], q1 = o[1], q2 = o[2], q3 = o[3], q4 = o[4], q5 = o[5], q6 = o[6], q7 = o[7], q8 = o[8], q9 = o[9];
    for (int64_t j = js; j < je; ++j) {
        const double *p = ox.eplane + 4 * (int64_t)(ws.nkey_b[j] & 0xffffffffu);
        const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
        if (p0 == 0.0 && p1 == 0.0 && p2 == 0.0) continue;
        q0 = q0 + weight * (p0 * p0);
        q1 = q1 + weight * (p0 * p1);
        q2 = q2 + weight * (p0 * p2);
        q3 = q3 + weight * (p0 * p3);
        q4 = q4 + weight * (p1 * p1);
        q5 = q5 + weight * (p1 * p2);
        q6 = q6 + weight * (p1 * p3);
        q7 = q7 + weight * (p2 * p2);
        q8 = q8 + weight * (p2 * p3);
        q9 = q9 + weight * (p3 * p3);
    }
    o[0] = q0; o[1] = q1; o[2] = q2; o[3] = q3; o[4] = q4;
    o[5] = q5; o[6] = q6; o[7] = q7; o[8] = q8; o[9] = q9;
}

__global__ void boundary_counts_kernel(Workspace ws, Open ox, int64_t *counts)
{
    counts[0] = (int64_t)ox.info->planes;
    counts[1] = (int64_t)ws.info->invalid;
}

// Step 2, per edge: the boundary edges of both ends are counted, the ends of any other edge without two uses flagged.
__global__ __launch_bounds__(kBlock) void class_edge_kernel(Mesh M, Workspace ws, Open ox)
{
    const int64_t e = gtid();
    if (e >= M.E || ws.nkey_a[2 * e] == kNone) return;
    const int32_t u = ws.uses[e];
    if (u == 2) return;
    const int64_t a = M.edges[2 * e], b = M.edges[2 * e + 1];
    if (u == 1) {
        atomicAdd(&ox.nb[a], 1);
        atomicAdd(&ox.nb[b], 1);
    } else {
        ox.bad[a] = 1;
        ox.bad[b] = 1;
    }
}

// Every edge of a face whose three edges are boundary edges (every writer stores the same 1).
__global__ __launch_bounds__(kBlock) void isolated_kernel(Mesh M, Workspace ws, Open ox)
{
    const int64_t f = gtid();
    if (f >= M.F) return;
    const int64_t e0 = M.face_edges[3 * f], e1 = M.face_edges[3 * f + 1], e2 = M.face_edges[3 * f + 2];
    if (e0 < 0 || e0 >= M.E || e1 < 0 || e1 >= M.E || e2 < 0 || e2 >= M.E) return;
    if (ws.uses[e0] != 1 || ws.uses[e1] != 1 || ws.uses[e2] != 1) return;
    ox.iso[e0] = 1;
    ox.iso[e1] = 1;
    ox.iso[e2] = 1;
}

__global__ __launch_bounds__(kBlock) void class_vertex_kernel(int64_t V, const uint8_t *vertex_lock, Workspace ws, Open ox)
{
    const int64_t v = gtid();
    if (v >= V) return;
    const int32_t nb = ox.nb[v];
    uint8_t c = kLocked;
    if (!(vertex_lock && vertex_lock[v]) && !ox.bad[v]) c = nb == 0 ? kInterior : nb == 2 ? kBorder : kLocked;
    ox.cls[v] = c;
    if (c == kLocked) atomicAdd(&ws.info->locked, 1ull);
    if (nb == 2 && !ox.bad[v]) atomicAdd(&ox.info->border, 1ull);
}

// The border end whose position an edge with two uses collapses to, or -1: the edge class that select and apply share.
__device__ __forceinline__ int64_t pinned_end(const Workspace &ws, const Open &ox, int64_t e, int64_t a, int64_t b)
{
    if (ws.uses[e] != 2 || ox.cls[a] == ox.cls[b]) return -1;
    return ox.cls[a] == kBorder ? a : b;
}

// Steps 3 to 5 and m1 in collapse mode, one thread per edge.
__global__ __launch_bounds__(kBlock) void candidate_open_kernel(Mesh M, Workspace ws, Open ox, double max_cost, uint64_t round)
{
    const int64_t e = gtid();
    if (e >= M.E) return;
    ws.key[e] = kNone;
    ws.skey_a[e] = kNone;
    if (ws.nkey_a[2 * e] == kNone) return;
    const int64_t a = M.edges[2 * e], b = M.edges[2 * e + 1];
    const uint8_t ca = ox.cls[a], cb = ox.cls[b];
    if (ca == kLocked || cb == kLocked) return;
    const int32_t u = ws.uses[e];
    if (u == 2) {
        if (ca == kBorder && cb == kBorder) return;        // a chord
    } else if (u != 1 || ox.iso[e]) {
        return;
    }
    double qe[10], z0, z1, z2, cost;
    collapse_point(M.p, M.Q, a, b, pinned_end(ws, ox, e, a, b), qe, z0, z1, z2, cost);
    if (cost > max_cost) return;
    atomicAdd(&ws.info->candidates, 1ull);

    if (!collapse_legal(M, ws, e, a, b, z0, z1, z2)) return;
    atomicAdd(&ws.info->legal, 1ull);
    const uint64_t bits = (uint64_t)__double_as_longlong(cost);
    const uint64_t key = (bits >> 52) << 52 | (mix((uint64_t)a << 32 | (uint64_t)b, round) & 0x1FFFFFull) << 31 | (uint64_t)e;
    ws.key[e] = key;
    ws.skey_a[e] = bits;
    atomicMin((unsigned long long *)&ws.m1[a], (unsigned long long)key);
    atomicMin((unsigned long long *)&ws.m1[b], (unsigned long long)key);
}

// Step 7: the faces the i-th edge of the sorted selection removes.
__global__ __launch_bounds__(kBlock) void weight_kernel(int64_t E, Workspace ws, Open ox)
{
    const int64_t i = gtid();
    if (i >= E) return;
    ox.weight[i] = ws.skey_b[i] == kNone ? 0 : ws.uses[ws.sval_b[i]];
}

__device__ __forceinline__ bool taken_at(const Workspace &ws, const Open &ox, int64_t i, int64_t faces_to_remove)
{
    return ws.skey_b[i] != kNone && (int64_t)ox.before[i] < faces_to_remove;
}

__global__ __launch_bounds__(kBlock) void budget_kernel(int64_t E, int64_t faces_to_remove, Workspace ws, Open ox)
{
    const int64_t i = gtid();
    if (i >= E || !taken_at(ws, ox, i, faces_to_remove)) return;
    atomicAdd(&ox.info->taken, 1ull);
    if (ox.weight[i] == 1) atomicAdd(&ox.info->boundary_taken, 1ull);
}

__global__ void open_counts_kernel(Workspace ws, Open ox, int64_t *counts)
{
    counts[0] = (int64_t)ws.info->candidates;
    counts[1] = (int64_t)ws.info->legal;
    counts[2] = (int64_t)ws.info->selected;
    counts[3] = (int64_t)ox.info->taken;
    counts[4] = (int64_t)ws.info->locked;
    counts[5] = (int64_t)ws.info->invalid;
    counts[6] = (int64_t)ox.info->boundary_taken;
    counts[7] = (int64_t)ox.info->border;
}

// Step 8 in collapse mode: as apply_kernel, with the edge class select saw.
__global__ __launch_bounds__(kBlock) void apply_open_kernel(double *p, double *Q, const int64_t *edges, int64_t E, int64_t V,
                                                            int64_t n, int64_t faces_to_remove, Workspace ws, Open ox)
{
    const int64_t i = gtid();
    if (i >= n || !taken_at(ws, ox, i, faces_to_remove)) return;
    const int64_t e = ws.sval_b[i];
    if (e < 0 || e >= E || !edge_ok(edges, e, V)) return;      // a workspace that select did not fill
    const int64_t a = edges[2 * e], b = edges[2 * e + 1];
    double qe[10], z0, z1, z2, cost;
    collapse_point(p, Q, a, b, pinned_end(ws, ox, e, a, b), qe, z0, z1, z2, cost);
    p[3 * a] = z0;
    p[3 * a + 1] = z1;
    p[3 * a + 2] = z2;
    double *qa = Q + 10 * a;
#pragma unroll
    for (int k = 0; k < 10; ++k) qa[k] = qe[k];
    ws.remap[b] = (int32_t)a;
}

__global__ __launch_bounds__(kBlock) void gather_vertex_kernel(const double *Q, const uint8_t *lock, const int64_t *vertex_map,
                                                               int64_t V, int64_t n_out, double *out_Q, uint8_t *out_lock,
                                                               int32_t *inverse)
{
    const int64_t j = gtid();
    if (j >= n_out) return;
    const int64_t s = vertex_map[j];
    if (s < 0 || s >= V) return;
#pragma unroll
    for (int k = 0; k < 10; ++k) out_Q[10 * j + k] = Q[10 * s + k];
    if (lock) out_lock[j] = lock[s];
    inverse[s] = (int32_t)j;
}

__global__ __launch_bounds__(kBlock) void gather_face_kernel(const int64_t *face_map, const int64_t *compact_face_map,
                                                             int64_t F, int64_t n_out, int64_t *out_face_map)
{
    const int64_t i = gtid();
    if (i >= n_out) return;
    const int64_t s = compact_face_map[i];
    if (s >= 0 && s < F) out_face_map[i] = face_map[s];
}

__global__ __launch_bounds__(kBlock) void target_kernel(int64_t *target, int64_t n, int64_t V, const int32_t *inverse)
{
    const int64_t i = gtid();
    if (i >= n) return;
    const int64_t t = target[i];
    if (t >= 0 && t < V) target[i] = inverse[t];
}

// The CSR of faces: keys, sort, runs.
int build_face_rows(const Mesh &M, Workspace &ws, hipStream_t s)
{
    QF_HIP_TRY(hipMemsetAsync(ws.fstart, 0, 8 * (size_t)M.V, s));
    QF_HIP_TRY(hipMemsetAsync(ws.fend, 0, 8 * (size_t)M.V, s));
    if (M.F == 0) return QF_OK;
    const int64_t n = 3 * M.F;
    QF_MESH_LAUNCH(face_key_kernel, n, M, ws);
    size_t tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_keys(ws.temp, tb, ws.fkey_a, ws.fkey_b, (size_t)n, 0, 64, s));
    QF_MESH_LAUNCH(range_kernel, n, ws.fkey_b, n, ws.fstart, ws.fend);
    return QF_OK;
}

// The CSR of vertex neighbours: the two keys `key_kernel` gives every edge, sort, runs.
int build_neighbour_rows(const Mesh &M, Workspace &ws, void (*key_kernel)(Mesh, Workspace), hipStream_t s)
{
    QF_HIP_TRY(hipMemsetAsync(ws.nstart, 0, 8 * (size_t)M.V, s));
    QF_HIP_TRY(hipMemsetAsync(ws.nend, 0, 8 * (size_t)M.V, s));
    if (M.E == 0) return QF_OK;
    QF_MESH_LAUNCH(key_kernel, M.E, M, ws);
    size_t tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_keys(ws.temp, tb, ws.nkey_a, ws.nkey_b, (size_t)(2 * M.E), 0, 64, s));
    QF_MESH_LAUNCH(range_kernel, 2 * M.E, ws.nkey_b, 2 * M.E, ws.nstart, ws.nend);
    return QF_OK;
}

}  // namespace

extern "C" int64_t qf_mesh_decimate_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges)) return -1;
    const size_t temp = temp_bytes_for(n_faces, n_edges, nullptr);
    if (temp == 0) return -1;
    return carve(nullptr, n_vertices, n_faces, n_edges, temp).bytes;
}

extern "C" int qf_mesh_vertex_quadrics(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                       double *quadrics, void *workspace, int64_t workspace_bytes, int64_t *counts,
                                       void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, 0) || !vertices || (n_faces > 0 && !faces) || !quadrics || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(n_faces, 0, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, n_vertices, n_faces, 0, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const Mesh M{vertices, faces, nullptr, nullptr, nullptr, n_vertices, n_faces, 0};

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    const int st = build_face_rows(M, ws, s);
    if (st != QF_OK) return st;
    QF_MESH_LAUNCH(plane_kernel, M.F, M, ws);
    QF_MESH_LAUNCH(quadric_kernel, M.V, M, ws, quadrics);
    hipLaunchKernelGGL(quadric_counts_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_collapse_select(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                       const int64_t *edges, int64_t n_edges, const int64_t *face_edges,
                                       const double *quadrics, const uint8_t *vertex_lock, double max_cost, int64_t round,
                                       int64_t max_take, void *workspace, int64_t workspace_bytes, int64_t *counts,
                                       void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || !vertices || (n_faces > 0 && (!faces || !face_edges)) ||
        (n_edges > 0 && !edges) || !quadrics || !workspace || !counts || !(max_cost >= 0.0) || round < 0 || max_take < 0)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(n_faces, n_edges, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, n_vertices, n_faces, n_edges, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const Mesh M{vertices, faces, edges, face_edges, quadrics, n_vertices, n_faces, n_edges};
    const int64_t V = M.V, F = M.F, E = M.E;

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ws.m1, 0xff, 8 * (size_t)V, s));
    int st = build_face_rows(M, ws, s);
    if (st != QF_OK) return st;
    QF_MESH_LAUNCH(lock_init_kernel, V, V, vertex_lock, ws);
    st = build_neighbour_rows(M, ws, edge_key_kernel, s);
    if (st != QF_OK) return st;
    if (E > 0) {
        QF_HIP_TRY(hipMemsetAsync(ws.uses, 0, 4 * (size_t)E, s));
        QF_MESH_LAUNCH(uses_kernel, 3 * F, M, ws);
        QF_MESH_LAUNCH(lock_edge_kernel, E, M, ws);
    }
    QF_MESH_LAUNCH(lock_count_kernel, V, V, ws);
    if (E > 0) {
        QF_MESH_LAUNCH(candidate_kernel, E, M, ws, max_cost, (uint64_t)round);
        QF_MESH_LAUNCH(min2_kernel, V, V, ws);
        QF_MESH_LAUNCH(select_kernel, E, M, ws);
        size_t tb = ws.temp_bytes;
        QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.skey_a, ws.skey_b, ws.sval_a, ws.sval_b, (size_t)E, 0, 64, s));
    }
    hipLaunchKernelGGL(collapse_counts_kernel, dim3(1), dim3(1), 0, s, ws, max_take, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_collapse_apply(double *vertices, int64_t n_vertices, int64_t *faces, int64_t n_faces,
                                      const int64_t *edges, int64_t n_edges, double *quadrics, int64_t max_take,
                                      int64_t *vertex_target, int64_t n_targets, void *workspace, int64_t workspace_bytes,
                                      void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || !vertices || (n_faces > 0 && !faces) || (n_edges > 0 && !edges) ||
        !quadrics || !workspace || max_take < 0 || n_targets < 0 || n_targets >= kMaxCount || (n_targets > 0 && !vertex_target))
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(n_faces, n_edges, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, n_vertices, n_faces, n_edges, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;

    QF_HIP_TRY(hipMemsetAsync(ws.remap, 0xff, 4 * (size_t)n_vertices, s));
    const int64_t n = max_take < n_edges ? max_take : n_edges;
    QF_MESH_LAUNCH(apply_kernel, n, vertices, quadrics, edges, n, ws);
    QF_MESH_LAUNCH(remap_kernel, 3 * n_faces, faces, 3 * n_faces, n_vertices, ws.remap);
    QF_MESH_LAUNCH(remap_kernel, n_targets, vertex_target, n_targets, n_vertices, ws.remap);
    return QF_OK;
}

extern "C" int qf_mesh_collapse_gather(const double *quadrics, const uint8_t *vertex_lock, const int64_t *face_map,
                                       int64_t n_vertices, int64_t n_faces, const int64_t *vertex_map,
                                       int64_t n_out_vertices, const int64_t *compact_face_map, int64_t n_out_faces,
                                       double *out_quadrics, uint8_t *out_lock, int64_t *out_face_map,
                                       int64_t *vertex_target, int64_t n_targets, void *workspace, int64_t workspace_bytes,
                                       void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, 0) || n_out_vertices < 0 || n_out_vertices > n_vertices || n_out_faces < 0 ||
        n_out_faces > n_faces || !quadrics || (n_faces > 0 && !face_map) || (!vertex_lock != !out_lock) ||
        (n_out_vertices > 0 && (!vertex_map || !out_quadrics)) || (n_out_faces > 0 && (!compact_face_map || !out_face_map)) ||
        n_targets < 0 || n_targets >= kMaxCount || (n_targets > 0 && !vertex_target) || !workspace ||
        workspace_bytes < 4 * n_vertices)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    int32_t *inverse = static_cast<int32_t *>(workspace);
    QF_HIP_TRY(hipMemsetAsync(inverse, 0xff, 4 * (size_t)n_vertices, s));
    QF_MESH_LAUNCH(gather_vertex_kernel, n_out_vertices, quadrics, vertex_lock, vertex_map, n_vertices, n_out_vertices,
                   out_quadrics, out_lock, inverse);
    QF_MESH_LAUNCH(gather_face_kernel, n_out_faces, face_map, compact_face_map, n_faces, n_out_faces, out_face_map);
    QF_MESH_LAUNCH(target_kernel, n_targets, vertex_target, n_targets, n_vertices, inverse);
    return QF_OK;
}

// ---- boundary = collapse: entry points -----------------------------------------------------------------------------------

namespace {

struct OpenSpace {
    Workspace ws;
    Open ox;
};

// 0 for a rocPRIM size query that failed.
int64_t carve_both(void *base, int64_t V, int64_t F, int64_t E, hipStream_t s, OpenSpace &out)
{
    const size_t temp = temp_bytes_for(F, E, s);
    const size_t scan = scan_bytes_for(E, s);
    if (temp == 0 || scan == 0) return 0;
    out.ws = carve(base, V, F, E, temp);
    out.ox = carve_open(base, out.ws.bytes, V, E, scan);
    return out.ox.bytes;
}

}  // namespace

extern "C" int64_t qf_mesh_decimate_open_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges)) return -1;
    OpenSpace sp;
    const int64_t bytes = carve_both(nullptr, n_vertices, n_faces, n_edges, nullptr, sp);
    return bytes > 0 ? bytes : -1;
}

extern "C" int qf_mesh_boundary_quadrics(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                         const int64_t *edges, int64_t n_edges, const int64_t *face_edges, double *quadrics,
                                         double boundary_weight, void *workspace, int64_t workspace_bytes, int64_t *counts,
                                         void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || !vertices || (n_faces > 0 && (!faces || !face_edges)) ||
        (n_edges > 0 && !edges) || !quadrics || !workspace || !counts || !(boundary_weight >= 0.0) || std::isinf(boundary_weight))
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    OpenSpace sp;
    const int64_t need = carve_both(workspace, n_vertices, n_faces, n_edges, s, sp);
    if (need == 0) return QF_ERR_HIP;
    if (workspace_bytes < need) return QF_ERR_INVALID_ARGUMENT;
    Workspace &ws = sp.ws;
    Open &ox = sp.ox;
    const Mesh M{vertices, faces, edges, face_edges, quadrics, n_vertices, n_faces, n_edges};
    const int64_t V = M.V, F = M.F, E = M.E;

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ox.info, 0, sizeof(OpenInfo), s));
    if (E > 0) {
        QF_HIP_TRY(hipMemsetAsync(ws.uses, 0, 4 * (size_t)E, s));
        QF_HIP_TRY(hipMemsetAsync(ox.eplane, 0, 32 * (size_t)E, s));
        QF_MESH_LAUNCH(uses_kernel, 3 * F, M, ws);
        QF_MESH_LAUNCH(boundary_plane_kernel, 3 * F, M, ws, ox);
        const int st = build_neighbour_rows(M, ws, boundary_key_kernel, s);
        if (st != QF_OK) return st;
        QF_MESH_LAUNCH(boundary_sum_kernel, V, V, ws, ox, boundary_weight, quadrics);
    }
    hipLaunchKernelGGL(boundary_counts_kernel, dim3(1), dim3(1), 0, s, ws, ox, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_collapse_select_open(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                            const int64_t *edges, int64_t n_edges, const int64_t *face_edges,
                                            const double *quadrics, const uint8_t *vertex_lock, double max_cost,
                                            int64_t round, int64_t faces_to_remove, void *workspace, int64_t workspace_bytes,
                                            int64_t *counts, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || !vertices || (n_faces > 0 && (!faces || !face_edges)) ||
        (n_edges > 0 && !edges) || !quadrics || !workspace || !counts || !(max_cost >= 0.0) || round < 0 ||
        faces_to_remove < 0)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    OpenSpace sp;
    const int64_t need = carve_both(workspace, n_vertices, n_faces, n_edges, s, sp);
    if (need == 0) return QF_ERR_HIP;
    if (workspace_bytes < need) return QF_ERR_INVALID_ARGUMENT;
    Workspace &ws = sp.ws;
    Open &ox = sp.ox;
    const Mesh M{vertices, faces, edges, face_edges, quadrics, n_vertices, n_faces, n_edges};
    const int64_t V = M.V, F = M.F, E = M.E;

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ox.info, 0, sizeof(OpenInfo), s));
    QF_HIP_TRY(hipMemsetAsync(ws.m1, 0xff, 8 * (size_t)V, s));
    QF_HIP_TRY(hipMemsetAsync(ox.nb, 0, 4 * (size_t)V, s));
    QF_HIP_TRY(hipMemsetAsync(ox.bad, 0, (size_t)V, s));
    int st = build_face_rows(M, ws, s);
    if (st != QF_OK) return st;
    st = build_neighbour_rows(M, ws, edge_key_kernel, s);
    if (st != QF_OK) return st;
    if (E > 0) {
        QF_HIP_TRY(hipMemsetAsync(ws.uses, 0, 4 * (size_t)E, s));
        QF_HIP_TRY(hipMemsetAsync(ox.iso, 0, (size_t)E, s));
        QF_MESH_LAUNCH(uses_kernel, 3 * F, M, ws);
        QF_MESH_LAUNCH(isolated_kernel, F, M, ws, ox);
        QF_MESH_LAUNCH(class_edge_kernel, E, M, ws, ox);
    }
    QF_MESH_LAUNCH(class_vertex_kernel, V, V, vertex_lock, ws, ox);
    if (E > 0) {
        QF_MESH_LAUNCH(candidate_open_kernel, E, M, ws, ox, max_cost, (uint64_t)round);
        QF_MESH_LAUNCH(min2_kernel, V, V, ws);
        QF_MESH_LAUNCH(select_kernel, E, M, ws);
        size_t tb = ws.temp_bytes;
        QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.skey_a, ws.skey_b, ws.sval_a, ws.sval_b, (size_t)E, 0, 64, s));
        QF_MESH_LAUNCH(weight_kernel, E, E, ws, ox);
        size_t sb = ox.temp_bytes;
        QF_HIP_TRY(rocprim::exclusive_scan(ox.temp, sb, ox.weight, ox.before, (int32_t)0, (size_t)E, rocprim::plus<int32_t>(), s));
        QF_MESH_LAUNCH(budget_kernel, E, E, faces_to_remove, ws, ox);
    }
    hipLaunchKernelGGL(open_counts_kernel, dim3(1), dim3(1), 0, s, ws, ox, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_collapse_apply_open(double *vertices, int64_t n_vertices, int64_t *faces, int64_t n_faces,
                                           const int64_t *edges, int64_t n_edges, double *quadrics, int64_t faces_to_remove,
                                           int64_t *vertex_target, int64_t n_targets, void *workspace,
                                           int64_t workspace_bytes, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || !vertices || (n_faces > 0 && !faces) || (n_edges > 0 && !edges) ||
        !quadrics || !workspace || faces_to_remove < 0 || n_targets < 0 || n_targets >= kMaxCount ||
        (n_targets > 0 && !vertex_target))
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    OpenSpace sp;
    const int64_t need = carve_both(workspace, n_vertices, n_faces, n_edges, s, sp);
    if (need == 0) return QF_ERR_HIP;
    if (workspace_bytes < need) return QF_ERR_INVALID_ARGUMENT;
    Workspace &ws = sp.ws;

    QF_HIP_TRY(hipMemsetAsync(ws.remap, 0xff, 4 * (size_t)n_vertices, s));
    // every taken edge removes at least one face, so no more than faces_to_remove are taken
    const int64_t n = faces_to_remove < n_edges ? faces_to_remove : n_edges;
    QF_MESH_LAUNCH(apply_open_kernel, n, vertices, quadrics, edges, n_edges, n_vertices, n, faces_to_remove, ws, sp.ox);
    QF_MESH_LAUNCH(remap_kernel, 3 * n_faces, faces, 3 * n_faces, n_vertices, ws.remap);
    QF_MESH_LAUNCH(remap_kernel, n_targets, vertex_target, n_targets, n_vertices, ws.remap);
    return QF_OK;
}
