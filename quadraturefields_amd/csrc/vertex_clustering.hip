// Vertex-clustering simplification of a triangle mesh (open3d's simplify_vertex_clustering, which the reference runs on
// the host in examples/downsample_mesh.py and mc_utils.downsample_mesh).  The rules (restated in
// numpy in tests/vertex_clustering_reference.py):
//   cells      lo = min over vertices - 0.5 s per axis; vertex v's cell is floor((v - lo) / s) per axis, in fp64;
//              at most 2^21 cells per axis, so a cell packs into the 63-bit key ix << 42 | iy << 21 | iz;
//   vertices   one per occupied cell, cells numbered in order of their smallest input vertex index;
//   average    the cell's vertices summed in ascending index, then one division by their count;
//   quadric    per face the plane (n, d) with n = (b - a) x (c - a) normalised (zero plane if |n| == 0); a vertex's
//              quadric sums p p^T over the distinct faces that use it in ascending face index, a cell's sums its
//              vertices' quadrics in ascending vertex index; y = adj(A) (b - A mean) / det A is accepted iff
//              det A > 1e-6 (tr A / 3)^3 and mean + y lies in the cell's box grown by half a voxel, else the mean;
//   faces      each face maps to its cells' ids; a face with two equal ids is dropped, the others are rotated to put
//              the smallest id first (winding kept), identical triples are kept once, output in ascending index of
//              the first face that produced each triple.
//
// Passes (one stream, no host wait inside a call):
//   count  reduce (min / max per axis, non-finite vertices, out-of-range faces) -> validate and lo -> cell keys ->
//          stable radix sort of (key, vertex) -> segment heads -> scans -> cell ids -> face triples -> two stable
//          radix sorts of (triple, face) -> keep flags of the first face per triple -> scan; counts[5];
//   emit   average: one thread per cell sums its sorted vertex run.  quadric: face planes, a stable radix sort of the
//          3F (vertex, face) incidences by vertex, then one thread per cell sums and solves.  Faces are written at
//          their scanned positions.
// Every sum runs in a fixed order in one thread, so results do not depend on the launch shape.  The file is compiled
// with -ffp-contract=off: every product and sum is rounded on its own.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "mesh_device.h"

namespace {

constexpr int kRedBlocks = 512;
constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr int64_t kAxisCells = int64_t(1) << 21;
constexpr uint32_t kDropped = 0x7fffffffu;      // above every cell id and vertex id (both < 2^31 - 1)
constexpr double kTau = 1e-6;

struct Info {
    double lo[3];
    int32_t valid;
    int32_t n_cells;        // written by the count pass
};

struct Workspace {
    Info *info;
    double *red;            // [kRedBlocks][6] per-block min xyz, max xyz over finite vertices
    int64_t *red_bad;       // [kRedBlocks][2] non-finite vertices, out-of-range faces
    uint64_t *key_a, *key_b;            // [V] cell keys, then sorted
    int32_t *vid_a, *vid_b;             // [V] vertex ids, then in sorted order
    int32_t *head;          // [V] 1 at the first sorted position of each cell
    int32_t *seg;           // [V] inclusive scan of head: segment (sorted run) index + 1
    int32_t *first;         // [V] by vertex: 1 if it is its cell's smallest vertex
    int32_t *rank;          // [V] exclusive scan of first: the cell id of a smallest vertex
    int32_t *seg_vid;       // [V] smallest vertex of each segment
    int32_t *seg_start;     // [V + 1] first sorted position of each segment, then V
    int32_t *cell_seg;      // [V] segment of each cell id
    int32_t *vcell;         // [V] cell id of each vertex
    int32_t *tri;           // [3F] rotated cell triple of each face (c0 = kDropped: dropped)
    uint64_t *fk_a, *fk_b;  // [F] c1 << 31 | c2, then sorted
    uint32_t *fk0_a, *fk0_b;            // [F] c0 in the first sort's order, then sorted
    int32_t *fid_a, *fid_b;             // [F] face ids
    int32_t *keep;          // [F] 1 for the first face of each kept triple
    int32_t *fpos;          // [F] exclusive scan of keep: output position
    uint32_t *ik_a, *ik_b;  // [3F] incidence vertex (kDropped: a repeated index within its face), then sorted
    int32_t *if_a, *if_b;   // [3F] incidence face
    int64_t *inc_start, *inc_end;       // [V] sorted incidence run of each vertex
    double *plane;          // [4F]
    void *temp;
    size_t temp_bytes;
    int64_t bytes;
};

// rocPRIM scratch for the largest of the sorts and scans below (host query).
size_t temp_bytes_for(int64_t V, int64_t F, hipStream_t s)
{
    size_t need = 0, b = 0;
    auto upd = [&](hipError_t e) {
        if (e != hipSuccess) return false;
        need = b > need ? b : need;
        return true;
    };
    const size_t v = (size_t)V, f = (size_t)(F > 0 ? F : 1), inc = 3 * f;
    if (!upd(rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                       (int32_t *)nullptr, v, 0, 63, s)))
        return 0;
    if (!upd(rocprim::inclusive_scan(nullptr, b, (int32_t *)nullptr, (int32_t *)nullptr, v, rocprim::plus<int32_t>(),
                                     s)))
        return 0;
    if (!upd(rocprim::exclusive_scan(nullptr, b, (int32_t *)nullptr, (int32_t *)nullptr, 0, v > f ? v : f,
                                     rocprim::plus<int32_t>(), s)))
        return 0;
    if (!upd(rocprim::radix_sort_pairs(nullptr, b, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                       (int32_t *)nullptr, f, 0, 62, s)))
        return 0;
    if (!upd(rocprim::radix_sort_pairs(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                       (int32_t *)nullptr, f, 0, 31, s)))
        return 0;
    if (!upd(rocprim::radix_sort_pairs(nullptr, b, (uint32_t *)nullptr, (uint32_t *)nullptr, (int32_t *)nullptr,
                                       (int32_t *)nullptr, inc, 0, 31, s)))
        return 0;
    return need > 0 ? need : 1;
}

Workspace carve(void *base, int64_t V, int64_t F, size_t temp)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.red = c.take<double>(6 * kRedBlocks);
    w.red_bad = c.take<int64_t>(2 * kRedBlocks);
    w.key_a = c.take<uint64_t>(V);
    w.key_b = c.take<uint64_t>(V);
    w.vid_a = c.take<int32_t>(V);
    w.vid_b = c.take<int32_t>(V);
    w.head = c.take<int32_t>(V);
    w.seg = c.take<int32_t>(V);
    w.first = c.take<int32_t>(V);
    w.rank = c.take<int32_t>(V);
    w.seg_vid = c.take<int32_t>(V);
    w.seg_start = c.take<int32_t>(V + 1);
    w.cell_seg = c.take<int32_t>(V);
    w.vcell = c.take<int32_t>(V);
    w.tri = c.take<int32_t>(3 * F);
    w.fk_a = c.take<uint64_t>(F);
    w.fk_b = c.take<uint64_t>(F);
    w.fk0_a = c.take<uint32_t>(F);
    w.fk0_b = c.take<uint32_t>(F);
    w.fid_a = c.take<int32_t>(F);
    w.fid_b = c.take<int32_t>(F);
    w.keep = c.take<int32_t>(F);
    w.fpos = c.take<int32_t>(F);
    w.ik_a = c.take<uint32_t>(3 * F);
    w.ik_b = c.take<uint32_t>(3 * F);
    w.if_a = c.take<int32_t>(3 * F);
    w.if_b = c.take<int32_t>(3 * F);
    w.inc_start = c.take<int64_t>(V);
    w.inc_end = c.take<int64_t>(V);
    w.plane = c.take<double>(4 * F);
    w.temp = c.take<char>((int64_t)temp);
    w.temp_bytes = temp;
    w.bytes = c.off;
    return w;
}

struct Mesh {
    const double *v;
    const int64_t *f;
    int64_t V, F;
    double s;
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

// One thread: lo, the cells needed per axis, the validity flag and counts[2..4]; counts[0..1] zeroed.
__global__ void finalize_kernel(Mesh M, Workspace ws, int64_t *counts)
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
    double most = 0.0;
    for (int k = 0; k < 3; ++k) {
        const double lo = mn[k] - 0.5 * M.s;
        ws.info->lo[k] = lo;
        const double q = floor((mx[k] - lo) / M.s) + 1.0;     // cells needed along axis k
        most = fmax(most, q);
    }
    const bool ok = bad_v == 0 && bad_f == 0 && most <= (double)kAxisCells;
    ws.info->valid = ok ? 1 : 0;
    ws.info->n_cells = 0;
    counts[0] = 0;
    counts[1] = 0;
    counts[2] = bad_v;
    counts[3] = bad_f;
    counts[4] = bad_v ? 0 : (most < 4.0e18 ? (int64_t)most : (int64_t)4e18);
}

__device__ __forceinline__ int64_t cell_coord(double x, double lo, double s)
{
    const double q = floor((x - lo) / s);
    return q < 0.0 ? 0 : (q > (double)(kAxisCells - 1) ? kAxisCells - 1 : (int64_t)q);   // in range when valid
}

__global__ __launch_bounds__(kBlock) void key_kernel(Mesh M, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= M.V) return;
    uint64_t key = 0;
    if (ws.info->valid) {
        const Info &I = *ws.info;
        const uint64_t ix = cell_coord(M.v[3 * i], I.lo[0], M.s);
        const uint64_t iy = cell_coord(M.v[3 * i + 1], I.lo[1], M.s);
        const uint64_t iz = cell_coord(M.v[3 * i + 2], I.lo[2], M.s);
        key = ix << 42 | iy << 21 | iz;
    }
    ws.key_a[i] = key;
    ws.vid_a[i] = (int32_t)i;
}

// Sorted position i starts a cell's run: head flag, and the run's smallest vertex (the first: the sort is stable) is
// marked by vertex id.
__global__ __launch_bounds__(kBlock) void head_kernel(int64_t V, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= V) return;
    const int h = i == 0 || ws.key_b[i] != ws.key_b[i - 1];
    ws.head[i] = h;
    ws.first[ws.vid_b[i]] = h;
}

__global__ __launch_bounds__(kBlock) void segment_kernel(int64_t V, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= V || !ws.head[i]) return;
    const int32_t sg = ws.seg[i] - 1, v = ws.vid_b[i];
    ws.seg_vid[sg] = v;
    ws.seg_start[sg] = (int32_t)i;
    ws.cell_seg[ws.rank[v]] = sg;
}

__global__ __launch_bounds__(kBlock) void vertex_cell_kernel(int64_t V, Workspace ws, int64_t *counts)
{
    const int64_t i = gtid();
    if (i >= V) return;
    const int32_t sg = ws.seg[i] - 1;
    ws.vcell[ws.vid_b[i]] = ws.rank[ws.seg_vid[sg]];
    if (i == V - 1) {
        ws.seg_start[sg + 1] = (int32_t)V;
        ws.info->n_cells = ws.info->valid ? sg + 1 : 0;
        counts[0] = ws.info->n_cells;
    }
}

// Face f -> its rotated cell triple and the first sort key (c1, c2); dropped faces get c0 = kDropped.
__global__ __launch_bounds__(kBlock) void triple_kernel(Mesh M, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= M.F) return;
    uint32_t c[3] = {kDropped, 0, 0};
    if (ws.info->valid) {
        const uint32_t a = (uint32_t)ws.vcell[M.f[3 * f]], b = (uint32_t)ws.vcell[M.f[3 * f + 1]],
                       d = (uint32_t)ws.vcell[M.f[3 * f + 2]];
        if (a != b && b != d && a != d) {
            if (a < b && a < d) {
                c[0] = a; c[1] = b; c[2] = d;
            } else if (b < d) {
                c[0] = b; c[1] = d; c[2] = a;
            } else {
                c[0] = d; c[1] = a; c[2] = b;
            }
        }
    }
    ws.tri[3 * f] = (int32_t)c[0];
    ws.tri[3 * f + 1] = (int32_t)c[1];
    ws.tri[3 * f + 2] = (int32_t)c[2];
    ws.fk_a[f] = (uint64_t)c[1] << 31 | c[2];
    ws.fid_a[f] = (int32_t)f;
}

__global__ __launch_bounds__(kBlock) void gather_c0_kernel(int64_t F, Workspace ws)
{
    const int64_t j = gtid();
    if (j >= F) return;
    ws.fk0_a[j] = (uint32_t)ws.tri[3 * (int64_t)ws.fid_b[j]];
}

// fid_a is sorted by (c0, c1, c2), ties in ascending face index: the first face of each run of equal triples is kept.
__global__ __launch_bounds__(kBlock) void keep_kernel(int64_t F, Workspace ws)
{
    const int64_t j = gtid();
    if (j >= F) return;
    const int64_t f = ws.fid_a[j];
    const int32_t *t = ws.tri + 3 * f;
    int k = (uint32_t)t[0] != kDropped;
    if (k && j > 0) {
        const int32_t *u = ws.tri + 3 * (int64_t)ws.fid_a[j - 1];
        k = !(u[0] == t[0] && u[1] == t[1] && u[2] == t[2]);
    }
    ws.keep[f] = k;
}

__global__ void face_total_kernel(int64_t F, Workspace ws, int64_t *counts)
{
    if (ws.info->valid) counts[1] = (int64_t)ws.fpos[F - 1] + ws.keep[F - 1];
}

// ---- emit ----------------------------------------------------------------------------------------------------------

__device__ __forceinline__ void cell_mean(const Mesh &M, const Workspace &ws, int32_t sg, double m[3])
{
    const int32_t b = ws.seg_start[sg], e = ws.seg_start[sg + 1];
    double sum[3] = {0.0, 0.0, 0.0};
    for (int32_t i = b; i < e; ++i) {
        const int64_t v = ws.vid_b[i];
        sum[0] = sum[0] + M.v[3 * v];
        sum[1] = sum[1] + M.v[3 * v + 1];
        sum[2] = sum[2] + M.v[3 * v + 2];
    }
    const double n = (double)(e - b);
    m[0] = sum[0] / n;
    m[1] = sum[1] / n;
    m[2] = sum[2] / n;
}

__global__ __launch_bounds__(kBlock) void average_kernel(Mesh M, Workspace ws, double *out, int64_t n_out)
{
    const int64_t c = gtid();
    if (c >= ws.info->n_cells || c >= n_out || !ws.info->valid) return;
    const int32_t sg = ws.cell_seg[c];
    double m[3];
    cell_mean(M, ws, sg, m);
    out[3 * c] = m[0];
    out[3 * c + 1] = m[1];
    out[3 * c + 2] = m[2];
}

__global__ __launch_bounds__(kBlock) void plane_kernel(Mesh M, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= M.F || !ws.info->valid) return;
    const double *a = M.v + 3 * M.f[3 * f], *b = M.v + 3 * M.f[3 * f + 1], *c = M.v + 3 * M.f[3 * f + 2];
    const double u0 = b[0] - a[0], u1 = b[1] - a[1], u2 = b[2] - a[2];
    const double w0 = c[0] - a[0], w1 = c[1] - a[1], w2 = c[2] - a[2];
    double n0 = u1 * w2 - u2 * w1;
    double n1 = u2 * w0 - u0 * w2;
    double n2 = u0 * w1 - u1 * w0;
    const double len = sqrt((n0 * n0 + n1 * n1) + n2 * n2);
    double d = 0.0;
    if (len == 0.0) {
        n0 = n1 = n2 = 0.0;
    } else {
        n0 = n0 / len;
        n1 = n1 / len;
        n2 = n2 / len;
        d = -((n0 * a[0] + n1 * a[1]) + n2 * a[2]);
    }
    double *p = ws.plane + 4 * f;
    p[0] = n0;
    p[1] = n1;
    p[2] = n2;
    p[3] = d;
}

// Incidence 3f + k -> (vertex, face); a vertex repeated within its face counts once, at its first position.
__global__ __launch_bounds__(kBlock) void incidence_kernel(Mesh M, Workspace ws)
{
    const int64_t i = gtid();
    if (i >= 3 * M.F) return;
    const int64_t f = i / 3, k = i - 3 * f;
    const int64_t *t = M.f + 3 * f;
    const bool dup = (k == 1 && t[1] == t[0]) || (k == 2 && (t[2] == t[0] || t[2] == t[1]));
    ws.ik_a[i] = (dup || !ws.info->valid) ? kDropped : (uint32_t)t[k];
    ws.if_a[i] = (int32_t)f;
}

__global__ __launch_bounds__(kBlock) void incidence_range_kernel(int64_t n_inc, Workspace ws)
{
    const int64_t j = gtid();
    if (j >= n_inc) return;
    const uint32_t v = ws.ik_b[j];
    if (v == kDropped) return;
    if (j == 0 || ws.ik_b[j - 1] != v) ws.inc_start[v] = j;
    if (j == n_inc - 1 || ws.ik_b[j + 1] != v) ws.inc_end[v] = j + 1;
}

__global__ __launch_bounds__(kBlock) void quadric_kernel(Mesh M, Workspace ws, double *out, int64_t n_out,
                                                         unsigned long long *n_fallback)
{
    const int64_t c = gtid();
    if (c >= ws.info->n_cells || c >= n_out || !ws.info->valid) return;
    const int32_t sg = ws.cell_seg[c];
    double m[3];
    cell_mean(M, ws, sg, m);
    // Q's upper triangle: q00 q01 q02 q03 q11 q12 q13 q22 q23 q33
    double Q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int32_t i = ws.seg_start[sg], e = ws.seg_start[sg + 1]; i < e; ++i) {
        const int64_t v = ws.vid_b[i];
        double q[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int64_t j = ws.inc_start[v], je = ws.inc_end[v]; j < je; ++j) {
            const double *p = ws.plane + 4 * (int64_t)ws.if_b[j];
            const double p0 = p[0], p1 = p[1], p2 = p[2], p3 = p[3];
            q[0] = q[0] + p0 * p0;
            q[1] = q[1] + p0 * p1;
            q[2] = q[2] + p0 * p2;
            q[3] = q[3] + p0 * p3;
            q[4] = q[4] + p1 * p1;
            q[5] = q[5] + p1 * p2;
            q[6] = q[6] + p1 * p3;
            q[7] = q[7] + p2 * p2;
            q[8] = q[8] + p2 * p3;
            q[9] = q[9] + p3 * p3;
        }
        for (int k = 0; k < 10; ++k) Q[k] = Q[k] + q[k];
    }
    const double a00 = Q[0], a01 = Q[1], a02 = Q[2], a11 = Q[4], a12 = Q[5], a22 = Q[7];
    const double b0 = -Q[3], b1 = -Q[6], b2 = -Q[8];
    const double r0 = b0 - ((a00 * m[0] + a01 * m[1]) + a02 * m[2]);
    const double r1 = b1 - ((a01 * m[0] + a11 * m[1]) + a12 * m[2]);
    const double r2 = b2 - ((a02 * m[0] + a12 * m[1]) + a22 * m[2]);
    const double c00 = a11 * a22 - a12 * a12;
    const double c01 = a12 * a02 - a01 * a22;
    const double c02 = a01 * a12 - a11 * a02;
    const double c11 = a00 * a22 - a02 * a02;
    const double c12 = a01 * a02 - a00 * a12;
    const double c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double t3 = ((a00 + a11) + a22) / 3.0;
    bool accept = det > kTau * ((t3 * t3) * t3);
    double x[3] = {m[0], m[1], m[2]};
    if (accept) {
        double y[3];
        y[0] = ((c00 * r0 + c01 * r1) + c02 * r2) / det;
        y[1] = ((c01 * r0 + c11 * r1) + c12 * r2) / det;
        y[2] = ((c02 * r0 + c12 * r1) + c22 * r2) / det;
        const uint64_t key = ws.key_b[ws.seg_start[sg]];
        const double idx[3] = {(double)(key >> 42), (double)((key >> 21) & (kAxisCells - 1)),
                               (double)(key & (kAxisCells - 1))};
        double z[3];
        for (int k = 0; k < 3; ++k) {
            z[k] = m[k] + y[k];
            const double lo = ws.info->lo[k] + (idx[k] - 0.5) * M.s;
            const double hi = ws.info->lo[k] + (idx[k] + 1.5) * M.s;
            accept = accept && z[k] >= lo && z[k] <= hi;
        }
        if (accept) {
            x[0] = z[0];
            x[1] = z[1];
            x[2] = z[2];
        }
    }
    if (!accept && n_fallback) atomicAdd(n_fallback, 1ull);
    out[3 * c] = x[0];
    out[3 * c + 1] = x[1];
    out[3 * c + 2] = x[2];
}

__global__ __launch_bounds__(kBlock) void face_emit_kernel(int64_t F, Workspace ws, int64_t *out, int64_t n_out)
{
    const int64_t f = gtid();
    if (f >= F || !ws.info->valid || !ws.keep[f]) return;
    const int64_t o = ws.fpos[f];
    if (o >= n_out) return;
    out[3 * o] = ws.tri[3 * f];
    out[3 * o + 1] = ws.tri[3 * f + 1];
    out[3 * o + 2] = ws.tri[3 * f + 2];
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && V < kMaxCount && F >= 0 && F < kMaxCount; }

bool make_mesh(const double *v, int64_t V, const int64_t *f, int64_t F, double s, Mesh *M)
{
    if (!sizes_ok(V, F) || !v || (F > 0 && !f) || !(s > 0.0) || !std::isfinite(s)) return false;
    M->v = v;
    M->f = f;
    M->V = V;
    M->F = F;
    M->s = s;
    return true;
}

}  // namespace

extern "C" int64_t qf_vertex_clustering_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!sizes_ok(n_vertices, n_faces)) return -1;
    const size_t temp = temp_bytes_for(n_vertices, n_faces, nullptr);
    if (temp == 0) return -1;
    return carve(nullptr, n_vertices, n_faces, temp).bytes;
}

extern "C" int qf_vertex_clustering_count(const double *vertices, int64_t n_vertices, const int64_t *faces,
                                          int64_t n_faces, double voxel_size, void *workspace, int64_t workspace_bytes,
                                          int64_t *counts, void *stream)
{
    Mesh M;
    if (!make_mesh(vertices, n_vertices, faces, n_faces, voxel_size, &M) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(M.V, M.F, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, M.V, M.F, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = M.V, F = M.F;
    size_t tb = ws.temp_bytes;

    hipLaunchKernelGGL(reduce_kernel, dim3(kRedBlocks), dim3(kBlock), 0, s, M, ws);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, M, ws, counts);
    QF_LAUNCH_CHECK();
    QF_MESH_LAUNCH(key_kernel, V, M, ws);
    QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.key_a, ws.key_b, ws.vid_a, ws.vid_b, (size_t)V, 0, 63, s));
    QF_MESH_LAUNCH(head_kernel, V, V, ws);
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::inclusive_scan(ws.temp, tb, ws.head, ws.seg, (size_t)V, rocprim::plus<int32_t>(), s));
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::exclusive_scan(ws.temp, tb, ws.first, ws.rank, 0, (size_t)V, rocprim::plus<int32_t>(), s));
    QF_MESH_LAUNCH(segment_kernel, V, V, ws);
    QF_MESH_LAUNCH(vertex_cell_kernel, V, V, ws, counts);
    if (F == 0) return QF_OK;
    QF_MESH_LAUNCH(triple_kernel, F, M, ws);
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.fk_a, ws.fk_b, ws.fid_a, ws.fid_b, (size_t)F, 0, 62, s));
    QF_MESH_LAUNCH(gather_c0_kernel, F, F, ws);
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.fk0_a, ws.fk0_b, ws.fid_b, ws.fid_a, (size_t)F, 0, 31, s));
    QF_MESH_LAUNCH(keep_kernel, F, F, ws);
    tb = ws.temp_bytes;
    QF_HIP_TRY(rocprim::exclusive_scan(ws.temp, tb, ws.keep, ws.fpos, 0, (size_t)F, rocprim::plus<int32_t>(), s));
    hipLaunchKernelGGL(face_total_kernel, dim3(1), dim3(1), 0, s, F, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_vertex_clustering_emit(const double *vertices, int64_t n_vertices, const int64_t *faces,
                                         int64_t n_faces, double voxel_size, int contraction, void *workspace,
                                         int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                                         int64_t *out_faces, int64_t n_out_faces, int64_t *n_fallback, void *stream)
{
    Mesh M;
    if (!make_mesh(vertices, n_vertices, faces, n_faces, voxel_size, &M) || !workspace)
        return QF_ERR_INVALID_ARGUMENT;
    if (contraction != QF_CLUSTER_AVERAGE && contraction != QF_CLUSTER_QUADRIC) return QF_ERR_INVALID_ARGUMENT;
    if (n_out_vertices < 0 || n_out_vertices > M.V || n_out_faces < 0 || n_out_faces > M.F ||
        (n_out_vertices > 0 && !out_vertices) || (n_out_faces > 0 && !out_faces))
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const size_t temp = temp_bytes_for(M.V, M.F, s);
    if (temp == 0) return QF_ERR_HIP;
    Workspace ws = carve(workspace, M.V, M.F, temp);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = M.V, F = M.F;
    unsigned long long *fb = reinterpret_cast<unsigned long long *>(n_fallback);
    if (fb) QF_HIP_TRY(hipMemsetAsync(fb, 0, sizeof(int64_t), s));

    if (n_out_vertices > 0) {
        if (contraction == QF_CLUSTER_AVERAGE) {
            QF_MESH_LAUNCH(average_kernel, n_out_vertices, M, ws, out_vertices, n_out_vertices);
        } else {
            QF_HIP_TRY(hipMemsetAsync(ws.inc_start, 0, 8 * V, s));
            QF_HIP_TRY(hipMemsetAsync(ws.inc_end, 0, 8 * V, s));
            if (F > 0) {
                QF_MESH_LAUNCH(plane_kernel, F, M, ws);
                QF_MESH_LAUNCH(incidence_kernel, 3 * F, M, ws);
                size_t tb = ws.temp_bytes;
                QF_HIP_TRY(rocprim::radix_sort_pairs(ws.temp, tb, ws.ik_a, ws.ik_b, ws.if_a, ws.if_b, (size_t)(3 * F),
                                                     0, 31, s));
                QF_MESH_LAUNCH(incidence_range_kernel, 3 * F, 3 * F, ws);
            }
            QF_MESH_LAUNCH(quadric_kernel, n_out_vertices, M, ws, out_vertices, n_out_vertices, fb);
        }
    }
    if (n_out_faces > 0) {
        QF_MESH_LAUNCH(face_emit_kernel, F, F, ws, out_faces, n_out_faces);
    }
    return QF_OK;
}
