// Marching cubes over a dense fp32 volume (the mesh extraction of the reference's examples/marching_cubes.py, which
// runs scikit-image on the host).  The rules (restated in numpy in
// tests/marching_cubes_reference.py):
//   inside     grid point g is inside iff a(g) = v(g) - level, in fp32, is > 0 (a point at the level is outside);
//   vertex     edge g -> g + e_axis is crossed iff its ends differ; t = a(g) / (a(g) - a(g + e_axis)) in fp32, from
//              the lower end always; the vertex's axis coordinate is x = (float)g_axis + t, its other two are g's;
//   merge      x == g_axis or x == g_axis + 1 puts the vertex on a grid point: every crossed edge that lands there
//              shares that point's one "corner" vertex;
//   decider    a cube face with diagonal corners p, q inside and r, s outside joins p and q iff
//              a_p a_q - a_r a_s > 0 in fp64 (exact products, exact sign), the same answer in both cells;
//   polygons   each face contributes directed segments from an entry edge to an exit edge of its boundary walked
//              counter-clockwise seen from outside the cell; they chain into closed loops, fanned from the loop's
//              smallest local edge id, loops in order of that id.  (v1 - v0) x (v2 - v0) points inside -> outside;
//   order      faces in C order of cells, then loop, then fan; vertices in C order of their grid point, the corner
//              vertex first, then the +axis-0, +axis-1, +axis-2 edge vertices.
// Local numbering: corner c = d0 | d1 << 1 | d2 << 2 (d_axis = offset along that axis); edge 4 * axis + m, where m
// holds the lower corner's offsets along the two other axes, the smaller axis in bit 0.
//
// Passes (one stream, no host wait between them):
//   count   one workgroup per kTile consecutive grid points: per point its vertex count (the layout below), a
//           workgroup-local exclusive scan of it stored as int32 in the workspace, and per workgroup the totals of
//           vertices, faces and non-finite samples;
//   scan    one workgroup: exclusive offsets of the per-workgroup totals, the grand totals into counts[3];
//   emit    the count pass's tiling again: vertices at (workgroup offset + local offset), faces at the workgroup's face
//           offset plus a scan of the recounted per-cell face counts.  A face's vertex ids come from the offsets of
//           its grid points, so emit reads the volume once more and the workspace where faces land.
// The file is compiled with -ffp-contract=off: t, x and the decider are rounded one operation at a time.
#pragma clang fp contract(off)

#include <cmath>

#include "qf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kItems = 16;
constexpr int64_t kTile = (int64_t)kBlock * kItems;          // grid points per workgroup
constexpr int64_t kMaxDim = int64_t(1) << 24;                // grid coordinates exact in fp32
constexpr int64_t kMaxPoints = int64_t(1) << 31;

struct Workspace {
    int32_t *local;       // [N] vertex offset of each grid point within its workgroup's tile
    int64_t *block_v;     // [nb] vertices per tile, then (scan) the tile's first vertex
    int64_t *block_f;     // [nb] faces per tile, then the tile's first face
    int64_t *block_bad;   // [nb] non-finite samples per tile
    int64_t bytes;
};

Workspace carve(void *base, int64_t n)
{
    const int64_t nb = (n + kTile - 1) / kTile;
    Workspace w;
    QfCarver c{base};
    w.local = c.take<int32_t>(n);
    w.block_v = c.take<int64_t>(nb);
    w.block_f = c.take<int64_t>(nb);
    w.block_bad = c.take<int64_t>(nb);
    w.bytes = c.off;
    return w;
}

struct Grid {
    const float *vol;
    int n[3];
    int64_t stride[3];    // n1 n2, n2, 1
    int64_t total;
    float level;
};

// The corners of cube face (axis a, side s) in counter-clockwise order seen from outside the cell: with (b, c) =
// (a+1, a+2) mod 3, the high side walks (b, c) offsets (0,0) (1,0) (1,1) (0,1) and the low side the reverse.
__constant__ int8_t kFaceCorner[6][4] = {
    {0, 4, 6, 2}, {1, 3, 7, 5},     // axis 0: low, high
    {0, 1, 5, 4}, {2, 6, 7, 3},     // axis 1
    {0, 2, 3, 1}, {4, 5, 7, 6},     // axis 2
};

__device__ __forceinline__ int edge_of_corners(int c0, int c1)
{
    const int d = c0 ^ c1, lo = c0 & c1;
    const int ax = d == 1 ? 0 : (d == 2 ? 1 : 2);
    const int o1 = ax == 0 ? 1 : 0, o2 = ax == 2 ? 1 : 2;
    return 4 * ax + (((lo >> o1) & 1) | (((lo >> o2) & 1) << 1));
}

__device__ __forceinline__ int edge_lower_corner(int e)
{
    const int ax = e >> 2, m = e & 3;
    const int o1 = ax == 0 ? 1 : 0, o2 = ax == 2 ? 1 : 2;
    return ((m & 1) << o1) | ((m >> 1) << o2);
}

enum : int { kNone = 0, kEdge = 1, kLow = 2, kHigh = 3 };

// The edge g -> g + e_axis with lower-end value alo: not crossed, an edge vertex at axis coordinate *x, or merged into
// the lower / upper grid point.
__device__ __forceinline__ int edge_land(float alo, float ahi, int g, float *x)
{
    if ((alo > 0.0f) == (ahi > 0.0f)) return kNone;
    const float t = alo / (alo - ahi);
    const float gf = (float)g;
    const float xv = gf + t;
    *x = xv;
    if (xv == gf) return kLow;
    if (xv == (float)(g + 1)) return kHigh;
    return kEdge;
}

__device__ __forceinline__ float sample(const Grid &G, int64_t p) { return G.vol[p] - G.level; }

// Vertex slots of grid point (c[0], c[1], c[2]) = p with value a: bit 0 the corner vertex, bit 1 + axis the edge
// vertex of its +axis edge (whose coordinate goes to xs[axis]).
__device__ __forceinline__ int point_layout(const Grid &G, const int c[3], int64_t p, float a, float xs[3])
{
    int mask = 0;
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {
        float x;
        if (c[ax] + 1 < G.n[ax]) {
            const int s = edge_land(a, sample(G, p + G.stride[ax]), c[ax], &x);
            if (s == kEdge) {
                mask |= 2 << ax;
                xs[ax] = x;
            } else if (s == kLow) {
                mask |= 1;
            }
        }
        if (c[ax] > 0 && edge_land(sample(G, p - G.stride[ax]), a, c[ax] - 1, &x) == kHigh) mask |= 1;
    }
    return mask;
}

// The polygon loops of a cell with corner values a[8]: next[e] is the local edge after e in its loop (next[e] = e for
// an edge that is not crossed); returns the crossed-edge mask.
__device__ __forceinline__ int cell_loops(const float a[8], int8_t next[12])
{
    int s = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) s |= (a[c] > 0.0f) << c;
#pragma unroll
    for (int e = 0; e < 12; ++e) next[e] = (int8_t)e;
    if (s == 0 || s == 255) return 0;
    int crossed = 0;
#pragma unroll
    for (int f = 0; f < 6; ++f) {
        int q[4], in[4], E[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            q[k] = kFaceCorner[f][k];
            in[k] = (s >> q[k]) & 1;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) E[k] = edge_of_corners(q[k], q[(k + 1) & 3]);
        const int n_in = in[0] + in[1] + in[2] + in[3];
        if (n_in == 0 || n_in == 4) continue;
        if (in[0] == in[2] && in[1] == in[3]) {           // four crossings: the asymptotic decider
            const int k0 = in[0] ? 0 : 1;                   // q[k0], q[k0 + 2] inside
            const double inside = (double)a[q[k0]] * (double)a[q[k0 + 2]];
            const double outside = (double)a[q[k0 + 1]] * (double)a[(q[(k0 + 3) & 3])];
            const bool join = inside - outside > 0.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (in[k] && !join) next[E[(k + 3) & 3]] = (int8_t)E[k];       // cut the inside corner off
                if (!in[k] && join) next[E[k]] = (int8_t)E[(k + 3) & 3];       // cut the outside corner off
                crossed |= 1 << E[k];
            }
        } else {                                           // two crossings: entry (out -> in) to exit (in -> out)
            int entry = 0, exit = 0;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int k1 = (k + 1) & 3;
                if (!in[k] && in[k1]) entry = E[k];
                if (in[k] && !in[k1]) exit = E[k];
            }
            next[entry] = (int8_t)exit;
            crossed |= (1 << entry) | (1 << exit);
        }
    }
    return crossed;
}

// Triangles of a cell's loops (crossed edges minus two per loop).
__device__ __forceinline__ int cell_face_count(int crossed, const int8_t next[12])
{
    int loops = 0, seen = 0;
    for (int e = 0; e < 12; ++e) {
        if (!((crossed >> e) & 1) || ((seen >> e) & 1)) continue;
        ++loops;
        int v = e;
        for (int it = 0; it < 12; ++it) {
            seen |= 1 << v;
            v = next[v];
            if (v == e) break;
        }
    }
    return __popc(crossed) - 2 * loops;
}

__device__ __forceinline__ void point_coords(const Grid &G, int64_t p, int c[3])
{
    const uint32_t u = (uint32_t)p;                          // p < 2^31
    const uint32_t r = u / (uint32_t)G.n[2];
    c[2] = (int)(u - r * (uint32_t)G.n[2]);
    c[0] = (int)(r / (uint32_t)G.n[1]);
    c[1] = (int)(r - (uint32_t)c[0] * (uint32_t)G.n[1]);
}

__device__ __forceinline__ bool is_cell(const Grid &G, const int c[3])
{
    return c[0] + 1 < G.n[0] && c[1] + 1 < G.n[1] && c[2] + 1 < G.n[2];
}

__device__ __forceinline__ void cell_values(const Grid &G, int64_t p, float a0, float a[8])
{
    a[0] = a0;
#pragma unroll
    for (int c = 1; c < 8; ++c)
        a[c] = sample(G, p + (c & 1) * G.stride[0] + ((c >> 1) & 1) * G.stride[1] + ((c >> 2) & 1) * G.stride[2]);
}

// Exclusive scan of v over the 256 lanes of the workgroup (4 waves of 64); *total = the sum.
__device__ __forceinline__ int block_exclusive_scan(int v, int *lds, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o, 64);
        if (lane >= o) x += y;
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    int before = 0, sum = 0;
#pragma unroll
    for (int q = 0; q < kBlock / 64; ++q) {
        const int s = lds[q];
        before += q < w ? s : 0;
        sum += s;
    }
    __syncthreads();
    *total = sum;
    return before + x - v;
}

__global__ __launch_bounds__(kBlock) void count_kernel(Grid G, Workspace ws)
{
    __shared__ int lds[kBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    int running = 0, faces = 0, bad = 0;
    for (int it = 0; it < kItems; ++it) {
        const int64_t p = base + it * kBlock + threadIdx.x;
        int nv = 0;
        if (p < G.total) {
            int c[3];
            point_coords(G, p, c);
            const float a = sample(G, p);
            bad += !isfinite(a);
            float xs[3];
            nv = __popc(point_layout(G, c, p, a, xs));
            if (is_cell(G, c)) {
                float av[8];
                int8_t next[12];
                cell_values(G, p, a, av);
                const int crossed = cell_loops(av, next);
                if (crossed) faces += cell_face_count(crossed, next);
            }
        }
        int sum;
        const int off = block_exclusive_scan(nv, lds, &sum);
        if (p < G.total) ws.local[p] = running + off;
        running += sum;
    }
    int f_total, bad_total;
    block_exclusive_scan(faces, lds, &f_total);
    block_exclusive_scan(bad, lds, &bad_total);
    if (threadIdx.x == 0) {
        ws.block_v[blockIdx.x] = running;
        ws.block_f[blockIdx.x] = f_total;
        ws.block_bad[blockIdx.x] = bad_total;
    }
}

constexpr int kScanThreads = 1024;

__global__ __launch_bounds__(kScanThreads) void scan_blocks_kernel(Workspace ws, int64_t nb, int64_t *counts)
{
    __shared__ int64_t sv[kScanThreads], sf[kScanThreads], sb[kScanThreads];
    const int t = threadIdx.x;
    const int64_t per = (nb + kScanThreads - 1) / kScanThreads;
    const int64_t lo = min(nb, t * per), hi = min(nb, lo + per);
    int64_t v = 0, f = 0, b = 0;
    for (int64_t q = lo; q < hi; ++q) {
        v += ws.block_v[q];
        f += ws.block_f[q];
        b += ws.block_bad[q];
    }
    sv[t] = v;
    sf[t] = f;
    sb[t] = b;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {
        const int64_t xv = t >= o ? sv[t - o] : 0, xf = t >= o ? sf[t - o] : 0, xb = t >= o ? sb[t - o] : 0;
        __syncthreads();
        sv[t] += xv;
        sf[t] += xf;
        sb[t] += xb;
        __syncthreads();
    }
    int64_t ov = sv[t] - v, of = sf[t] - f;
    for (int64_t q = lo; q < hi; ++q) {
        const int64_t nv = ws.block_v[q], nf = ws.block_f[q];
        ws.block_v[q] = ov;
        ws.block_f[q] = of;
        ov += nv;
        of += nf;
    }
    if (t == kScanThreads - 1) {
        counts[0] = sv[t];
        counts[1] = sf[t];
        counts[2] = sb[t];
    }
}

__device__ __forceinline__ int64_t point_first_vertex(const Workspace &ws, int64_t q)
{
    return ws.block_v[q / kTile] + ws.local[q];
}

// Global id of the vertex on local edge e of the cell at grid coordinates c (corner values a).
__device__ __forceinline__ int64_t edge_vertex_id(const Grid &G, const Workspace &ws, const int c[3], int64_t p,
                                                  const float a[8], int e)
{
    const int lc = edge_lower_corner(e), ax = e >> 2;
    int g[3] = {c[0] + (lc & 1), c[1] + ((lc >> 1) & 1), c[2] + ((lc >> 2) & 1)};
    const int64_t gp = p + (lc & 1) * G.stride[0] + ((lc >> 1) & 1) * G.stride[1] + ((lc >> 2) & 1) * G.stride[2];
    float x;
    const int s = edge_land(a[lc], a[lc | (1 << ax)], g[ax], &x);
    if (s == kHigh) return point_first_vertex(ws, gp + G.stride[ax]);
    if (s == kLow) return point_first_vertex(ws, gp);
    float xs[3];
    const int mask = point_layout(G, g, gp, a[lc], xs);
    return point_first_vertex(ws, gp) + __popc(mask & ((2 << ax) - 1));
}

__global__ __launch_bounds__(kBlock) void emit_kernel(Grid G, Workspace ws, float *verts, int64_t n_verts,
                                                      int32_t *faces, int64_t n_faces)
{
    __shared__ int lds[kBlock / 64];
    const int64_t base = (int64_t)blockIdx.x * kTile;
    int64_t face_next = ws.block_f[blockIdx.x];
    for (int it = 0; it < kItems; ++it) {
        const int64_t p = base + it * kBlock + threadIdx.x;
        int c[3] = {0, 0, 0};
        float av[8];
        int8_t next[12];
        int crossed = 0, nf = 0;
        if (p < G.total) {
            point_coords(G, p, c);
            const float a = sample(G, p);
            float xs[3];
            const int mask = point_layout(G, c, p, a, xs);
            if (mask) {
                int64_t id = ws.block_v[blockIdx.x] + ws.local[p];
                for (int slot = 0; slot < 4; ++slot) {
                    if (!((mask >> slot) & 1)) continue;
                    if (id < n_verts) {
                        float *v = verts + 3 * id;
                        v[0] = (float)c[0];
                        v[1] = (float)c[1];
                        v[2] = (float)c[2];
                        if (slot > 0) v[slot - 1] = xs[slot - 1];
                    }
                    ++id;
                }
            }
            if (is_cell(G, c)) {
                cell_values(G, p, a, av);
                crossed = cell_loops(av, next);
                if (crossed) nf = cell_face_count(crossed, next);
            }
        }
        int sum;
        const int off = block_exclusive_scan(nf, lds, &sum);
        if (crossed) {
            int64_t fid = face_next + off;
            int seen = 0;
            for (int e = 0; e < 12; ++e) {
                if (!((crossed >> e) & 1) || ((seen >> e) & 1)) continue;
                const int64_t v0 = edge_vertex_id(G, ws, c, p, av, e);
                int e1 = next[e];
                seen |= (1 << e) | (1 << e1);
                int64_t v1 = edge_vertex_id(G, ws, c, p, av, e1);
                for (int k = 0; k < 10; ++k) {
                    const int e2 = next[e1];
                    if (e2 == e) break;
                    seen |= 1 << e2;
                    const int64_t v2 = edge_vertex_id(G, ws, c, p, av, e2);
                    if (fid < n_faces) {
                        int32_t *t = faces + 3 * fid;
                        t[0] = (int32_t)v0;
                        t[1] = (int32_t)v1;
                        t[2] = (int32_t)v2;
                    }
                    ++fid;
                    e1 = e2;
                    v1 = v2;
                }
            }
        }
        face_next += sum;
    }
}

bool make_grid(const float *volume, int64_t n0, int64_t n1, int64_t n2, float level, Grid *G)
{
    if (qf_marching_cubes_workspace_bytes(n0, n1, n2) < 0 || !volume || !std::isfinite(level)) return false;
    G->vol = volume;
    G->n[0] = (int)n0;
    G->n[1] = (int)n1;
    G->n[2] = (int)n2;
    G->stride[0] = n1 * n2;
    G->stride[1] = n2;
    G->stride[2] = 1;
    G->total = n0 * n1 * n2;
    G->level = level;
    return true;
}

}  // namespace

extern "C" int64_t qf_marching_cubes_workspace_bytes(int64_t n0, int64_t n1, int64_t n2)
{
    if (n0 < 2 || n1 < 2 || n2 < 2 || n0 > kMaxDim || n1 > kMaxDim || n2 > kMaxDim) return -1;
    const int64_t n01 = n0 * n1;                             // < 2^48
    if (n01 >= kMaxPoints || n01 * n2 >= kMaxPoints) return -1;
    return carve(nullptr, n01 * n2).bytes;
}

extern "C" int qf_marching_cubes_count(const float *volume, int64_t n0, int64_t n1, int64_t n2, float level,
                                       void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream)
{
    Grid G;
    if (!make_grid(volume, n0, n1, n2, level, &G) || !workspace || !counts ||
        workspace_bytes < qf_marching_cubes_workspace_bytes(n0, n1, n2))
        return QF_ERR_INVALID_ARGUMENT;
    const Workspace ws = carve(workspace, G.total);
    const int64_t nb = (G.total + kTile - 1) / kTile;
    hipStream_t s = qf_stream(stream);
    hipLaunchKernelGGL(count_kernel, dim3((unsigned)nb), dim3(kBlock), 0, s, G, ws);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_blocks_kernel, dim3(1), dim3(kScanThreads), 0, s, ws, nb, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_marching_cubes_emit(const float *volume, int64_t n0, int64_t n1, int64_t n2, float level,
                                      const void *workspace, int64_t workspace_bytes, float *verts, int64_t n_verts,
                                      int32_t *faces, int64_t n_faces, void *stream)
{
    Grid G;
    if (!make_grid(volume, n0, n1, n2, level, &G) || !workspace ||
        workspace_bytes < qf_marching_cubes_workspace_bytes(n0, n1, n2))
        return QF_ERR_INVALID_ARGUMENT;
    if (n_verts < 0 || n_verts >= kMaxPoints || n_faces < 0 || n_faces >= kMaxPoints || (n_verts > 0 && !verts) ||
        (n_faces > 0 && !faces))
        return QF_ERR_INVALID_ARGUMENT;
    if (n_verts == 0 && n_faces == 0) return QF_OK;
    const Workspace ws = carve(const_cast<void *>(workspace), G.total);
    const int64_t nb = (G.total + kTile - 1) / kTile;
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)nb), dim3(kBlock), 0, qf_stream(stream), G, ws, verts, n_verts,
                       faces, n_faces);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
