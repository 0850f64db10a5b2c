// Making a mesh a manifold with boundary on the device (include/qf_mesh_manifold.h; the rule is DESIGN.md section 3.9e,
// restated in numpy in tests/mesh_manifold_reference.py): the mesh is cut along its edges with three or more faces and
// every vertex is split into one copy per fan.  Integer work only, and no floating-point operation at all: coordinates
// move as 64-bit words.
//
// Passes of qf_mesh_manifold_count (one stream, no host wait):
//   classify  per face: validity and degeneracy -> state[f]; parent[c] = c for its three corners;
//   uses      per half-edge of a proper face: an integer atomicAdd on uses[e], atomicMin / atomicMax of the half-edge id
//             into lo[e] / hi[e]; for uses == 2 these two are the pair;
//   link      per edge: the tallies of uses; for uses == 2 the two corner pairs with equal vertex indices are united in
//             mesh_device.h's lock-free union-find over the 3 F corners, so a class's root is its lowest corner whatever
//             the arrival order;
//   flatten   per face: parent[c] = root(c) for its corners, a root lowers vmin[vertex] to itself (integer atomicMin: the
//             lowest class of every vertex), and the faces with a complex edge are tallied;
//   extras    per corner: flag[c] = 1 iff c is the root of a class that is not vmin of its vertex; split[v] marks the
//             vertices that have one;
//   scan      output rank of every extra class: mesh_device.h's three-launch scan;
//   finalize  the split vertices tallied, then counts[8].
// Every tally is an integer sum (a wave sum and one atomic per wave), so no result depends on the launch shape or the
// arrival order.
#include "mesh_device.h"
#include "qf_mesh_manifold.h"

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;

enum : uint8_t { kProper = 0, kDegenerate = 1, kInvalid = 2 };

struct Info {
    unsigned long long n_invalid, n_degenerate, n_split, n_complex_edges, n_complex_faces, n_boundary, n_same_direction;
    int32_t extra_total;
};

// The arrays emit reads come first and do not depend on E: emit is not told E.
struct Workspace {
    Info *info;
    uint32_t *vmin;         // [V] the lowest root among the corners of the vertex; all ones (above every corner) if none
    uint8_t *state;         // [F] kProper, kDegenerate or kInvalid
    int32_t *parent;        // [3F] union-find forest over the corners, then every corner's root
    uint8_t *flag;          // [3F] 1: the corner is the root of an extra class
    int32_t *pos;           // [3F] exclusive scan of flag
    int32_t *part;          // per-workgroup sums of the scan
    int64_t emit_bytes;     // what emit needs
    uint8_t *split;         // [V] 1: the vertex has an extra class          } one block,
    int32_t *uses;          // [E] half-edges of proper faces on the edge     } cleared together
    uint32_t *hi;           // [E] the highest of them                        }
    uint32_t *lo;           // [E] the lowest of them
    int64_t zero_bytes;     // from split to the end of hi
    int64_t bytes;
};

Workspace carve(void *base, int64_t V, int64_t F, int64_t E)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.vmin = c.take<uint32_t>(V);
    w.state = c.take<uint8_t>(F);
    w.parent = c.take<int32_t>(3 * F);
    w.flag = c.take<uint8_t>(3 * F);
    w.pos = c.take<int32_t>(3 * F);
    w.part = c.take<int32_t>(qf_div_up(3 * F, kScanItems));
    w.emit_bytes = c.off;
    w.split = c.take<uint8_t>(V);
    w.uses = c.take<int32_t>(E);
    w.hi = c.take<uint32_t>(E);
    w.zero_bytes = c.off - w.emit_bytes;
    w.lo = c.take<uint32_t>(E);
    w.bytes = c.off;
    return w;
}

struct Job {
    const int64_t *f;
    const int64_t *fe;
    int64_t V, F, E;
};

__global__ __launch_bounds__(kBlock) void classify_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int invalid = 0, degenerate = 0;
    if (f < J.F) {
        const int64_t a = J.f[3 * f], b = J.f[3 * f + 1], c = J.f[3 * f + 2];
        uint8_t st = kProper;
        if (a < 0 || a >= J.V || b < 0 || b >= J.V || c < 0 || c >= J.V) {
            st = kInvalid;
        } else if (a == b || b == c || c == a) {
            st = kDegenerate;
        } else {
            const int64_t e0 = J.fe[3 * f], e1 = J.fe[3 * f + 1], e2 = J.fe[3 * f + 2];
            if (e0 < 0 || e0 >= J.E || e1 < 0 || e1 >= J.E || e2 < 0 || e2 >= J.E) st = kInvalid;
        }
        invalid = st == kInvalid;
        degenerate = st == kDegenerate;
        ws.state[f] = st;
        const int32_t c0 = (int32_t)(3 * f);
        ws.parent[c0] = c0;
        ws.parent[c0 + 1] = c0 + 1;
        ws.parent[c0 + 2] = c0 + 2;
    }
    tally(&ws.info->n_invalid, invalid);
    tally(&ws.info->n_degenerate, degenerate);
}

__global__ __launch_bounds__(kBlock) void uses_kernel(Job J, Workspace ws)
{
    const int64_t h = gtid();
    if (h >= 3 * J.F || ws.info->n_invalid != 0 || ws.state[h / 3] != kProper) return;
    const int64_t e = J.fe[h];
    atomicAdd(ws.uses + e, 1);
    atomicMin(ws.lo + e, (uint32_t)h);
    atomicMax(ws.hi + e, (uint32_t)h);
}

__global__ __launch_bounds__(kBlock) void link_kernel(Job J, Workspace ws)
{
    const int64_t e = gtid();
    int boundary = 0, complex_edge = 0, same_direction = 0;
    if (e < J.E && ws.info->n_invalid == 0) {
        const int32_t u = ws.uses[e];
        boundary = u == 1;
        complex_edge = u > 2;
        if (u == 2) {
            const int32_t h0 = (int32_t)ws.lo[e], h1 = (int32_t)ws.hi[e];
            const int32_t f0 = h0 / 3, f1 = h1 / 3;
            const int32_t k0 = h0 - 3 * f0, k1 = h1 - 3 * f1;
            const int32_t a0 = h0, a1 = 3 * f0 + (k0 == 2 ? 0 : k0 + 1);
            const int32_t b0 = h1, b1 = 3 * f1 + (k1 == 2 ? 0 : k1 + 1);
            const int64_t va0 = J.f[a0], va1 = J.f[a1], vb0 = J.f[b0], vb1 = J.f[b1];
            if (va0 == vb0 && va1 == vb1) {             // the two half-edges run the same way
                same_direction = 1;
                uf_union(ws.parent, a0, b0);
                uf_union(ws.parent, a1, b1);
            } else if (va0 == vb1 && va1 == vb0) {
                uf_union(ws.parent, a0, b1);
                uf_union(ws.parent, a1, b0);
            }                                           // else face_edges is not these faces': nothing is linked
        }
    }
    tally(&ws.info->n_boundary, boundary);
    tally(&ws.info->n_complex_edges, complex_edge);
    tally(&ws.info->n_same_direction, same_direction);
}

__global__ __launch_bounds__(kBlock) void flatten_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int complex_face = 0;
    if (f < J.F && ws.info->n_invalid == 0 && ws.state[f] == kProper) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const int32_t c = (int32_t)(3 * f + k);
            const int32_t x = uf_root(ws.parent, c);
            __hip_atomic_store(ws.parent + c, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (x == c) atomicMin(ws.vmin + J.f[c], (uint32_t)c);
            complex_face |= ws.uses[J.fe[c]] > 2;
        }
    }
    tally(&ws.info->n_complex_faces, complex_face);
}

__global__ __launch_bounds__(kBlock) void extras_kernel(Job J, Workspace ws)
{
    const int64_t c = gtid();
    if (c >= 3 * J.F) return;
    uint8_t extra = 0;
    if (ws.info->n_invalid == 0 && ws.state[c / 3] == kProper && ws.parent[c] == (int32_t)c) {
        const int64_t v = J.f[c];
        if (ws.vmin[v] != (uint32_t)c) {
            extra = 1;
            ws.split[v] = 1;
        }
    }
    ws.flag[c] = extra;
}

__global__ __launch_bounds__(kBlock) void split_count_kernel(int64_t V, Workspace ws)
{
    const int64_t v = gtid();
    tally(&ws.info->n_split, v < V && ws.split[v] != 0);
}

__global__ void finalize_kernel(int64_t V, Workspace ws, int64_t *counts)
{
    const Info &I = *ws.info;
    const bool ok = I.n_invalid == 0;
    counts[0] = ok ? V + I.extra_total : 0;
    counts[1] = ok ? (int64_t)I.n_split : 0;
    counts[2] = ok ? (int64_t)I.n_complex_edges : 0;
    counts[3] = ok ? (int64_t)I.n_complex_faces : 0;
    counts[4] = ok ? (int64_t)I.n_boundary : 0;
    counts[5] = ok ? (int64_t)I.n_same_direction : 0;
    counts[6] = ok ? (int64_t)I.n_degenerate : 0;
    counts[7] = (int64_t)I.n_invalid;
}

// ---- emit ----------------------------------------------------------------------------------------------------------

// the coordinates move as 64-bit words: the copy keeps every bit, NaN payloads included
__device__ __forceinline__ void copy_row(const uint64_t *__restrict__ src, int64_t v, uint64_t *__restrict__ out, int64_t o)
{
    out[3 * o] = src[3 * v];
    out[3 * o + 1] = src[3 * v + 1];
    out[3 * o + 2] = src[3 * v + 2];
}

__global__ __launch_bounds__(kBlock) void vertex_emit_kernel(const uint64_t *__restrict__ src, int64_t V, Workspace ws,
                                                             uint64_t *__restrict__ out, int64_t n_out, int64_t *vertex_map)
{
    const int64_t v = gtid();
    if (v >= V || v >= n_out || ws.info->n_invalid != 0) return;
    copy_row(src, v, out, v);
    if (vertex_map) vertex_map[v] = v;
}

// one thread per corner: the face entry, and the row of the extra class the corner is the root of
__global__ __launch_bounds__(kBlock) void corner_emit_kernel(const uint64_t *__restrict__ src, const int64_t *__restrict__ faces,
                                                             int64_t V, int64_t F, Workspace ws, uint64_t *__restrict__ out,
                                                             int64_t n_out, int64_t *__restrict__ out_faces,
                                                             int64_t *vertex_map)
{
    const int64_t c = gtid();
    if (c >= 3 * F || ws.info->n_invalid != 0) return;
    const int64_t v = faces[c];
    int64_t index = v;
    if (ws.state[c / 3] == kProper) {
        const int32_t root = ws.parent[c];
        if (ws.vmin[v] != (uint32_t)root) index = V + ws.pos[root];
        if (ws.flag[c]) {
            const int64_t o = V + ws.pos[c];
            if (o < n_out) {
                copy_row(src, v, out, o);
                if (vertex_map) vertex_map[o] = v;
            }
        }
    }
    out_faces[c] = index;
}

bool sizes_ok(int64_t V, int64_t F, int64_t E)
{
    return V >= 1 && V < kMaxCount && F >= 0 && F < kMaxCount && 3 * F < kMaxCount && E >= 0 && E < kMaxCount;
}

}  // namespace

extern "C" int64_t qf_mesh_manifold_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges)) return -1;
    return carve(nullptr, n_vertices, n_faces, n_edges).bytes;
}

extern "C" int qf_mesh_manifold_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *face_edges,
                                      int64_t n_edges, void *workspace, int64_t workspace_bytes, int64_t *counts,
                                      void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, n_edges) || (n_faces > 0 && (!faces || !face_edges)) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = n_vertices, F = n_faces, E = n_edges;
    Workspace ws = carve(workspace, V, F, E);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const Job J{faces, face_edges, V, F, E};

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ws.vmin, 0xff, 4 * (size_t)V, s));
    QF_HIP_TRY(hipMemsetAsync(ws.split, 0, (size_t)ws.zero_bytes, s));
    if (E > 0) QF_HIP_TRY(hipMemsetAsync(ws.lo, 0xff, 4 * (size_t)E, s));
    if (F > 0) {
        QF_MESH_LAUNCH(classify_kernel, F, J, ws);
        QF_MESH_LAUNCH(uses_kernel, 3 * F, J, ws);
        QF_MESH_LAUNCH(link_kernel, E, J, ws);
        QF_MESH_LAUNCH(flatten_kernel, F, J, ws);
        QF_MESH_LAUNCH(extras_kernel, 3 * F, J, ws);
        const int st = scan_bytes(ws.flag, 3 * F, ItemNonZero{}, ws.part, ws.pos, &ws.info->extra_total, s);
        if (st != QF_OK) return st;
        QF_MESH_LAUNCH(split_count_kernel, V, V, ws);
    }
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, V, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_manifold_emit(const double *vertices, const int64_t *faces, int64_t n_faces, int64_t n_vertices,
                                     void *workspace, int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                                     int64_t *out_faces, int64_t *vertex_map, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces, 0) || !vertices || (n_faces > 0 && (!faces || !out_faces)) || !workspace)
        return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = n_vertices, F = n_faces;
    if (n_out_vertices < 0 || n_out_vertices > V + 3 * F || (n_out_vertices > 0 && !out_vertices))
        return QF_ERR_INVALID_ARGUMENT;
    Workspace ws = carve(workspace, V, F, 0);
    if (workspace_bytes < ws.emit_bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const uint64_t *src = reinterpret_cast<const uint64_t *>(vertices);
    uint64_t *out = reinterpret_cast<uint64_t *>(out_vertices);
    if (n_out_vertices > 0) {
        QF_MESH_LAUNCH(vertex_emit_kernel, V, src, V, ws, out, n_out_vertices, vertex_map);
    }
    QF_MESH_LAUNCH(corner_emit_kernel, 3 * F, src, faces, V, F, ws, out, n_out_vertices, out_faces, vertex_map);
    return QF_OK;
}
