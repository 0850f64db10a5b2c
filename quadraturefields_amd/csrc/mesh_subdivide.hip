// Mesh refinement on the device (include/qf_mesh_subdivide.h; the rules are DESIGN.md section 3.9c, restated in numpy in
// tests/mesh_subdivide_reference.py): the undirected edges of a mesh numbered by first appearance (stage A) and a
// conforming midpoint split of the faces along any marked subset of them (stage B).  Integer work only; the one piece of
// arithmetic is the fp64 midpoint.
//
// Passes of qf_mesh_edges_count (one stream, no host wait):
//   classify  per face: validity, degenerate -> state[f];
//   insert    an open-addressing hash table of half-edge ids keyed by the pair (min, max), at least 6 F slots, filled
//             with mesh_device.h's claim-or-lower insert; a half-edge also adds one to its slot's use count;
//   flag      first[h] = the slot of h holds h: the lowest half-edge of every pair, whatever the arrival order; the
//             boundary edges are those whose use count is one;
//   scan      exclusive scan of first[] over the half-edges, mesh_device.h's three launches: the edge ids;
//   finalize  counts[4].
// qf_mesh_subdivide_count: classify (validity, marked edges per face -> children per face; the lowest half-edge of every
// marked edge with an integer atomicMin, which is the one thread that writes the new vertex), the scans of the children and
// of the marks, finalize.  Every tally is an integer sum, so no result depends on the launch shape or the arrival order.
#include "mesh_device.h"
#include "qf_mesh_subdivide.h"

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr int64_t kMaxEdgeFaces = (kMaxCount - 1) / 3;      // 3 F < 2^31: a half-edge id fits 31 bits
constexpr int64_t kMaxSplitFaces = int64_t(1) << 29;        // 4 F < 2^31

enum : uint8_t { kValid = 0, kDegenerate = 1, kInvalid = 2 };

// validity and degeneracy of face f; the three indices as 32-bit values when valid
__device__ __forceinline__ uint8_t load_face(const int64_t *faces, int64_t f, int64_t V, int32_t v[3])
{
    const int64_t a = faces[3 * f], b = faces[3 * f + 1], c = faces[3 * f + 2];
    if (a < 0 || a >= V || b < 0 || b >= V || c < 0 || c >= V) return kInvalid;
    v[0] = (int32_t)a;
    v[1] = (int32_t)b;
    v[2] = (int32_t)c;
    return (a == b || b == c || a == c) ? kDegenerate : kValid;
}

// =================================================================================================== stage A: the edges

struct EdgeInfo {
    unsigned long long n_invalid, n_degenerate, n_boundary;
    int32_t edge_total;
};

struct EdgeWorkspace {
    EdgeInfo *info;
    uint8_t *state;         // [F] kValid, kDegenerate or kInvalid
    uint32_t *table;        // [slots] the lowest half-edge of the pair that claimed the slot
    uint32_t *uses;         // [slots] the half-edges of that pair
    uint32_t *slot;         // [3F] the slot that holds the half-edge's pair
    uint8_t *first;         // [3F] 1: the half-edge is the lowest of its pair
    int32_t *pos;           // [3F] exclusive scan of first
    int32_t *part;          // per-workgroup sums of the scan
    int64_t slots;          // a power of two >= max(6 F, 64)
    int64_t bytes;
};

EdgeWorkspace carve_edges(void *base, int64_t F)
{
    EdgeWorkspace w;
    const int64_t H = 3 * F;
    QfCarver c{base};
    w.info = c.take<EdgeInfo>(1);
    w.state = c.take<uint8_t>(F);
    w.slots = table_slots(H);
    w.table = c.take<uint32_t>(w.slots);
    w.uses = c.take<uint32_t>(w.slots);
    w.slot = c.take<uint32_t>(H);
    w.first = c.take<uint8_t>(H);
    w.pos = c.take<int32_t>(H);
    w.part = c.take<int32_t>(qf_div_up(H, kScanItems));
    w.bytes = c.off;
    return w;
}

__device__ __forceinline__ uint64_t pair_key(const int64_t *faces, uint32_t h)
{
    const uint32_t f = h / 3, k = h - 3 * f;
    const uint32_t a = (uint32_t)faces[3 * (int64_t)f + k], b = (uint32_t)faces[3 * (int64_t)f + (k == 2 ? 0 : k + 1)];
    return a < b ? ((uint64_t)a << 32 | b) : ((uint64_t)b << 32 | a);
}

__device__ __forceinline__ uint64_t pair_hash(uint64_t key)
{
    uint64_t h = key * 0x9e3779b97f4a7c15ull;
    h ^= h >> 32;
    h *= 0xbf58476d1ce4e5b9ull;
    return h ^ (h >> 29);
}

__global__ __launch_bounds__(kBlock) void edge_classify_kernel(const int64_t *faces, int64_t F, int64_t V, EdgeWorkspace ws)
{
    const int64_t f = gtid();
    int invalid = 0, degenerate = 0;
    if (f < F) {
        int32_t v[3];
        const uint8_t st = load_face(faces, f, V, v);
        ws.state[f] = st;
        invalid = st == kInvalid;
        degenerate = st == kDegenerate;
    }
    tally(&ws.info->n_invalid, invalid);
    tally(&ws.info->n_degenerate, degenerate);
}

// A half-edge of a valid face enters the table under its pair (claim_or_lower of mesh_device.h: at most 3 F of the
// >= 6 F slots are ever claimed).
__global__ __launch_bounds__(kBlock) void edge_insert_kernel(const int64_t *faces, int64_t H, EdgeWorkspace ws)
{
    const int64_t h = gtid();
    if (h >= H || ws.info->n_invalid != 0 || ws.state[h / 3] != kValid) return;
    const uint64_t key = pair_key(faces, (uint32_t)h);
    const uint64_t s = claim_or_lower(ws.table, (uint64_t)ws.slots - 1, pair_hash(key), (uint32_t)h,
                                      [&](uint32_t g) { return pair_key(faces, g) == key; });
    atomicAdd(ws.uses + s, 1u);
    ws.slot[h] = (uint32_t)s;
}

__global__ __launch_bounds__(kBlock) void edge_flag_kernel(int64_t H, EdgeWorkspace ws)
{
    const int64_t h = gtid();
    int boundary = 0;
    if (h < H) {
        uint8_t first = 0;
        if (ws.info->n_invalid == 0 && ws.state[h / 3] == kValid) {
            const uint32_t s = ws.slot[h];
            first = ws.table[s] == (uint32_t)h;
            boundary = first && ws.uses[s] == 1u;
        }
        ws.first[h] = first;
    }
    tally(&ws.info->n_boundary, boundary);
}

__global__ void edge_finalize_kernel(EdgeWorkspace ws, int64_t *counts)
{
    const EdgeInfo &I = *ws.info;
    const bool ok = I.n_invalid == 0;
    counts[0] = ok ? I.edge_total : 0;
    counts[1] = ok ? (int64_t)I.n_degenerate : 0;
    counts[2] = (int64_t)I.n_invalid;
    counts[3] = ok ? (int64_t)I.n_boundary : 0;
}

__global__ __launch_bounds__(kBlock) void edge_emit_kernel(const int64_t *faces, int64_t H, EdgeWorkspace ws, int64_t *edges,
                                                           int64_t n_edges, int64_t *face_edges)
{
    const int64_t h = gtid();
    if (h >= H || ws.info->n_invalid != 0) return;
    if (ws.state[h / 3] != kValid) {
        face_edges[h] = -1;
        return;
    }
    const int64_t e = ws.pos[ws.table[ws.slot[h]]];
    face_edges[h] = e;
    if (ws.first[h] && e < n_edges) {
        const uint64_t key = pair_key(faces, (uint32_t)h);
        edges[2 * e] = (int64_t)(key >> 32);
        edges[2 * e + 1] = (int64_t)(key & 0xffffffffu);
    }
}

bool edge_sizes_ok(int64_t V, int64_t F) { return V >= 1 && V < kMaxCount && F >= 0 && F <= kMaxEdgeFaces; }

// ==================================================================================================== stage B: the split

struct SplitInfo {
    unsigned long long n_invalid;
    unsigned long long n_one_two;       // faces with one marked edge in the low word, with two in the high word
    unsigned long long n_three;
    int32_t face_total, mark_total;
};

struct SplitWorkspace {
    SplitInfo *info;
    uint8_t *children;      // [F] output faces of face f: 1 + its marked edges (1 for a degenerate face, 0 when invalid)
    int32_t *fpos;          // [F] exclusive scan of children
    int32_t *epos;          // [E] exclusive scan of (edge_mark != 0)
    int32_t *owner;         // [E] the lowest half-edge on a marked edge: the one that writes its vertex
    int32_t *fpart, *epart; // per-workgroup sums of the two scans
    int64_t bytes;
};

SplitWorkspace carve_split(void *base, int64_t F, int64_t E)
{
    SplitWorkspace w;
    QfCarver c{base};
    w.info = c.take<SplitInfo>(1);
    w.children = c.take<uint8_t>(F);
    w.fpos = c.take<int32_t>(F);
    w.epos = c.take<int32_t>(E);
    w.owner = c.take<int32_t>(E);
    w.fpart = c.take<int32_t>(qf_div_up(F, kScanItems));
    w.epart = c.take<int32_t>(qf_div_up(E, kScanItems));
    w.bytes = c.off;
    return w;
}

struct SplitJob {
    const int64_t *f, *fe;
    const uint8_t *mark;
    int64_t V, F, E;
};

// state of face f, its indices, its edge ids and which of them are marked (bit k); a degenerate face has no marks
__device__ __forceinline__ uint8_t load_split_face(const SplitJob &J, int64_t f, int32_t v[3], int32_t e[3], int *marks)
{
    *marks = 0;
    const uint8_t st = load_face(J.f, f, J.V, v);
    if (st != kValid) return st;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t id = J.fe[3 * f + k];
        if (id < 0 || id >= J.E) {
            *marks = 0;
            return kInvalid;
        }
        e[k] = (int32_t)id;
        if (J.mark[id]) *marks |= 1 << k;
    }
    return kValid;
}

// The faces with 1, 2 and 3 marked edges are tallied per workgroup and added with at most two atomics per workgroup (the
// counts of 1 and 2 share a 64-bit word, each below 2^31): one atomic per wave and counter, all on one cache line, took
// longer than the rest of the pass at a 10 % mark.  The faces with none are the rest.
__global__ __launch_bounds__(kBlock) void split_classify_kernel(SplitJob J, SplitWorkspace ws)
{
    __shared__ int s_tally[kBlock / 64][4];
    const int64_t f = gtid();
    int invalid = 0, n = -1;
    if (f < J.F) {
        int32_t v[3], e[3];
        int marks;
        const uint8_t st = load_split_face(J, f, v, e, &marks);
        invalid = st == kInvalid;
        n = invalid ? -1 : __popc(marks);
        ws.children[f] = invalid ? 0 : (uint8_t)(1 + n);
#pragma unroll
        for (int k = 0; k < 3; ++k)
            if (marks >> k & 1) atomicMin(ws.owner + e[k], (int32_t)(3 * f + k));
    }
    int t[4] = {invalid, n == 1, n == 2, n == 3};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) t[c] += __shfl_xor(t[c], off, 64);
        if ((threadIdx.x & 63) == 0) s_tally[threadIdx.x >> 6][c] = t[c];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long sum[4];
        for (int c = 0; c < 4; ++c) {
            sum[c] = 0;
            for (int w = 0; w < kBlock / 64; ++w) sum[c] += (unsigned long long)s_tally[w][c];
        }
        if (sum[0]) atomicAdd(&ws.info->n_invalid, sum[0]);
        if (sum[1] | sum[2]) atomicAdd(&ws.info->n_one_two, sum[1] | sum[2] << 32);
        if (sum[3]) atomicAdd(&ws.info->n_three, sum[3]);
    }
}

__global__ void split_finalize_kernel(SplitWorkspace ws, int64_t V, int64_t F, int64_t *counts)
{
    const SplitInfo &I = *ws.info;
    const bool ok = I.n_invalid == 0;
    const int64_t one = (int64_t)(I.n_one_two & 0xffffffffu), two = (int64_t)(I.n_one_two >> 32), three = (int64_t)I.n_three;
    counts[0] = ok ? I.face_total : 0;
    counts[1] = ok ? V + I.mark_total : 0;
    counts[2] = ok ? F - one - two - three : 0;
    counts[3] = ok ? one : 0;
    counts[4] = ok ? two : 0;
    counts[5] = ok ? three : 0;
    counts[6] = (int64_t)I.n_invalid;
}

// the coordinates move as 64-bit words: the copy keeps every bit, NaN payloads included
__global__ __launch_bounds__(kBlock) void split_copy_vertices_kernel(const uint64_t *src, int64_t V, SplitWorkspace ws,
                                                                     uint64_t *out, int64_t n_out, int64_t *parents)
{
    const int64_t v = gtid();
    if (v >= V || v >= n_out || ws.info->n_invalid != 0) return;
    out[3 * v] = src[3 * v];
    out[3 * v + 1] = src[3 * v + 1];
    out[3 * v + 2] = src[3 * v + 2];
    if (parents) {
        parents[2 * v] = v;
        parents[2 * v + 1] = v;
    }
}

__device__ __forceinline__ void put_face(int64_t *out, int64_t n_out, int64_t *face_map, int64_t o, int64_t parent,
                                         int64_t a, int64_t b, int64_t c)
{
    if (o < 0 || o >= n_out) return;
    out[3 * o] = a;
    out[3 * o + 1] = b;
    out[3 * o + 2] = c;
    if (face_map) face_map[o] = parent;
}

__global__ __launch_bounds__(kBlock) void split_emit_kernel(SplitJob J, SplitWorkspace ws, const double *vertices,
                                                            double *out_v, int64_t n_out_v, int64_t *parents,
                                                            int64_t *out_f, int64_t n_out_f, int64_t *face_map)
{
    const int64_t f = gtid();
    if (f >= J.F || ws.info->n_invalid != 0) return;
    const int64_t o = ws.fpos[f];
    int32_t v[3], e[3];
    int marks;
    const uint8_t st = load_split_face(J, f, v, e, &marks);
    if (st == kInvalid) return;
    if (st == kDegenerate) {
        put_face(out_f, n_out_f, face_map, o, f, v[0], v[1], v[2]);
        return;
    }
    int64_t m[3] = {0, 0, 0};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!(marks >> k & 1)) continue;
        m[k] = J.V + ws.epos[e[k]];
        if (ws.owner[e[k]] != (int32_t)(3 * f + k) || m[k] < J.V || m[k] >= n_out_v) continue;
        const int32_t a = v[k], b = v[k == 2 ? 0 : k + 1];
        const int64_t lo = a < b ? a : b, hi = a < b ? b : a;
#pragma unroll
        for (int c = 0; c < 3; ++c) out_v[3 * m[k] + c] = 0.5 * (vertices[3 * lo + c] + vertices[3 * hi + c]);
        if (parents) {
            parents[2 * m[k]] = lo;
            parents[2 * m[k] + 1] = hi;
        }
    }
    switch (marks) {
    case 0:
        put_face(out_f, n_out_f, face_map, o, f, v[0], v[1], v[2]);
        break;
    case 1: case 2: case 4: {
        const int k = marks == 1 ? 0 : marks == 2 ? 1 : 2;
        const int64_t u0 = v[k], u1 = v[(k + 1) % 3], u2 = v[(k + 2) % 3], mid = m[k];
        put_face(out_f, n_out_f, face_map, o, f, u0, mid, u2);
        put_face(out_f, n_out_f, face_map, o + 1, f, mid, u1, u2);
        break;
    }
    case 7:
        put_face(out_f, n_out_f, face_map, o, f, v[0], m[0], m[2]);
        put_face(out_f, n_out_f, face_map, o + 1, f, m[0], v[1], m[1]);
        put_face(out_f, n_out_f, face_map, o + 2, f, m[2], m[1], v[2]);
        put_face(out_f, n_out_f, face_map, o + 3, f, m[0], m[1], m[2]);
        break;
    default: {                                  // two marked: edge j is not
        const int j = marks == 6 ? 0 : marks == 5 ? 1 : 2;
        const int64_t u0 = v[(j + 1) % 3], u1 = v[(j + 2) % 3], u2 = v[j];
        const int64_t a = m[(j + 1) % 3], b = m[(j + 2) % 3];
        put_face(out_f, n_out_f, face_map, o, f, a, u1, b);
        if (u0 < u2) {
            put_face(out_f, n_out_f, face_map, o + 1, f, u0, a, b);
            put_face(out_f, n_out_f, face_map, o + 2, f, u0, b, u2);
        } else {
            put_face(out_f, n_out_f, face_map, o + 1, f, u0, a, u2);
            put_face(out_f, n_out_f, face_map, o + 2, f, a, b, u2);
        }
        break;
    }
    }
}

bool split_sizes_ok(int64_t V, int64_t F, int64_t E)
{
    return V >= 1 && V < kMaxCount && F >= 0 && F < kMaxSplitFaces && E >= 0 && E <= 3 * F && V + E < kMaxCount;
}

bool make_split_job(const int64_t *f, int64_t F, int64_t V, const int64_t *fe, int64_t E, const uint8_t *mark, SplitJob *J)
{
    if (!split_sizes_ok(V, F, E) || (F > 0 && (!f || !fe)) || (E > 0 && !mark)) return false;
    J->f = f;
    J->fe = fe;
    J->mark = mark;
    J->V = V;
    J->F = F;
    J->E = E;
    return true;
}

}  // namespace

extern "C" int64_t qf_mesh_edges_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!edge_sizes_ok(n_vertices, n_faces)) return -1;
    return carve_edges(nullptr, n_faces).bytes;
}

extern "C" int qf_mesh_edges_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, void *workspace,
                                   int64_t workspace_bytes, int64_t *counts, void *stream)
{
    if (!edge_sizes_ok(n_vertices, n_faces) || (n_faces > 0 && !faces) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    EdgeWorkspace ws = carve_edges(workspace, n_faces);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const int64_t F = n_faces, H = 3 * n_faces;

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(EdgeInfo), s));
    if (F > 0) {
        QF_HIP_TRY(hipMemsetAsync(ws.table, 0xff, 4 * (size_t)ws.slots, s));
        QF_HIP_TRY(hipMemsetAsync(ws.uses, 0, 4 * (size_t)ws.slots, s));
        QF_MESH_LAUNCH(edge_classify_kernel, F, faces, F, n_vertices, ws);
        QF_MESH_LAUNCH(edge_insert_kernel, H, faces, H, ws);
        QF_MESH_LAUNCH(edge_flag_kernel, H, H, ws);
    }
    const int st = scan_bytes(ws.first, H, ItemNonZero{}, ws.part, ws.pos, &ws.info->edge_total, s);
    if (st != QF_OK) return st;
    hipLaunchKernelGGL(edge_finalize_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_edges_emit(const int64_t *faces, int64_t n_faces, int64_t n_vertices, void *workspace,
                                  int64_t workspace_bytes, int64_t *edges, int64_t n_edges, int64_t *face_edges,
                                  void *stream)
{
    if (!edge_sizes_ok(n_vertices, n_faces) || (n_faces > 0 && (!faces || !face_edges)) || !workspace)
        return QF_ERR_INVALID_ARGUMENT;
    if (n_edges < 0 || n_edges > 3 * n_faces || (n_edges > 0 && !edges)) return QF_ERR_INVALID_ARGUMENT;
    EdgeWorkspace ws = carve_edges(workspace, n_faces);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    const int64_t H = 3 * n_faces;
    QF_MESH_LAUNCH(edge_emit_kernel, H, faces, H, ws, edges, n_edges, face_edges);
    return QF_OK;
}

extern "C" int64_t qf_mesh_subdivide_workspace_bytes(int64_t n_vertices, int64_t n_faces, int64_t n_edges)
{
    if (!split_sizes_ok(n_vertices, n_faces, n_edges)) return -1;
    return carve_split(nullptr, n_faces, n_edges).bytes;
}

extern "C" int qf_mesh_subdivide_count(const int64_t *faces, int64_t n_faces, int64_t n_vertices, const int64_t *face_edges,
                                       int64_t n_edges, const uint8_t *edge_mark, void *workspace, int64_t workspace_bytes,
                                       int64_t *counts, void *stream)
{
    SplitJob J;
    if (!make_split_job(faces, n_faces, n_vertices, face_edges, n_edges, edge_mark, &J) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    SplitWorkspace ws = carve_split(workspace, J.F, J.E);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(SplitInfo), s));
    if (J.E > 0) QF_HIP_TRY(hipMemsetAsync(ws.owner, 0x7f, 4 * (size_t)J.E, s));    // 0x7f7f7f7f: above every half-edge id
    QF_MESH_LAUNCH(split_classify_kernel, J.F, J, ws);
    int st = scan_bytes(ws.children, J.F, ItemValue{}, ws.fpart, ws.fpos, &ws.info->face_total, s);
    if (st != QF_OK) return st;
    st = scan_bytes(edge_mark, J.E, ItemNonZero{}, ws.epart, ws.epos, &ws.info->mark_total, s);
    if (st != QF_OK) return st;
    hipLaunchKernelGGL(split_finalize_kernel, dim3(1), dim3(1), 0, s, ws, J.V, J.F, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_subdivide_emit(const double *vertices, const int64_t *faces, int64_t n_faces, int64_t n_vertices,
                                      const int64_t *face_edges, int64_t n_edges, const uint8_t *edge_mark, void *workspace,
                                      int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                                      int64_t *out_faces, int64_t n_out_faces, int64_t *face_map, int64_t *vertex_parents,
                                      void *stream)
{
    SplitJob J;
    if (!make_split_job(faces, n_faces, n_vertices, face_edges, n_edges, edge_mark, &J) || !workspace || !vertices)
        return QF_ERR_INVALID_ARGUMENT;
    if (n_out_vertices < 0 || n_out_vertices > J.V + J.E || n_out_faces < 0 || n_out_faces > 4 * J.F ||
        (n_out_vertices > 0 && !out_vertices) || (n_out_faces > 0 && !out_faces))
        return QF_ERR_INVALID_ARGUMENT;
    SplitWorkspace ws = carve_split(workspace, J.F, J.E);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    if (n_out_vertices > 0) {
        QF_MESH_LAUNCH(split_copy_vertices_kernel, J.V, reinterpret_cast<const uint64_t *>(vertices), J.V, ws,
                       reinterpret_cast<uint64_t *>(out_vertices), n_out_vertices, vertex_parents);
    }
    if (J.F > 0 && (n_out_faces > 0 || n_out_vertices > J.V)) {
        QF_MESH_LAUNCH(split_emit_kernel, J.F, J, ws, vertices, out_vertices, n_out_vertices, vertex_parents, out_faces,
                       n_out_faces, face_map);
    }
    return QF_OK;
}
