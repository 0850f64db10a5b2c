// Mesh clean-up on the device (include/qf_mesh_compact.h; the rules are DESIGN.md section 3.9b, restated in numpy in
// tests/mesh_compact_reference.py): faces selected by a keep mask, degenerate and duplicate faces dropped, small
// connected components dropped, unreferenced vertices removed and the faces remapped.  Integer work only.
//
// Passes of qf_mesh_compact_count (one stream, no host wait):
//   init      parent[v] = v, csize[v] = 0, used[v] = (vertices are all kept);
//   classify  per face: validity, mask, degenerate -> state[f]; the sorted index triple -> tri[3f..] (int32);
//   dup       an open-addressing hash table of face ids keyed by the sorted triple, at least 2 F slots, filled with
//             mesh_device.h's claim-or-lower insert; afterwards a face is a duplicate iff its slot holds another id.
//             The lowest index wins whatever the arrival order, and faces already dropped are never entered, so they
//             are nobody's "earlier copy".  (No library sort: rocPRIM's onesweep kernels use scratch and a look-back
//             spin.);
//   union     mesh_device.h's lock-free union-find over vertices: a tree's root is its smallest vertex whatever the
//             arrival order;
//   flatten   parent[v] = root(v);  size: one integer atomic per surviving face on csize[root];
//   island    faces of components below M dropped, the vertices of the final faces marked;
//   scans     output positions of faces and vertices: mesh_device.h's three-launch scan, once each;
//   finalize  counts[8].
// Every tally is an integer sum, so no result depends on the launch shape or the arrival order.
#include "mesh_device.h"
#include "qf_mesh_compact.h"

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr uint32_t kDropped = 0x7fffffffu;      // above every vertex index (V < 2^31, so an index is <= 2^31 - 2)
constexpr int kAllFlags = QF_MESH_REMOVE_DEGENERATE | QF_MESH_REMOVE_DUPLICATES | QF_MESH_REMOVE_UNREFERENCED;

enum : uint8_t { kAlive = 0, kByMask = 1, kDegenerate = 2, kDuplicate = 3, kIsland = 4, kInvalid = 5 };

struct Info {
    unsigned long long n_invalid, n_mask, n_degenerate, n_duplicate, n_island, n_components;
    int32_t face_total, vertex_total;
};

struct Workspace {
    Info *info;
    int32_t *parent;        // [V] union-find forest, then every vertex's root
    int32_t *csize;         // [V] surviving faces of the component whose root is v
    uint8_t *used;          // [V] 1: the vertex is kept
    int32_t *vpos;          // [V] exclusive scan of used
    uint8_t *state;         // [F] kAlive or why the face was dropped
    int32_t *tri;           // [3F] each face's indices sorted ascending
    int32_t *fpos;          // [F] exclusive scan of (state == kAlive)
    uint32_t *table;        // [slots] the lowest surviving face id of the sorted triple that claimed the slot
    uint32_t *slot;         // [F] the slot that holds the face's triple
    int64_t slots;          // a power of two >= max(2 F, 64)
    int32_t *vpart, *fpart; // per-workgroup sums of the two scans
    int64_t bytes;
};

Workspace carve(void *base, int64_t V, int64_t F)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.parent = c.take<int32_t>(V);
    w.csize = c.take<int32_t>(V);
    w.used = c.take<uint8_t>(V);
    w.vpos = c.take<int32_t>(V);
    w.state = c.take<uint8_t>(F);
    w.tri = c.take<int32_t>(3 * F);
    w.fpos = c.take<int32_t>(F);
    w.slots = table_slots(F);
    w.table = c.take<uint32_t>(w.slots);
    w.slot = c.take<uint32_t>(F);
    w.vpart = c.take<int32_t>(qf_div_up(V, kScanItems));
    w.fpart = c.take<int32_t>(qf_div_up(F, kScanItems));
    w.bytes = c.off;
    return w;
}

struct Job {
    const double *v;
    const int64_t *f;
    const uint8_t *keep;
    int64_t V, F;
    int32_t flags;
    int32_t M;
};

__global__ __launch_bounds__(kBlock) void init_kernel(int64_t V, Workspace ws, int all_used)
{
    const int64_t v = gtid();
    if (v >= V) return;
    ws.parent[v] = (int32_t)v;
    ws.csize[v] = 0;
    ws.used[v] = (uint8_t)all_used;
}

__global__ __launch_bounds__(kBlock) void classify_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int invalid = 0, by_mask = 0, degenerate = 0;
    if (f < J.F) {
        const int64_t a = J.f[3 * f], b = J.f[3 * f + 1], c = J.f[3 * f + 2];
        uint8_t st = kAlive;
        uint32_t lo = kDropped, mid = kDropped, hi = kDropped;
        if (a < 0 || a >= J.V || b < 0 || b >= J.V || c < 0 || c >= J.V) {
            st = kInvalid;
            invalid = 1;
        } else {
            const uint32_t x = (uint32_t)a, y = (uint32_t)b, z = (uint32_t)c;
            lo = min(x, min(y, z));
            hi = max(x, max(y, z));
            mid = (uint32_t)(((uint64_t)x + y + z) - lo - hi);
            if (J.keep && J.keep[f] == 0) {
                st = kByMask;
                by_mask = 1;
            } else if ((J.flags & QF_MESH_REMOVE_DEGENERATE) && (lo == mid || mid == hi)) {
                st = kDegenerate;
                degenerate = 1;
            }
        }
        ws.state[f] = st;
        ws.tri[3 * f] = (int32_t)lo;
        ws.tri[3 * f + 1] = (int32_t)mid;
        ws.tri[3 * f + 2] = (int32_t)hi;
    }
    tally(&ws.info->n_invalid, invalid);
    tally(&ws.info->n_mask, by_mask);
    tally(&ws.info->n_degenerate, degenerate);
}

__device__ __forceinline__ uint64_t triple_hash(uint32_t lo, uint32_t mid, uint32_t hi)
{
    uint64_t h = ((uint64_t)lo << 32 | mid) * 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
    h = (h + hi) * 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    h *= 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}

// A surviving face enters the table under its sorted triple (claim_or_lower of mesh_device.h).
__global__ __launch_bounds__(kBlock) void duplicate_insert_kernel(int64_t F, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= F || ws.info->n_invalid != 0 || ws.state[f] != kAlive) return;
    const int32_t lo = ws.tri[3 * f], mid = ws.tri[3 * f + 1], hi = ws.tri[3 * f + 2];
    const uint64_t hash = triple_hash((uint32_t)lo, (uint32_t)mid, (uint32_t)hi);
    ws.slot[f] = (uint32_t)claim_or_lower(ws.table, (uint64_t)ws.slots - 1, hash, (uint32_t)f, [&](uint32_t g) {
        const int32_t *t = ws.tri + 3 * (int64_t)g;
        return t[0] == lo && t[1] == mid && t[2] == hi;
    });
}

__global__ __launch_bounds__(kBlock) void duplicate_mark_kernel(int64_t F, Workspace ws)
{
    const int64_t f = gtid();
    int dup = 0;
    if (f < F && ws.info->n_invalid == 0 && ws.state[f] == kAlive && ws.table[ws.slot[f]] != (uint32_t)f) {
        ws.state[f] = kDuplicate;
        dup = 1;
    }
    tally(&ws.info->n_duplicate, dup);
}

__global__ __launch_bounds__(kBlock) void union_kernel(int64_t F, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= F || ws.info->n_invalid != 0 || ws.state[f] != kAlive) return;
    const int32_t a = ws.tri[3 * f], b = ws.tri[3 * f + 1], c = ws.tri[3 * f + 2];
    uf_union(ws.parent, a, b);
    uf_union(ws.parent, b, c);
}

__global__ __launch_bounds__(kBlock) void flatten_kernel(int64_t V, Workspace ws)
{
    const int64_t v = gtid();
    if (v >= V || ws.info->n_invalid != 0) return;
    __hip_atomic_store(ws.parent + v, uf_root(ws.parent, (int32_t)v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kBlock) void component_size_kernel(int64_t F, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= F || ws.info->n_invalid != 0 || ws.state[f] != kAlive) return;
    atomicAdd(ws.csize + ws.parent[ws.tri[3 * f]], 1);
}

__global__ __launch_bounds__(kBlock) void component_count_kernel(int64_t V, Workspace ws)
{
    const int64_t v = gtid();
    const int root = v < V && ws.info->n_invalid == 0 && ws.csize[v] > 0;
    tally(&ws.info->n_components, root);
}

__global__ __launch_bounds__(kBlock) void island_kernel(int64_t F, Workspace ws, int32_t M, int mark)
{
    const int64_t f = gtid();
    int island = 0;
    if (f < F && ws.info->n_invalid == 0 && ws.state[f] == kAlive) {
        const int32_t a = ws.tri[3 * f], b = ws.tri[3 * f + 1], c = ws.tri[3 * f + 2];
        if (M >= 2 && ws.csize[ws.parent[a]] < M) {
            ws.state[f] = kIsland;
            island = 1;
        } else if (mark) {
            ws.used[a] = 1;
            ws.used[b] = 1;
            ws.used[c] = 1;
        }
    }
    tally(&ws.info->n_island, island);
}

__global__ void finalize_kernel(Workspace ws, int64_t *counts)
{
    const Info &I = *ws.info;
    const bool ok = I.n_invalid == 0;
    counts[0] = ok ? I.face_total : 0;
    counts[1] = ok ? I.vertex_total : 0;
    counts[2] = ok ? (int64_t)I.n_mask : 0;
    counts[3] = ok ? (int64_t)I.n_degenerate : 0;
    counts[4] = ok ? (int64_t)I.n_duplicate : 0;
    counts[5] = ok ? (int64_t)I.n_island : 0;
    counts[6] = ok ? (int64_t)I.n_components : 0;
    counts[7] = (int64_t)I.n_invalid;
}

// ---- emit ----------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(kBlock) void face_emit_kernel(Job J, Workspace ws, int64_t *out, int64_t n_out,
                                                           int64_t *face_map)
{
    const int64_t f = gtid();
    if (f >= J.F || ws.info->n_invalid != 0 || ws.state[f] != kAlive) return;
    const int64_t o = ws.fpos[f];
    if (o >= n_out) return;
    const bool remap = J.flags & QF_MESH_REMOVE_UNREFERENCED;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t i = J.f[3 * f + k];
        out[3 * o + k] = remap ? (int64_t)ws.vpos[i] : i;
    }
    if (face_map) face_map[o] = f;
}

// the coordinates move as 64-bit words: the copy keeps every bit, NaN payloads included
__global__ __launch_bounds__(kBlock) void vertex_emit_kernel(Job J, Workspace ws, uint64_t *out, int64_t n_out,
                                                             int64_t *vertex_map)
{
    const int64_t v = gtid();
    if (v >= J.V || ws.info->n_invalid != 0 || !ws.used[v]) return;
    const int64_t o = ws.vpos[v];
    if (o >= n_out) return;
    const uint64_t *src = reinterpret_cast<const uint64_t *>(J.v) + 3 * v;
    out[3 * o] = src[0];
    out[3 * o + 1] = src[1];
    out[3 * o + 2] = src[2];
    if (vertex_map) vertex_map[o] = v;
}

__global__ __launch_bounds__(kBlock) void mark_hit_faces_kernel(const int32_t *__restrict__ hit_tri,
                                                                const int32_t *__restrict__ hit_count, int64_t n_slots,
                                                                int32_t max_hits, int64_t n_faces, uint8_t *mask,
                                                                unsigned long long *out_of_range)
{
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    int bad = 0;
    for (int64_t i = gtid(); i < n_slots; i += stride) {
        const int32_t id = hit_tri[i];
        bool considered;
        if (hit_count) {
            const int64_t r = i / max_hits;
            const int32_t k = (int32_t)(i - r * max_hits), c = hit_count[r];
            considered = k < (c < max_hits ? c : max_hits);
        } else {
            considered = id >= 0;
        }
        if (!considered) continue;
        if (id >= 0 && id < n_faces)
            mask[id] = 1;
        else
            ++bad;
    }
    if (out_of_range) tally(out_of_range, bad);
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && V < kMaxCount && F >= 0 && F < kMaxCount; }

bool make_job(const double *v, int64_t V, const int64_t *f, int64_t F, const uint8_t *keep, int32_t flags, int64_t M,
              Job *J)
{
    if (!sizes_ok(V, F) || !v || (F > 0 && !f) || (flags & ~kAllFlags) || M < 0 || M >= kMaxCount) return false;
    J->v = v;
    J->f = f;
    J->keep = keep;
    J->V = V;
    J->F = F;
    J->flags = flags;
    J->M = (int32_t)M;
    return true;
}

}  // namespace

extern "C" int64_t qf_mesh_compact_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!sizes_ok(n_vertices, n_faces)) return -1;
    return carve(nullptr, n_vertices, n_faces).bytes;
}

extern "C" int qf_mesh_compact_count(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                     const uint8_t *keep, int32_t flags, int64_t min_component_faces, void *workspace,
                                     int64_t workspace_bytes, int64_t *counts, void *stream)
{
    Job J;
    if (!make_job(vertices, n_vertices, faces, n_faces, keep, flags, min_component_faces, &J) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    Workspace ws = carve(workspace, J.V, J.F);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = J.V, F = J.F;
    const int unref = (flags & QF_MESH_REMOVE_UNREFERENCED) ? 1 : 0;

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_MESH_LAUNCH(init_kernel, V, V, ws, unref ? 0 : 1);
    if (F > 0) {
        QF_MESH_LAUNCH(classify_kernel, F, J, ws);
        if (flags & QF_MESH_REMOVE_DUPLICATES) {
            QF_HIP_TRY(hipMemsetAsync(ws.table, 0xff, 4 * (size_t)ws.slots, s));
            QF_MESH_LAUNCH(duplicate_insert_kernel, F, F, ws);
            QF_MESH_LAUNCH(duplicate_mark_kernel, F, F, ws);
        }
        QF_MESH_LAUNCH(union_kernel, F, F, ws);
        QF_MESH_LAUNCH(flatten_kernel, V, V, ws);
        QF_MESH_LAUNCH(component_size_kernel, F, F, ws);
        QF_MESH_LAUNCH(component_count_kernel, V, V, ws);
        QF_MESH_LAUNCH(island_kernel, F, F, ws, J.M, unref);
    }
    int st = scan_bytes(ws.state, F, ItemEquals{kAlive}, ws.fpart, ws.fpos, &ws.info->face_total, s);
    if (st != QF_OK) return st;
    st = scan_bytes(ws.used, V, ItemEquals{1}, ws.vpart, ws.vpos, &ws.info->vertex_total, s);
    if (st != QF_OK) return st;
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_compact_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                    const uint8_t *keep, int32_t flags, int64_t min_component_faces, void *workspace,
                                    int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                                    int64_t *out_faces, int64_t n_out_faces, int64_t *face_map, int64_t *vertex_map,
                                    void *stream)
{
    Job J;
    if (!make_job(vertices, n_vertices, faces, n_faces, keep, flags, min_component_faces, &J) || !workspace)
        return QF_ERR_INVALID_ARGUMENT;
    if (n_out_vertices < 0 || n_out_vertices > J.V || n_out_faces < 0 || n_out_faces > J.F ||
        (n_out_vertices > 0 && !out_vertices) || (n_out_faces > 0 && !out_faces))
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    Workspace ws = carve(workspace, J.V, J.F);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    if (n_out_vertices > 0) {
        QF_MESH_LAUNCH(vertex_emit_kernel, J.V, J, ws, reinterpret_cast<uint64_t *>(out_vertices), n_out_vertices,
                       vertex_map);
    }
    if (n_out_faces > 0) {
        QF_MESH_LAUNCH(face_emit_kernel, J.F, J, ws, out_faces, n_out_faces, face_map);
    }
    return QF_OK;
}

extern "C" int qf_mark_hit_faces(const int32_t *hit_tri, const int32_t *hit_count, int64_t n_rays, int32_t max_hits,
                                 int64_t n_faces, uint8_t *mask, int64_t *out_of_range, void *stream)
{
    if (n_rays < 0 || max_hits < 1 || n_faces < 0 || n_faces >= kMaxCount) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays >= (int64_t(1) << 40) / max_hits) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays == 0) return QF_OK;
    if (!hit_tri || (n_faces > 0 && !mask)) return QF_ERR_INVALID_ARGUMENT;
    const int64_t n_slots = n_rays * max_hits;
    QF_SIMPLE_LAUNCH(mark_hit_faces_kernel, n_slots, hit_tri, hit_count, n_slots, max_hits, n_faces, mask,
                     reinterpret_cast<unsigned long long *>(out_of_range));
    return QF_OK;
}
