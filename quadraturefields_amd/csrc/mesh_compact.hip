// Mesh clean-up on the device (include/qf_mesh_compact.h; the rules are DESIGN.md section 3.9b, restated in numpy in
// tests/mesh_compact_reference.py): faces selected by a keep mask, degenerate and duplicate faces dropped, small
// connected components dropped, unreferenced vertices removed and the faces remapped.  Integer work only.
//
// Passes of qf_mesh_compact_count (one stream, no host wait):
//   init      parent[v] = v, csize[v] = 0, used[v] = (vertices are all kept);
//   classify  per face: validity, mask, degenerate -> state[f]; the sorted index triple -> tri[3f..] (int32);
//   dup       an open-addressing hash table of face ids keyed by the sorted triple, at least 2 F slots: a surviving
//             face claims the first empty slot of its probe sequence with compare-and-swap, or lowers the id of the slot
//             that already holds its triple with an integer atomicMin; afterwards a face is a duplicate iff its slot
//             holds another id.  The lowest index wins whatever the arrival order, and faces already dropped are never
//             entered, so they are nobody's "earlier copy".  (No library sort: rocPRIM's onesweep kernels use scratch
//             and a look-back spin.);
//   union     lock-free union-find over vertices: the larger root is hooked under the smaller with compare-and-swap, so
//             a tree's root is its smallest vertex whatever the arrival order; a failed swap continues from the value
//             it read (another thread made progress), nothing waits;
//   flatten   parent[v] = root(v);  size: one integer atomic per surviving face on csize[root];
//   island    faces of components below M dropped, the vertices of the final faces marked;
//   scans     output positions of faces and vertices: three launches each, block scans in the style of scan.hip;
//   finalize  counts[8].
// Every tally is an integer sum, so no result depends on the launch shape or the arrival order.
#include "qf_common.h"
#include "qf_mesh_compact.h"

namespace {

constexpr int kBlock = 256;
constexpr int kScanItems = 1024;                // items per workgroup in the scans
constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr uint32_t kDropped = 0x7fffffffu;      // above every vertex index (V < 2^31, so an index is <= 2^31 - 2)
constexpr uint32_t kEmpty = 0xffffffffu;        // an unclaimed slot of the duplicate table (a face id is < 2^31)
constexpr int kAllFlags = QF_MESH_REMOVE_DEGENERATE | QF_MESH_REMOVE_DUPLICATES | QF_MESH_REMOVE_UNREFERENCED;

enum : uint8_t { kAlive = 0, kByMask = 1, kDegenerate = 2, kDuplicate = 3, kIsland = 4, kInvalid = 5 };

inline int64_t align_up(int64_t x) { return (x + 255) & ~int64_t(255); }

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

int64_t table_slots(int64_t F)
{
    int64_t t = 64;
    while (t < 2 * F) t <<= 1;
    return t;
}

Workspace carve(void *base, int64_t V, int64_t F)
{
    Workspace w;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { char *p = static_cast<char *>(base) + off; off += align_up(bytes); return p; };
    w.info = reinterpret_cast<Info *>(take(sizeof(Info)));
    w.parent = reinterpret_cast<int32_t *>(take(4 * V));
    w.csize = reinterpret_cast<int32_t *>(take(4 * V));
    w.used = reinterpret_cast<uint8_t *>(take(V));
    w.vpos = reinterpret_cast<int32_t *>(take(4 * V));
    w.state = reinterpret_cast<uint8_t *>(take(F));
    w.tri = reinterpret_cast<int32_t *>(take(12 * F));
    w.fpos = reinterpret_cast<int32_t *>(take(4 * F));
    w.slots = table_slots(F);
    w.table = reinterpret_cast<uint32_t *>(take(4 * w.slots));
    w.slot = reinterpret_cast<uint32_t *>(take(4 * F));
    w.vpart = reinterpret_cast<int32_t *>(take(4 * qf_div_up(V, kScanItems)));
    w.fpart = reinterpret_cast<int32_t *>(take(4 * qf_div_up(F, kScanItems)));
    w.bytes = off;
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

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

// Sum of `v` over the wave, added to *dst by one lane.  Every lane of the wave must call it.
__device__ __forceinline__ void tally(unsigned long long *dst, int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x, halving the path on the way: a parent only ever moves to a smaller vertex of the same tree, so the
// atomicMin keeps every concurrent reader on a valid path.
__device__ __forceinline__ int32_t uf_find(int32_t *parent, int32_t x)
{
    int32_t p = load_parent(parent, x);
    while (p != x) {
        const int32_t gp = load_parent(parent, p);
        if (gp != p) atomicMin(parent + x, gp);
        x = p;
        p = gp;
    }
    return x;
}

__device__ __forceinline__ void uf_union(int32_t *parent, int32_t a, int32_t b)
{
    while (true) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
        if (a == b) return;
        const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
        const int32_t old = atomicCAS(parent + hi, hi, lo);
        if (old == hi) return;
        a = old;            // hi was hooked under `old` by another thread meanwhile: go on from there
        b = lo;
    }
}

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

// A surviving face walks its probe sequence to the first slot that is empty (claimed with compare-and-swap) or holds a
// face with the same sorted triple (whose id it lowers to its own if smaller).  A slot's triple never changes once it is
// claimed, and a failed swap goes on with the id it read: nothing waits.  At most F of the >= 2 F slots are ever claimed,
// so the walk ends.
__global__ __launch_bounds__(kBlock) void duplicate_insert_kernel(int64_t F, Workspace ws)
{
    const int64_t f = gtid();
    if (f >= F || ws.info->n_invalid != 0 || ws.state[f] != kAlive) return;
    const int32_t lo = ws.tri[3 * f], mid = ws.tri[3 * f + 1], hi = ws.tri[3 * f + 2];
    const uint64_t wrap = (uint64_t)ws.slots - 1;
    uint64_t s = triple_hash((uint32_t)lo, (uint32_t)mid, (uint32_t)hi) & wrap;
    while (true) {
        uint32_t g = __hip_atomic_load(ws.table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == kEmpty) {
            g = atomicCAS(ws.table + s, kEmpty, (uint32_t)f);
            if (g == kEmpty) break;
        }
        const int32_t *t = ws.tri + 3 * (int64_t)g;
        if (t[0] == lo && t[1] == mid && t[2] == hi) {
            if ((uint32_t)f < g) atomicMin(ws.table + s, (uint32_t)f);
            break;
        }
        s = (s + 1) & wrap;
    }
    ws.slot[f] = (uint32_t)s;
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
    int32_t x = (int32_t)v, p = load_parent(ws.parent, x);
    while (p != x) {
        x = p;
        p = load_parent(ws.parent, x);
    }
    __hip_atomic_store(ws.parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
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

// ---- exclusive scan of the flags (src[i] == match) over n items: per-workgroup sums, one workgroup scans those, every
// workgroup scans its own items from its base (scan.hip's three launches)
__device__ __forceinline__ int32_t block_inclusive_scan(int32_t v, int32_t *s_wave, int32_t *total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int32_t o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    if (lane == 63) s_wave[wave] = v;
    __syncthreads();
    int32_t base = 0, sum = 0;
    for (int w = 0; w < kBlock / 64; ++w) {
        if (w < wave) base += s_wave[w];
        sum += s_wave[w];
    }
    __syncthreads();
    *total = sum;
    return v + base;
}

__global__ __launch_bounds__(kBlock) void scan_partials_kernel(const uint8_t *__restrict__ src, int64_t n, uint8_t match,
                                                               int32_t *__restrict__ partial)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * (kScanItems / kBlock);
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems / kBlock; ++k) v += (i0 + k < n && src[i0 + k] == match) ? 1 : 0;
    int32_t total;
    block_inclusive_scan(v, s_wave, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup; every thread owns a contiguous run of the partial sums
__global__ __launch_bounds__(kBlock) void scan_bases_kernel(int32_t *partial, int64_t n_blocks, int32_t *total_out)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int64_t per = (n_blocks + kBlock - 1) / kBlock;
    const int64_t i0 = (int64_t)threadIdx.x * per, i1 = i0 + per < n_blocks ? i0 + per : n_blocks;
    int32_t sum = 0;
    for (int64_t i = i0; i < i1; ++i) sum += partial[i];
    int32_t total;
    int32_t run = block_inclusive_scan(sum, s_wave, &total) - sum;
    for (int64_t i = i0; i < i1; ++i) {
        const int32_t v = partial[i];
        partial[i] = run;
        run += v;
    }
    if (threadIdx.x == 0) *total_out = total;
}

__global__ __launch_bounds__(kBlock) void scan_positions_kernel(const uint8_t *__restrict__ src, int64_t n, uint8_t match,
                                                                const int32_t *__restrict__ partial,
                                                                int32_t *__restrict__ pos)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * (kScanItems / kBlock);
    int32_t c[kScanItems / kBlock], v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems / kBlock; ++k) {
        c[k] = (i0 + k < n && src[i0 + k] == match) ? 1 : 0;
        v += c[k];
    }
    int32_t total;
    int32_t run = partial[blockIdx.x] + block_inclusive_scan(v, s_wave, &total) - v;
#pragma unroll
    for (int k = 0; k < kScanItems / kBlock; ++k) {
        if (i0 + k < n) pos[i0 + k] = run;
        run += c[k];
    }
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

unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

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

int scan_flags(const uint8_t *src, int64_t n, uint8_t match, int32_t *partial, int32_t *pos, int32_t *total, hipStream_t s)
{
    if (n == 0) return QF_OK;           // the total stays at the zero the workspace's info block starts with
    const int64_t n_blocks = qf_div_up(n, kScanItems);
    hipLaunchKernelGGL(scan_partials_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, src, n, match, partial);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_bases_kernel, dim3(1), dim3(kBlock), 0, s, partial, n_blocks, total);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_positions_kernel, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, src, n, match, partial, pos);
    QF_LAUNCH_CHECK();
    return QF_OK;
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
    hipLaunchKernelGGL(init_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, ws, unref ? 0 : 1);
    QF_LAUNCH_CHECK();
    if (F > 0) {
        hipLaunchKernelGGL(classify_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, J, ws);
        QF_LAUNCH_CHECK();
        if (flags & QF_MESH_REMOVE_DUPLICATES) {
            QF_HIP_TRY(hipMemsetAsync(ws.table, 0xff, 4 * (size_t)ws.slots, s));
            hipLaunchKernelGGL(duplicate_insert_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, F, ws);
            QF_LAUNCH_CHECK();
            hipLaunchKernelGGL(duplicate_mark_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, F, ws);
            QF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(union_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, F, ws);
        QF_LAUNCH_CHECK();
        hipLaunchKernelGGL(flatten_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, ws);
        QF_LAUNCH_CHECK();
        hipLaunchKernelGGL(component_size_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, F, ws);
        QF_LAUNCH_CHECK();
        hipLaunchKernelGGL(component_count_kernel, dim3(blocks(V)), dim3(kBlock), 0, s, V, ws);
        QF_LAUNCH_CHECK();
        hipLaunchKernelGGL(island_kernel, dim3(blocks(F)), dim3(kBlock), 0, s, F, ws, J.M, unref);
        QF_LAUNCH_CHECK();
    }
    int st = scan_flags(ws.state, F, kAlive, ws.fpart, ws.fpos, &ws.info->face_total, s);
    if (st != QF_OK) return st;
    st = scan_flags(ws.used, V, 1, ws.vpart, ws.vpos, &ws.info->vertex_total, s);
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
        hipLaunchKernelGGL(vertex_emit_kernel, dim3(blocks(J.V)), dim3(kBlock), 0, s, J, ws,
                           reinterpret_cast<uint64_t *>(out_vertices), n_out_vertices, vertex_map);
        QF_LAUNCH_CHECK();
    }
    if (n_out_faces > 0) {
        hipLaunchKernelGGL(face_emit_kernel, dim3(blocks(J.F)), dim3(kBlock), 0, s, J, ws, out_faces, n_out_faces, face_map);
        QF_LAUNCH_CHECK();
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
