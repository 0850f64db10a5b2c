// Welding vertices by position on the device (include/qf_mesh_weld.h; the rule is DESIGN.md section 3.9g, restated in
// numpy in tests/mesh_weld_reference.py).  The only floating-point work is the cell quotient and the distance test of
// rule 2, each operation rounded on its own (the file is built with -ffp-contract=off); coordinates move as 64-bit words.
//
// Passes of qf_mesh_weld_count (one stream, no host wait):
//   cells     per vertex: finite test; the key (h > 0: the integer cell floor(x / s) per axis; h == 0: the three
//             coordinates' bits with -0.0 made +0.0), the loose and out-of-range tallies, parent[v] = v;
//   faces     per face: the invalid tally;
//   insert    per finite vertex: an open-addressing table of >= 2 V slots keyed by the key, filled with mesh_device.h's
//             claim-or-lower insert, so a slot ends with the lowest vertex id of its key; with h > 0 the vertex is also
//             pushed on the slot's list with one atomicExch (the list is read only in the next launch);
//   link      h > 0 only, per finite vertex: the members with a lower index of the 27 cells around its own are tested
//             under rule 2 and united in mesh_device.h's lock-free union-find, so a class's root is its lowest index
//             whatever the arrival order; the arithmetic is skipped when both already share a root.  Quadratic in a
//             cell's population, which counts[4] reports;
//   flatten   per vertex: parent[v] = root (h == 0: the lowest id of its slot, whose members are equal by construction,
//             so the pass is linear whatever the input), and the class sizes (integer atomicAdd);
//   roots     per vertex: flag[v] = 1 iff v is a root; the classes of two or more and the largest class;
//   scan      output row of every root: mesh_device.h's three-launch scan;
//   tally     per face: faces that were not degenerate and now are;
//   finalize  counts[8].
// Every tally is an integer sum or maximum (a wave reduction and one atomic per wave), so no result depends on the
// launch shape or the arrival order.
#include "mesh_device.h"
#include "qf_mesh_weld.h"

#include <cfloat>
#include <cmath>

namespace {

constexpr int64_t kMaxCount = int64_t(1) << 31;
constexpr double kCellLimit = 2251799813685248.0;   // 2^51

enum : uint8_t { kFinite = 0, kLoose = 1, kOutOfRange = 2 };

struct Info {
    unsigned long long n_invalid, n_out_of_range, n_loose, n_multi, n_collapsed;
    unsigned int max_class, max_cell;
    int32_t root_total;
};

struct Workspace {
    Info *info;
    int32_t *parent;        // [V] union-find forest, then every vertex's root
    uint8_t *flag;          // [V] 1: the vertex is a root
    int32_t *pos;           // [V] exclusive scan of flag: the output row of a root
    int32_t *part;          // per-workgroup sums of the scan
    uint8_t *state;         // [V] kFinite, kLoose or kOutOfRange
    int64_t *key;           // [3V] the cell, or the canonical coordinate bits
    uint32_t *slot;         // [V] the slot that holds the vertex's key
    uint32_t *next;         // [V] the next member of the slot's list
    int32_t *size;          // [V] members of the class rooted here
    uint32_t *table;        // [slots] the lowest vertex id of the key that claimed the slot   } one block,
    uint32_t *head;         // [slots] the first member of the slot's list                     } set to all ones together
    int64_t slots;          // a power of two >= max(2 V, 64)
    int64_t bytes;
};

Workspace carve(void *base, int64_t V)
{
    Workspace w;
    QfCarver c{base};
    w.info = c.take<Info>(1);
    w.parent = c.take<int32_t>(V);
    w.flag = c.take<uint8_t>(V);
    w.pos = c.take<int32_t>(V);
    w.part = c.take<int32_t>(qf_div_up(V, kScanItems));
    w.state = c.take<uint8_t>(V);
    w.key = c.take<int64_t>(3 * V);
    w.slot = c.take<uint32_t>(V);
    w.next = c.take<uint32_t>(V);
    w.size = c.take<int32_t>(V);
    w.slots = table_slots(V);
    w.table = c.take<uint32_t>(w.slots);        // 4 * slots is a multiple of 256: head follows at once
    w.head = c.take<uint32_t>(w.slots);
    w.bytes = c.off;
    return w;
}

struct Job {
    const double *v;
    const int64_t *f;
    int64_t V, F;
    double cell;            // s; 0 for h == 0
    double h2;              // h * h
};

__device__ __forceinline__ bool refused(const Workspace &ws)
{
    return ws.info->n_invalid != 0 || ws.info->n_out_of_range != 0;
}

__device__ __forceinline__ uint64_t key_hash(int64_t a, int64_t b, int64_t c)
{
    uint64_t h = (uint64_t)a * 0x9e3779b97f4a7c15ull;
    h ^= h >> 29;
    h = (h + (uint64_t)b) * 0xbf58476d1ce4e5b9ull;
    h ^= h >> 32;
    h = (h + (uint64_t)c) * 0x94d049bb133111ebull;
    return h ^ (h >> 31);
}

__device__ __forceinline__ bool finite_bits(uint64_t w) { return (w & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }

__global__ __launch_bounds__(kBlock) void cells_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    int loose = 0, out_of_range = 0;
    if (v < J.V) {
        const uint64_t *w = reinterpret_cast<const uint64_t *>(J.v) + 3 * v;
        const uint64_t wx = w[0], wy = w[1], wz = w[2];
        uint8_t st = kFinite;
        int64_t kx = 0, ky = 0, kz = 0;
        if (!(finite_bits(wx) && finite_bits(wy) && finite_bits(wz))) {
            st = kLoose;
        } else if (J.cell > 0.0) {
            const double cx = floor(J.v[3 * v] / J.cell), cy = floor(J.v[3 * v + 1] / J.cell),
                         cz = floor(J.v[3 * v + 2] / J.cell);
            // a quotient that is not finite fails the comparisons too
            if (fabs(cx) < kCellLimit && fabs(cy) < kCellLimit && fabs(cz) < kCellLimit) {
                kx = (int64_t)cx;
                ky = (int64_t)cy;
                kz = (int64_t)cz;
            } else {
                st = kOutOfRange;
            }
        } else {
            const uint64_t negative_zero = 0x8000000000000000ull;
            kx = (int64_t)(wx == negative_zero ? 0 : wx);
            ky = (int64_t)(wy == negative_zero ? 0 : wy);
            kz = (int64_t)(wz == negative_zero ? 0 : wz);
        }
        loose = st == kLoose;
        out_of_range = st == kOutOfRange;
        ws.state[v] = st;
        ws.key[3 * v] = kx;
        ws.key[3 * v + 1] = ky;
        ws.key[3 * v + 2] = kz;
        ws.parent[v] = (int32_t)v;
        ws.next[v] = kEmpty;
    }
    tally(&ws.info->n_loose, loose);
    tally(&ws.info->n_out_of_range, out_of_range);
}

__global__ __launch_bounds__(kBlock) void faces_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int invalid = 0;
    if (f < J.F) {
        const int64_t a = J.f[3 * f], b = J.f[3 * f + 1], c = J.f[3 * f + 2];
        invalid = a < 0 || a >= J.V || b < 0 || b >= J.V || c < 0 || c >= J.V;
    }
    tally(&ws.info->n_invalid, invalid);
}

// whether vertex g has the key (kx, ky, kz)
struct SameKey {
    const int64_t *key;
    int64_t kx, ky, kz;
    __device__ __forceinline__ bool operator()(uint32_t g) const
    {
        const int64_t *k = key + 3 * (int64_t)g;
        return k[0] == kx && k[1] == ky && k[2] == kz;
    }
};

// A finite vertex enters the table under its key (claim_or_lower of mesh_device.h).
__global__ __launch_bounds__(kBlock) void insert_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    if (v >= J.V || refused(ws) || ws.state[v] != kFinite) return;
    const int64_t kx = ws.key[3 * v], ky = ws.key[3 * v + 1], kz = ws.key[3 * v + 2];
    const uint64_t s = claim_or_lower(ws.table, (uint64_t)ws.slots - 1, key_hash(kx, ky, kz), (uint32_t)v,
                                      SameKey{ws.key, kx, ky, kz});
    ws.slot[v] = (uint32_t)s;
    if (J.cell > 0.0) ws.next[v] = atomicExch(ws.head + s, (uint32_t)v);
}

// The slot that holds the key, or kEmpty.
__device__ __forceinline__ uint32_t key_slot(const Workspace &ws, int64_t kx, int64_t ky, int64_t kz)
{
    return find_slot(ws.table, (uint64_t)ws.slots - 1, key_hash(kx, ky, kz), SameKey{ws.key, kx, ky, kz});
}

__global__ __launch_bounds__(kBlock) void link_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    int population = 0;
    if (v < J.V && !refused(ws) && ws.state[v] == kFinite) {
        const double x = J.v[3 * v], y = J.v[3 * v + 1], z = J.v[3 * v + 2];
        const int64_t kx = ws.key[3 * v], ky = ws.key[3 * v + 1], kz = ws.key[3 * v + 2];
        const uint32_t own = ws.slot[v];
        const bool lowest = ws.table[own] == (uint32_t)v;          // the cell's lowest member counts its population
        for (int n = 0; n < 27; ++n) {
            const int ox = n % 3 - 1, oy = (n / 3) % 3 - 1, oz = n / 9 - 1;
            const uint32_t s = n == 13 ? own : key_slot(ws, kx + ox, ky + oy, kz + oz);
            if (s == kEmpty) continue;
            for (uint32_t u = ws.head[s]; u != kEmpty; u = ws.next[u]) {
                if (n == 13 && lowest) ++population;
                if ((int64_t)u >= v) continue;
                const int32_t ru = uf_find(ws.parent, (int32_t)u), rv = uf_find(ws.parent, (int32_t)v);
                if (ru == rv) continue;
                const double dx = x - J.v[3 * (int64_t)u], dy = y - J.v[3 * (int64_t)u + 1], dz = z - J.v[3 * (int64_t)u + 2];
                if (((dx * dx + dy * dy) + dz * dz) <= J.h2) uf_union_roots(ws.parent, ru, rv);
            }
        }
    }
    tally_max(&ws.info->max_cell, population);
}

__global__ __launch_bounds__(kBlock) void flatten_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    if (v >= J.V || refused(ws)) return;
    int32_t x = (int32_t)v;
    if (ws.state[v] == kFinite) {
        if (J.cell > 0.0)
            x = uf_root(ws.parent, x);
        else
            x = (int32_t)ws.table[ws.slot[v]];
    }
    __hip_atomic_store(ws.parent + v, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    atomicAdd(ws.size + x, 1);
}

__global__ __launch_bounds__(kBlock) void roots_kernel(Job J, Workspace ws)
{
    const int64_t v = gtid();
    int multi = 0, size = 0;
    if (v < J.V) {
        const bool root = !refused(ws) && ws.parent[v] == (int32_t)v;
        ws.flag[v] = root;
        if (root) {
            size = ws.size[v];
            multi = size >= 2;
        }
    }
    tally(&ws.info->n_multi, multi);
    tally_max(&ws.info->max_class, size);
}

__global__ __launch_bounds__(kBlock) void face_tally_kernel(Job J, Workspace ws)
{
    const int64_t f = gtid();
    int collapsed = 0;
    if (f < J.F && !refused(ws)) {
        const int64_t a = J.f[3 * f], b = J.f[3 * f + 1], c = J.f[3 * f + 2];
        if (a != b && b != c && c != a) {
            const int32_t ra = ws.parent[a], rb = ws.parent[b], rc = ws.parent[c];
            collapsed = ra == rb || rb == rc || rc == ra;
        }
    }
    tally(&ws.info->n_collapsed, collapsed);
}

__global__ void finalize_kernel(Job J, Workspace ws, int64_t *counts)
{
    const Info &I = *ws.info;
    const bool ok = I.n_invalid == 0 && I.n_out_of_range == 0;
    counts[0] = ok ? (int64_t)I.root_total : 0;
    counts[1] = ok ? (int64_t)I.n_multi : 0;
    counts[2] = ok ? (int64_t)I.max_class : 0;
    counts[3] = ok ? (int64_t)I.n_collapsed : 0;
    counts[4] = ok && J.cell > 0.0 ? (int64_t)I.max_cell : 0;
    counts[5] = ok ? (int64_t)I.n_loose : 0;
    counts[6] = (int64_t)I.n_out_of_range;
    counts[7] = (int64_t)I.n_invalid;
}

// ---- emit ----------------------------------------------------------------------------------------------------------

// one thread per input vertex: its class, and the row and map entry of the class it is the root of; the coordinates move
// as 64-bit words, so the copy keeps every bit, NaN payloads included
__global__ __launch_bounds__(kBlock) void vertex_emit_kernel(const uint64_t *__restrict__ src, int64_t V, Workspace ws,
                                                             uint64_t *__restrict__ out, int64_t n_out,
                                                             int64_t *__restrict__ vertex_map,
                                                             int64_t *__restrict__ vertex_class)
{
    const int64_t v = gtid();
    if (v >= V || refused(ws)) return;
    if (vertex_class) vertex_class[v] = ws.pos[ws.parent[v]];
    if (ws.flag[v]) {
        const int64_t o = ws.pos[v];
        if (o < n_out) {
            out[3 * o] = src[3 * v];
            out[3 * o + 1] = src[3 * v + 1];
            out[3 * o + 2] = src[3 * v + 2];
            if (vertex_map) vertex_map[o] = v;
        }
    }
}

__global__ __launch_bounds__(kBlock) void face_emit_kernel(const int64_t *__restrict__ faces, int64_t F, Workspace ws,
                                                           int64_t *__restrict__ out_faces)
{
    const int64_t c = gtid();
    if (c >= 3 * F || refused(ws)) return;
    out_faces[c] = ws.pos[ws.parent[faces[c]]];
}

bool sizes_ok(int64_t V, int64_t F) { return V >= 1 && V < kMaxCount && F >= 0 && F < kMaxCount; }

}  // namespace

extern "C" int64_t qf_mesh_weld_workspace_bytes(int64_t n_vertices, int64_t n_faces)
{
    if (!sizes_ok(n_vertices, n_faces)) return -1;
    return carve(nullptr, n_vertices).bytes;
}

extern "C" int qf_mesh_weld_count(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                  double tolerance, void *workspace, int64_t workspace_bytes, int64_t *counts, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces) || !vertices || (n_faces > 0 && !faces) || !workspace || !counts)
        return QF_ERR_INVALID_ARGUMENT;
    if (!(tolerance >= 0.0) || !(tolerance <= DBL_MAX)) return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = n_vertices, F = n_faces;
    Workspace ws = carve(workspace, V);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    // rule 1's cell edge: 2 max(h, 2^-510), +inf when h * h is not finite; 0 stands for h == 0
    const double h2 = tolerance * tolerance;
    double cell = 0.0;
    if (tolerance > 0.0) cell = h2 <= DBL_MAX ? 2.0 * (tolerance > 0x1p-510 ? tolerance : 0x1p-510) : INFINITY;
    const Job J{vertices, faces, V, F, cell, h2};

    QF_HIP_TRY(hipMemsetAsync(ws.info, 0, sizeof(Info), s));
    QF_HIP_TRY(hipMemsetAsync(ws.size, 0, 4 * (size_t)V, s));
    QF_HIP_TRY(hipMemsetAsync(ws.table, 0xff, 8 * (size_t)ws.slots, s));        // table and head
    QF_MESH_LAUNCH(cells_kernel, V, J, ws);
    QF_MESH_LAUNCH(faces_kernel, F, J, ws);
    QF_MESH_LAUNCH(insert_kernel, V, J, ws);
    if (cell > 0.0) {
        QF_MESH_LAUNCH(link_kernel, V, J, ws);
    }
    QF_MESH_LAUNCH(flatten_kernel, V, J, ws);
    QF_MESH_LAUNCH(roots_kernel, V, J, ws);
    const int st = scan_bytes(ws.flag, V, ItemNonZero{}, ws.part, ws.pos, &ws.info->root_total, s);
    if (st != QF_OK) return st;
    QF_MESH_LAUNCH(face_tally_kernel, F, J, ws);
    hipLaunchKernelGGL(finalize_kernel, dim3(1), dim3(1), 0, s, J, ws, counts);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_mesh_weld_emit(const double *vertices, int64_t n_vertices, const int64_t *faces, int64_t n_faces,
                                 void *workspace, int64_t workspace_bytes, double *out_vertices, int64_t n_out_vertices,
                                 int64_t *out_faces, int64_t *vertex_map, int64_t *vertex_class, void *stream)
{
    if (!sizes_ok(n_vertices, n_faces) || !vertices || (n_faces > 0 && (!faces || !out_faces)) || !workspace)
        return QF_ERR_INVALID_ARGUMENT;
    const int64_t V = n_vertices, F = n_faces;
    if (n_out_vertices < 0 || n_out_vertices > V || (n_out_vertices > 0 && !out_vertices)) return QF_ERR_INVALID_ARGUMENT;
    Workspace ws = carve(workspace, V);
    if (workspace_bytes < ws.bytes) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t s = qf_stream(stream);
    if (n_out_vertices > 0 || vertex_class) {
        QF_MESH_LAUNCH(vertex_emit_kernel, V, reinterpret_cast<const uint64_t *>(vertices), V, ws,
                       reinterpret_cast<uint64_t *>(out_vertices), n_out_vertices, vertex_map, vertex_class);
    }
    QF_MESH_LAUNCH(face_emit_kernel, 3 * F, faces, F, ws, out_faces);
    return QF_OK;
}
