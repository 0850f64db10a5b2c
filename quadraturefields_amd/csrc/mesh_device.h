// Device primitives shared by the mesh-processing stages (mesh_compact, mesh_manifold, mesh_subdivide, mesh_weld; the
// helpers at the top also by mesh_sample, mesh_decimate, vertex_clustering and uv_atlas).  Integer work only.  Everything
// sits in an anonymous namespace: each stage keeps its own instantiation of the kernel templates, and no symbol is
// exported.
#pragma once
#include "qf_common.h"

namespace {

constexpr int kBlock = 256;                     // threads per workgroup of every mesh kernel
constexpr int kScanItems = 1024;                // items per workgroup in scan_bytes
constexpr uint32_t kEmpty = 0xffffffffu;        // an unclaimed table slot (an id is < 2^31)

__device__ __forceinline__ int64_t gtid() { return (int64_t)blockIdx.x * blockDim.x + threadIdx.x; }

inline unsigned blocks(int64_t n) { return (unsigned)((n + kBlock - 1) / kBlock); }

// One thread per item on the entry point's stream `s`; nothing is launched for no items.  Returns QF_ERR_HIP from the
// enclosing function if the launch fails.
#define QF_MESH_LAUNCH(kernel, count, ...)                                                         \
    do {                                                                                           \
        if ((count) > 0) {                                                                         \
            hipLaunchKernelGGL(kernel, dim3(blocks(count)), dim3(kBlock), 0, s, __VA_ARGS__);      \
            QF_LAUNCH_CHECK();                                                                     \
        }                                                                                          \
    } while (0)

// Sum of `v` over the wave, added to *dst by one lane.  Every lane of the wave must call it.
__device__ __forceinline__ void tally(unsigned long long *dst, int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(dst, (unsigned long long)v);
}

// Maximum of `v` (>= 0) over the wave, raised into *dst by one lane.  Every lane of the wave must call it.
__device__ __forceinline__ void tally_max(unsigned int *dst, int v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, (unsigned int)v);
}

__device__ __forceinline__ void tally_max(unsigned long long *dst, unsigned long long v)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    if ((threadIdx.x & 63) == 0 && v) atomicMax(dst, v);
}

// ---- lock-free union-find over parent[], which starts as parent[x] = x.  The larger root is hooked under the smaller
// with compare-and-swap, so a tree's root is its smallest member whatever the arrival order.  A parent only ever moves to
// a smaller member of the same tree, so every concurrent reader stays on a valid path; a failed swap goes on from the
// value it read (another thread made progress), and nothing waits.

__device__ __forceinline__ int32_t load_parent(const int32_t *parent, int32_t x)
{
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Root of x, halving the path on the way with atomicMin.
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

// Root of x without writing: for the flatten passes, which run after the last union.
__device__ __forceinline__ int32_t uf_root(const int32_t *parent, int32_t x)
{
    int32_t p = load_parent(parent, x);
    while (p != x) {
        x = p;
        p = load_parent(parent, x);
    }
    return x;
}

// One attempt to hook the larger of the roots a and b under the smaller.  True: they are united.  False: the larger one
// was hooked under another member by another thread meanwhile, and a and b are the two members to go on from.
__device__ __forceinline__ bool uf_hook(int32_t *parent, int32_t &a, int32_t &b)
{
    if (a == b) return true;
    const int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    const int32_t old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return true;
    a = old;
    b = lo;
    return false;
}

// Unites the trees of a and b, which are roots as far as the caller saw.
__device__ __forceinline__ void uf_union_roots(int32_t *parent, int32_t a, int32_t b)
{
    while (!uf_hook(parent, a, b)) {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
    }
}

// Unites the trees of any two members: find both, then the roots form.  Written as one loop, so that the two walks of
// uf_find are inlined once and not a second time for the retry.
__device__ __forceinline__ void uf_union(int32_t *parent, int32_t a, int32_t b)
{
    do {
        a = uf_find(parent, a);
        b = uf_find(parent, b);
    } while (!uf_hook(parent, a, b));
}

// ---- open-addressing table of ids keyed by whatever the id stands for (a face's sorted triple, a vertex's cell, a
// half-edge's pair).  The table has table_slots(n) slots for at most n ids and starts as all kEmpty.

inline int64_t table_slots(int64_t n)
{
    int64_t t = 64;
    while (t < 2 * n) t <<= 1;
    return t;
}

// `id` walks its probe sequence from `hash` to the first slot that is empty (claimed with compare-and-swap) or holds an
// id with the same key (which it lowers to its own if smaller), and returns that slot; wrap = slots - 1.  same_key(g)
// tells whether occupant g has id's key.  A slot's key never changes once it is claimed, and a failed swap goes on with
// the id it read: nothing waits.  At most n of the >= 2 n slots are ever claimed, so the walk ends.  Afterwards a slot
// holds the lowest id of its key, whatever the arrival order.
template <typename SameKey>
__device__ __forceinline__ uint64_t claim_or_lower(uint32_t *table, uint64_t wrap, uint64_t hash, uint32_t id,
                                                   SameKey same_key)
{
    uint64_t s = hash & wrap;
    while (true) {
        uint32_t g = __hip_atomic_load(table + s, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (g == kEmpty) {
            g = atomicCAS(table + s, kEmpty, id);
            if (g == kEmpty) break;
        }
        if (same_key(g)) {
            if (id < g) atomicMin(table + s, id);
            break;
        }
        s = (s + 1) & wrap;
    }
    return s;
}

// The slot that holds the key, or kEmpty: the probe sequence of an absent key ends at an unclaimed slot.  Only for
// launches after the last insert.
template <typename SameKey>
__device__ __forceinline__ uint32_t find_slot(const uint32_t *table, uint64_t wrap, uint64_t hash, SameKey same_key)
{
    uint64_t s = hash & wrap;
    while (true) {
        const uint32_t g = table[s];
        if (g == kEmpty) return kEmpty;
        if (same_key(g)) return (uint32_t)s;
        s = (s + 1) & wrap;
    }
}

// ---- exclusive scan of n uint8 items into int32 positions, three launches (the shape of scan.hip): per-workgroup sums,
// one workgroup scans those, every workgroup scans its own items from its base.  What a byte counts for is the Item.

struct ItemEquals {                             // 1 where the byte equals `match`
    uint8_t match;
    __device__ __forceinline__ int32_t operator()(uint8_t b) const { return b == match ? 1 : 0; }
};
struct ItemNonZero {                            // 1 where the byte is not zero
    __device__ __forceinline__ int32_t operator()(uint8_t b) const { return b ? 1 : 0; }
};
struct ItemValue {                              // the byte itself
    __device__ __forceinline__ int32_t operator()(uint8_t b) const { return b; }
};

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

template <typename Item>
__global__ __launch_bounds__(kBlock) void scan_partials_kernel(const uint8_t *__restrict__ src, int64_t n, Item item,
                                                               int32_t *__restrict__ partial)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * (kScanItems / kBlock);
    int32_t v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems / kBlock; ++k) v += i0 + k < n ? item(src[i0 + k]) : 0;
    int32_t total;
    block_inclusive_scan(v, s_wave, &total);
    if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one workgroup; every thread owns a contiguous run of the partial sums.  (A template only so that a file that never
// scans does not carry the kernel.)
template <typename = void>
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

template <typename Item>
__global__ __launch_bounds__(kBlock) void scan_positions_kernel(const uint8_t *__restrict__ src, int64_t n, Item item,
                                                                const int32_t *__restrict__ partial,
                                                                int32_t *__restrict__ pos)
{
    __shared__ int32_t s_wave[kBlock / 64];
    const int64_t i0 = (int64_t)blockIdx.x * kScanItems + (int64_t)threadIdx.x * (kScanItems / kBlock);
    int32_t c[kScanItems / kBlock], v = 0;
#pragma unroll
    for (int k = 0; k < kScanItems / kBlock; ++k) {
        c[k] = i0 + k < n ? item(src[i0 + k]) : 0;
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

// pos[i] = the sum of item(src[j]) over j < i, *total = the sum over all n; partial holds qf_div_up(n, kScanItems) words.
template <typename Item>
int scan_bytes(const uint8_t *src, int64_t n, Item item, int32_t *partial, int32_t *pos, int32_t *total, hipStream_t s)
{
    if (n == 0) return QF_OK;           // the total stays at the zero the workspace's info block starts with
    const int64_t n_blocks = qf_div_up(n, kScanItems);
    hipLaunchKernelGGL(scan_partials_kernel<Item>, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, src, n, item, partial);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_bases_kernel<>, dim3(1), dim3(kBlock), 0, s, partial, n_blocks, total);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(scan_positions_kernel<Item>, dim3((unsigned)n_blocks), dim3(kBlock), 0, s, src, n, item, partial,
                       pos);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

}  // namespace
