// Device-side BVH construction: a linear BVH that goes straight to the 8-wide tree of bvh.h by range splitting over
// Morton-sorted triangles.  No binary tree is built and nothing is handed bottom-up through atomics.  The rules
// (restated in numpy in tests/bvh_device_build_reference.py):
//   centroid   the triangle's box centre 0.5f * (lo + hi), as the host builder takes it;
//   key        per axis q = min((uint)((c - clo) * scale), 2^21 - 1) with scale = 2^21 / (chi - clo) in fp32 (0 for an axis
//              of zero, infinite or undefined extent), clo / chi = the centroid bounds; code = the 63-bit interleave with
//              x at bits 3b + 2, y at 3b + 1, z at 3b;
//   order      stable radix sort of (code, triangle id), ids ascending on input: the sorted order is the leaf order;
//   leaf       a range of at most 8 sorted positions;
//   split      of [l, r]: equal end codes -> [l, l + (r - l) / 2] and the rest; otherwise the left half is every position
//              whose code agrees with code[l] on the common prefix of code[l] and code[r] plus one bit (binary search);
//   node       over a range of more than 8: the two halves of its split; while it has fewer than 8 children and some
//              child holds more than 8 triangles, the child with the most (leftmost on a tie) is replaced, in place, by
//              its two halves.  Children fill slots 0..h-1 left to right, the rest are empty.  A mesh of at most 8
//              triangles is a root with one leaf child;
//   levels     breadth first: an inner child's node index is the next level's base plus the exclusive scan of the
//              per-node inner-child counts, so nodes come out in level order, the same on every run;
//   boxes      after the topology, bottom-up, by the refit rule (qf_bvh_refit_boxes) with the build's eps;
//   stack      need(n) = max(h, h - 1 + max need(inner child)) bottom-up; max_stack8 = max(1, need(root)) + 1.
//
// Node capacity.  A node with an inner child has exactly 8 children (it stopped splitting only because it was full); a
// node without one ("bottom") covers at least 9 triangles of its own.  With T nodes of the first kind and B of the
// second, the T + B - 1 tree edges are the inner children, so the first kind owns 8T - (T + B - 1) leaf children of at
// least one triangle each: n >= 7T - B + 1 + 9B, hence T + B <= (n - 1) / 7.  The allocation holds max(1, (n - 1) / 7)
// nodes, every write is checked against it, and the level loop fails rather than exceed it.
//
// Visibility: every dependency between passes is a kernel boundary on one stream; no launch hands plain stores from one
// workgroup to another, nothing spins or polls, every loop has a static bound.  The file is compiled with
// -ffp-contract=off: every product and sum is rounded on its own.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>
#include <new>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>

#include "bvh.h"
#include "qf_common.h"

namespace {

constexpr int kBlock = 256;
constexpr int kRedBlocks = 512;          // fixed launch shape of the reduction: the fp64 area sum has ONE order
constexpr int kMaxLevels = 96;
constexpr int kAxisBits = 21;
constexpr float kAxisCells = 2097152.f;  // 2^21
constexpr uint32_t kAxisMax = (1u << kAxisBits) - 1u;

// Bounds of the finite triangles' vertices and centroids, their area, the count of the others.
struct Info {
    float vlo[3], vhi[3], clo[3], chi[3];
    double area;
    int64_t bad;
};

__device__ __forceinline__ void info_reset(Info &a)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.vlo[k] = a.clo[k] = INFINITY;
        a.vhi[k] = a.chi[k] = -INFINITY;
    }
    a.area = 0.0;
    a.bad = 0;
}

__device__ __forceinline__ void info_merge(Info &a, const Info &b)
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        a.vlo[k] = fminf(a.vlo[k], b.vlo[k]);
        a.vhi[k] = fmaxf(a.vhi[k], b.vhi[k]);
        a.clo[k] = fminf(a.clo[k], b.clo[k]);
        a.chi[k] = fmaxf(a.chi[k], b.chi[k]);
    }
    a.area += b.area;
    a.bad += b.bad;
}

// Tree reduction over the block in LDS: the pairing depends on the block size alone.
__device__ void block_reduce(Info &mine, Info *out)
{
    __shared__ Info sh[kBlock];
    const int tid = threadIdx.x;
    sh[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int stride = kBlock / 2; stride > 0; stride >>= 1) {
        if (tid < stride) {
            Info a = sh[tid];
            info_merge(a, sh[tid + stride]);
            sh[tid] = a;
        }
        __syncthreads();
    }
    if (tid == 0) *out = sh[0];
}

__device__ __forceinline__ void tri_box(const float *v, float lo[3], float hi[3])
{
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        lo[k] = fminf(fminf(v[k], v[3 + k]), v[6 + k]);
        hi[k] = fmaxf(fmaxf(v[k], v[3 + k]), v[6 + k]);
    }
}

__global__ void __launch_bounds__(kBlock) reduce_tris_kernel(const float *verts, int64_t n_tri, Info *partial)
{
    Info mine;
    info_reset(mine);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_tri; i += (int64_t)kRedBlocks * kBlock) {
        float v[9];
        bool finite = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            v[k] = verts[i * 9 + k];
            finite = finite && isfinite(v[k]);
        }
        if (!finite) {
            ++mine.bad;
            continue;
        }
        float lo[3], hi[3];
        tri_box(v, lo, hi);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = 0.5f * (lo[k] + hi[k]);
            mine.vlo[k] = fminf(mine.vlo[k], lo[k]);
            mine.vhi[k] = fmaxf(mine.vhi[k], hi[k]);
            mine.clo[k] = fminf(mine.clo[k], c);
            mine.chi[k] = fmaxf(mine.chi[k], c);
        }
        const double e1[3] = {(double)v[3] - v[0], (double)v[4] - v[1], (double)v[5] - v[2]};
        const double e2[3] = {(double)v[6] - v[0], (double)v[7] - v[1], (double)v[8] - v[2]};
        const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        mine.area += 0.5 * sqrt(cx * cx + cy * cy + cz * cz);
    }
    block_reduce(mine, partial + blockIdx.x);
}

// one block: partial[kRedBlocks] -> info
__global__ void __launch_bounds__(kBlock) reduce_final_kernel(const Info *partial, Info *info)
{
    Info mine;
    info_reset(mine);
    for (int i = threadIdx.x; i < kRedBlocks; i += kBlock) info_merge(mine, partial[i]);
    block_reduce(mine, info);
}

__device__ __forceinline__ uint64_t expand21(uint32_t q)
{
    uint64_t x = q & 0x1fffffu;
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

struct KeyFrame {
    float lo[3], scale[3];
};

__global__ void morton_keys_kernel(const float *verts, int64_t n_tri, KeyFrame f, uint64_t *key, int32_t *id)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_tri; i += (int64_t)gridDim.x * blockDim.x) {
        float v[9], lo[3], hi[3];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = verts[i * 9 + k];
        tri_box(v, lo, hi);
        uint32_t q[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float c = 0.5f * (lo[k] + hi[k]);
            const float d = c - f.lo[k];
            const float t = d * f.scale[k];
            q[k] = t >= 0.f ? (t >= (float)kAxisMax ? kAxisMax : (uint32_t)t) : 0u;      // NaN -> 0
        }
        key[i] = expand21(q[0]) << 2 | expand21(q[1]) << 1 | expand21(q[2]);
        id[i] = (int32_t)i;
    }
}

// leaf order: sorted position -> (v0.xyz, original id bits), (v1.xyz, 0), (v2.xyz, 0)
__global__ void gather_tris_kernel(const float *verts, const int32_t *sorted_id, int64_t n_tri, float4 *tris)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_tri; i += (int64_t)gridDim.x * blockDim.x) {
        const int32_t id = sorted_id[i];
        const float *v = verts + (int64_t)id * 9;
        tris[i * 3 + 0] = make_float4(v[0], v[1], v[2], __int_as_float(id));
        tris[i * 3 + 1] = make_float4(v[3], v[4], v[5], 0.f);
        tris[i * 3 + 2] = make_float4(v[6], v[7], v[8], 0.f);
    }
}

// Last position of the left half of [l, r], l < r (file comment: split).
__device__ int split_range(const uint64_t *code, int l, int r)
{
    const uint64_t a = code[l], b = code[r];
    if (a == b) return l + (r - l) / 2;
    const int shift = 63 - __clzll((long long)(a ^ b));     // the first differing bit; the codes agree above it
    int lo = l, hi = r;                                     // lo is in the left half, hi in the right
    for (int step = 0; step < 32; ++step) {                 // r - l < 2^28
        if (hi - lo <= 1) break;
        const int mid = lo + (hi - lo) / 2;
        if (((code[mid] ^ a) >> shift) == 0) lo = mid; else hi = mid;
    }
    return lo;
}

// Children of the node over [l, r]: boundaries s[0] < s[1] < .. < s[h] (child j = [s[j], s[j+1] - 1]) in this thread's
// LDS column (stride kBlock); returns h.
__device__ int node_children(const uint64_t *code, int l, int r, int *s)
{
    if (r - l + 1 <= QF_BVH8_LEAF_MAX) {
        s[0] = l;
        s[kBlock] = r + 1;
        return 1;
    }
    s[0] = l;
    s[kBlock] = split_range(code, l, r) + 1;
    s[2 * kBlock] = r + 1;
    int h = 2;
    for (int it = 0; it < 6; ++it) {
        int best = -1, best_n = QF_BVH8_LEAF_MAX;
        for (int i = 0; i < 8; ++i) {
            if (i >= h) break;
            const int c = s[(i + 1) * kBlock] - s[i * kBlock];
            if (c > best_n) { best_n = c; best = i; }
        }
        if (best < 0) break;
        const int m = split_range(code, s[best * kBlock], s[(best + 1) * kBlock] - 1);
        for (int j = 7; j > 0; --j)
            if (j <= h && j > best) s[(j + 1) * kBlock] = s[j * kBlock];
        s[(best + 1) * kBlock] = m + 1;
        ++h;
    }
    return h;
}

__global__ void init_root_kernel(int2 *ranges, int n_tri) { ranges[0] = make_int2(0, n_tri - 1); }

__global__ void __launch_bounds__(kBlock) count_children_kernel(const uint64_t *code, const int2 *ranges, int n_level, int32_t *cnt)
{
    __shared__ int bounds[9 * kBlock];
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= n_level) return;
    int *s = bounds + threadIdx.x;
    const int2 rg = ranges[m];
    const int h = node_children(code, rg.x, rg.y, s);
    int inner = 0;
    for (int j = 0; j < 8; ++j)
        if (j < h && s[(j + 1) * kBlock] - s[j * kBlock] > QF_BVH8_LEAF_MAX) ++inner;
    cnt[m] = inner;
}

// Writes the tokens of level [level_base, level_base + n_level) and the ranges of the next level; boxes come later.
__global__ void __launch_bounds__(kBlock) emit_level_kernel(const uint64_t *code, const int2 *ranges, const int32_t *cnt,
                                                            const int32_t *off, int n_level, int level_base, int capacity,
                                                            float4 *nodes, int2 *next_ranges, int32_t *next_count)
{
    __shared__ int bounds[9 * kBlock];
    const int m = blockIdx.x * kBlock + threadIdx.x;
    if (m >= n_level) return;
    const int node = level_base + m;
    const int next_base = level_base + n_level;
    const int first = off[m];
    if (m == n_level - 1) *next_count = first + cnt[m];
    if (node >= capacity) return;
    int *s = bounds + threadIdx.x;
    const int2 rg = ranges[m];
    const int h = node_children(code, rg.x, rg.y, s);
    int k = 0;
    for (int j = 0; j < 8; ++j) {
        float4 *c = nodes + (int64_t)node * 16 + 2 * j;
        if (j >= h) {
            c[0] = make_float4(INFINITY, INFINITY, INFINITY, -INFINITY);
            c[1] = make_float4(-INFINITY, -INFINITY, __int_as_float(QF_BVH8_EMPTY), 0.f);
            continue;
        }
        const int a = s[j * kBlock], size = s[(j + 1) * kBlock] - a;
        int token;
        if (size <= QF_BVH8_LEAF_MAX) {
            token = ~((a << 3) | (size - 1));
        } else {
            const int pos = first + k++;
            token = next_base + pos;
            if (token < capacity) next_ranges[pos] = make_int2(a, a + size - 1);      // pos < capacity - next_base
        }
        c[0] = make_float4(0.f, 0.f, 0.f, 0.f);
        c[1] = make_float4(0.f, 0.f, __int_as_float(token), 0.f);
    }
}

// need(n) of the level [node0, node1); the levels below are done
__global__ void stack_level_kernel(const float *nodes, int node0, int node1, int32_t *need)
{
    const int n = node0 + blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= node1) return;
    int h = 0, deepest = 0;
    for (int j = 0; j < 8; ++j) {
        const int tok = __float_as_int(nodes[(int64_t)n * 64 + 8 * j + 6]);
        if (tok == QF_BVH8_EMPTY) continue;
        ++h;
        if (tok >= 0) deepest = max(deepest, need[tok]);
    }
    need[n] = max(h, h - 1 + deepest);
}

struct DeviceBlock {
    void *p = nullptr;
    ~DeviceBlock() { if (p) (void)hipFree(p); }
};

struct HandleGuard {
    qf_bvh *bvh = nullptr;
    ~HandleGuard()      // error paths only: a copy into the handle's host vectors may still be in flight
    {
        if (!bvh) return;
        (void)hipDeviceSynchronize();
        qf_bvh_destroy(bvh);
    }
};

struct PassTimer {
    hipEvent_t ev[QF_BVH_BUILD_PASSES + 1] = {};
    bool on = false;
    int n = 0;
    ~PassTimer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t start(bool want)
    {
        on = want;
        if (!on) return hipSuccess;
        for (hipEvent_t &e : ev) {
            hipError_t rc = hipEventCreate(&e);
            if (rc != hipSuccess) return rc;
        }
        return hipSuccess;
    }
    hipError_t mark(hipStream_t st) { return on && n <= QF_BVH_BUILD_PASSES ? hipEventRecord(ev[n++], st) : hipSuccess; }
};

size_t rocprim_temp_bytes(size_t n_tri, size_t capacity, hipStream_t st)
{
    size_t sort = 0, scan = 0;
    if (rocprim::radix_sort_pairs(nullptr, sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (int32_t *)nullptr,
                                  (int32_t *)nullptr, n_tri, 0, 63, st) != hipSuccess)
        return 0;
    if (rocprim::exclusive_scan(nullptr, scan, (int32_t *)nullptr, (int32_t *)nullptr, 0, capacity,
                                rocprim::plus<int32_t>(), st) != hipSuccess)
        return 0;
    const size_t need = sort > scan ? sort : scan;
    return need > 0 ? need : 1;
}

int build_device(const float *d_tri_verts, int64_t n_tri, hipStream_t st, float *pass_ms, int64_t *peak_bytes, qf_bvh **out)
{
    HandleGuard guard;
    qf_bvh *bvh = guard.bvh = new (std::nothrow) qf_bvh();
    if (!bvh) return QF_ERR_INVALID_ARGUMENT;
    bvh->n_tri = n_tri;
    bvh->nodes8_mirrored = false;
    if (pass_ms)
        for (int k = 0; k < QF_BVH_BUILD_PASSES; ++k) pass_ms[k] = 0.f;
    if (peak_bytes) *peak_bytes = 0;
    const int64_t capacity = n_tri > 8 ? (n_tri - 1) / 7 : 1;          // nodes (file comment)
    QF_HIP_TRY(hipMalloc((void **)&bvh->d_nodes8, (size_t)capacity * 64 * sizeof(float)));
    QF_HIP_TRY(hipMalloc((void **)&bvh->d_tris, (size_t)(n_tri > 0 ? n_tri : 1) * 12 * sizeof(float)));
    if (n_tri == 0) {                                                  // as qf_bvh_create: a handle with no nodes
        bvh->nodes8_mirrored = true;
        *out = bvh;
        guard.bvh = nullptr;
        return QF_OK;
    }

    // ---- temporary memory, one block ----
    const size_t temp_bytes = rocprim_temp_bytes((size_t)n_tri, (size_t)capacity, st);
    if (temp_bytes == 0) return QF_ERR_HIP;
    int64_t off = 0;
    auto take = [&](int64_t bytes) { const int64_t at = off; off += qf_align_up(bytes); return at; };
    const int64_t o_info = take(sizeof(Info)), o_partial = take((int64_t)sizeof(Info) * kRedBlocks);
    const int64_t o_key_a = take(8 * n_tri), o_key_b = take(8 * n_tri), o_id_a = take(4 * n_tri), o_id_b = take(4 * n_tri);
    const int64_t o_rg_a = take(8 * capacity), o_rg_b = take(8 * capacity), o_cnt = take(4 * capacity), o_off = take(4 * capacity);
    const int64_t o_need = take(4 * capacity), o_next = take(4), o_temp = take((int64_t)temp_bytes);
    DeviceBlock block;
    QF_HIP_TRY(hipMalloc(&block.p, (size_t)off));
    char *base = static_cast<char *>(block.p);
    Info *d_info = reinterpret_cast<Info *>(base + o_info), *d_partial = reinterpret_cast<Info *>(base + o_partial);
    uint64_t *key_a = reinterpret_cast<uint64_t *>(base + o_key_a), *key_b = reinterpret_cast<uint64_t *>(base + o_key_b);
    int32_t *id_a = reinterpret_cast<int32_t *>(base + o_id_a), *id_b = reinterpret_cast<int32_t *>(base + o_id_b);
    int2 *rg_cur = reinterpret_cast<int2 *>(base + o_rg_a), *rg_next = reinterpret_cast<int2 *>(base + o_rg_b);
    int32_t *d_cnt = reinterpret_cast<int32_t *>(base + o_cnt), *d_off = reinterpret_cast<int32_t *>(base + o_off);
    int32_t *d_need = reinterpret_cast<int32_t *>(base + o_need), *d_next = reinterpret_cast<int32_t *>(base + o_next);
    void *d_temp = base + o_temp;
    if (peak_bytes) *peak_bytes = off + capacity * 256 + n_tri * 48;

    PassTimer timer;
    QF_HIP_TRY(timer.start(pass_ms != nullptr));
    QF_HIP_TRY(timer.mark(st));

    // ---- pass 0: boxes, centroids, bounds, area, non-finite count; the one read-back of the bounds ----
    hipLaunchKernelGGL(reduce_tris_kernel, dim3(kRedBlocks), dim3(kBlock), 0, st, d_tri_verts, n_tri, d_partial);
    QF_LAUNCH_CHECK();
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(kBlock), 0, st, d_partial, d_info);
    QF_LAUNCH_CHECK();
    Info info;
    QF_HIP_TRY(hipMemcpyAsync(&info, d_info, sizeof(Info), hipMemcpyDeviceToHost, st));
    QF_HIP_TRY(hipStreamSynchronize(st));
    if (info.bad != 0) return QF_ERR_INVALID_ARGUMENT;
    bvh->eps = qf_bvh_eps_from_bounds(info.vlo, info.vhi);
    {
        const double ex = (double)info.vhi[0] - info.vlo[0], ey = (double)info.vhi[1] - info.vlo[1], ez = (double)info.vhi[2] - info.vlo[2];
        const double box = 2.0 * (ex * ey + ey * ez + ex * ez);
        bvh->depth_complexity64 = box > 0.0 ? 2.0 * info.area / box : 0.0;
        bvh->depth_complexity = (float)bvh->depth_complexity64;
    }
    QF_HIP_TRY(timer.mark(st));

    // ---- pass 1: keys ----
    KeyFrame frame;
    for (int k = 0; k < 3; ++k) {
        const float ext = info.chi[k] - info.clo[k];
        frame.lo[k] = info.clo[k];
        frame.scale[k] = ext > 0.f && std::isfinite(ext) ? kAxisCells / ext : 0.f;
    }
    hipLaunchKernelGGL(morton_keys_kernel, dim3(qf_grid_1d(n_tri, kBlock)), dim3(kBlock), 0, st, d_tri_verts, n_tri, frame, key_a, id_a);
    QF_LAUNCH_CHECK();
    QF_HIP_TRY(timer.mark(st));

    // ---- pass 2: stable sort; pass 3: triangles in leaf order, and the host copy of the ids ----
    size_t tb = temp_bytes;
    QF_HIP_TRY(rocprim::radix_sort_pairs(d_temp, tb, key_a, key_b, id_a, id_b, (size_t)n_tri, 0, 63, st));
    QF_HIP_TRY(timer.mark(st));
    hipLaunchKernelGGL(gather_tris_kernel, dim3(qf_grid_1d(n_tri, kBlock)), dim3(kBlock), 0, st, d_tri_verts, id_b, n_tri,
                       reinterpret_cast<float4 *>(bvh->d_tris));
    QF_LAUNCH_CHECK();
    bvh->h_tri_ids.resize((size_t)n_tri);
    QF_HIP_TRY(hipMemcpyAsync(bvh->h_tri_ids.data(), id_b, (size_t)n_tri * 4, hipMemcpyDeviceToHost, st));
    QF_HIP_TRY(timer.mark(st));

    // ---- pass 4: topology, level by level ----
    hipLaunchKernelGGL(init_root_kernel, dim3(1), dim3(1), 0, st, rg_cur, (int)n_tri);
    QF_LAUNCH_CHECK();
    bvh->level_start8.assign(1, 0);
    int64_t level_base = 0, n_level = 1;
    for (int level = 0;; ++level) {
        if (level >= kMaxLevels || level_base + n_level > capacity) return QF_ERR_UNSUPPORTED;     // cannot happen
        const unsigned blocks = (unsigned)qf_div_up(n_level, kBlock);
        hipLaunchKernelGGL(count_children_kernel, dim3(blocks), dim3(kBlock), 0, st, key_b, rg_cur, (int)n_level, d_cnt);
        QF_LAUNCH_CHECK();
        QF_HIP_TRY(rocprim::exclusive_scan(nullptr, tb, d_cnt, d_off, 0, (size_t)n_level, rocprim::plus<int32_t>(), st));
        if (tb > temp_bytes) return QF_ERR_UNSUPPORTED;
        QF_HIP_TRY(rocprim::exclusive_scan(d_temp, tb, d_cnt, d_off, 0, (size_t)n_level, rocprim::plus<int32_t>(), st));
        hipLaunchKernelGGL(emit_level_kernel, dim3(blocks), dim3(kBlock), 0, st, key_b, rg_cur, d_cnt, d_off, (int)n_level,
                           (int)level_base, (int)capacity, reinterpret_cast<float4 *>(bvh->d_nodes8), rg_next, d_next);
        QF_LAUNCH_CHECK();
        int32_t next = 0;
        QF_HIP_TRY(hipMemcpyAsync(&next, d_next, 4, hipMemcpyDeviceToHost, st));
        QF_HIP_TRY(hipStreamSynchronize(st));
        level_base += n_level;
        bvh->level_start8.push_back((int32_t)level_base);
        if (next <= 0) break;
        n_level = next;
        int2 *t = rg_cur; rg_cur = rg_next; rg_next = t;
    }
    bvh->n_nodes8 = level_base;
    const int levels = (int)bvh->level_start8.size() - 1;
    bvh->max_depth = levels;
    QF_HIP_TRY(timer.mark(st));

    // ---- pass 5: boxes; pass 6: the stack bound ----
    if (int rc = qf_bvh_refit_boxes(bvh, bvh->eps, st)) return rc;
    QF_HIP_TRY(timer.mark(st));
    for (int l = levels - 1; l >= 0; --l) {
        const int n0 = bvh->level_start8[(size_t)l], n1 = bvh->level_start8[(size_t)l + 1];
        hipLaunchKernelGGL(stack_level_kernel, dim3((unsigned)qf_div_up(n1 - n0, kBlock)), dim3(kBlock), 0, st, bvh->d_nodes8, n0, n1, d_need);
        QF_LAUNCH_CHECK();
    }
    int32_t need0 = 0;
    QF_HIP_TRY(hipMemcpyAsync(&need0, d_need, 4, hipMemcpyDeviceToHost, st));
    QF_HIP_TRY(timer.mark(st));
    QF_HIP_TRY(hipStreamSynchronize(st));
    bvh->max_stack8 = (need0 > 1 ? need0 : 1) + 1;
    if (pass_ms)
        for (int k = 0; k < QF_BVH_BUILD_PASSES; ++k) QF_HIP_TRY(hipEventElapsedTime(&pass_ms[k], timer.ev[k], timer.ev[k + 1]));
    if (bvh->max_stack8 > QF_BVH8_MAX_STACK) return QF_ERR_UNSUPPORTED;     // cannot happen; the guard frees
    bvh->chunk_dirty = true;
    *out = bvh;
    guard.bvh = nullptr;
    return QF_OK;
}

}  // namespace

extern "C" int qf_bvh_create_device_timed(const float *d_tri_verts, int64_t n_tri, void *stream, float *pass_ms,
                                          int64_t *peak_bytes, qf_bvh **out)
{
    if (!out || n_tri < 0 || n_tri >= (1 << 28) || (n_tri > 0 && !d_tri_verts)) return QF_ERR_INVALID_ARGUMENT;
    return build_device(d_tri_verts, n_tri, qf_stream(stream), pass_ms, peak_bytes, out);
}

extern "C" int qf_bvh_create_device(const float *d_tri_verts, int64_t n_tri, void *stream, qf_bvh **out)
{
    return qf_bvh_create_device_timed(d_tri_verts, n_tri, stream, nullptr, nullptr, out);
}
