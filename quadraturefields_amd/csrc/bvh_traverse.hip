// The general multi-hit intersector: 8-wide BVH traversal, eight lanes per ray, and the repair pass that re-runs it
// for the rays the camera-coherent passes (raster.hip) could not finish.
#include "exact_common.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Wide-BVH multi-hit traversal: EIGHT LANES PER RAY.  A node of the 8-wide tree (bvh.h) is 8 children x 32 B; lane j of
// a ray's octet loads child j (the octet reads the node's 256 contiguous bytes), tests its box, and the octet's hit
// mask comes out of one ballot.  A leaf holds up to 8 triangles: lane j runs the exact test on triangle j.  So one
// dependent step decides 8 boxes or 8 triangles (the binary one-ray-per-lane walk of round 1 needed ~3 dependent node
// fetches for the same decision and kept a 64-entry stack per LANE in scratch), a wave carries 8 rays instead of 64 --
// eight times the waves for the same batch, which is what a latency-bound walk over a 2^17-ray training batch lacks --
// and the per-ray state (stack, K-list) lives in LDS, shared by the octet:
//   * stack: tokens of the hit children not taken yet; the nearest hit child is taken next (DPP min over the octet);
//     the capacity is the tree's exact bound, computed by the builder (qf_bvh::max_stack8);
//   * K-list: 64-bit (t, tri) keys, unordered while there is room, then K-nearest replacement with the worst entry
//     found by the octet together; t_limit = the worst entry's t prunes boxes;
//   * at the end the octet rank-sorts the list (each lane ranks every 8th entry) and writes the row ascending.
// min_sep > 0 adds the reference's multi-hit rule (trimesh 3.23.5 ray_pyembree.intersects_id, called at
// examples/mesh_utils.py:350-354): after a kept hit at t_prev the ray is re-originated min_sep past it, so the next
// kept hit is the first with t > t_prev + min_sep -- hits closer than that, and the second copy of a duplicated face,
// are never returned.  The chain runs over the sorted list; when the K-list was full and the chain kept fewer than K
// the traversal runs again for the hits beyond the page (lower bound = the page's last key), until K are kept or a
// page comes back not full.
constexpr int kOctRays = 32;                    // rays per workgroup: 256 threads = 4 waves x 8 octets
constexpr int kTravThreads = kOctRays * 8;
constexpr int kDone = (int)0x80000000;          // == QF_BVH8_EMPTY; no leaf token takes this value (n_tri < 2^28)
constexpr int kMaxPages = 4096;

#define QF_DPP_QUAD_1032 0xB1
#define QF_DPP_QUAD_2301 0x4E
#define QF_DPP_HALF_MIRROR 0x141

__device__ __forceinline__ unsigned oct_min_u32(unsigned v)
{
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_QUAD_1032, 0xf, 0xf, true));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_QUAD_2301, 0xf, 0xf, true));
    v = min(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_HALF_MIRROR, 0xf, 0xf, true));
    return v;
}
__device__ __forceinline__ unsigned oct_max_u32(unsigned v)
{
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_QUAD_1032, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_QUAD_2301, 0xf, 0xf, true));
    v = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, QF_DPP_HALF_MIRROR, 0xf, 0xf, true));
    return v;
}
template <int kCtrl>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, kCtrl, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), kCtrl, 0xf, 0xf, true);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t oct_max_u64(uint64_t v)
{
    uint64_t o = dpp_u64<QF_DPP_QUAD_1032>(v); v = o > v ? o : v;
    o = dpp_u64<QF_DPP_QUAD_2301>(v); v = o > v ? o : v;
    o = dpp_u64<QF_DPP_HALF_MIRROR>(v); v = o > v ? o : v;
    return v;
}
// value of lane `src` (0..7) of this octet
__device__ __forceinline__ int oct_bcast(int v, int oct_base, int src)
{
    return __builtin_amdgcn_ds_bpermute((oct_base + src) << 2, v);
}
// LDS written by one lane of the octet is read by the others: same wave, LDS operations complete in order; this only
// keeps the compiler from moving them across each other
__device__ __forceinline__ void oct_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

struct OctList {
    uint64_t *keys;      // [K] in LDS
    int K, j;
    int count;           // entries in keys (octet-uniform)
    uint64_t worst;      // valid when count == K: the largest key, at worst_slot
    int worst_slot;

    __device__ __forceinline__ void find_worst()
    {
        uint64_t m = 0;
        int slot = 0;
        for (int i = j; i < K; i += 8) {
            const uint64_t k = keys[i];
            if (k >= m) { m = k; slot = i; }
        }
        worst = oct_max_u64(m);
        worst_slot = (int)oct_max_u32(m == worst ? (unsigned)slot : 0u);     // keys are unique: one lane holds it
    }
};

struct TravArgs {
    const float4 *nodes, *tris;
    const float *rays_o, *rays_d;
    int64_t n_rays;
    int root_is_valid, max_hits, image_width, image_height, tiles_x, n_blocks, blocks_per_xcd, stack_cap;
    int stripe_blocks;           // > 0: image-shaped launch, blocks per stripe of the XCD comb (see xcd_block)
    int list_cap;                // entries of the LDS K-list: max_hits, or a few more when the re-origin rule is on
    float min_sep;
    int32_t *hit_tri;
    float *hit_t;
    int32_t *hit_count;
    uint64_t *keep_mask;         // repair launch only (see bvh8_repair_kernel)
    int32_t *raw_count;
    int tcol_offset;             // repair launch: float offset of the [K][256] distance columns in the LDS
    const int32_t *all_flag;     // repair launch, or NULL: *all_flag != 0 -> EVERY ray is traversed (camera_rays_check)
};

// LDS of a workgroup: [kOctRays][K] keys | [kOctRays][K] sorted (only when min_sep > 0) | [kOctRays][stack_cap] stack
extern __shared__ uint64_t trav_lds[];

// The re-origin rule for a ray whose complete, unordered list (c <= K entries) is in hit_t / hit_tri, WITHOUT rewriting
// the list: bit i of the result = the i-th hit in (t, tri) order is kept.  Octet-uniform; *kept_out = number kept.
__device__ __forceinline__ uint64_t oct_keep_mask(const TravArgs &a, int64_t ray, int c, int j, int q, int *kept_out)
{
    const int K = a.max_hits, Kc = a.list_cap;
    uint64_t *keys = trav_lds + (size_t)q * Kc;
    uint64_t *sorted = trav_lds + (size_t)kOctRays * Kc + (size_t)q * Kc;
    for (int e = j; e < c; e += 8) keys[e] = hit_key(a.hit_t[ray * K + e], a.hit_tri[ray * K + e]);
    oct_lds_sync();
    for (int e = j; e < c; e += 8) {
        const uint64_t k = keys[e];
        int rank = 0;
        for (int i = 0; i < c; ++i) rank += keys[i] < k ? 1 : 0;
        sorted[rank] = k;
    }
    oct_lds_sync();
    float last = key_t(sorted[0]);
    int kept = 1;
    uint64_t mask = 1ull;
    for (int i = 1; i < c; ++i) {
        const float t = key_t(sorted[i]);
        if (t > last + a.min_sep) { mask |= 1ull << i; ++kept; last = t; }
    }
    oct_lds_sync();
    *kept_out = kept;
    return mask;
}

// One ray, traversed by the 8 lanes of an octet (j = lane in the octet, q = the octet's LDS slot in the workgroup).
// kOrdered: the nearest hit child is taken next (octet-wide DPP minimum), so that a full K-list's t_limit prunes the boxes
// behind it.  false: the first hit child in slot order -- on a scene whose rays meet far fewer than K triangles the lists
// (almost) never fill, nothing is pruned whatever the order, and the minimum is pure cost (round 4: frame 0.961 -> 0.917
// ms, 2^17 random rays 0.549 -> 0.528).  The hits found are the same either way; bvh_launch picks by the mesh's depth
// complexity.
template <bool kOrdered>
__device__ __forceinline__ void oct_traverse_ray(const TravArgs &ta, int64_t ray, int j, int q, int oct_base)
{
    const int K = ta.max_hits;
    // With the re-origin rule on the list holds a few more than K entries: the chain usually drops a hit or two (a
    // grazing ray crosses a shell twice within min_sep), and with exactly K collected every drop would cost another
    // whole traversal for the next page.
    const int Kc = ta.list_cap;
    const float min_sep = ta.min_sep;
    const float4 *__restrict__ nodes = ta.nodes;
    const float4 *__restrict__ tris = ta.tris;
    const int stack_cap = ta.stack_cap;
    uint64_t *keys = trav_lds + (size_t)q * Kc;
    uint64_t *sorted = trav_lds + (size_t)kOctRays * Kc + (size_t)q * Kc;        // only when min_sep > 0
    int *stack = reinterpret_cast<int *>(trav_lds + (size_t)kOctRays * Kc * (min_sep > 0.0f ? 2 : 1)) + (size_t)q * stack_cap;
    const float *rays_o = ta.rays_o, *rays_d = ta.rays_d;
    const int root_is_valid = ta.root_is_valid;
    float *hit_t = ta.hit_t;
    int32_t *hit_tri = ta.hit_tri, *hit_count = ta.hit_count;
    uint64_t *keep_mask = ta.keep_mask;
    int32_t *raw_count = ta.raw_count;
    const float ox = rays_o[ray * 3], oy = rays_o[ray * 3 + 1], oz = rays_o[ray * 3 + 2];
    const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
    const float ix = safe_inv(dx), iy = safe_inv(dy), iz = safe_inv(dz);
    const float nx = -(ox * ix), ny = -(oy * iy), nz = -(oz * iz);
    float *my_t = hit_t + ray * K;
    int32_t *my_tri = hit_tri + ray * K;

    OctList list;
    list.keys = keys; list.K = Kc; list.j = j;
    int kept = 0;                    // hits written so far (min_sep chain)
    float last_t = 0.0f;             // t of the last kept hit
    uint64_t lo_key = 0;             // page lower bound: only keys > lo_key are collected
    float t_lo = 0.0f, t_accept = 0.0f;      // box pruning below the page / hits the chain would drop anyway

    for (int page = 0; page < kMaxPages; ++page) {
        list.count = 0;
        list.worst = ~0ull;
        list.worst_slot = 0;
        float t_limit = INFINITY;
        int sp = 0;
        int cur = root_is_valid ? 0 : kDone;
        while (cur != kDone) {
            while (cur >= 0) {
                const float4 *np = nodes + (size_t)cur * 16 + j * 2;
                const float4 a = np[0];                 // lo.xyz, hi.x
                const float4 b = np[1];                 // hi.yz, token, 0
                const float ax = __builtin_fmaf(a.x, ix, nx), bx = __builtin_fmaf(a.w, ix, nx);
                const float ay = __builtin_fmaf(a.y, iy, ny), by = __builtin_fmaf(b.x, iy, ny);
                const float az = __builtin_fmaf(a.z, iz, nz), bz = __builtin_fmaf(b.y, iz, nz);
                const float tn = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), 0.0f));
                const float tf = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)) * 1.0000005f;
                const int tok = __float_as_int(b.z);
                // conservative: the boxes were inflated on the host, the exit distance is widened, NaN counts as a hit
                const bool hit = tok != kDone && !(tn > tf) && !(tn * 0.999999f > t_limit) && !(tf < t_lo);
                const unsigned m8 = (unsigned)(__ballot(hit) >> oct_base) & 0xffu;
                if (m8 == 0) {
                    cur = kDone;
                    if (sp > 0) cur = stack[--sp];
                    continue;
                }
                const int n = __popc(m8);
                int nearest;
                if (kOrdered) {
                    const unsigned key = hit ? ((__float_as_uint(tn) & ~7u) | (unsigned)j) : 0xffffffffu;
                    nearest = (int)(oct_min_u32(key) & 7u);
                } else {
                    nearest = __ffs(m8) - 1;
                }
                if (hit && j != nearest) {
                    const unsigned others = m8 & ~(1u << nearest);
                    stack[sp + __popc(others & ((1u << j) - 1u))] = tok;
                }
                sp += n - 1;
                cur = oct_bcast(tok, oct_base, nearest);
                oct_lds_sync();
            }
            if (cur == kDone) break;
            {
                const int packed = ~cur;
                const int first = packed >> 3, cnt = (packed & 7) + 1;
                bool h = false;
                uint64_t key = 0;
                if (j < cnt) {
                    const float4 a = tris[(size_t)(first + j) * 3 + 0];
                    const float4 b = tris[(size_t)(first + j) * 3 + 1];
                    const float4 c = tris[(size_t)(first + j) * 3 + 2];
                    float t;
                    if (mt_hit(a, b, c, ox, oy, oz, dx, dy, dz, &t)) {
                        key = hit_key(t, __float_as_int(a.w));
                        h = key > lo_key && t > t_accept && key < list.worst;
                    }
                }
                const unsigned m8 = (unsigned)(__ballot(h) >> oct_base) & 0xffu;
                if (m8) {
                    const int n = __popc(m8);
                    if (list.count + n <= Kc) {
                        if (h) keys[list.count + __popc(m8 & ((1u << j) - 1u))] = key;
                        list.count += n;
                        oct_lds_sync();
                        if (list.count == Kc) list.find_worst();
                    } else {                                    // the list fills up or is full: one hit at a time
                        for (unsigned mm = m8; mm; mm &= mm - 1u) {
                            const int src = __ffs(mm) - 1;
                            const uint64_t k = ((uint64_t)(unsigned)oct_bcast((int)(unsigned)(key >> 32), oct_base, src) << 32) |
                                               (unsigned)oct_bcast((int)(unsigned)key, oct_base, src);
                            if (list.count < Kc) {
                                if (j == 0) keys[list.count] = k;
                                ++list.count;
                                oct_lds_sync();
                                if (list.count == Kc) list.find_worst();
                            } else if (k < list.worst) {
                                if (j == 0) keys[list.worst_slot] = k;
                                oct_lds_sync();
                                list.find_worst();
                            }
                        }
                    }
                    if (list.count == Kc) t_limit = key_t(list.worst);
                }
            }
            cur = kDone;
            if (sp > 0) cur = stack[--sp];
        }

        // rank sort of the page: lane j ranks entries j, j+8, ... (keys are unique, so the ranks are a permutation)
        const int count = list.count;
        if (!(min_sep > 0.0f)) {
            for (int e = j; e < count; e += 8) {
                const uint64_t k = keys[e];
                int rank = 0;
                for (int i = 0; i < count; ++i) rank += keys[i] < k ? 1 : 0;
                my_t[rank] = key_t(k);
                my_tri[rank] = key_id(k);
            }
            kept = count;
            break;
        }
        for (int e = j; e < count; e += 8) {
            const uint64_t k = keys[e];
            int rank = 0;
            for (int i = 0; i < count; ++i) rank += keys[i] < k ? 1 : 0;
            sorted[rank] = k;
        }
        oct_lds_sync();
        // the re-origin chain, front to back (octet-uniform; lane 0 writes)
        for (int i = 0; i < count && kept < K; ++i) {
            const uint64_t k = sorted[i];
            const float t = key_t(k);
            if (kept == 0 || t > last_t + min_sep) {
                if (j == 0) { my_t[kept] = t; my_tri[kept] = key_id(k); }
                ++kept;
                last_t = t;
            }
        }
        if (count < Kc || kept >= K) break;         // every hit of the ray has been seen, or K are kept
        lo_key = sorted[Kc - 1];
        t_lo = key_t(lo_key) * 0.999999f;
        t_accept = last_t + min_sep;                // anything closer is dropped by the chain whatever follows
        oct_lds_sync();
    }
    for (int i = kept + j; i < K; i += 8) { my_t[i] = INFINITY; my_tri[i] = -1; }
    if (j == 0) {
        hit_count[ray] = kept;
        if (keep_mask) { keep_mask[ray] = kept >= 64 ? ~0ull : ((1ull << kept) - 1ull); raw_count[ray] = kept; }
    }
}

// XCD-aware block order: hardware deals workgroups round-robin to the 8 XCDs (private L2 each).  A plain batch: XCD x
// walks the x-th CONTIGUOUS eighth of the blocks (one slice of the batch), so its L2 only has to hold that slice's part
// of the tree.  An image: contiguous eighths are row bands, and the object sits in the middle ones -- the XCDs of the
// top and bottom bands idle while two XCDs carry the frame (PMC: one resident wave per SIMD on average).  So the image
// is dealt in STRIPES of two tile rows (8 pixel rows): stripe s goes to XCD s % 8, every XCD gets a comb over the whole
// image (balanced), and consecutive blocks of an XCD are still neighbouring tiles of one stripe (L2-friendly).
__device__ __forceinline__ int xcd_block(const TravArgs &a)
{
    const int x = (int)(blockIdx.x & 7), k = (int)(blockIdx.x >> 3);
    if (a.stripe_blocks > 0) {
        const int s = k / a.stripe_blocks, p = k - s * a.stripe_blocks;
        return (s * 8 + x) * a.stripe_blocks + p;
    }
    return x * a.blocks_per_xcd + k;
}

// Every ray of the batch: a workgroup = 32 rays (image-shaped batches: 8x4 pixels, a wave = 4x2 pixels).
template <bool kOrdered>
__global__ __launch_bounds__(kTravThreads) void bvh8_traverse_kernel(TravArgs a)
{
    const int tid = threadIdx.x, j = tid & 7, q = tid >> 3;
    const int oct_base = (tid & 63) & 56;               // first lane of this octet within its wave
    const int block = xcd_block(a);
    if (block >= a.n_blocks) return;
    int64_t ray;
    if (a.image_width > 0) {
        const int w = q >> 3, r = q & 7;
        const int px = (block % a.tiles_x) * 8 + (w & 1) * 4 + (r & 3);
        const int py = (block / a.tiles_x) * 4 + (w >> 1) * 2 + (r >> 2);
        if (px >= a.image_width || py >= a.image_height) return;
        ray = (int64_t)py * a.image_width + px;
    } else {
        ray = (int64_t)block * kOctRays + q;
    }
    if (ray >= a.n_rays) return;
    oct_traverse_ray<kOrdered>(a, ray, j, q, oct_base);
}

// The repair pass after the camera-coherent intersector: only the rays whose candidate list overflowed (count > K) are
// traversed.  With keep_mask (and min_sep > 0) the same launch decides the re-origin rule for every OTHER ray's
// complete, unordered list without rewriting it (oct_keep_mask): keep_mask[ray], raw_count[ray] = the length of the
// stored list, hit_count[ray] = the number kept -- qf_pack_samples sorts the list the same way and drops the masked
// entries.  A workgroup owns 256 consecutive rays: one lane per ray classifies them (coalesced count reads; rays with
// fewer than two hits are finished here), the rays that need an octet are compacted into an LDS list, and the
// workgroup's 32 octets work that list off -- no octet idles on a background ray.
__global__ __launch_bounds__(kTravThreads) void bvh8_repair_kernel(TravArgs a)
{
    __shared__ int s_list[kTravThreads];
    __shared__ int s_n;
    const int tid = threadIdx.x, j = tid & 7, q = tid >> 3;
    const int oct_base = (tid & 63) & 56;
    const int block = (int)blockIdx.x;          // consecutive blocks on different XCDs: the work (object rays) is spread evenly
    if (block >= a.n_blocks) return;
    const int K = a.max_hits;
    if (tid == 0) s_n = 0;
    __syncthreads();
    const int64_t ray0 = (int64_t)block * kTravThreads;
    {
        const int64_t ray = ray0 + tid;
        if (ray < a.n_rays) {
            const int c = a.hit_count[ray];
            int need = 0;
            // all_flag raised: the rays were not the camera's pixel grid, the camera-coherent passes returned at once and
            // the lists are empty -- this launch IS the intersection then, exact for any rays
            if (c > K || (a.all_flag && *a.all_flag)) need = 2;
            else if (a.keep_mask) {
                // The rule can only drop a hit if two of the ray's hits lie within min_sep of each other.  One lane
                // tests that on the distances alone -- no sort: with no such pair every hit is kept whatever the order
                // -- and only the (rare) rays with a close pair go to an octet for the sorted chain.  The margin covers
                // the rounding of the chain's fp32 addition, so "no close pair" can never hide a drop.
                bool close_pair = false;
                if (c >= 2) {
                    const float *row = a.hit_t + ray * K;
                    float *col = reinterpret_cast<float *>(trav_lds) + a.tcol_offset + tid;      // [K][kTravThreads]
                    for (int i0 = 0; i0 < c; i0 += 8) {
                        float v[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) v[u] = (i0 + u < c) ? row[i0 + u] : 0.0f;
#pragma unroll
                        for (int u = 0; u < 8; ++u)
                            if (i0 + u < c) col[(i0 + u) * kTravThreads] = v[u];
                    }
                    const float ms = a.min_sep * 1.0001f;
                    for (int i = 1; i < c; ++i) {
                        const float ti = col[i * kTravThreads];
                        for (int k = 0; k < i; ++k) {
                            const float tk = col[k * kTravThreads];
                            close_pair |= !(fabsf(ti - tk) > ms + 4e-7f * fmaxf(ti, tk));
                        }
                    }
                }
                if (close_pair) need = 1;
                else { a.keep_mask[ray] = c >= 64 ? ~0ull : ((1ull << c) - 1ull); a.raw_count[ray] = c; }
            }
            if (need) s_list[atomicAdd(&s_n, 1)] = tid | (need << 16);
        }
    }
    __syncthreads();
    const int n = s_n;
    for (int e = q; e < n; e += kOctRays) {
        const int entry = s_list[e];
        const int64_t ray = ray0 + (entry & 0xffff);
        if ((entry >> 16) == 2) {
            oct_traverse_ray<true>(a, ray, j, q, oct_base);      // the rays that overflowed K: their lists DO fill
        } else {
            const int c = a.hit_count[ray];
            int kept;
            const uint64_t mask = oct_keep_mask(a, ray, c, j, q, &kept);
            if (j == 0) { a.keep_mask[ray] = mask; a.raw_count[ray] = c; a.hit_count[ray] = kept; }
        }
    }
}

}  // namespace

static int bvh_launch(const qf_bvh *bvh, const float *rays_o, const float *rays_d, int64_t n_rays, int32_t max_hits,
                      int32_t image_width, int32_t *hit_tri, float *hit_t, int32_t *hit_count, int only_overflowed,
                      uint64_t *keep_mask, int32_t *raw_count, void *stream, const int32_t *all_flag = nullptr)
{
    if (!bvh || n_rays < 0 || max_hits < 1 || max_hits > kMaxHits || image_width < 0) return QF_ERR_INVALID_ARGUMENT;
    if (bvh->n_tri >= (1 << 28)) return QF_ERR_UNSUPPORTED;      // leaf tokens of the traversal pack (first, count)
    if (n_rays == 0) return QF_OK;
    if (!rays_o || !rays_d || !hit_tri || !hit_t || !hit_count) return QF_ERR_INVALID_ARGUMENT;
    int height = 0, tiles_x = 0;
    int64_t n_blocks = qf_div_up(n_rays, kOctRays);
    if (image_width > 0) {
        if (n_rays % image_width) return QF_ERR_INVALID_ARGUMENT;
        height = (int)(n_rays / image_width);
        tiles_x = (image_width + 7) / 8;
        n_blocks = (int64_t)tiles_x * ((height + 3) / 4);
    }
    const bool sep = bvh->min_sep > 0.0f;
    const int stack_cap = (bvh->max_stack8 < 2 ? 2 : bvh->max_stack8) | 1;       // odd row stride
    // headroom only in the repair launch (dense scenes: every traversed ray fills its list); the all-rays traversal
    // keeps the smaller LDS footprint (measured: +6 % on a frame, +8 % on a training batch with the headroom)
    const int list_cap = (sep && only_overflowed) ? (max_hits + 8 < kMaxHits ? max_hits + 8 : kMaxHits) : max_hits;
    size_t lds = (size_t)kOctRays * ((size_t)list_cap * 8 * (sep ? 2 : 1) + (size_t)stack_cap * 4);
    const size_t tcol_offset = (lds + 3) / 4;
    if (only_overflowed && sep && keep_mask) lds = tcol_offset * 4 + (size_t)kTravThreads * max_hits * 4;   // distance columns
    if (lds > 160 * 1024 - 2048) return QF_ERR_UNSUPPORTED;
    TravArgs a;
    a.nodes = reinterpret_cast<const float4 *>(bvh->d_nodes8);
    a.tris = reinterpret_cast<const float4 *>(bvh->d_tris);
    a.rays_o = rays_o; a.rays_d = rays_d; a.n_rays = n_rays;
    a.root_is_valid = bvh->n_tri > 0 ? 1 : 0;
    a.max_hits = (int)max_hits; a.image_width = (int)image_width; a.image_height = height; a.tiles_x = tiles_x;
    a.stack_cap = stack_cap; a.list_cap = list_cap; a.min_sep = sep ? bvh->min_sep : 0.0f;
    a.hit_tri = hit_tri; a.hit_t = hit_t; a.hit_count = hit_count;
    a.keep_mask = (only_overflowed && sep) ? keep_mask : nullptr;
    a.raw_count = a.keep_mask ? raw_count : nullptr;
    a.tcol_offset = (int)tcol_offset;
    a.all_flag = only_overflowed ? all_flag : nullptr;
    if (only_overflowed) n_blocks = qf_div_up(n_rays, kTravThreads);        // 256 consecutive rays per workgroup
    int64_t per_xcd = qf_div_up(n_blocks, 8);
    a.stripe_blocks = 0;
    if (!only_overflowed) {
        // image: stripes of two tile rows; a large plain batch: stripes of 256 blocks (8 192 consecutive rays) -- it may well
        // be a row-major image handed over without its width, and contiguous eighths would be as lopsided as bands
        // (1.65 -> 1.01 ms for the bench frame); batches under 2^18 rays keep contiguous eighths (a 2^17-ray batch sorted
        // by camera and pixel: 0.42 ms contiguous, 0.63 ms in 64-block stripes)
        a.stripe_blocks = image_width > 0 ? tiles_x * 2 : 256;
        if (n_blocks < (int64_t)a.stripe_blocks * (image_width > 0 ? 16 : 32)) a.stripe_blocks = 0;
    }
    if (a.stripe_blocks > 0) {
        const int64_t stripes = qf_div_up(n_blocks, a.stripe_blocks);
        per_xcd = qf_div_up(stripes, 8) * a.stripe_blocks;
    }
    if (per_xcd * 8 > 0x7fffffff) return QF_ERR_UNSUPPORTED;
    a.n_blocks = (int)n_blocks; a.blocks_per_xcd = (int)per_xcd;
    // front-to-back order only pays when the K-lists fill: a mesh whose rays meet K/2 triangles or more on average
    const bool ordered = bvh->depth_complexity >= 0.5f * (float)max_hits;
    const void *fn = only_overflowed ? reinterpret_cast<const void *>(bvh8_repair_kernel)
                                     : (ordered ? reinterpret_cast<const void *>(bvh8_traverse_kernel<true>)
                                                : reinterpret_cast<const void *>(bvh8_traverse_kernel<false>));
    if (lds > 48 * 1024) QF_HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (only_overflowed)
        hipLaunchKernelGGL(bvh8_repair_kernel, dim3((unsigned)(per_xcd * 8)), dim3(kTravThreads), lds, qf_stream(stream), a);
    else if (ordered)
        hipLaunchKernelGGL(bvh8_traverse_kernel<true>, dim3((unsigned)(per_xcd * 8)), dim3(kTravThreads), lds, qf_stream(stream), a);
    else
        hipLaunchKernelGGL(bvh8_traverse_kernel<false>, dim3((unsigned)(per_xcd * 8)), dim3(kTravThreads), lds, qf_stream(stream), a);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_bvh_intersect(const qf_bvh *bvh, const float *rays_o, const float *rays_d, int64_t n_rays,
                                int32_t max_hits, int32_t image_width, int32_t *hit_tri, float *hit_t,
                                int32_t *hit_count, void *stream)
{
    return bvh_launch(bvh, rays_o, rays_d, n_rays, max_hits, image_width, hit_tri, hit_t, hit_count, 0, nullptr, nullptr,
                      stream);
}

extern "C" int qf_bvh_repair_overflow(const qf_bvh *bvh, const float *rays_o, const float *rays_d, int64_t n_rays,
                                      int32_t max_hits, int32_t image_width, int32_t *hit_tri, float *hit_t,
                                      int32_t *hit_count, uint64_t *keep_mask, int32_t *raw_count,
                                      const int32_t *traverse_all_flag, void *stream)
{
    if ((keep_mask == nullptr) != (raw_count == nullptr)) return QF_ERR_INVALID_ARGUMENT;
    return bvh_launch(bvh, rays_o, rays_d, n_rays, max_hits, image_width, hit_tri, hit_t, hit_count, 1, keep_mask, raw_count,
                      stream, traverse_all_flag);
}
