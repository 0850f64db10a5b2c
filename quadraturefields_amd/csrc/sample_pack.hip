// Per-ray hit lists -> packed samples sorted by (ray, depth): ray-major (pack_samples_kernel) or in the coherent tile
// order of a render-only frame (pack_tiles_kernel), and the per-ray re-sorts of packed samples by depth.
#include "exact_common.h"

#pragma clang fp contract(off)

namespace {

// The network itself: kN entries in registers ((t, tri) keys with ids, distances alone without), the first `cnt` of them
// live, sorted and left in the lane's LDS row.
template <int kN, bool kTri>
__device__ __forceinline__ void sort_to_row(float (&t)[kN], int32_t (&id)[kN], int cnt, float *row_t, int32_t *row_i)
{
    if (kTri) {
        uint64_t key[kN];
#pragma unroll
        for (int k = 0; k < kN; ++k) key[k] = k < cnt ? hit_key(t[k], id[k]) : ~0ull;
#pragma unroll
        for (int k = 2; k <= kN; k <<= 1) {
#pragma unroll
            for (int i = 0; i < kN; ++i) {
                const int l = i ^ (k - 1);
                if (l > i) { const uint64_t a = key[i], b = key[l]; key[i] = a < b ? a : b; key[l] = a < b ? b : a; }
            }
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
                for (int i = 0; i < kN; ++i) {
                    const int l = i ^ j;
                    if (l > i) { const uint64_t a = key[i], b = key[l]; key[i] = a < b ? a : b; key[l] = a < b ? b : a; }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kN; ++k)
            if (k < cnt) { row_t[k] = key_t(key[k]); row_i[k] = key_id(key[k]); }
    } else {
#pragma unroll
        for (int k = 0; k < kN; ++k) t[k] = k < cnt ? t[k] : INFINITY;
#pragma unroll
        for (int k = 2; k <= kN; k <<= 1) {
#pragma unroll
            for (int i = 0; i < kN; ++i) {
                const int l = i ^ (k - 1);
                if (l > i) { const float a = t[i], b = t[l]; t[i] = fminf(a, b); t[l] = fmaxf(a, b); }
            }
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
                for (int i = 0; i < kN; ++i) {
                    const int l = i ^ j;
                    if (l > i) { const float a = t[i], b = t[l]; t[i] = fminf(a, b); t[l] = fmaxf(a, b); }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < kN; ++k)
            if (k < cnt) row_t[k] = t[k];
    }
}

// The bitonic sort of sort_row_32 (exact_common.h) fed straight from global memory (the pack kernels): lane = ray reads
// ITS OWN list -- rows of K entries, four entries per request (f32x4u) -- into the network's registers, sorts, and leaves
// the sorted list in its LDS row for the loops that index it by rank.  Every load of the list is independent of the others, so the wave
// waits for memory once; the staged variant (coalesced loop -> LDS -> registers) waited once per loop iteration, which
// is what a tile wave's time was made of (one wave per tile, nothing to overlap with).  kN = 16 or 32: network size,
// picked per tile from its longest list.  `deepest` (wave-uniform) bounds what is read.
template <int kN, bool kTri>
__device__ __forceinline__ void load_sort_row(const float *__restrict__ g_t, const int32_t *__restrict__ g_i, int K,
                                              int cnt, int deepest, float *row_t, int32_t *row_i)
{
    float t[kN];
    int32_t id[kN];
#pragma unroll
    for (int j = 0; j < kN / 4; ++j) {
        f32x4u v = {INFINITY, INFINITY, INFINITY, INFINITY};
        i32x4u w = {-1, -1, -1, -1};
        if (4 * j < deepest) {                                  // wave-uniform; deepest <= K
            if (4 * j + 3 < K) {                                // the whole quartet lies inside the row: one request
                v = *reinterpret_cast<const f32x4u *>(g_t + 4 * j);
                if (kTri) w = *reinterpret_cast<const i32x4u *>(g_i + 4 * j);
            } else {                                            // the row's last 1..3 entries
#pragma unroll
                for (int e = 0; e < 3; ++e)
                    if (4 * j + e < K) {
                        v[e] = g_t[4 * j + e];
                        if (kTri) w[e] = g_i[4 * j + e];
                    }
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) { t[4 * j + e] = v[e]; id[4 * j + e] = w[e]; }
    }
    sort_to_row<kN, kTri>(t, id, cnt, row_t, row_i);
}

// A binned pixel's list (pack_tiles_kernel<kTri, true>): its `cnt` unordered entries are in its LDS row already, put
// there record by record; the same network sorts them in place.
template <int kN, bool kTri>
__device__ __forceinline__ void sort_row_in_place(int cnt, int deepest, float *row_t, int32_t *row_i)
{
    float t[kN];
    int32_t id[kN];
#pragma unroll
    for (int k = 0; k < kN; ++k) {
        t[k] = INFINITY;
        id[k] = -1;
        if (k < deepest && k < cnt) {                           // (k < deepest: wave-uniform, deepest <= K = the row's length)
            t[k] = row_t[k];
            if (kTri) id[k] = row_i[k];
        }
    }
    sort_to_row<kN, kTri>(t, id, cnt, row_t, row_i);
}

// sampling_raytrace_numpy (mesh_utils.py:359-387): per-ray hit lists (in ANY order) -> packed samples sorted by
// (ray, depth).  A workgroup owns 128 consecutive rays, i.e. one contiguous slice of every output array:
//   1. the rays' [K] rows of hit_t / hit_tri are loaded into LDS with coalesced reads;
//   2. lane = ray: in-LDS insertion sort by (t, tri) -- the intersector's pass order -- then the stable sort by the
//      float64 depth |o + t d - o| of mesh_utils.py:371-375 (a no-op unless rounding reverses two near-equal hits);
//      each (ray, rank) drops its id into a slot map of the slice;
//   3. lane = output sample: coalesced writes of the six sample arrays.
constexpr int kPackRays = 128;

__device__ __forceinline__ double sample_depth64(float t, const double o[3], const double d[3], double p[3])
{
    const double td = (double)t;
    p[0] = o[0] + td * d[0];
    p[1] = o[1] + td * d[1];
    p[2] = o[2] + td * d[2];
    const double qx = p[0] - o[0], qy = p[1] - o[1], qz = p[2] - o[2];
    return sqrt((qx * qx + qy * qy) + qz * qz);      // np.linalg.norm(points - origins, axis=1)
}

__global__ __launch_bounds__(kPackRays) void pack_samples_kernel(
    const float *__restrict__ rays_o, const float *__restrict__ rays_d, int64_t n_rays, int max_hits,
    const int32_t *__restrict__ hit_tri, const float *__restrict__ hit_t, const int32_t *__restrict__ hit_count,
    const int64_t *__restrict__ ray_offset, float *__restrict__ xyz, float *__restrict__ dirs,
    int64_t *__restrict__ index_ray, float *__restrict__ depth, int64_t *__restrict__ index_tri,
    float *__restrict__ origins, const int32_t *__restrict__ inverse, float *__restrict__ xyz_c,
    float *__restrict__ dirs_c, float *__restrict__ depth_c, const uint64_t *__restrict__ keep_mask,
    const int32_t *__restrict__ raw_count, float min_sep, int32_t *__restrict__ close_flag)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = max_hits, Kp = max_hits | 1;            // odd row stride: conflict-free column access
    float *s_t = reinterpret_cast<float *>(smem);
    int32_t *s_tri = reinterpret_cast<int32_t *>(s_t + kPackRays * Kp);
    uint16_t *s_map = reinterpret_cast<uint16_t *>(s_tri + kPackRays * Kp);
    __shared__ int s_region;

    const int tid = threadIdx.x;
    const int64_t ray0 = (int64_t)blockIdx.x * kPackRays;
    const int nr = (int)((n_rays - ray0) < kPackRays ? (n_rays - ray0) : kPackRays);
    int cnt = 0;
    if (tid < nr) {
        cnt = keep_mask ? raw_count[ray0 + tid] : hit_count[ray0 + tid];
        if (cnt > K) cnt = K;
    }
    if (K <= 32) {
        // lane = ray reads its own list into registers, sorts it by (t, tri) and leaves it in its LDS row (load_sort_row):
        // one memory wait per wave instead of one per iteration of a staging loop
        int deepest = cnt;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const int other = __shfl_xor(deepest, off, 64);
            deepest = other > deepest ? other : deepest;
        }
        const int64_t own = tid < nr ? ray0 + tid : ray0;
        if (deepest > 16) load_sort_row<32, true>(hit_t + own * K, hit_tri + own * K, K, cnt, deepest, s_t + tid * Kp, s_tri + tid * Kp);
        else if (deepest > 0) load_sort_row<16, true>(hit_t + own * K, hit_tri + own * K, K, cnt, deepest, s_t + tid * Kp, s_tri + tid * Kp);
    } else {
        for (int i = tid; i < nr * K; i += kPackRays) {
            const int r = i / K, k = i - r * K;
            s_t[r * Kp + k] = hit_t[ray0 * K + i];
            s_tri[r * Kp + k] = hit_tri[ray0 * K + i];
        }
    }
    if (tid == 0) s_region = 0;
    __syncthreads();

    const int64_t block_base = ray_offset[ray0];
    if (tid < nr) {
        const int64_t ray = ray0 + tid;
        float *row_t = s_t + tid * Kp;
        int32_t *row_i = s_tri + tid * Kp;
        if (K > 32) {                                         // (t, tri) ascending; K <= 32 is sorted already
            for (int i = 1; i < cnt; ++i) {
                const float t = row_t[i];
                const int id = row_i[i];
                int j = i - 1;
                while (j >= 0 && hit_less(t, id, row_t[j], row_i[j])) { row_t[j + 1] = row_t[j]; row_i[j + 1] = row_i[j]; --j; }
                row_t[j + 1] = t;
                row_i[j + 1] = id;
            }
        }
        if (keep_mask) {                                      // the re-origin rule, decided by qf_bvh_repair_overflow
            const uint64_t mask = keep_mask[ray];
            int kept = 0;
            for (int i = 0; i < cnt; ++i)
                if ((mask >> i) & 1ull) { row_t[kept] = row_t[i]; row_i[kept] = row_i[i]; ++kept; }
            cnt = kept;
        } else if (close_flag && min_sep > 0.0f) {
            // optimistic route: the lists were packed as if the rule dropped nothing; here, with the list sorted, that
            // is checked exactly (the chain drops a hit iff some hit is not more than min_sep behind its predecessor).
            // A violation raises the frame's flag: the host then decides the rule per ray (keep_mask) and packs again.
            bool drop = false;
            for (int i = 1; i < cnt; ++i) drop |= !(row_t[i] > row_t[i - 1] + min_sep);
            if (drop) *close_flag = 1;
        }
        if (cnt > 1) {
            const double o64[3] = {(double)rays_o[ray * 3], (double)rays_o[ray * 3 + 1], (double)rays_o[ray * 3 + 2]};
            const double d64[3] = {(double)rays_d[ray * 3], (double)rays_d[ray * 3 + 1], (double)rays_d[ray * 3 + 2]};
            double p[3];
            double prev = sample_depth64(row_t[0], o64, d64, p);
            bool sorted = true;
            for (int k = 1; k < cnt; ++k) {
                const double dk = sample_depth64(row_t[k], o64, d64, p);
                sorted = sorted && !(prev > dk);
                prev = dk;
            }
            if (!sorted) {                                     // rare: stable insertion by depth, depths recomputed
                for (int i = 1; i < cnt; ++i) {
                    const float t = row_t[i];
                    const int id = row_i[i];
                    const double di = sample_depth64(t, o64, d64, p);
                    int j = i - 1;
                    while (j >= 0 && sample_depth64(row_t[j], o64, d64, p) > di) { row_t[j + 1] = row_t[j]; row_i[j + 1] = row_i[j]; --j; }
                    row_t[j + 1] = t;
                    row_i[j + 1] = id;
                }
            }
        }
        const int local = (int)(ray_offset[ray] - block_base);
        for (int k = 0; k < cnt; ++k) s_map[local + k] = (uint16_t)((tid << 8) | k);
        if (tid == nr - 1) s_region = local + cnt;
    }
    __syncthreads();

    const int region = s_region;
    for (int j = tid; j < region; j += kPackRays) {
        const int m = s_map[j];
        const int rl = m >> 8, k = m & 255;
        const int64_t ray = ray0 + rl;
        const float ox = rays_o[ray * 3], oy = rays_o[ray * 3 + 1], oz = rays_o[ray * 3 + 2];
        const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
        const double o64[3] = {(double)ox, (double)oy, (double)oz};
        const double d64[3] = {(double)dx, (double)dy, (double)dz};
        double p[3];
        const double dep = sample_depth64(s_t[rl * Kp + k], o64, d64, p);
        // vectors / (|vectors| + 1e-7) in float32 (mesh_utils.py:369-370)
        const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz) + 1e-7f;
        const int64_t o = block_base + j;
        if (xyz) {              // the ray-major position / direction / origin arrays are optional (see qf_hip.h)
            xyz[o * 3 + 0] = (float)p[0];
            xyz[o * 3 + 1] = (float)p[1];
            xyz[o * 3 + 2] = (float)p[2];
            dirs[o * 3 + 0] = dx / nrm;
            dirs[o * 3 + 1] = dy / nrm;
            dirs[o * 3 + 2] = dz / nrm;
            origins[o * 3 + 0] = ox;
            origins[o * 3 + 1] = oy;
            origins[o * 3 + 2] = oz;
        }
        index_ray[o] = ray;
        depth[o] = (float)dep;
        index_tri[o] = (int64_t)s_tri[rl * Kp + k];
        if (inverse) {          // a second copy at the sample's place in the field kernel's processing order
            const int64_t c = inverse[o];
            xyz_c[c * 3 + 0] = (float)p[0];
            xyz_c[c * 3 + 1] = (float)p[1];
            xyz_c[c * 3 + 2] = (float)p[2];
            dirs_c[c * 3 + 0] = dx / nrm;
            dirs_c[c * 3 + 1] = dy / nrm;
            dirs_c[c * 3 + 2] = dz / nrm;
            if (depth_c) depth_c[c] = (float)dep;
        }
    }
}

// The same packing for a frame that is only going to be RENDERED (row-major width x height image, no ray-major
// arrays wanted): one wave per 8x8 pixel tile, lane = pixel.  The tile's hit lists are staged and sorted exactly as in
// pack_samples_kernel (same comparisons, same re-origin handling, same float64 depth order); then step k writes the
// rank-k samples of the tile's pixels -- position, direction, depth -- at tile_base[tile] + (slots of the ranks
// before) + (pixels before this one that also have a rank-k hit): the coherent order of qf_coherent_layout, produced
// by the ballots directly, so neither the order, nor its inverse, nor index_ray / index_tri / ray-major depths exist
// for such a frame.  Values are pack_samples_kernel's bit for bit (tests).
// kBins (qf_pack_tiles_bins, K <= 32): the lists come from the tile's hit bin (qf_raster_intersect_tiles) -- one dense run
// of min(tile_cursor, 64 K) records, dealt to the pixels' LDS rows by the pixel-in-tile they carry (LDS counters) --
// except for the pixels of tile_mask (repaired by qf_bvh_repair_overflow: their per-ray rows hold the exact K nearest)
// and for every pixel when the pass's ray flag is up (the pass wrote nothing, the repair traversed every ray): those
// read their per-ray row as without bins.  From the sorted rows onwards nothing differs.
template <bool kTri, bool kBins>
__global__ __launch_bounds__(64) void pack_tiles_kernel(
    const float *__restrict__ rays_o, const float *__restrict__ rays_d, int w, int h, int tiles_x, int n_tiles, int max_hits,
    const int32_t *__restrict__ hit_tri, const float *__restrict__ hit_t, const int32_t *__restrict__ hit_count,
    const int64_t *__restrict__ tile_base, const int64_t *__restrict__ total, float *__restrict__ xyz_c,
    float *__restrict__ dirs_c, float *__restrict__ depth_c, int32_t *__restrict__ tri_c, const uint64_t *__restrict__ keep_mask,
    const int32_t *__restrict__ raw_count, float min_sep, int32_t *__restrict__ final_count, int32_t *__restrict__ dropped,
    const int32_t *__restrict__ tile_cursor, const uint64_t *__restrict__ tile_mask, const uint2 *__restrict__ bins,
    const int32_t *__restrict__ ray_flag)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int K = max_hits, Kp = max_hits | 1;            // odd row stride: conflict-free column access
    // kTri = false: distances only -- the triangle ids are not part of the output then, and hits with equal t are the
    // same sample in either order.  kTri = true (tri_c wanted: baked-texture frames look their texels up by triangle):
    // ids staged too and the lists sorted by (t, tri) like everywhere else, so that ties resolve to the same triangle.
    float *s_t = reinterpret_cast<float *>(smem);
    int32_t *s_tri = reinterpret_cast<int32_t *>(s_t + 64 * Kp);
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int px0 = (tile % tiles_x) * 8, py0 = (tile / tiles_x) * 8;
    const int cols = (w - px0) < 8 ? (w - px0) : 8, rows = (h - py0) < 8 ? (h - py0) : 8;
    const int px = px0 + (lane & 7), py = py0 + (lane >> 3);
    const bool inside = px < w && py < h;
    const int64_t ray = inside ? (int64_t)py * w + px : 0;
    int cnt = 0;
    if (inside) {
        cnt = keep_mask ? raw_count[ray] : hit_count[ray];
        if (cnt > K) cnt = K;
    }
    // the longest list of the tile bounds what is staged: background tiles (40 % of an orbit frame) leave at once, the
    // others read their first `deepest` slots instead of all K
    int deepest = cnt;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const int other = __shfl_xor(deepest, off, 64);
        deepest = other > deepest ? other : deepest;
    }
    if (deepest == 0) {                                       // wave-uniform
        if (final_count && inside) final_count[ray] = 0;
        return;
    }
    float *row_t = s_t + lane * Kp;
    int32_t *row_i = s_tri + lane * Kp;                       // only touched when kTri
    // everything the wave reads from memory is asked for here, before anything waits: the ray, the tile's first slot and
    // (below) the lists
    const float ox = rays_o[ray * 3], oy = rays_o[ray * 3 + 1], oz = rays_o[ray * 3 + 2];
    const float dx = rays_d[ray * 3], dy = rays_d[ray * 3 + 1], dz = rays_d[ray * 3 + 2];
    int64_t base = tile_base[tile];
    if (kBins) {
        __shared__ int s_fill[64];
        const unsigned long long by_row = (ray_flag && *ray_flag) ? ~0ull : tile_mask[tile];
        const int cap = 64 * K;
        const int cursor = tile_cursor[tile];
        const int n = by_row == ~0ull ? 0 : (cursor < cap ? cursor : cap);
        const uint2 *run = bins + (int64_t)tile * cap;
        s_fill[lane] = 0;
        __syncthreads();
        for (int i = lane; i < n; i += 64) {
            const uint2 rec = run[i];
            const int p = (int)(rec.y & 63u);
            const int at = atomicAdd(&s_fill[p], 1);
            if (!((by_row >> p) & 1ull) && at < K) {          // (a binned pixel holds at most K records)
                s_t[p * Kp + at] = __uint_as_float(rec.x);
                if (kTri) s_tri[p * Kp + at] = (int32_t)(rec.y >> 6);
            }
        }
        __syncthreads();
        const bool own_row = (by_row >> lane) & 1ull;
        if (deepest <= 16) {
            if (own_row) load_sort_row<16, kTri>(hit_t + ray * K, hit_tri + ray * K, K, cnt, deepest, row_t, row_i);
            else sort_row_in_place<16, kTri>(cnt, deepest, row_t, row_i);
        } else {
            if (own_row) load_sort_row<32, kTri>(hit_t + ray * K, hit_tri + ray * K, K, cnt, deepest, row_t, row_i);
            else sort_row_in_place<32, kTri>(cnt, deepest, row_t, row_i);
        }
    } else if (K <= 32) {
        // lists of up to 32 hits: global memory -> registers -> sorted -> the lane's own LDS row (load_sort_row); no lane
        // reads another lane's row below, so no barrier
        if (deepest <= 16) load_sort_row<16, kTri>(hit_t + ray * K, hit_tri + ray * K, K, cnt, deepest, row_t, row_i);
        else load_sort_row<32, kTri>(hit_t + ray * K, hit_tri + ray * K, K, cnt, deepest, row_t, row_i);
    } else {
        // stage: the lists of a tile row's pixels lie K apart
        for (int yy = 0; yy < rows; ++yy) {
            const int64_t row_ray0 = (int64_t)(py0 + yy) * w + px0;
            for (int i = lane; i < cols * deepest; i += 64) {
                const int r = i / deepest, k = i - r * deepest;
                s_t[(yy * 8 + r) * Kp + k] = hit_t[(row_ray0 + r) * K + k];
                if (kTri) s_tri[(yy * 8 + r) * Kp + k] = hit_tri[(row_ray0 + r) * K + k];
            }
        }
        __syncthreads();
    }
    double o64[3] = {0.0, 0.0, 0.0}, d64[3] = {0.0, 0.0, 0.0};
    float dn[3] = {0.0f, 0.0f, 0.0f};
    int n_dropped = 0;
    if (inside) {
        if (K > 32) {                                         // t (or (t, tri)) ascending; K <= 32 is sorted already
            for (int i = 1; i < cnt; ++i) {
                const float t = row_t[i];
                const int id = kTri ? row_i[i] : 0;
                int j = i - 1;
                while (j >= 0 && (kTri ? hit_less(t, id, row_t[j], row_i[j]) : t < row_t[j])) {
                    row_t[j + 1] = row_t[j];
                    if (kTri) row_i[j + 1] = row_i[j];
                    --j;
                }
                row_t[j + 1] = t;
                if (kTri) row_i[j + 1] = id;
            }
        }
        if (keep_mask) {                                      // the re-origin rule, decided by qf_bvh_repair_overflow
            const uint64_t mask = keep_mask[ray];
            int kept = 0;
            for (int i = 0; i < cnt; ++i)
                if ((mask >> i) & 1ull) { row_t[kept] = row_t[i]; if (kTri) row_i[kept] = row_i[i]; ++kept; }
            cnt = kept;
        } else if (min_sep > 0.0f && cnt > 1) {
            // the re-origin rule on the sorted list, as filter_hits_kernel applies it: a hit is kept iff it is the first
            // or lies more than min_sep behind the last kept one.  The tile's slots were allotted from the counts before
            // the rule; what it drops leaves a gap at the end of the tile (filled below).
            float last_t = row_t[0];
            int kept = 1;
            for (int i = 1; i < cnt; ++i) {
                const float t = row_t[i];
                if (t > last_t + min_sep) { row_t[kept] = t; if (kTri) row_i[kept] = row_i[i]; ++kept; last_t = t; }
            }
            n_dropped = cnt - kept;
            cnt = kept;
        }
        if (cnt > 0) {
            o64[0] = (double)ox; o64[1] = (double)oy; o64[2] = (double)oz;
            d64[0] = (double)dx; d64[1] = (double)dy; d64[2] = (double)dz;
            // vectors / (|vectors| + 1e-7) in float32 (mesh_utils.py:369-370)
            const float nrm = sqrtf((dx * dx + dy * dy) + dz * dz) + 1e-7f;
            dn[0] = dx / nrm; dn[1] = dy / nrm; dn[2] = dz / nrm;
        }
        if (cnt > 1) {
            double p[3];
            double prev = sample_depth64(row_t[0], o64, d64, p);
            bool sorted = true;
            for (int k = 1; k < cnt; ++k) {
                const double dk = sample_depth64(row_t[k], o64, d64, p);
                sorted = sorted && !(prev > dk);
                prev = dk;
            }
            if (!sorted) {                                     // rare: stable insertion by depth, depths recomputed
                for (int i = 1; i < cnt; ++i) {
                    const float t = row_t[i];
                    const int id = kTri ? row_i[i] : 0;
                    const double di = sample_depth64(t, o64, d64, p);
                    int j = i - 1;
                    while (j >= 0 && sample_depth64(row_t[j], o64, d64, p) > di) {
                        row_t[j + 1] = row_t[j];
                        if (kTri) row_i[j + 1] = row_i[j];
                        --j;
                    }
                    row_t[j + 1] = t;
                    if (kTri) row_i[j + 1] = id;
                }
            }
        }
    }
    if (final_count && inside) final_count[ray] = cnt;
    const unsigned long long below = (1ull << lane) - 1ull;
    float first_xyz[3] = {0.0f, 0.0f, 0.0f};                  // this lane's nearest sample, for the gap fill
    for (int k = 0;; ++k) {
        const unsigned long long mask = __ballot(cnt > k);
        if (mask == 0ull) break;                              // wave-uniform exit
        if (cnt > k) {
            const int64_t c = base + __popcll(mask & below);
            double p[3];
            const double dep = sample_depth64(row_t[k], o64, d64, p);
            xyz_c[c * 3 + 0] = (float)p[0];
            xyz_c[c * 3 + 1] = (float)p[1];
            xyz_c[c * 3 + 2] = (float)p[2];
            dirs_c[c * 3 + 0] = dn[0];
            dirs_c[c * 3 + 1] = dn[1];
            dirs_c[c * 3 + 2] = dn[2];
            depth_c[c] = (float)dep;
            if (kTri) tri_c[c] = (int32_t)row_i[k];
            if (k == 0) { first_xyz[0] = (float)p[0]; first_xyz[1] = (float)p[1]; first_xyz[2] = (float)p[2]; }
        }
        base += __popcll(mask);
    }
    // Slots the rule emptied: the field kernel streams [0, total) and must find finite points everywhere, nobody reads
    // what it computes there (qf_composite_tiles walks the kept counts).  They get a copy of the tile's first sample.
    const unsigned long long any_drop = __ballot(n_dropped > 0);
    if (any_drop) {
        const int64_t end = tile + 1 < n_tiles ? tile_base[tile + 1] : *total;
        const int src = __ffsll((long long)__ballot(cnt > 0)) - 1;       // a tile that dropped something kept something
        const float gx = __shfl(first_xyz[0], src, 64), gy = __shfl(first_xyz[1], src, 64), gz = __shfl(first_xyz[2], src, 64);
        const float hx = __shfl(dn[0], src, 64), hy = __shfl(dn[1], src, 64), hz = __shfl(dn[2], src, 64);
        const int gtri = kTri ? __shfl((int)row_i[0], src, 64) : 0;
        for (int64_t c = base + lane; c < end; c += 64) {
            xyz_c[c * 3 + 0] = gx; xyz_c[c * 3 + 1] = gy; xyz_c[c * 3 + 2] = gz;
            dirs_c[c * 3 + 0] = hx; dirs_c[c * 3 + 1] = hy; dirs_c[c * 3 + 2] = hz;
            depth_c[c] = 0.0f;
            if (kTri) tri_c[c] = (int32_t)gtri;
        }
        int sum = n_dropped;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) sum += __shfl_xor(sum, off, 64);
        if (lane == 0 && dropped) atomicAdd(dropped, sum);
    }
}

// the frame's dropped-hit count -> pinned host memory (host_out[2]), one thread; the counter is left at zero for the
// caller's next frame (which then needs no memset launch of its own)
__global__ void publish_dropped_kernel(int32_t *dropped, int64_t *host_out)
{
    host_out[2] = (int64_t)*dropped;
    *dropped = 0;
}

// Stable per-ray insertion sort of sample indices by fp32 depth (np.lexsort((depth, index_ray)) on grouped rays).
__global__ void resort_kernel(const int64_t *index_ray, const float *depth, int64_t n, int64_t *perm)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ray = index_ray[i];
        if (i != 0 && index_ray[i - 1] == ray) continue;
        perm[i] = i;
        for (int64_t k = i + 1; k < n && index_ray[k] == ray; ++k) {
            const float dk = depth[k];
            int64_t j = k - 1;
            while (j >= i && depth[perm[j]] > dk) { perm[j + 1] = perm[j]; --j; }
            perm[j + 1] = k;
        }
    }
}

// sampling_indexing (mesh_utils.py:389-412) in one pass: the stable per-ray re-sort by depth AND the gathers of the
// sample arrays through the resulting permutation AND the pack boundaries.  A workgroup owns RS_CHUNK consecutive
// samples (+ halo: a ray of the mesh path has at most QF_BVH_MAX_HITS = 64 samples, so rays starting in the chunk end
// inside the staged window); depths and ray ids are staged in LDS, the first samples of the rays are compacted so that
// consecutive lanes sort different rays (insertion sort of local indices, = np.lexsort((depth, ray)) on grouped
// rays), and the arrays are then written coalesced, reading from (almost always nearly the same) source positions.
// Rays that run past the window take the slow path through global memory.
constexpr int RS_THREADS = 256;
constexpr int RS_CHUNK = 1024;
constexpr int RS_HALO = 64;
constexpr int RS_STAGE = RS_CHUNK + RS_HALO;

__global__ __launch_bounds__(RS_THREADS) void resort_samples_kernel(
    const int64_t *index_ray, const float *depth, int64_t n, const float *points, const float *origins,
    const float *vectors, const int64_t *index_tri, int64_t *perm, float *out_points, float *out_depth,
    float *out_origins, float *out_vectors, int64_t *out_index_tri, uint8_t *boundary, const int32_t *inverse,
    float *out_points_c, float *out_vectors_c)
{
    __shared__ float s_depth[RS_STAGE];
    __shared__ int64_t s_ray[RS_STAGE + 1];
    __shared__ int s_src[RS_STAGE];                  // local source index of the sample that lands at each position
    __shared__ uint8_t s_mine[RS_STAGE];
    __shared__ int s_heads[RS_CHUNK];
    __shared__ int s_nheads;
    const int64_t n_chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
    for (int64_t chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
        const int64_t b0 = chunk * RS_CHUNK;
        const int staged = (int)((n - b0 < RS_STAGE) ? (n - b0) : RS_STAGE);
        const int own = (int)((n - b0 < RS_CHUNK) ? (n - b0) : RS_CHUNK);
        if (threadIdx.x == 0) {
            s_ray[0] = b0 > 0 ? index_ray[b0 - 1] : 0;
            s_nheads = 0;
        }
        for (int k = threadIdx.x; k < staged; k += RS_THREADS) {
            s_depth[k] = depth[b0 + k];
            s_ray[k + 1] = index_ray[b0 + k];
            s_mine[k] = 0;
        }
        __syncthreads();
        for (int k = threadIdx.x; k < own; k += RS_THREADS) {
            const bool head = (b0 + k == 0) || s_ray[k] != s_ray[k + 1];
            if (boundary) boundary[b0 + k] = head ? 1 : 0;
            if (head) s_heads[atomicAdd(&s_nheads, 1)] = k;
        }
        __syncthreads();
        const int n_heads = s_nheads;
        for (int h = threadIdx.x; h < n_heads; h += RS_THREADS) {
            const int k = s_heads[h];
            const int64_t ray = s_ray[k + 1];
            int end = k + 1;
            while (end < staged && s_ray[end + 1] == ray) ++end;
            const bool spills = end == staged && b0 + staged < n && index_ray[b0 + staged] == ray;
            if (!spills) {
                s_src[k] = k;
                s_mine[k] = 1;
                for (int q = k + 1; q < end; ++q) {
                    const float dq = s_depth[q];
                    int j = q - 1;
                    while (j >= k && s_depth[s_src[j]] > dq) { s_src[j + 1] = s_src[j]; --j; }
                    s_src[j + 1] = q;
                    s_mine[q] = 1;
                }
            } else {                                  // longer than the window: sort and gather through global memory
                const int64_t i = b0 + k;
                int64_t e = i + 1;
                while (e < n && index_ray[e] == ray) ++e;
                // perm doubles as the work array; without one, fall back to a selection by rank
                for (int64_t q = i; q < e; ++q) {
                    const float dq = depth[q];
                    int64_t rank = 0;
                    for (int64_t r = i; r < e; ++r) {
                        const float dr = depth[r];
                        rank += (dr < dq) || (dr == dq && r < q);
                    }
                    const int64_t dst = i + rank;
                    if (perm) perm[dst] = q;
                    out_depth[dst] = dq;
                    if (out_index_tri) out_index_tri[dst] = index_tri[q];
                    const int64_t pos_c = inverse ? (int64_t)inverse[dst] : 0;
                    for (int c = 0; c < 3; ++c) {
                        out_points[dst * 3 + c] = points[q * 3 + c];
                        if (out_origins) out_origins[dst * 3 + c] = origins[q * 3 + c];
                        out_vectors[dst * 3 + c] = vectors[q * 3 + c];
                        if (inverse) {
                            out_points_c[pos_c * 3 + c] = points[q * 3 + c];
                            out_vectors_c[pos_c * 3 + c] = vectors[q * 3 + c];
                        }
                    }
                }
            }
        }
        __syncthreads();
        for (int k = threadIdx.x; k < staged; k += RS_THREADS) {
            if (!s_mine[k]) continue;
            const int64_t src = b0 + s_src[k], dst = b0 + k;
            if (perm) perm[dst] = src;
            out_depth[dst] = s_depth[s_src[k]];
            if (out_index_tri) out_index_tri[dst] = index_tri[src];
        }
        for (int e = threadIdx.x; e < 3 * staged; e += RS_THREADS) {
            const int k = e / 3, c = e - 3 * k;
            if (!s_mine[k]) continue;
            const int64_t src = (b0 + s_src[k]) * 3 + c, dst = b0 * 3 + e;
            const float pv = points[src], vv = vectors[src];
            out_points[dst] = pv;
            if (out_origins) out_origins[dst] = origins[src];
            out_vectors[dst] = vv;
            if (inverse) {                            // second copy at the sample's place in the coherent order
                const int64_t pc = (int64_t)inverse[b0 + k] * 3 + c;
                out_points_c[pc] = pv;
                out_vectors_c[pc] = vv;
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int qf_pack_samples(const float *rays_o, const float *rays_d, int64_t n_rays, int32_t max_hits,
                               const int32_t *hit_tri, const float *hit_t, const int32_t *hit_count,
                               const int64_t *ray_offset, float *xyz, float *dirs, int64_t *index_ray, float *depth,
                               int64_t *index_tri, float *origins, const int32_t *inverse, float *xyz_c, float *dirs_c,
                               float *depth_c, const uint64_t *keep_mask, const int32_t *raw_count,
                               float min_separation, int32_t *close_flag, void *stream)
{
    if ((keep_mask == nullptr) != (raw_count == nullptr)) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays < 0 || max_hits < 1 || max_hits > kMaxHits) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays == 0) return QF_OK;
    if (!rays_o || !rays_d || !hit_tri || !hit_t || !hit_count || !ray_offset) return QF_ERR_INVALID_ARGUMENT;
    if (inverse && (!xyz_c || !dirs_c)) return QF_ERR_INVALID_ARGUMENT;
    if (!index_ray || !depth || !index_tri) return QF_ERR_INVALID_ARGUMENT;
    if ((xyz || dirs || origins) && (!xyz || !dirs || !origins)) return QF_ERR_INVALID_ARGUMENT;
    if (!xyz && !inverse) return QF_ERR_INVALID_ARGUMENT;      // the positions have to go somewhere
    const int Kp = max_hits | 1;
    const size_t lds = (size_t)kPackRays * Kp * 8 + (size_t)kPackRays * max_hits * 2 + 64;
    const int64_t blocks = qf_div_up(n_rays, kPackRays);
    if (blocks > 0x7fffffff) return QF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(pack_samples_kernel, dim3((unsigned)blocks), dim3(kPackRays), lds, qf_stream(stream), rays_o, rays_d,
                       n_rays, (int)max_hits, hit_tri, hit_t, hit_count, ray_offset, xyz, dirs, index_ray, depth, index_tri,
                       origins, inverse, xyz_c, dirs_c, depth_c, keep_mask, raw_count, min_separation, close_flag);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

// qf_pack_tiles and qf_pack_tiles_bins (tile_cursor / tile_mask / bins set)
static int pack_tiles_launch(const float *rays_o, const float *rays_d, int32_t width, int32_t height, int32_t max_hits,
                             const int32_t *hit_tri, const float *hit_t, const int32_t *hit_count, const int64_t *tile_base,
                             const int64_t *total, float *xyz_c, float *dirs_c, float *depth_c, int32_t *tri_c,
                             const uint64_t *keep_mask, const int32_t *raw_count, float min_separation,
                             int32_t *final_count, int32_t *dropped, int64_t *host_out, int32_t dropped_is_zero,
                             const int32_t *tile_cursor, const uint64_t *tile_mask, const void *bins, const int32_t *ray_flag,
                             void *stream)
{
    if ((keep_mask == nullptr) != (raw_count == nullptr)) return QF_ERR_INVALID_ARGUMENT;
    if (width < 1 || height < 1 || max_hits < 1 || max_hits > kMaxHits) return QF_ERR_INVALID_ARGUMENT;
    if (!rays_o || !rays_d || !hit_t || !hit_count || !tile_base || !total || !xyz_c || !dirs_c || !depth_c)
        return QF_ERR_INVALID_ARGUMENT;
    if (tri_c && !hit_tri) return QF_ERR_INVALID_ARGUMENT;
    const bool rule_here = !keep_mask && min_separation > 0.0f;
    if (rule_here && (!final_count || !dropped)) return QF_ERR_INVALID_ARGUMENT;     // the counts change: they must go somewhere
    if (host_out && !dropped) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    if (dropped && !host_out && !dropped_is_zero) QF_HIP_TRY(hipMemsetAsync(dropped, 0, sizeof(int32_t), st));
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const float sep = rule_here ? min_separation : 0.0f;
    // with triangle ids the LDS rows stage them beside the distances
    auto *kernel = bins ? (tri_c ? pack_tiles_kernel<true, true> : pack_tiles_kernel<false, true>)
                        : (tri_c ? pack_tiles_kernel<true, false> : pack_tiles_kernel<false, false>);
    const size_t lds = (size_t)64 * (max_hits | 1) * (tri_c ? 8 : 4);
    hipLaunchKernelGGL(kernel, dim3((unsigned)(tiles_x * tiles_y)), dim3(64), lds, st, rays_o, rays_d, (int)width, (int)height,
                       tiles_x, tiles_x * tiles_y, (int)max_hits, hit_tri, hit_t, hit_count, tile_base, total, xyz_c, dirs_c,
                       depth_c, tri_c, keep_mask, raw_count, sep, final_count, dropped, tile_cursor, tile_mask,
                       reinterpret_cast<const uint2 *>(bins), ray_flag);
    if (host_out) hipLaunchKernelGGL(publish_dropped_kernel, dim3(1), dim3(1), 0, st, dropped, host_out);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_pack_tiles(const float *rays_o, const float *rays_d, int32_t width, int32_t height, int32_t max_hits,
                             const int32_t *hit_tri, const float *hit_t, const int32_t *hit_count, const int64_t *tile_base,
                             const int64_t *total, float *xyz_c, float *dirs_c, float *depth_c, int32_t *tri_c,
                             const uint64_t *keep_mask, const int32_t *raw_count, float min_separation,
                             int32_t *final_count, int32_t *dropped, int64_t *host_out, int32_t dropped_is_zero,
                             void *stream)
{
    return pack_tiles_launch(rays_o, rays_d, width, height, max_hits, hit_tri, hit_t, hit_count, tile_base, total, xyz_c, dirs_c,
                             depth_c, tri_c, keep_mask, raw_count, min_separation, final_count, dropped, host_out,
                             dropped_is_zero, nullptr, nullptr, nullptr, nullptr, stream);
}

extern "C" int qf_pack_tiles_bins(const float *rays_o, const float *rays_d, int32_t width, int32_t height, int32_t max_hits,
                                  const int32_t *hit_tri, const float *hit_t, const int32_t *hit_count,
                                  const int64_t *tile_base, const int64_t *total, float *xyz_c, float *dirs_c, float *depth_c,
                                  int32_t *tri_c, float min_separation, int32_t *final_count, int32_t *dropped,
                                  int64_t *host_out, int32_t dropped_is_zero, const int32_t *tile_cursor,
                                  const uint64_t *tile_mask, const void *bins, const int32_t *ray_flag, void *stream)
{
    if (!tile_cursor || !tile_mask || !bins || max_hits > 32) return QF_ERR_INVALID_ARGUMENT;
    if (!hit_tri) return QF_ERR_INVALID_ARGUMENT;           // (a repaired pixel's row: the repair writes ids on every route)
    return pack_tiles_launch(rays_o, rays_d, width, height, max_hits, hit_tri, hit_t, hit_count, tile_base, total, xyz_c, dirs_c,
                             depth_c, tri_c, nullptr, nullptr, min_separation, final_count, dropped, host_out, dropped_is_zero,
                             tile_cursor, tile_mask, bins, ray_flag, stream);
}

extern "C" int qf_resort_by_depth(const int64_t *index_ray, const float *depth, int64_t n, int64_t *perm, void *stream)
{
    if (n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!index_ray || !depth || !perm) return QF_ERR_INVALID_ARGUMENT;
    QF_SIMPLE_LAUNCH(resort_kernel, n, index_ray, depth, n, perm);
    return QF_OK;
}

extern "C" int qf_resort_samples(const int64_t *index_ray, const float *depth, int64_t n, const float *points,
                                 const float *origins, const float *vectors, const int64_t *index_tri, int64_t *perm,
                                 float *out_points, float *out_depth, float *out_origins, float *out_vectors,
                                 int64_t *out_index_tri, uint8_t *boundary, const int32_t *inverse, float *out_points_c,
                                 float *out_vectors_c, void *stream)
{
    if (n < 0) return QF_ERR_INVALID_ARGUMENT;
    if (n == 0) return QF_OK;
    if (!index_ray || !depth || !points || !vectors || !out_points || !out_depth || !out_vectors ||
        (out_origins && !origins) || (out_index_tri && !index_tri) || (inverse && (!out_points_c || !out_vectors_c)))
        return QF_ERR_INVALID_ARGUMENT;
    const int64_t n_chunks = (n + RS_CHUNK - 1) / RS_CHUNK;
    hipLaunchKernelGGL(resort_samples_kernel, dim3((unsigned)(n_chunks < 65536 ? n_chunks : 65536)), dim3(RS_THREADS), 0,
                       qf_stream(stream), index_ray, depth, n, points, origins, vectors, index_tri, perm, out_points,
                       out_depth, out_origins, out_vectors, out_index_tri, boundary, inverse, out_points_c, out_vectors_c);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
