// The camera-coherent intersector: triangles rasterised against the pixel grid of one pinhole camera (plain, culled
// and depth-slab passes; the plain pass also with its hits binned per 8x8 tile), the device-side camera check, the K-nearest selection of the wide passes and the per-ray
// sort / re-origin filter of the hit lists.
#include <type_traits>

#include "exact_common.h"

#pragma clang fp contract(off)

namespace {

// ---------------------------------------------------------------------------------------------------------
// Camera-coherent intersector: when the rays are the pixel grid of one pinhole camera (every eval frame of the
// reference: nerf_synthetic.py:310-373), the set of rays that can hit a triangle is bounded by the triangle's
// projected screen box.  Each triangle is tested only against those pixels -- with the SAME mt_hit() on the SAME
// (o, d) values as the BVH path, so the hits are bit-identical -- and appended to the pixel's list with one
// atomic.  No tree, no stack, coalesced triangle reads; the lists are sorted afterwards (sort_hits_kernel).
struct RasterCam {
    float r00, r01, r02, r10, r11, r12, r20, r21, r22;   // c2w[:3,:3]: columns = camera right / up / back
    float cx, cy, cz;                                      // camera centre
    float fx, fy, px0, py0;                                // pixel = f * (x/z) + p0   (p0 = principal - 0.5)
    int w, h;
};

// kRasterLanes lanes cooperate on one triangle and share its screen box round-robin.
// Guard band in pixels around the projected triangle.  A pixel-centre ray that the fp32 Moller-Trumbore test accepts
// lies, in exact arithmetic, within c * eps * f pixels of the projected triangle (numerator rounding over |det|,
// c ~ 10, eps = 2^-24, f = focal length in pixels: ~1e-3 px at f = 1111, ~3e-3 px at f = 2700), and the projected
// vertices carry ~1e-4 px of rounding.  0.25 px leaves two orders of magnitude.
constexpr float kRasterGuard = 0.25f;

// kWide: the lists are [slot][ray] (capacity max_hits = the wide capacity), for select_nearest_kernel's coalesced reads.
// One triangle against the pixels of its screen box, lane ``sub`` of kRasterLanes (the body of both raster kernels).
// kSlab (depth-slab pass, raster_slab_kernel): only hits with slab.t_lo <= t < slab.t_hi are accepted, a pixel that
// already holds slab.stop_at candidates is skipped before its ray is even loaded, and a candidate is ONE 8-byte key
// (t bits << 32 | tri) in slab.keys [capacity][n_rays].
struct SlabArgs {
    float t_lo, t_hi;
    int stop_at;
    uint64_t *keys;
    const float4 *ray_rec;           // per ray (d.xyz, count when this slab's pass started as int bits); NULL for the first slab
};

// A triangle's screen-space set-up, shared by the passes below: the pixel box it can touch and (when its orientation
// is reliable) the three guard-banded edge functions.  false: no pixel can be hit.
struct TriSetup {
    int x0, x1, y0, y1;
    bool use_edges;
    float ea[3], eb[3], ec[3];
};

__device__ __forceinline__ bool tri_setup(const float4 a, const float4 b, const float4 c, const RasterCam &cam, TriSetup &s)
{
    // conservative screen box of the triangle (projection of a convex set is inside the box of its vertices)
    float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
    int behind = 0;
    const float4 vs[3] = {a, b, c};
    float sxs[3], sys[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const float dx = vs[k].x - cam.cx, dy = vs[k].y - cam.cy, dz = vs[k].z - cam.cz;
        const float xc = cam.r00 * dx + cam.r10 * dy + cam.r20 * dz;    // R^T (v - c)
        const float yc = cam.r01 * dx + cam.r11 * dy + cam.r21 * dz;
        const float zc = cam.r02 * dx + cam.r12 * dy + cam.r22 * dz;
        const float zv = -zc;                                           // depth along the viewing direction
        if (!(zv > 1e-6f)) { ++behind; sxs[k] = sys[k] = 0.0f; continue; }
        const float sx = cam.fx * (xc / zv) + cam.px0;
        const float sy = -cam.fy * (yc / zv) + cam.py0;
        sxs[k] = sx; sys[k] = sy;
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx);
        miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
    if (behind == 3) return false;           // entirely behind the camera: t > 0 is impossible
    // Conservative 2-D reject before any memory is touched: a pixel can only be hit if it lies inside the projected
    // triangle grown by the guard band, i.e. on the inner side of every edge line moved outwards by the guard
    // (|edge| is over-estimated by its L1 length).  Skipped for triangles that straddle the camera plane or project
    // (almost) edge-on, where the orientation is not reliable; the exact test below decides in every case.
    s.use_edges = false;
    if (behind > 0) {                        // straddles the camera plane: no finite box, test every pixel
        s.x0 = 0; s.y0 = 0; s.x1 = cam.w - 1; s.y1 = cam.h - 1;
    } else {
        s.x0 = (int)fmaxf(floorf(minx - kRasterGuard), 0.0f);
        s.y0 = (int)fmaxf(floorf(miny - kRasterGuard), 0.0f);
        s.x1 = (int)fminf(ceilf(maxx + kRasterGuard), (float)(cam.w - 1));
        s.y1 = (int)fminf(ceilf(maxy + kRasterGuard), (float)(cam.h - 1));
        if (!(maxx + kRasterGuard >= 0.0f) || !(maxy + kRasterGuard >= 0.0f) ||
            !(minx - kRasterGuard <= (float)(cam.w - 1)) || !(miny - kRasterGuard <= (float)(cam.h - 1)))
            return false;
        const float area2 = (sxs[1] - sxs[0]) * (sys[2] - sys[0]) - (sys[1] - sys[0]) * (sxs[2] - sxs[0]);
        if (fabsf(area2) > 1e-2f) {
            s.use_edges = true;
            const float sgn = area2 > 0.0f ? 1.0f : -1.0f;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const int k1 = (k + 1) % 3;
                const float ex = sxs[k1] - sxs[k], ey = sys[k1] - sys[k];
                // E(p) = sgn * ((p.y - v.y) * ex - (p.x - v.x) * ey): positive at the opposite vertex.
                // keep p iff E(p) >= -guard * (|ex| + |ey|) - slack
                s.ea[k] = -sgn * ey;
                s.eb[k] = sgn * ex;
                s.ec[k] = -(s.ea[k] * sxs[k] + s.eb[k] * sys[k]) + (kRasterGuard + 0.05f) * (fabsf(ex) + fabsf(ey)) + 1e-3f;
            }
        }
    }
    return true;
}

// ---- hit bins (the plain render-only frame, qf_raster_intersect_tiles): an accepted hit goes to the bin of its pixel's
// 8x8 tile -- one dense run of at most 64 * K eight-byte records (t bits, tri << 6 | pixel in tile) per tile -- instead
// of taking a slot in its pixel's list with a returning device-wide atomic of its own.  A wave stages its hits in LDS
// (an LDS atomic per hit) and, after its last pixel, reserves space with ONE returning atomicAdd on tile_cursor[tile] per
// distinct tile among each 64 staged hits; the reservation that runs past the capacity writes nothing beyond it and the
// cursor keeps counting (tile_count_kernel then sends the whole tile to the repair).  Aggregating where the hit is found
// instead -- among the lanes that find one in the same loop iteration -- was measured and did not pay: the atomic's round
// trip stays in the per-candidate chain (profiles/r5/hit_bins.md).
constexpr int kBinStage = 256;           // staged hits per wave (16 triangles find 64 on average); the rest go one by one
constexpr int kBinIdBits = 26;           // triangle ids that fit beside the 6-bit pixel
struct BinStage { int n; int tile[kBinStage]; uint2 rec[kBinStage]; };
struct TileBins {
    int32_t *cursor;                     // [n_tiles]
    uint2 *bins;                         // [n_tiles][cap]
    int cap;                             // 64 * max_hits
    BinStage *stage;                     // the wave's own LDS area
};

// the lanes that call this together share one reservation per distinct tile
__device__ __forceinline__ void bin_records(const TileBins &tb, int tile, uint2 rec)
{
    const int lane = (int)__lane_id();
    for (;;) {
        const int t0 = __builtin_amdgcn_readfirstlane(tile);
        const unsigned long long m = __ballot(tile == t0);
        if (tile == t0) {
            const int rank = __popcll(m & ((1ull << lane) - 1ull));
            int base = 0;
            if (rank == 0) base = atomicAdd(&tb.cursor[t0], __popcll(m));
            base = __shfl(base, __ffsll((long long)m) - 1, 64);
            if (base + rank < tb.cap) tb.bins[(int64_t)t0 * tb.cap + base + rank] = rec;
            break;
        }
    }
}

template <int kRasterLanes, bool kWide, bool kSlab = false, bool kBins = false>
__device__ __forceinline__ void raster_triangle(const float4 *__restrict__ tris, int64_t tri_i, int sub, const RasterCam &cam,
                                                const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                int max_hits, int32_t *__restrict__ hit_tri, float *__restrict__ hit_t,
                                                int32_t *__restrict__ hit_count, int32_t *__restrict__ overflow,
                                                const bool cam_origin, const SlabArgs slab = SlabArgs(),
                                                const TileBins bins = TileBins())
{
    const float4 a = tris[tri_i * 3 + 0], b = tris[tri_i * 3 + 1], c = tris[tri_i * 3 + 2];
    const int id = __float_as_int(a.w);
    TriSetup ts;
    if (!tri_setup(a, b, c, cam, ts)) return;
    const int x0 = ts.x0, x1 = ts.x1, y0 = ts.y0, y1 = ts.y1;
    const bool use_edges = ts.use_edges;
    const float *ea = ts.ea, *eb = ts.eb, *ec = ts.ec;
    const int bw = x1 - x0 + 1;
    const int total = bw * (y1 - y0 + 1);
    int px = x0 + sub % bw, py = y0 + sub / bw;
    for (int q = sub; q < total; q += kRasterLanes) {
        const int cx_ = px, cy_ = py;
        px += kRasterLanes;
        while (px > x1) { px -= bw; ++py; }
        if (use_edges) {
            const float fx_ = (float)cx_, fy_ = (float)cy_;
            if (ea[0] * fx_ + eb[0] * fy_ + ec[0] < 0.0f || ea[1] * fx_ + eb[1] * fy_ + ec[1] < 0.0f ||
                ea[2] * fx_ + eb[2] * fy_ + ec[2] < 0.0f)
                continue;
        }
        const int64_t ray = (int64_t)cy_ * cam.w + cx_;
        // the pixel's K nearest are all in nearer slabs.  Decided on the count the pixel had when this pass STARTED: the
        // live count also moves with this slab's own hits, and stopping on it would keep an arbitrary subset of them
        // (the count rides in one 16-byte record with the ray's direction: one request and one round trip for both; read
        // separately they were two of each per candidate pixel of the later passes)
        float dx, dy, dz;
        if (kSlab && slab.ray_rec) {
            const float4 rr = slab.ray_rec[ray];
            if (__float_as_int(rr.w) >= slab.stop_at) continue;
            dx = rr.x; dy = rr.y; dz = rr.z;
        } else {
            dx = rays_d[ray * 3]; dy = rays_d[ray * 3 + 1]; dz = rays_d[ray * 3 + 2];
        }
        // the origin: the camera centre when camera_rays_check has verified that every ray's origin IS that value bit for bit
        // (one scattered 12-byte load less per candidate pixel: 17 % of the pass), the ray's own otherwise
        float ox = cam.cx, oy = cam.cy, oz = cam.cz;
        if (!cam_origin) { ox = rays_o[ray * 3]; oy = rays_o[ray * 3 + 1]; oz = rays_o[ray * 3 + 2]; }
        // origin and direction arrive together: without the pin the compiler sinks the origin's load behind mt_hit's
        // det != 0 branch, a second memory round trip per pixel (measured: configs[2] intersection 2.90 -> 2.62 ms)
        asm volatile("" : "+v"(ox), "+v"(oy), "+v"(oz), "+v"(dx), "+v"(dy), "+v"(dz));
        float t;
        if (!mt_hit(a, b, c, ox, oy, oz, dx, dy, dz, &t)) continue;
        if (kSlab) {
            if (!(t >= slab.t_lo && t < slab.t_hi)) continue;       // this hit belongs to another slab's pass
            const int slot = atomicAdd(&hit_count[ray], 1);
            if (slot < max_hits) slab.keys[(int64_t)slot * ((int64_t)cam.w * cam.h) + ray] = hit_key(t, id);
            else atomicAdd(overflow, 1);
            continue;
        }
        if (kBins) {
            const int tile = (cy_ >> 3) * ((cam.w + 7) >> 3) + (cx_ >> 3);
            const uint2 rec = make_uint2(__float_as_uint(t), ((uint32_t)id << 6) | (uint32_t)((cy_ & 7) * 8 + (cx_ & 7)));
            const int at = atomicAdd(&bins.stage->n, 1);
            if (at < kBinStage) { bins.stage->tile[at] = tile; bins.stage->rec[at] = rec; }
            else bin_records(bins, tile, rec);
            continue;
        }
        const int slot = atomicAdd(&hit_count[ray], 1);
        if (slot < max_hits) {
            const int64_t at = kWide ? (int64_t)slot * ((int64_t)cam.w * cam.h) + ray : ray * max_hits + slot;
            hit_t[at] = t;
            if (hit_tri) hit_tri[at] = id;      // (NULL: a render-only frame's tile pack never reads the ids)
        } else {
            atomicAdd(overflow, 1);      // more than max_hits candidates: the caller re-runs the exact K-nearest BVH path
        }
    }
}

template <int kRasterLanes, bool kWide>
__global__ __launch_bounds__(256) void raster_kernel(const float4 *__restrict__ tris, int64_t n_tri, RasterCam cam,
                                                     const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                     int max_hits, int32_t *__restrict__ hit_tri, float *__restrict__ hit_t,
                                                     int32_t *__restrict__ hit_count, int32_t *__restrict__ overflow,
                                                     const int32_t *__restrict__ ray_flag)
{
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t tri_i = gid / kRasterLanes;
    const int sub = (int)(gid % kRasterLanes);
    if (tri_i >= n_tri) return;
    if (ray_flag && *ray_flag) return;           // not this camera's pixel grid (camera_rays_check): the BVH answers
    const bool cam_origin = ray_flag != nullptr; // verified: every origin IS the camera centre
    raster_triangle<kRasterLanes, kWide>(tris, tri_i, sub, cam, rays_o, rays_d, max_hits, hit_tri, hit_t, hit_count, overflow,
                                         cam_origin);
}

// raster_kernel<kRasterLanes, false> with the hits going to the tile bins.  No lane leaves before the flush: the staged
// hits are handed out by lane index.
template <int kRasterLanes>
__global__ __launch_bounds__(256) void raster_bins_kernel(const float4 *__restrict__ tris, int64_t n_tri, RasterCam cam,
                                                          const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                          int max_hits, int32_t *__restrict__ tile_cursor,
                                                          uint2 *__restrict__ bin_records_out,
                                                          const int32_t *__restrict__ ray_flag)
{
    __shared__ BinStage s_stage[4];
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t tri_i = gid / kRasterLanes;
    const int sub = (int)(gid % kRasterLanes);
    if (ray_flag && *ray_flag) return;           // see raster_kernel (grid-uniform)
    const bool cam_origin = ray_flag != nullptr;
    const int lane = (int)(threadIdx.x & 63);
    TileBins tb;
    tb.cursor = tile_cursor;
    tb.bins = bin_records_out;
    tb.cap = 64 * max_hits;
    tb.stage = &s_stage[threadIdx.x >> 6];
    if (lane == 0) tb.stage->n = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");       // (the area is the wave's own: no barrier between waves)
    __builtin_amdgcn_wave_barrier();
    if (tri_i < n_tri)
        raster_triangle<kRasterLanes, false, false, true>(tris, tri_i, sub, cam, rays_o, rays_d, max_hits, nullptr, nullptr,
                                                          nullptr, nullptr, cam_origin, SlabArgs(), tb);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    __builtin_amdgcn_wave_barrier();
    const int n = tb.stage->n < kBinStage ? tb.stage->n : kBinStage;
    for (int i = lane; i < n; i += 64) bin_records(tb, tb.stage->tile[i], tb.stage->rec[i]);
}

// One wave per 8x8 tile after raster_bins_kernel: the tile's records -> the 64 hit_count words of its pixels (what the
// flat pass's per-pixel atomics leave: the number of candidates, past K included), the frame's overflow word (+ count - K
// per pixel, as the flat pass adds one per candidate past K; it only steers the caller's policy) and the tile's word of tile_mask: bit p set = pixel p's
// list is not in the bin -- it collected more than K candidates and is qf_bvh_repair_overflow's -- so the pack reads its
// per-ray row.  A bin that ran over its 64 * K records (some pixel of it holds more than K then) marks all its pixels.
// Every count of the frame is written here: the route has no hit_count fill.
__global__ __launch_bounds__(64) void tile_count_kernel(const int32_t *__restrict__ tile_cursor, const uint2 *__restrict__ bins,
                                                        int max_hits, int w, int h, int tiles_x,
                                                        int32_t *__restrict__ hit_count, int32_t *__restrict__ overflow,
                                                        uint64_t *__restrict__ tile_mask)
{
    __shared__ int s_cnt[64];
    const int tile = blockIdx.x, lane = threadIdx.x;
    const int cap = 64 * max_hits;
    const int cursor = tile_cursor[tile];
    const int n = cursor < cap ? cursor : cap;
    const int px = (tile % tiles_x) * 8 + (lane & 7), py = (tile / tiles_x) * 8 + (lane >> 3);
    const bool inside = px < w && py < h;
    int c = 0;
    if (n > 0) {                                              // wave-uniform
        s_cnt[lane] = 0;
        __syncthreads();
        const uint2 *run = bins + (int64_t)tile * cap;
        for (int i = lane; i < n; i += 64) atomicAdd(&s_cnt[run[i].y & 63u], 1);
        __syncthreads();
        c = s_cnt[lane];
    }
    int over = c > max_hits ? c - max_hits : 0;
    if (cursor > cap) {                                       // records were lost: the whole tile goes to the repair
        c = c > max_hits ? c : max_hits + 1;
        // (its candidates past K: at least cursor - cap, and exactly that when every pixel of the tile holds K or more)
        over = lane == 0 ? cursor - cap : 0;
    }
    if (inside) hit_count[(int64_t)py * w + px] = c;
    const unsigned long long mask = __ballot(inside && c > max_hits);
    if (mask) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) over += __shfl_xor(over, off, 64);
        if (lane == 0) atomicAdd(overflow, over);
    }
    if (lane == 0) tile_mask[tile] = mask;
}

// The precondition of the whole camera-coherent route, VERIFIED (round 4): ray i of the batch must be pixel
// (i % w, i / w) of this camera -- the reference's consistent ray set (nerf_synthetic.py:341-366: every ray starts at
// c2w[:3,3], its direction is the normalised pixel-centre direction).  Per ray:
//   * the origin equals the camera centre BIT FOR BIT (the passes then take it from the camera struct; the test uses
//     -0.0 for 0.0);
//   * the direction, projected with the very projection the triangle set-up uses, lands within kRayPixelTol of its own
//     pixel centre -- an order of magnitude inside the 0.25 px guard band, two above the rounding of a consistent ray
//     (3e-4 px at f = 1111, 3e-3 px at f = 8900) -- and in front of the camera;
//   * the direction has unit length (| |d|^2 - 1 | <= kRayUnitTol): the depth-slab passes bin by DISTANCE and accept by
//     t (0.1 % margin), the re-origin rule compares t with a world distance.
// Any violation (jittered directions of add_ray_direction_noise, nerf_synthetic.py:335-340; a stale or wrong camera;
// another up_sample; rays in another order; off-centre origins) raises *flag (zeroed by the caller's fill).  A raised
// flag makes every camera-coherent pass return at once and qf_bvh_repair_overflow traverse EVERY ray through the BVH
// -- exact for any rays -- instead of the guard-band reject silently dropping hits.  15.4 MB streamed per 800x800 frame.
constexpr float kRayPixelTol = 0.02f;
constexpr float kRayUnitTol = 1e-4f;

__device__ __forceinline__ void camera_rays_check(const uint32_t *__restrict__ o_bits, const float *__restrict__ rays_d,
                                                  int64_t n_rays, const RasterCam &cam, int32_t *__restrict__ flag,
                                                  int64_t first, int64_t stride)
{
    const uint32_t c0 = __float_as_uint(cam.cx), c1 = __float_as_uint(cam.cy), c2 = __float_as_uint(cam.cz);
    bool bad = false;
    for (int64_t r = first; r < n_rays; r += stride) {
        const uint32_t o0 = o_bits[r * 3], o1 = o_bits[r * 3 + 1], o2 = o_bits[r * 3 + 2];
        const float dx = rays_d[r * 3], dy = rays_d[r * 3 + 1], dz = rays_d[r * 3 + 2];
        bad = bad || o0 != c0 || o1 != c1 || o2 != c2;
        const float xc = cam.r00 * dx + cam.r10 * dy + cam.r20 * dz;    // R^T d, as tri_setup projects R^T (v - c)
        const float yc = cam.r01 * dx + cam.r11 * dy + cam.r21 * dz;
        const float zv = -(cam.r02 * dx + cam.r12 * dy + cam.r22 * dz);
        const float sx = cam.fx * (xc / zv) + cam.px0, sy = -cam.fy * (yc / zv) + cam.py0;
        const float px = (float)(int)(r % cam.w), py = (float)(int)(r / cam.w);
        // (negated comparisons: a NaN anywhere counts as a violation)
        bad = bad || !(zv > 0.0f) || !(fabsf(sx - px) <= kRayPixelTol) || !(fabsf(sy - py) <= kRayPixelTol) ||
              !(fabsf(dx * dx + dy * dy + dz * dz - 1.0f) <= kRayUnitTol);
    }
    if (bad) *flag = 1;
}

__global__ void camera_rays_check_kernel(const uint32_t *__restrict__ o_bits, const float *__restrict__ rays_d, int64_t n_rays,
                                         RasterCam cam, int32_t *__restrict__ flag)
{
    camera_rays_check(o_bits, rays_d, n_rays, cam, flag, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                      (int64_t)gridDim.x * blockDim.x);
}

// ---- triangle culling for cameras that see a PART of the scene (the row bands of parallel.ShardedFrameRenderer: every
// rank used to project all F triangles for its eighth of the rows).  The triangles are stored in BVH leaf order, so a
// chunk of kCullChunk consecutive ones is a compact piece of surface; chunk_boxes_kernel (once per build / refit) keeps
// its bounding box, cull_chunks_kernel (per frame, one lane per chunk) projects the box's corners with the triangle
// projection above and drops the chunk when its screen box misses the image by more than the guard band -- the same
// conservative reject raster_triangle applies per triangle, so no hit can be lost -- and raster_culled_kernel walks the
// compacted list with a resident grid.  The order in which hits arrive at a pixel's list changes; the lists are sorted
// afterwards (and were never in a defined order).
constexpr int kCullChunk = 64;

__global__ __launch_bounds__(256) void chunk_boxes_kernel(const float4 *__restrict__ tris, int64_t n_tri, int n_chunks,
                                                          float4 *__restrict__ boxes)
{
    const int chunk = (int)(((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6), lane = threadIdx.x & 63;
    if (chunk >= n_chunks) return;
    const int64_t t = (int64_t)chunk * kCullChunk + lane;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    if (t < n_tri) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float4 v = tris[t * 3 + k];
            lo[0] = fminf(lo[0], v.x); lo[1] = fminf(lo[1], v.y); lo[2] = fminf(lo[2], v.z);
            hi[0] = fmaxf(hi[0], v.x); hi[1] = fmaxf(hi[1], v.y); hi[2] = fmaxf(hi[2], v.z);
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            lo[k] = fminf(lo[k], __shfl_xor(lo[k], off, 64));
            hi[k] = fmaxf(hi[k], __shfl_xor(hi[k], off, 64));
        }
    }
    if (lane == 0) {
        boxes[chunk * 2 + 0] = make_float4(lo[0], lo[1], lo[2], 0.0f);
        boxes[chunk * 2 + 1] = make_float4(hi[0], hi[1], hi[2], 0.0f);
    }
}

// counters[2]: this call appends to counters[parity] and zeroes counters[parity ^ 1] for the next call on the handle
// (stream order: the previous call's raster kernel, which read it, is done) -- no memset launch per frame.
__global__ void cull_chunks_kernel(const float4 *__restrict__ boxes, int n_chunks, RasterCam cam, int32_t *__restrict__ visible,
                                   int32_t *__restrict__ counters, int parity, const uint32_t *__restrict__ o_bits,
                                   const float *__restrict__ rays_d, int64_t n_rays, int32_t *__restrict__ ray_flag)
{
    const int chunk = blockIdx.x * blockDim.x + threadIdx.x;
    if (chunk == 0) counters[parity ^ 1] = 0;
    // (this launch precedes the pass anyway: it also carries the pass's ray check, see camera_rays_check_kernel)
    if (ray_flag) camera_rays_check(o_bits, rays_d, n_rays, cam, ray_flag, chunk, (int64_t)gridDim.x * blockDim.x);
    if (chunk >= n_chunks) return;
    const float4 lo = boxes[chunk * 2], hi = boxes[chunk * 2 + 1];
    if (!(lo.x <= hi.x)) return;                                  // empty chunk
    float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
    bool keep = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float dx = ((k & 1) ? hi.x : lo.x) - cam.cx, dy = ((k & 2) ? hi.y : lo.y) - cam.cy, dz = ((k & 4) ? hi.z : lo.z) - cam.cz;
        const float xc = cam.r00 * dx + cam.r10 * dy + cam.r20 * dz;
        const float yc = cam.r01 * dx + cam.r11 * dy + cam.r21 * dz;
        const float zc = cam.r02 * dx + cam.r12 * dy + cam.r22 * dz;
        const float zv = -zc;
        if (!(zv > 1e-4f)) { keep = true; continue; }             // a corner at or behind the camera plane: no finite box
        const float sx = cam.fx * (xc / zv) + cam.px0, sy = -cam.fy * (yc / zv) + cam.py0;
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx);
        miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
    // the convex hull of the projected corners contains every projected triangle of the chunk; one extra pixel of margin
    // on top of the per-triangle guard band covers the rounding of these eight projections
    const float g = kRasterGuard + 1.0f;
    if (!keep)
        keep = (maxx + g >= 0.0f) && (maxy + g >= 0.0f) && (minx - g <= (float)(cam.w - 1)) && (miny - g <= (float)(cam.h - 1));
    if (keep) visible[atomicAdd(&counters[parity], 1)] = chunk;
}

template <int kRasterLanes, bool kWide>
__global__ __launch_bounds__(256) void raster_culled_kernel(const float4 *__restrict__ tris, int64_t n_tri, RasterCam cam,
                                                            const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                            int max_hits, int32_t *__restrict__ hit_tri, float *__restrict__ hit_t,
                                                            int32_t *__restrict__ hit_count, int32_t *__restrict__ overflow,
                                                            const int32_t *__restrict__ visible, const int32_t *__restrict__ n_visible,
                                                            const int32_t *__restrict__ ray_flag)
{
    if (ray_flag && *ray_flag) return;           // see raster_kernel
    const bool cam_origin = ray_flag != nullptr;
    constexpr int kTrisPerBlock = 256 / kRasterLanes;
    constexpr int kBlocksPerChunk = kCullChunk / kTrisPerBlock;       // 1 / 2 / 4 for 4 / 8 / 16 lanes per triangle
    const int n_items = *n_visible * kBlocksPerChunk;
    const int sub = threadIdx.x % kRasterLanes;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {  // workgroup-uniform
        const int chunk = visible[item / kBlocksPerChunk];
        const int64_t tri_i = (int64_t)chunk * kCullChunk + (item % kBlocksPerChunk) * kTrisPerBlock + threadIdx.x / kRasterLanes;
        if (tri_i < n_tri)
            raster_triangle<kRasterLanes, kWide>(tris, tri_i, sub, cam, rays_o, rays_d, max_hits, hit_tri, hit_t, hit_count, overflow,
                                                 cam_origin);
    }
}

// ---- depth slabs for dense scenes (BASELINE configs[2]: 36 thin shells, up to 72 crossings per ray, K = 25).  The wide
// pass above collects EVERY crossing of a ray (up to 4K slots, one returning atomic + a scattered write each) only for
// the selection to drop three quarters of them.  Here the visible triangle chunks are binned by their distance from the
// camera into n_slabs slabs of equal thickness (a chunk goes to every slab its distance range touches), the slabs are
// rasterised NEAREST FIRST in separate launches, a hit is accepted only by the pass of the slab its t falls into, and a
// pixel that holds stop_at candidates when a pass starts is skipped by it: all its hits nearer than this slab are
// already in its list -- a complete depth prefix -- and they are enough.  Exact: the slab passes partition the hits by t
// (edges computed by the same expression everywhere), a chunk's slabs cover the t of every hit it can produce (unit
// camera rays: t is the distance from the camera centre; 0.1 % margin), and stop_at = selection capacity + 1 keeps
// "the prefix was the whole list" distinguishable in select_nearest_kernel.  A pixel still overshoots by the hits of
// the slab in which it crosses stop_at, so the candidate lists need stop_at + (crossings per slab) slots, not 4K.
constexpr int kMaxSlabs = 16;

struct SlabCtl {                       // device control block of one frame
    uint32_t dist_min_bits, dist_max_bits;     // over the visible chunks; positive floats order like their bit patterns
    int32_t n_visible;
    int32_t slab_count[kMaxSlabs];
};

__device__ __forceinline__ void slab_range(const SlabCtl *ctl, int n_slabs, float *lo, float *width)
{
    const float dmin = __uint_as_float(ctl->dist_min_bits) * 0.999f, dmax = __uint_as_float(ctl->dist_max_bits) * 1.001f;
    *lo = dmin;
    *width = fmaxf(dmax - dmin, 1e-12f) / (float)n_slabs;
}

// [edge(j), edge(j+1)) in t; the first slab has no lower and the last no upper bound
__device__ __forceinline__ void slab_edges(const SlabCtl *ctl, int n_slabs, int j, float *t_lo, float *t_hi)
{
#pragma clang fp contract(off)
    float lo, w;
    slab_range(ctl, n_slabs, &lo, &w);
    *t_lo = j == 0 ? -INFINITY : lo + (float)j * w;
    *t_hi = j == n_slabs - 1 ? INFINITY : lo + (float)(j + 1) * w;
}

__global__ void slab_init_kernel(SlabCtl *ctl)
{
    ctl->dist_min_bits = 0x7f800000u;      // +inf
    ctl->dist_max_bits = 0u;
    ctl->n_visible = 0;
    for (int j = 0; j < kMaxSlabs; ++j) ctl->slab_count[j] = 0;
}

// cull_chunks_kernel + every visible chunk's distance range from the camera centre
__global__ void slab_cull_kernel(const float4 *__restrict__ boxes, int n_chunks, RasterCam cam, int32_t *__restrict__ visible,
                                 float2 *__restrict__ range, SlabCtl *ctl)
{
    const int chunk = blockIdx.x * blockDim.x + threadIdx.x;
    if (chunk >= n_chunks) return;
    const float4 lo = boxes[chunk * 2], hi = boxes[chunk * 2 + 1];
    if (!(lo.x <= hi.x)) return;
    float minx = INFINITY, maxx = -INFINITY, miny = INFINITY, maxy = -INFINITY;
    bool keep = false;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float dx = ((k & 1) ? hi.x : lo.x) - cam.cx, dy = ((k & 2) ? hi.y : lo.y) - cam.cy, dz = ((k & 4) ? hi.z : lo.z) - cam.cz;
        const float xc = cam.r00 * dx + cam.r10 * dy + cam.r20 * dz;
        const float yc = cam.r01 * dx + cam.r11 * dy + cam.r21 * dz;
        const float zc = cam.r02 * dx + cam.r12 * dy + cam.r22 * dz;
        const float zv = -zc;
        if (!(zv > 1e-4f)) { keep = true; continue; }
        const float sx = cam.fx * (xc / zv) + cam.px0, sy = -cam.fy * (yc / zv) + cam.py0;
        minx = fminf(minx, sx); maxx = fmaxf(maxx, sx);
        miny = fminf(miny, sy); maxy = fmaxf(maxy, sy);
    }
    const float g = kRasterGuard + 1.0f;
    if (!keep)
        keep = (maxx + g >= 0.0f) && (maxy + g >= 0.0f) && (minx - g <= (float)(cam.w - 1)) && (miny - g <= (float)(cam.h - 1));
    if (!keep) return;
    // nearest and farthest point of the box from the camera centre
    const float nx = fmaxf(fmaxf(lo.x - cam.cx, cam.cx - hi.x), 0.0f), ny = fmaxf(fmaxf(lo.y - cam.cy, cam.cy - hi.y), 0.0f);
    const float nz = fmaxf(fmaxf(lo.z - cam.cz, cam.cz - hi.z), 0.0f);
    const float fx = fmaxf(fabsf(lo.x - cam.cx), fabsf(hi.x - cam.cx)), fy = fmaxf(fabsf(lo.y - cam.cy), fabsf(hi.y - cam.cy));
    const float fz = fmaxf(fabsf(lo.z - cam.cz), fabsf(hi.z - cam.cz));
    const float dmin = sqrtf(nx * nx + ny * ny + nz * nz) * 0.9999f, dmax = sqrtf(fx * fx + fy * fy + fz * fz) * 1.0001f + 1e-30f;
    visible[atomicAdd(&ctl->n_visible, 1)] = chunk;
    range[chunk] = make_float2(dmin, dmax);
    atomicMin(&ctl->dist_min_bits, __float_as_uint(dmin));
    atomicMax(&ctl->dist_max_bits, __float_as_uint(dmax));
}

// Every visible chunk goes to the slabs its distance range [dmin, dmax] (margins included) touches: j with
// edge(j+1) > dmin and edge(j) <= dmax -- decided by comparing with the EDGES the passes bin their hits by, so the
// assignment is a superset of the slabs a chunk's hits can fall into without a slab of slack either side (a first
// version added one: every chunk was rasterised three times).  The per-slab list positions are allotted per workgroup
// (LDS counters, one global atomic per slab and workgroup): 46 000 chunks on eight global counters took 1.4 ms.
__global__ __launch_bounds__(256) void slab_assign_kernel(const int32_t *__restrict__ visible, const float2 *__restrict__ range,
                                                          SlabCtl *ctl, int n_slabs, int n_chunks, int32_t *__restrict__ lists)
{
    __shared__ int s_cnt[kMaxSlabs], s_base[kMaxSlabs];
    if (threadIdx.x < kMaxSlabs) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    int chunk = -1, j0 = 0, j1 = -1;
    if (e < ctl->n_visible) {
        chunk = visible[e];
        const float2 r = range[chunk];
        const float dlo = r.x * 0.999f, dhi = r.y * 1.001f;
        j0 = n_slabs;
        for (int j = 0; j < n_slabs; ++j) {
            float t_lo, t_hi;
            slab_edges(ctl, n_slabs, j, &t_lo, &t_hi);
            if (t_hi > dlo && t_lo <= dhi) { j0 = j < j0 ? j : j0; j1 = j; }
        }
        for (int j = j0; j <= j1; ++j) atomicAdd(&s_cnt[j], 1);
    }
    __syncthreads();
    if (threadIdx.x < n_slabs) s_base[threadIdx.x] = s_cnt[threadIdx.x] ? atomicAdd(&ctl->slab_count[threadIdx.x], s_cnt[threadIdx.x]) : 0;
    __syncthreads();
    for (int j = j0; j <= j1; ++j) lists[(int64_t)j * n_chunks + atomicAdd(&s_base[j], 1)] = chunk;
}

// Between two slab passes: every ray's direction and the count its pixel holds now, as one 16-byte record (the stop rule
// of the next pass is decided on THIS count, see raster_triangle).
__global__ void slab_ray_records_kernel(const float *__restrict__ rays_d, const int32_t *__restrict__ hit_count, int64_t n,
                                        float4 *__restrict__ rec)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        rec[i] = make_float4(rays_d[i * 3], rays_d[i * 3 + 1], rays_d[i * 3 + 2], __int_as_float(hit_count[i]));
}

template <int kRasterLanes>
__global__ __launch_bounds__(256) void raster_slab_kernel(const float4 *__restrict__ tris, int64_t n_tri, RasterCam cam,
                                                          const float *__restrict__ rays_o, const float *__restrict__ rays_d,
                                                          int capacity, uint64_t *__restrict__ keys, int32_t *__restrict__ hit_count,
                                                          int32_t *__restrict__ overflow, const int32_t *__restrict__ list,
                                                          const SlabCtl *__restrict__ ctl, int slab_j, int n_slabs, int stop_at,
                                                          const float4 *__restrict__ ray_rec,
                                                          const int32_t *__restrict__ ray_flag)
{
    if (ray_flag && *ray_flag) return;           // see raster_kernel
    const bool cam_origin = ray_flag != nullptr;
    constexpr int kTrisPerBlock = 256 / kRasterLanes;
    constexpr int kBlocksPerChunk = kCullChunk / kTrisPerBlock;
    const int n_items = ctl->slab_count[slab_j] * kBlocksPerChunk;
    SlabArgs sa;
    slab_edges(ctl, n_slabs, slab_j, &sa.t_lo, &sa.t_hi);
    sa.stop_at = stop_at;
    sa.keys = keys;
    sa.ray_rec = ray_rec;
    const int sub = threadIdx.x % kRasterLanes;
    for (int item = blockIdx.x; item < n_items; item += gridDim.x) {
        const int chunk = list[item / kBlocksPerChunk];
        const int64_t tri_i = (int64_t)chunk * kCullChunk + (item % kBlocksPerChunk) * kTrisPerBlock + threadIdx.x / kRasterLanes;
        if (tri_i < n_tri)
            raster_triangle<kRasterLanes, true, true>(tris, tri_i, sub, cam, rays_o, rays_d, capacity, nullptr, nullptr,
                                                      hit_count, overflow, cam_origin, sa);
    }
}

// Dense scenes (more than K candidates on most rays): the camera-coherent pass collects up to `wide` candidates per
// ray in [slot][ray] lists, and this kernel keeps each ray's K nearest under (t, tri) -- the rule of
// bvh_traverse_kernel -- in the ordinary [ray][K] lists (arrival order; qf_pack_samples sorts).  lane = ray, its K
// running entries in a private LDS column.  Rays that lost candidates even at `wide` keep count > K and go to
// qf_bvh_repair_overflow.
constexpr int kSelectBlock = 64;     // one wave: K = 64 (+ headroom) needs 36 KB of LDS
constexpr int kSelectHeadroom = 8;   // with the re-origin rule: candidates kept beyond K so that dropped hits can be replaced
__host__ __device__ inline int select_capacity(int max_hits, int wide, float min_sep)
{
    const int cap = min_sep > 0.0f ? max_hits + kSelectHeadroom : max_hits;
    return cap < wide ? cap : wide;
}
// the first `count` keys of a lane's LDS column -> its [K] row of the hit lists, four entries per memory request
__device__ __forceinline__ void write_row_from_keys(const uint64_t *lk, int count, float *row_t, int32_t *row_i)
{
    int i = 0;
    for (; i + 4 <= count; i += 4) {
        f32x4u t4;
        i32x4u i4;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint64_t k = lk[(i + e) * kSelectBlock];
            t4[e] = key_t(k);
            i4[e] = key_id(k);
        }
        *reinterpret_cast<f32x4u *>(row_t + i) = t4;
        *reinterpret_cast<i32x4u *>(row_i + i) = i4;
    }
    for (; i < count; ++i) {
        const uint64_t k = lk[i * kSelectBlock];
        row_t[i] = key_t(k);
        row_i[i] = key_id(k);
    }
}

// kKeys: the candidates are 8-byte keys (t bits << 32 | tri) in wide_key [wide][n_rays] (the depth-slab pass).
template <bool kKeys>
__global__ __launch_bounds__(kSelectBlock) void select_nearest_kernel(int64_t n_rays, int wide, int max_hits, float min_sep,
                                                                      const int32_t *__restrict__ wide_tri,
                                                                      const float *__restrict__ wide_t,
                                                                      const uint64_t *__restrict__ wide_key,
                                                                      int32_t *__restrict__ hit_tri, float *__restrict__ hit_t,
                                                                      int32_t *__restrict__ hit_count)
{
    // the lane's column: [cap][block] 8-byte keys (t bits << 32 | tri) -- key order IS the (t, tri) order, so the
    // insertion below is one LDS read, one 64-bit compare and one LDS write per shifted entry (it was two of each on
    // separate t / tri columns: selection 0.42 -> 0.3 ms on configs[2])
    extern __shared__ __attribute__((aligned(8))) unsigned char select_lds[];
    const int cap = select_capacity(max_hits, wide, min_sep);
    uint64_t *lk = reinterpret_cast<uint64_t *>(select_lds) + threadIdx.x;
    const int64_t r = (int64_t)blockIdx.x * kSelectBlock + threadIdx.x;
    if (r >= n_rays) return;
    const int cnt = hit_count[r];
    if (cnt > wide) return;
    float *row_t = hit_t + r * max_hits;
    int32_t *row_i = hit_tri + r * max_hits;
    if (cnt <= max_hits) {
        // a plain copy, eight slots per memory round trip (one slot per trip made this path -- most rays of a frame --
        // the kernel's duration: a wave per 64 rays, few waves per CU next to the selection's LDS columns)
        constexpr int kCopy = 8;
        for (int i0 = 0; i0 < cnt; i0 += kCopy) {
            float tb[kCopy];
            int ib[kCopy];
#pragma unroll
            for (int u = 0; u < kCopy; ++u) {
                const int i = i0 + u < cnt ? i0 + u : cnt - 1;
                if (kKeys) {
                    const uint64_t k = wide_key[(int64_t)i * n_rays + r];
                    tb[u] = key_t(k);
                    ib[u] = key_id(k);
                } else {
                    tb[u] = wide_t[(int64_t)i * n_rays + r];
                    ib[u] = wide_tri[(int64_t)i * n_rays + r];
                }
            }
#pragma unroll
            for (int q = 0; q < kCopy / 4; ++q) {
                if (i0 + 4 * q + 4 <= cnt) {                    // a whole quartet: one request per array
                    *reinterpret_cast<f32x4u *>(row_t + i0 + 4 * q) = (f32x4u){tb[4 * q], tb[4 * q + 1], tb[4 * q + 2], tb[4 * q + 3]};
                    *reinterpret_cast<i32x4u *>(row_i + i0 + 4 * q) = (i32x4u){ib[4 * q], ib[4 * q + 1], ib[4 * q + 2], ib[4 * q + 3]};
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (i0 + 4 * q + e < cnt) { row_t[i0 + 4 * q + e] = tb[4 * q + e]; row_i[i0 + 4 * q + e] = ib[4 * q + e]; }
                }
            }
        }
        return;
    }
    // the `held` nearest candidates under (t, tri) (all of them when cnt <= cap), kept SORTED in the column as they
    // arrive: an insertion shifts half the column on average, about what re-finding the maximum after a replacement
    // cost, and there is no sort left to do afterwards.  The candidates are read eight slots at a time: one slot per
    // pass is a dependent global load per pass, eight independent loads in flight cost the same latency once.
    const int held = cnt < cap ? cnt : cap;
    constexpr int kBatch = 8;
    int n = 0;
    uint64_t max_key = 0;                    // the column's last (largest) entry, in registers for the common reject
    for (int i0 = 0; i0 < cnt; i0 += kBatch) {
        uint64_t kb[kBatch];
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            const int i = i0 + u < cnt ? i0 + u : cnt - 1;
            if (kKeys) kb[u] = wide_key[(int64_t)i * n_rays + r];
            else kb[u] = hit_key(wide_t[(int64_t)i * n_rays + r], wide_tri[(int64_t)i * n_rays + r]);
        }
#pragma unroll
        for (int u = 0; u < kBatch; ++u) {
            if (i0 + u >= cnt) break;
            const uint64_t key = kb[u];
            int m;                           // entries of the column that stay: [0, m)
            if (n < held) {
                m = n;
                ++n;
            } else {
                if (!(key < max_key)) continue;
                m = n - 1;                   // the last entry falls out
            }
            // position by bisection (log2 dependent LDS reads instead of one per shifted entry), then the move with its
            // reads issued four at a time ahead of the writes (independent of each other; LDS executes a wave's
            // operations in order)
            int lo = 0, hi = m;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (lk[mid * kSelectBlock] < key) lo = mid + 1;
                else hi = mid;
            }
            int j = m - 1;
            for (; j - 3 >= lo; j -= 4) {
                const uint64_t a0 = lk[j * kSelectBlock], a1 = lk[(j - 1) * kSelectBlock], a2 = lk[(j - 2) * kSelectBlock],
                               a3 = lk[(j - 3) * kSelectBlock];
                lk[(j + 1) * kSelectBlock] = a0;
                lk[j * kSelectBlock] = a1;
                lk[(j - 1) * kSelectBlock] = a2;
                lk[(j - 2) * kSelectBlock] = a3;
            }
            for (; j >= lo; --j) lk[(j + 1) * kSelectBlock] = lk[j * kSelectBlock];
            lk[lo * kSelectBlock] = key;
            max_key = lk[(n - 1) * kSelectBlock];
        }
    }
    if (min_sep <= 0.0f) {                   // held == K: any order will do, qf_pack_samples sorts (this one is sorted)
        write_row_from_keys(lk, max_hits, row_t, row_i);
        hit_count[r] = max_hits;
        return;
    }
    // The re-origin rule (bvh8_traverse_kernel) runs over a ray's hits in ascending order, so the K nearest alone do
    // not decide it: every hit the chain drops lets a farther one in.  Run the chain over the held prefix of the
    // ray's hits.  K kept hits are the answer whatever lies behind; fewer are the answer only if the prefix was the
    // whole list.  Otherwise the ray goes to the paged BVH traversal (count > K marks it for qf_bvh_repair_overflow).
    float last_t = key_t(lk[0]);
    int kept = 1;                            // compacted in place: slot `kept` never runs ahead of slot i
    for (int i = 1; i < held && kept < max_hits; ++i) {
        const uint64_t k = lk[i * kSelectBlock];
        const float t = key_t(k);
        if (!(t > last_t + min_sep)) continue;
        last_t = t;
        lk[kept * kSelectBlock] = k;
        ++kept;
    }
    if (kept < max_hits && cnt > held) return;      // hit_count[r] stays > K
    write_row_from_keys(lk, kept, row_t, row_i);
    hit_count[r] = kept;
}

// In-place ascending (t, tri) sort of every ray's (unordered) list, the re-origin rule (min_sep > 0: keep a hit iff it
// is the first or lies more than min_sep behind the last kept one -- see bvh8_traverse_kernel), padding and count
// clamp.  Exact for rays whose list holds ALL their hits (count <= K); the camera-coherent path sends every other ray
// through the BVH repair first.  A workgroup stages 128 rays' rows in LDS (coalesced both ways), lane = ray.
constexpr int kFilterRays = 128;
__global__ __launch_bounds__(kFilterRays) void filter_hits_kernel(int64_t n_rays, int max_hits, float min_sep,
                                                                  int32_t *__restrict__ hit_tri, float *__restrict__ hit_t,
                                                                  int32_t *__restrict__ hit_count)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char filter_smem[];
    const int K = max_hits, Kp = max_hits | 1;
    float *s_t = reinterpret_cast<float *>(filter_smem);
    int32_t *s_tri = reinterpret_cast<int32_t *>(s_t + kFilterRays * Kp);
    const int tid = threadIdx.x;
    const int64_t ray0 = (int64_t)blockIdx.x * kFilterRays;
    const int nr = (int)((n_rays - ray0) < kFilterRays ? (n_rays - ray0) : kFilterRays);
    for (int i = tid; i < nr * K; i += kFilterRays) {
        const int r = i / K, k = i - r * K;
        s_t[r * Kp + k] = hit_t[ray0 * K + i];
        s_tri[r * Kp + k] = hit_tri[ray0 * K + i];
    }
    __syncthreads();
    if (tid < nr) {
        int cnt = hit_count[ray0 + tid];
        if (cnt > K) cnt = K;
        float *row_t = s_t + tid * Kp;
        int32_t *row_i = s_tri + tid * Kp;
        if (K <= 32) {
            if (cnt > 1) sort_row_32<true>(row_t, row_i, cnt);
        } else {
            for (int i = 1; i < cnt; ++i) {
                const float t = row_t[i];
                const int id = row_i[i];
                int j = i - 1;
                while (j >= 0 && hit_less(t, id, row_t[j], row_i[j])) { row_t[j + 1] = row_t[j]; row_i[j + 1] = row_i[j]; --j; }
                row_t[j + 1] = t;
                row_i[j + 1] = id;
            }
        }
        if (min_sep > 0.0f && cnt > 1) {
            int kept = 1;
            float last_t = row_t[0];
            for (int i = 1; i < cnt; ++i) {
                const float t = row_t[i];
                if (t > last_t + min_sep) { row_t[kept] = t; row_i[kept] = row_i[i]; ++kept; last_t = t; }
            }
            cnt = kept;
        }
        for (int i = cnt; i < K; ++i) { row_t[i] = INFINITY; row_i[i] = -1; }
        hit_count[ray0 + tid] = cnt;
    }
    __syncthreads();
    for (int i = tid; i < nr * K; i += kFilterRays) {
        const int r = i / K, k = i - r * K;
        hit_t[ray0 * K + i] = s_t[r * Kp + k];
        hit_tri[ray0 * K + i] = s_tri[r * Kp + k];
    }
}

}  // namespace

static int filter_launch(int64_t n_rays, int32_t max_hits, float min_sep, int32_t *hit_tri, float *hit_t,
                         int32_t *hit_count, hipStream_t st)
{
    const int Kp = max_hits | 1;
    const size_t lds = (size_t)kFilterRays * Kp * 8;
    const int64_t blocks = qf_div_up(n_rays, kFilterRays);
    if (blocks > 0x7fffffff) return QF_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(filter_hits_kernel, dim3((unsigned)blocks), dim3(kFilterRays), lds, st, n_rays, (int)max_hits, min_sep,
                       hit_tri, hit_t, hit_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_filter_hits(const qf_bvh *bvh, int64_t n_rays, int32_t max_hits, int32_t *hit_tri, float *hit_t,
                              int32_t *hit_count, void *stream)
{
    if (!bvh || n_rays < 0 || max_hits < 1 || max_hits > kMaxHits) return QF_ERR_INVALID_ARGUMENT;
    if (n_rays == 0 || !(bvh->min_sep > 0.0f)) return QF_OK;       // rule off: the lists stay as they are
    if (!hit_tri || !hit_t || !hit_count) return QF_ERR_INVALID_ARGUMENT;
    return filter_launch(n_rays, max_hits, bvh->min_sep, hit_tri, hit_t, hit_count, qf_stream(stream));
}

static RasterCam make_raster_cam(const qf_camera *cam)
{
    RasterCam rc;
    const float *m = cam->c2w;     // row-major 3x4
    rc.r00 = m[0]; rc.r01 = m[1]; rc.r02 = m[2]; rc.cx = m[3];
    rc.r10 = m[4]; rc.r11 = m[5]; rc.r12 = m[6]; rc.cy = m[7];
    rc.r20 = m[8]; rc.r21 = m[9]; rc.r22 = m[10]; rc.cz = m[11];
    rc.fx = cam->fx; rc.fy = cam->fy;
    rc.px0 = cam->cx - 0.5f;       // camera_dir.x = (x - cx + 0.5) / fx
    rc.py0 = cam->cy - 0.5f;
    rc.w = cam->width; rc.h = cam->height;
    return rc;
}

// chunk boxes of the handle's triangles (allocated on first use, recomputed after a build / refit)
static int ensure_chunk_boxes(qf_bvh *bvh, hipStream_t st)
{
    const int64_t n_chunks = qf_div_up(bvh->n_tri, kCullChunk);
    if (n_chunks > 0x3fffffff) return QF_ERR_UNSUPPORTED;
    if (!bvh->d_chunk_box) {
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_chunk_box, (size_t)n_chunks * 2 * sizeof(float4)));
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_visible, (size_t)(n_chunks + 2) * sizeof(int32_t)));
        QF_HIP_TRY(hipMemsetAsync(bvh->d_visible, 0, 2 * sizeof(int32_t), st));        // the two counters
        bvh->chunk_dirty = true;
        bvh->cull_parity = 0;
    }
    if (bvh->chunk_dirty) {
        hipLaunchKernelGGL(chunk_boxes_kernel, dim3((unsigned)qf_div_up(n_chunks * 64, 256)), dim3(256), 0, st,
                           reinterpret_cast<const float4 *>(bvh->d_tris), bvh->n_tri, (int)n_chunks,
                           reinterpret_cast<float4 *>(bvh->d_chunk_box));
        QF_LAUNCH_CHECK();
        bvh->chunk_dirty = false;
    }
    return QF_OK;
}

// zero the counts, the overflow counter and the origin flag: one fill launch when the caller laid them out back to back
// (hit_count [n_rays] | overflow | origin flag)
static int raster_zero(int64_t n_rays, int32_t *hit_count, int32_t *overflow, int32_t *origin_flag, hipStream_t st)
{
    int64_t words = n_rays;
    bool ovf_done = false, flag_done = origin_flag == nullptr;
    if (overflow == hit_count + words) { ++words; ovf_done = true; }
    if (ovf_done && origin_flag == hit_count + words) { ++words; flag_done = true; }
    QF_HIP_TRY(hipMemsetAsync(hit_count, 0, (size_t)words * sizeof(int32_t), st));
    if (!ovf_done) QF_HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(int32_t), st));
    if (!flag_done) QF_HIP_TRY(hipMemsetAsync(origin_flag, 0, sizeof(int32_t), st));
    return QF_OK;
}

// Lanes per triangle: the per-triangle set-up (projection, edge equations) is replicated in every lane, so few lanes win
// for pixel-sized triangles (measured on the 983 040-triangle 800x800 frame: 1/2/4/8 lanes -> 0.33/0.25/0.22/0.23 ms);
// meshes that are coarse relative to the image get more lanes per triangle.  (A band's pass is latency-, not
// throughput-bound, but more lanes per triangle did not help it either: N = 8 band 0.35 / 0.37 / 0.36 ms with 4 / 8 / 16
// lanes.)
static int raster_lanes(int64_t n_rays, int64_t n_tri)
{
    const int64_t pixels_per_tri = n_rays / n_tri;
    return pixels_per_tri > 64 ? 16 : (pixels_per_tri > 8 ? 8 : 4);
}

// f(std::integral_constant<int, L>()) for the kernel instantiation with L = `lanes` (16, 8 or 4) lanes per triangle
template <typename F>
static void with_lanes(int lanes, F &&f)
{
    switch (lanes) {
    case 16: f(std::integral_constant<int, 16>()); break;
    case 8: f(std::integral_constant<int, 8>()); break;
    default: f(std::integral_constant<int, 4>()); break;
    }
}

// the resident grid of a pass over a chunk list (raster_culled_kernel, raster_slab_kernel)
static unsigned chunk_grid(int64_t n_chunks, int lanes)
{
    const int64_t items = n_chunks * (kCullChunk * lanes / 256);
    const int64_t cap = (int64_t)qf_cu_count_cached() * 8;
    return (unsigned)(items < cap ? items : cap);
}

// the ray check of the passes without a cull launch to carry it (cull_chunks_kernel does, see camera_rays_check_kernel)
static void camera_check_launch(const RasterCam &rc, const float *rays_o, const float *rays_d, int64_t n_rays,
                                int32_t *origin_flag, hipStream_t st)
{
    if (origin_flag)
        hipLaunchKernelGGL(camera_rays_check_kernel, dim3(qf_grid_1d(n_rays, 256)), dim3(256), 0, st,
                           reinterpret_cast<const uint32_t *>(rays_o), rays_d, n_rays, rc, origin_flag);
}

static int raster_launch(qf_bvh *bvh, const qf_camera *cam, const float *rays_o, const float *rays_d, int64_t n_rays,
                         int capacity, bool wide, int32_t *hit_tri, float *hit_t, int32_t *hit_count, int32_t *overflow,
                         int32_t *origin_flag, bool cull, hipStream_t st, bool skip_ids = false)
{
    if (skip_ids) hit_tri = nullptr;         // the pass leaves the id lists alone (qf_raster_intersect sort_lists = 2)
    const int rc_zero = raster_zero(n_rays, hit_count, overflow, origin_flag, st);
    if (rc_zero != QF_OK) return rc_zero;
    if (bvh->n_tri == 0) return QF_OK;
    const RasterCam rc = make_raster_cam(cam);
    const float4 *tris4 = reinterpret_cast<const float4 *>(bvh->d_tris);
    const int lanes = raster_lanes(n_rays, bvh->n_tri);
    const int64_t blocks = qf_div_up(bvh->n_tri * lanes, 256);
    if (blocks > 0x7fffffff) return QF_ERR_UNSUPPORTED;
    if (cull) {
        // chunk boxes (once per build / refit), the visible-chunk list of this camera, then a resident grid over it
        const int64_t n_chunks = qf_div_up(bvh->n_tri, kCullChunk);
        const int rc_boxes = ensure_chunk_boxes(bvh, st);
        if (rc_boxes != QF_OK) return rc_boxes;
        float4 *boxes = reinterpret_cast<float4 *>(bvh->d_chunk_box);
        int32_t *counters = bvh->d_visible, *visible = bvh->d_visible + 2;
        const int parity = bvh->cull_parity;
        bvh->cull_parity ^= 1;
        bvh->cull_last = parity;
        hipLaunchKernelGGL(cull_chunks_kernel, dim3((unsigned)qf_div_up(n_chunks, 256)), dim3(256), 0, st, boxes,
                           (int)n_chunks, rc, visible, counters, parity, reinterpret_cast<const uint32_t *>(rays_o), rays_d,
                           n_rays, origin_flag);
        QF_LAUNCH_CHECK();
        with_lanes(lanes, [&](auto L) {
            auto *kernel = wide ? raster_culled_kernel<decltype(L)::value, true> : raster_culled_kernel<decltype(L)::value, false>;
            hipLaunchKernelGGL(kernel, dim3(chunk_grid(n_chunks, lanes)), dim3(256), 0, st, tris4, bvh->n_tri, rc, rays_o, rays_d,
                               capacity, hit_tri, hit_t, hit_count, overflow, visible, counters + parity, origin_flag);
        });
    } else {
        camera_check_launch(rc, rays_o, rays_d, n_rays, origin_flag, st);
        QF_LAUNCH_CHECK();
        with_lanes(lanes, [&](auto L) {
            auto *kernel = wide ? raster_kernel<decltype(L)::value, true> : raster_kernel<decltype(L)::value, false>;
            hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, tris4, bvh->n_tri, rc, rays_o, rays_d, capacity,
                               hit_tri, hit_t, hit_count, overflow, origin_flag);
        });
    }
    QF_LAUNCH_CHECK();
    return QF_OK;
}

static bool raster_args_ok(const qf_bvh *bvh, const qf_camera *cam, int64_t n_rays, int32_t max_hits)
{
    if (!bvh || !cam || n_rays < 0 || max_hits < 1 || max_hits > kMaxHits) return false;
    if (cam->width < 1 || cam->height < 1 || (int64_t)cam->width * cam->height != n_rays) return false;
    return cam->fx > 0.0f && cam->fy > 0.0f;
}

extern "C" int qf_raster_intersect(qf_bvh *bvh, const qf_camera *cam, const float *rays_o, const float *rays_d,
                                   int64_t n_rays, int32_t max_hits, int32_t *hit_tri, float *hit_t, int32_t *hit_count,
                                   int32_t *overflow, int32_t sort_lists, int32_t cull_chunks, int32_t *origin_flag,
                                   void *stream)
{
    if (!raster_args_ok(bvh, cam, n_rays, max_hits)) return QF_ERR_INVALID_ARGUMENT;
    if (!rays_o || !rays_d || !hit_tri || !hit_t || !hit_count || !overflow) return QF_ERR_INVALID_ARGUMENT;
    if (sort_lists < 0 || sort_lists > 2) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    const int rc = raster_launch(bvh, cam, rays_o, rays_d, n_rays, (int)max_hits, false, hit_tri, hit_t, hit_count, overflow,
                                 origin_flag, cull_chunks != 0, st, sort_lists == 2);
    if (rc != QF_OK) return rc;
    if (sort_lists == 1 && n_rays > 0) return filter_launch(n_rays, max_hits, bvh->min_sep, hit_tri, hit_t, hit_count, st);
    return QF_OK;
}

extern "C" int64_t qf_hit_bins_bytes(int32_t width, int32_t height, int32_t max_hits)
{
    if (width < 1 || height < 1 || max_hits < 1 || max_hits > kMaxHits) return -1;
    return (int64_t)((width + 7) / 8) * ((height + 7) / 8) * 64 * max_hits * (int64_t)sizeof(uint2);
}

extern "C" int qf_raster_intersect_tiles(qf_bvh *bvh, const qf_camera *cam, const float *rays_o, const float *rays_d,
                                         int64_t n_rays, int32_t max_hits, int32_t *tile_cursor, uint64_t *tile_mask,
                                         void *bins, int64_t bins_bytes, int32_t *hit_count, int32_t *overflow,
                                         int32_t *origin_flag, void *stream)
{
    if (!raster_args_ok(bvh, cam, n_rays, max_hits)) return QF_ERR_INVALID_ARGUMENT;
    if (!rays_o || !rays_d || !tile_cursor || !tile_mask || !bins || !hit_count || !overflow) return QF_ERR_INVALID_ARGUMENT;
    if (bins_bytes < qf_hit_bins_bytes(cam->width, cam->height, max_hits)) return QF_ERR_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(bins) % sizeof(uint2) || reinterpret_cast<uintptr_t>(tile_mask) % sizeof(uint64_t))
        return QF_ERR_INVALID_ARGUMENT;
    if (bvh->n_tri >= (1 << kBinIdBits)) return QF_ERR_UNSUPPORTED;         // the record's id field
    hipStream_t st = qf_stream(stream);
    const int tiles_x = (cam->width + 7) / 8, n_tiles = tiles_x * ((cam->height + 7) / 8);
    // only the cursors, the overflow word and the ray flag are zeroed: tile_count_kernel writes every count
    QF_HIP_TRY(hipMemsetAsync(tile_cursor, 0, (size_t)n_tiles * sizeof(int32_t), st));
    if (origin_flag == overflow + 1) {
        QF_HIP_TRY(hipMemsetAsync(overflow, 0, 2 * sizeof(int32_t), st));
    } else {
        QF_HIP_TRY(hipMemsetAsync(overflow, 0, sizeof(int32_t), st));
        if (origin_flag) QF_HIP_TRY(hipMemsetAsync(origin_flag, 0, sizeof(int32_t), st));
    }
    const RasterCam rc = make_raster_cam(cam);
    uint2 *records = reinterpret_cast<uint2 *>(bins);
    if (bvh->n_tri > 0) {
        const int lanes = raster_lanes(n_rays, bvh->n_tri);
        const int64_t blocks = qf_div_up(bvh->n_tri * lanes, 256);
        if (blocks > 0x7fffffff) return QF_ERR_UNSUPPORTED;
        camera_check_launch(rc, rays_o, rays_d, n_rays, origin_flag, st);
        QF_LAUNCH_CHECK();
        with_lanes(lanes, [&](auto L) {
            hipLaunchKernelGGL(raster_bins_kernel<decltype(L)::value>, dim3((unsigned)blocks), dim3(256), 0, st,
                               reinterpret_cast<const float4 *>(bvh->d_tris), bvh->n_tri, rc, rays_o, rays_d, (int)max_hits,
                               tile_cursor, records, origin_flag);
        });
    }
    hipLaunchKernelGGL(tile_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, st, tile_cursor, records, (int)max_hits,
                       rc.w, rc.h, tiles_x, hit_count, overflow, tile_mask);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_raster_intersect_wide(qf_bvh *bvh, const qf_camera *cam, const float *rays_o, const float *rays_d,
                                        int64_t n_rays, int32_t max_hits, int32_t wide_hits, int32_t *wide_tri,
                                        float *wide_t, int32_t *hit_tri, float *hit_t, int32_t *hit_count,
                                        int32_t *overflow, int32_t cull_chunks, int32_t *origin_flag, void *stream)
{
    if (!raster_args_ok(bvh, cam, n_rays, max_hits)) return QF_ERR_INVALID_ARGUMENT;
    if (wide_hits < max_hits || wide_hits > 4096) return QF_ERR_INVALID_ARGUMENT;
    if (!rays_o || !rays_d || !wide_tri || !wide_t || !hit_tri || !hit_t || !hit_count || !overflow)
        return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    const int rc = raster_launch(bvh, cam, rays_o, rays_d, n_rays, (int)wide_hits, true, wide_tri, wide_t, hit_count, overflow,
                                 origin_flag, cull_chunks != 0, st);
    if (rc != QF_OK) return rc;
    if (n_rays == 0) return QF_OK;
    const size_t lds = (size_t)select_capacity(max_hits, wide_hits, bvh->min_sep) * kSelectBlock * 2 * sizeof(float);
    hipLaunchKernelGGL(select_nearest_kernel<false>, dim3((unsigned)qf_div_up(n_rays, kSelectBlock)), dim3(kSelectBlock), lds, st,
                       n_rays, (int)wide_hits, (int)max_hits, bvh->min_sep, wide_tri, wide_t, (const uint64_t *)nullptr, hit_tri,
                       hit_t, hit_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int qf_raster_intersect_slabs(qf_bvh *bvh, const qf_camera *cam, const float *rays_o, const float *rays_d,
                                         int64_t n_rays, int32_t max_hits, int32_t wide_hits, int32_t n_slabs,
                                         uint64_t *wide_keys, int32_t *hit_tri, float *hit_t, int32_t *hit_count,
                                         int32_t *overflow, int32_t *origin_flag, void *stream)
{
    if (!raster_args_ok(bvh, cam, n_rays, max_hits)) return QF_ERR_INVALID_ARGUMENT;
    if (n_slabs < 2 || n_slabs > kMaxSlabs) return QF_ERR_INVALID_ARGUMENT;
    const int sel_cap = select_capacity(max_hits, wide_hits, bvh->min_sep);
    if (wide_hits <= sel_cap + 1 || wide_hits > 4096) return QF_ERR_INVALID_ARGUMENT;     // room beyond stop_at for one slab's hits
    if (!rays_o || !rays_d || !wide_keys || !hit_tri || !hit_t || !hit_count || !overflow) return QF_ERR_INVALID_ARGUMENT;
    hipStream_t st = qf_stream(stream);
    const int rc_zero = raster_zero(n_rays, hit_count, overflow, origin_flag, st);
    if (rc_zero != QF_OK) return rc_zero;
    if (n_rays == 0 || bvh->n_tri == 0) return QF_OK;
    const int rc_boxes = ensure_chunk_boxes(bvh, st);
    if (rc_boxes != QF_OK) return rc_boxes;
    const int64_t n_chunks = qf_div_up(bvh->n_tri, kCullChunk);
    if (!bvh->d_slab_range) {
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_slab_range, (size_t)n_chunks * sizeof(float2)));
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_slab_lists, (size_t)n_chunks * kMaxSlabs * sizeof(int32_t)));
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_slab_ctl, sizeof(SlabCtl)));
    }
    const RasterCam rc = make_raster_cam(cam);
    const float4 *tris4 = reinterpret_cast<const float4 *>(bvh->d_tris);
    const float4 *boxes = reinterpret_cast<const float4 *>(bvh->d_chunk_box);
    int32_t *visible = bvh->d_visible + 2;
    bvh->cull_last = -1;                     // slab_cull_kernel overwrites the culled passes' list (its count is the control block's)
    float2 *range = reinterpret_cast<float2 *>(bvh->d_slab_range);
    SlabCtl *ctl = reinterpret_cast<SlabCtl *>(bvh->d_slab_ctl);
    camera_check_launch(rc, rays_o, rays_d, n_rays, origin_flag, st);
    hipLaunchKernelGGL(slab_init_kernel, dim3(1), dim3(1), 0, st, ctl);
    hipLaunchKernelGGL(slab_cull_kernel, dim3((unsigned)qf_div_up(n_chunks, 256)), dim3(256), 0, st, boxes, (int)n_chunks, rc,
                       visible, range, ctl);
    hipLaunchKernelGGL(slab_assign_kernel, dim3((unsigned)qf_div_up(n_chunks, 256)), dim3(256), 0, st, visible, range, ctl,
                       (int)n_slabs, (int)n_chunks, bvh->d_slab_lists);
    QF_LAUNCH_CHECK();
    const int lanes = raster_lanes(n_rays, bvh->n_tri);
    const unsigned grid = chunk_grid(n_chunks, lanes);
    const int stop_at = sel_cap + 1;
    // the counts at the start of each later pass, in one record with the ray's direction: rewritten between the passes
    if (bvh->slab_snapshot_rays < n_rays) {
        // hipFree synchronises the device: grow geometrically, so that a renderer whose ray count creeps up (row bands
        // that move with the cost profile) frees O(log n) times in its life and a steady-state frame never does
        const int64_t grown = bvh->slab_snapshot_rays * 2 > n_rays ? bvh->slab_snapshot_rays * 2 : n_rays;
        if (bvh->d_slab_snapshot) (void)hipFree(bvh->d_slab_snapshot);
        bvh->d_slab_snapshot = nullptr;
        bvh->slab_snapshot_rays = 0;
        QF_HIP_TRY(hipMalloc((void **)&bvh->d_slab_snapshot, (size_t)grown * sizeof(float4)));
        bvh->slab_snapshot_rays = grown;
    }
    float4 *snapshot = reinterpret_cast<float4 *>(bvh->d_slab_snapshot);
    for (int j = 0; j < n_slabs; ++j) {
        if (j > 0) {
            hipLaunchKernelGGL(slab_ray_records_kernel, dim3(qf_grid_1d(n_rays, 256)), dim3(256), 0, st, rays_d, hit_count,
                               n_rays, snapshot);
            QF_LAUNCH_CHECK();
        }
        const int32_t *list = bvh->d_slab_lists + (int64_t)j * n_chunks;
        with_lanes(lanes, [&](auto L) {
            hipLaunchKernelGGL(raster_slab_kernel<decltype(L)::value>, dim3(grid), dim3(256), 0, st, tris4, bvh->n_tri, rc, rays_o,
                               rays_d, (int)wide_hits, wide_keys, hit_count, overflow, list, ctl, j, (int)n_slabs, stop_at,
                               j == 0 ? (const float4 *)nullptr : snapshot, origin_flag);
        });
    }
    QF_LAUNCH_CHECK();
    const size_t lds = (size_t)sel_cap * kSelectBlock * 2 * sizeof(float);
    hipLaunchKernelGGL(select_nearest_kernel<true>, dim3((unsigned)qf_div_up(n_rays, kSelectBlock)), dim3(kSelectBlock), lds, st,
                       n_rays, (int)wide_hits, (int)max_hits, bvh->min_sep, (const int32_t *)nullptr, (const float *)nullptr,
                       wide_keys, hit_tri, hit_t, hit_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}

extern "C" int64_t qf_bvh_copy_visible_chunks(const qf_bvh *bvh, int32_t *chunks_host, int64_t capacity, void *stream)
{
    if (!bvh || capacity < 0 || (capacity > 0 && !chunks_host)) return QF_ERR_INVALID_ARGUMENT;
    if (!bvh->d_visible || bvh->cull_last < 0) return QF_ERR_INVALID_ARGUMENT;     // no culled call whose list is still there
    QF_HIP_TRY(hipStreamSynchronize(qf_stream(stream)));
    int32_t n = 0;
    QF_HIP_TRY(hipMemcpy(&n, bvh->d_visible + bvh->cull_last, sizeof(int32_t), hipMemcpyDeviceToHost));
    const int64_t n_chunks = qf_div_up(bvh->n_tri, kCullChunk);
    if (n < 0 || n > n_chunks) return QF_ERR_HIP;                                  // (the list holds n_chunks entries)
    const int64_t take = n < capacity ? n : capacity;
    if (take > 0) QF_HIP_TRY(hipMemcpy(chunks_host, bvh->d_visible + 2, (size_t)take * sizeof(int32_t), hipMemcpyDeviceToHost));
    return n;
}
