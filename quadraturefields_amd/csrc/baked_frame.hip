// The baked-texture frame, shaded and composited front to back in ONE launch with early ray termination
// (DESIGN.md section 3.5b): composite_tiles_kernel's walk -- one wave per 8x8 tile, lane = pixel, step k handles the
// rank-k samples of the tile in depth order -- in which every lane SHADES its own sample (texture_shade_packed_kernel's
// texel lookup, decode and SG shading: texture_device.h) instead of reading a colour / density that a first launch wrote,
// and stops fetching once the optical depth in front of its next sample exceeds stop_tau.
//
// The rule: the rank-k sample of a pixel (k < count) contributes iff the optical depth accumulated before it satisfies
// cum <= stop_tau, cum being the fp32 value composite_step keeps (cum = cum + sigma * delta, each rounded on its own).
// A sample that does not contribute is not shaded and adds nothing to any sum; a pixel that has stopped stays stopped;
// stop_tau = +inf never stops (not even at cum = +inf).  The slots of the tile order depend on the counts alone, so the
// ballots that locate rank k run over count > k, never over "still alive".
#include "qf_common.h"
#include "composite_device.h"
#include "texture_device.h"

namespace {

constexpr int kTileWaves = 4;         // tiles in flight per workgroup: 256 threads fill the dequantiser tables once

// A step is a chain of dependent requests: the slot (triangle id, position, depth: contiguous runs) -> the triangle
// record (a 128-byte gather) -> the texel record (a 64-byte gather) -> the arithmetic.  The chain is software-pipelined
// one stage per iteration: iteration k asks for the texel record of rank k+1 (from the triangle record that arrived
// during iteration k-1), the triangle record of rank k+2 and the slot of rank k+3, and then shades rank k.  Everything
// ahead of rank k is SPECULATIVE: fetched for lanes that have not stopped by the time of the request, whether or not
// they contribute in the end -- what counts as shaded is the rule, not what was fetched.  Every speculative address
// comes from a valid slot (count > rank), so it is a valid triangle id and a clamped texel.
// The view direction is the same for all of a pixel's samples: pack_tiles_kernel (qf_pack_tiles, qf_pack_tiles_bins)
// writes one normalised vector per lane to every slot of that lane, the same bits -- it is read once, at rank 0.
__global__ __launch_bounds__(64 * kTileWaves) void texture_composite_tiles_kernel(
    const uint8_t *__restrict__ records, int size, int n_lobes, int sigmoid_codec, float lambda_thres,
    const TexelRecord *__restrict__ tri_records, const float *__restrict__ xyz_c, const float *__restrict__ dirs_c,
    const float *__restrict__ depth_c, const int32_t *__restrict__ tri_c, const int32_t *__restrict__ hit_count, int max_hits,
    const int64_t *__restrict__ tile_base, int w, int h, int tiles_x, int n_tiles, float delta_const, int bg_mode,
    const float *__restrict__ bkgd, float stop_tau, float *__restrict__ out_rgb, float *__restrict__ out_alpha,
    float *__restrict__ out_depth, float *__restrict__ out_packed, int32_t *__restrict__ shaded_count)
{
    __shared__ DequantTables s_tab;
    dequant_tables_fill(s_tab, threadIdx.x, sigmoid_codec, lambda_thres);
    __syncthreads();                                   // the only barrier: from here on the waves run on their own
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n16 = texel_record_pieces(n_lobes);
    const bool never = stop_tau == INFINITY;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int tile = blockIdx.x * kTileWaves + wave; tile < n_tiles; tile += gridDim.x * kTileWaves) {   // wave-uniform
        int64_t ray = 0;
        int cnt = 0;
        const int inside = qf_tile_lane_ray(tile, lane, w, h, tiles_x, 0, &ray);
        if (inside) cnt = hit_count[ray] < max_hits ? hit_count[ray] : max_hits;
        RayAccum acc;
        int n_shaded = 0;
        const unsigned long long mask0 = __ballot(cnt > 0);
        if (mask0 != 0ull) {                           // wave-uniform
            int64_t base = tile_base[tile];            // first slot of the rank the slot stage asks for next
            bool alive = true;                         // no sample of this pixel has failed the rule yet
            // the slot of rank 0 and the view direction
            int tri_a = 0;
            float xa = 0.0f, ya = 0.0f, za = 0.0f, dep_a = 0.0f;          // slot stage: rank k+2 at iteration k
            float dx = 0.0f, dy = 0.0f, dz = 0.0f;
            if (cnt > 0) {
                const int64_t pos = base + __popcll(mask0 & below);
                tri_a = tri_c[pos];
                xa = xyz_c[pos * 3]; ya = xyz_c[pos * 3 + 1]; za = xyz_c[pos * 3 + 2];
                dep_a = depth_c[pos];
                dx = dirs_c[pos * 3]; dy = dirs_c[pos * 3 + 1]; dz = dirs_c[pos * 3 + 2];
            }
            base += __popcll(mask0);
            float xb = 0.0f, yb = 0.0f, zb = 0.0f, dep_b = 0.0f;          // position / depth of rank k+1
            TexelRecord tr = {};                                           // triangle record of rank k+1
            uint32_t w0[kTexelRecord / 4], w1[kTexelRecord / 4];           // texel records of ranks k and k+1
#pragma unroll
            for (int i = 0; i < kTexelRecord / 4; ++i) w0[i] = w1[i] = 0u;
            float dep0 = 0.0f;
            for (int k = -2;; ++k) {
                // anyone left to shade at rank k or behind it?  (wave-uniform exit: a tile whose pixels have all stopped
                // or run out leaves at once)
                if (k >= 0 && __ballot(cnt > k && alive) == 0ull) break;
                // 1. rank k+1: its triangle record is here -> texel -> ask for the texel record
                if (k + 1 >= 0 && cnt > k + 1 && alive) {
                    int64_t rc[2];
                    texel_from_record(tr, xb, yb, zb, size, rc);
                    texel_record_load(records, rc[0] * size + rc[1], n16, w1);
                }
                // 2. rank k+2: ask for its triangle record (the id arrived with the slot)
                if (cnt > k + 2 && alive) tr = tri_records[tri_a];
                // 3. rank k+3: ask for its slot
                const unsigned long long next = __ballot(cnt > k + 3);
                int tri_n = 0;
                float xn = 0.0f, yn = 0.0f, zn = 0.0f, dep_n = 0.0f;
                if (cnt > k + 3 && alive) {
                    const int64_t pos = base + __popcll(next & below);
                    tri_n = tri_c[pos];
                    xn = xyz_c[pos * 3]; yn = xyz_c[pos * 3 + 1]; zn = xyz_c[pos * 3 + 2];
                    dep_n = depth_c[pos];
                }
                base += __popcll(next);
                // 4. rank k: the rule, then shade and composite
                if (k >= 0 && cnt > k && alive) {
                    if (never || acc.cum <= stop_tau) {
                        float c[3], sg;
                        texel_record_shade(s_tab, w0, n_lobes, dx, dy, dz, c, &sg);
                        const float tau = sample_tau(sg, delta_const);
                        composite_step(acc, tau, sample_alpha(tau), c[0], c[1], c[2], dep0);
                        ++n_shaded;
                    } else {
                        alive = false;
                    }
                }
                // every stage moves up one rank
#pragma unroll
                for (int i = 0; i < kTexelRecord / 4; ++i) w0[i] = w1[i];
                dep0 = dep_b;
                xb = xa; yb = ya; zb = za; dep_b = dep_a;
                tri_a = tri_n; xa = xn; ya = yn; za = zn; dep_a = dep_n;
            }
        }
        if (!inside) continue;
        float px[3];
        if (cnt > 0) {
            composite_blend(acc, bg_mode, bkgd, px);
        } else {                                       // fill_background_kernel's values
            px[0] = px[1] = px[2] = (bg_mode == QF_BG_BLACK || bg_mode == QF_BG_NONE) ? 0.0f : 1.0f;
        }
        if (shaded_count) shaded_count[ray] = n_shaded;
        if (out_packed) {              // [n, 5] = rgb | alpha | depth per pixel, as composite_tiles_kernel
            float *o = out_packed + ray * 5;
            o[0] = px[0]; o[1] = px[1]; o[2] = px[2]; o[3] = acc.ca; o[4] = acc.cd;
            continue;
        }
        out_rgb[ray * 3 + 0] = px[0];
        out_rgb[ray * 3 + 1] = px[1];
        out_rgb[ray * 3 + 2] = px[2];
        out_alpha[ray] = acc.ca;
        out_depth[ray] = acc.cd;
    }
}

}  // namespace

extern "C" int qf_texture_composite_tiles(const uint8_t *records, int32_t texture_size, int32_t n_lobes, int32_t sigmoid_codec,
                                          float lambda_thres, const void *triangle_records, const float *xyz_c,
                                          const float *dirs_c, const float *depth_c, const int32_t *tri_c,
                                          const int32_t *hit_count, int32_t max_hits, const int64_t *tile_base, int32_t width,
                                          int32_t height, float delta_const, int32_t bg_mode, const float *bkgd, float stop_tau,
                                          float *out_rgb, float *out_alpha, float *out_depth, float *out_packed,
                                          int32_t *shaded_count, void *stream)
{
    if (!records || !triangle_records || texture_size < 1) return QF_ERR_INVALID_ARGUMENT;
    if (n_lobes < 1 || n_lobes > QF_MAX_LOBES) return QF_ERR_UNSUPPORTED;
    if (width < 1 || height < 1 || max_hits < 1 || bg_mode < 0 || bg_mode > 3) return QF_ERR_INVALID_ARGUMENT;
    if (!xyz_c || !dirs_c || !depth_c || !tri_c || !hit_count || !tile_base) return QF_ERR_INVALID_ARGUMENT;
    if (!out_packed && (!out_rgb || !out_alpha || !out_depth)) return QF_ERR_INVALID_ARGUMENT;
    if (bg_mode == QF_BG_CUSTOM && !bkgd) return QF_ERR_INVALID_ARGUMENT;
    if (!(stop_tau >= 0.0f)) return QF_ERR_INVALID_ARGUMENT;                  // NaN or negative
    const int tiles_x = (width + 7) / 8, tiles_y = (height + 7) / 8;
    const int64_t n_tiles = (int64_t)tiles_x * tiles_y;
    if (n_tiles > (1 << 30)) return QF_ERR_INVALID_ARGUMENT;                   // the kernel's tile loop counts in int
    hipLaunchKernelGGL(texture_composite_tiles_kernel, dim3(qf_grid_1d(n_tiles * 64, 64 * kTileWaves)), dim3(64 * kTileWaves), 0,
                       qf_stream(stream), records, (int)texture_size, (int)n_lobes, (int)sigmoid_codec, lambda_thres,
                       static_cast<const TexelRecord *>(triangle_records), xyz_c, dirs_c, depth_c, tri_c, hit_count,
                       (int)max_hits, tile_base, (int)width, (int)height, tiles_x, (int)n_tiles, delta_const, (int)bg_mode, bkgd,
                       stop_tau, out_rgb, out_alpha, out_depth, out_packed, shaded_count);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
