// The front-to-back tile walk of the vertex-baked frames (DESIGN.md sections 3.5d and 3.5f), ONE copy for the fp32 table
// (vertex_baked.hip) and the quantised records (vertex_quant.hip): the two kernels differ only in where the three vertex
// rows of a sample come from, which is the `Rows` functor -- rows(v0, v1, v2, b, blend) fills the blend of the rows of
// vertices v0, v1, v2 with the weights b.  The rule, the pipeline and the outputs are the same instructions in both.
#pragma once
#include "composite_device.h"
#include "vertex_baked_device.h"

namespace {

constexpr int kVertexTileWaves = 4;   // tiles in flight per workgroup (the waves run on their own inside the walk)

// texture_composite_tiles_kernel's walk and rule (baked_frame.hip) with the vertex-baked shading.  A step is the chain
// slot (triangle id, position, depth: contiguous runs) -> triangle record (a 128-byte gather) -> three vertex rows
// (`rows`) -> the arithmetic.  The first two links are software-pipelined: iteration k asks for the slot of rank k+2 and
// the triangle record of rank k+1 and then shades rank k.  The vertex rows are NOT fetched ahead: a rank of fp32 rows in
// flight would be 3 * 12 more 16-byte pieces (144 registers) per lane at 6 lobes, and the rows of a sample that fails the
// rule are never read.  The record of rank k is consumed (barycentrics and vertex ids: 6 registers) before the record of
// rank k+1 is asked for into the same registers.  Everything ahead of rank k is speculative, fetched for lanes that have
// not stopped at the time of the request; every speculative address comes from a valid slot (count > rank).
// The view direction is the same for all of a pixel's samples (the tile pack writes one normalised vector per lane to
// every slot of that lane): it is read once, at rank 0.
template <class Rows>
__device__ __forceinline__ void vertex_tiles_walk(
    const Rows &rows, int n_lobes, const VertexTriRecord *__restrict__ tri_records, const float *__restrict__ xyz_c,
    const float *__restrict__ dirs_c, const float *__restrict__ depth_c, const int32_t *__restrict__ tri_c,
    const int32_t *__restrict__ hit_count, int max_hits, const int64_t *__restrict__ tile_base, int w, int h, int tiles_x,
    int n_tiles, float delta_const, int bg_mode, const float *__restrict__ bkgd, float stop_tau, float *__restrict__ out_rgb,
    float *__restrict__ out_alpha, float *__restrict__ out_depth, float *__restrict__ out_packed,
    int32_t *__restrict__ shaded_count)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool never = stop_tau == INFINITY;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int tile = blockIdx.x * kVertexTileWaves + wave; tile < n_tiles; tile += gridDim.x * kVertexTileWaves) {   // wave-uniform
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
            float xa = 0.0f, ya = 0.0f, za = 0.0f, dep_a = 0.0f;          // slot stage: rank k+1 at the top of iteration k
            float dx = 0.0f, dy = 0.0f, dz = 0.0f;
            if (cnt > 0) {
                const int64_t pos = base + __popcll(mask0 & below);
                tri_a = tri_c[pos];
                xa = xyz_c[pos * 3]; ya = xyz_c[pos * 3 + 1]; za = xyz_c[pos * 3 + 2];
                dep_a = depth_c[pos];
                dx = dirs_c[pos * 3]; dy = dirs_c[pos * 3 + 1]; dz = dirs_c[pos * 3 + 2];
            }
            base += __popcll(mask0);
            float x0 = 0.0f, y0 = 0.0f, z0 = 0.0f, dep0 = 0.0f;           // position / depth of rank k
            VertexTriRecord tr = {};                                       // triangle record of rank k, then of rank k+1
            for (int k = -1;; ++k) {
                // anyone left to shade at rank k or behind it?  (wave-uniform exit: a tile whose pixels have all stopped
                // or run out leaves at once)
                if (k >= 0 && __ballot(cnt > k && alive) == 0ull) break;
                // 1. rank k: the rule; its record is here -> barycentrics and vertex ids
                bool shade = false;
                float b[3] = {0.0f, 0.0f, 0.0f};
                int v0 = 0, v1 = 0, v2 = 0;
                if (k >= 0 && cnt > k && alive) {
                    if (never || acc.cum <= stop_tau) {
                        shade = true;
                        vertex_barycentrics(tr, x0, y0, z0, b);
                        v0 = tr.v[0]; v1 = tr.v[1]; v2 = tr.v[2];
                    } else {
                        alive = false;
                    }
                }
                // 2. rank k+1: ask for its triangle record (the id arrived with the slot)
                if (cnt > k + 1 && alive) tr = tri_records[tri_a];
                // 3. rank k+2: ask for its slot
                const unsigned long long next = __ballot(cnt > k + 2);
                int tri_n = 0;
                float xn = 0.0f, yn = 0.0f, zn = 0.0f, dep_n = 0.0f;
                if (cnt > k + 2 && alive) {
                    const int64_t pos = base + __popcll(next & below);
                    tri_n = tri_c[pos];
                    xn = xyz_c[pos * 3]; yn = xyz_c[pos * 3 + 1]; zn = xyz_c[pos * 3 + 2];
                    dep_n = depth_c[pos];
                }
                base += __popcll(next);
                // 4. rank k: the rows, the blend, shade and composite
                if (shade) {
                    float blend[kVertexRowMax];
                    rows(v0, v1, v2, b, blend);
                    float c[3];
                    vertex_blend_shade(blend, n_lobes, dx, dy, dz, c);
                    const float tau = sample_tau(vertex_blend_sigma(blend, n_lobes), delta_const);
                    composite_step(acc, tau, sample_alpha(tau), c[0], c[1], c[2], dep0);
                    ++n_shaded;
                }
                // every stage moves up one rank
                x0 = xa; y0 = ya; z0 = za; dep0 = dep_a;
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
