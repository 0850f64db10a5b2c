// Shared helpers of the index-exact kernels for gfx950: BVH multi-hit traversal (bvh_traverse.hip), the
// camera-coherent raster passes (raster.hip), sample packing / per-ray sorting (sample_pack.hip), texel lookup and
// baked-texture decode (texture.hip) and occupancy-grid marching (grid_march.hip).  Those translation units are
// compiled with -ffp-contract=off: every comparison that decides an INTEGER output (triangle id, hit count, sample
// order, texel index) uses a fixed sequence of individually rounded IEEE operations, restated independently by the
// oracle (oracle/intersect_ref.c, oracle/quantize.py), so those outputs are bit-exact against it.
//
// Replaces: trimesh/Embree `intersects_id` and the OptiX
// `Intersector.find_intersections` (examples/mesh_utils.py:77-96,350-354), the numpy argsort/lexsort
// of sampling_raytrace_numpy / sampling_indexing (mesh_utils.py:359-381,394-403),
// trimesh.triangles.points_to_barycentric + UV lookup (examples/utils.py:1055-1063) and
// FeatureCompression.get_features_from_texture_map (examples/texture_utils.py:149-175).
#pragma once
#include "qf_common.h"
#include "bvh.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxHits = QF_BVH_MAX_HITS;

// fp32 Moller-Trumbore, operation order shared verbatim (as a contract, not as code) with the oracle.
__device__ __forceinline__ bool mt_hit(const float4 a, const float4 b, const float4 c, const float ox, const float oy,
                                       const float oz, const float dx, const float dy, const float dz, float *t_out)
{
    const float e1x = b.x - a.x, e1y = b.y - a.y, e1z = b.z - a.z;
    const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
    const float px = dy * e2z - dz * e2y;
    const float py = dz * e2x - dx * e2z;
    const float pz = dx * e2y - dy * e2x;
    const float det = (e1x * px + e1y * py) + e1z * pz;
    if (!(det != 0.0f)) return false;
    const float inv = 1.0f / det;
    const float tx = ox - a.x, ty = oy - a.y, tz = oz - a.z;
    const float u = ((tx * px + ty * py) + tz * pz) * inv;
    if (!(u >= 0.0f && u <= 1.0f)) return false;
    const float qx = ty * e1z - tz * e1y;
    const float qy = tz * e1x - tx * e1z;
    const float qz = tx * e1y - ty * e1x;
    const float v = ((dx * qx + dy * qy) + dz * qz) * inv;
    if (!(v >= 0.0f && u + v <= 1.0f)) return false;
    const float t = ((e2x * qx + e2y * qy) + e2z * qz) * inv;
    if (!(t > 0.0f)) return false;
    *t_out = t;
    return true;
}

__device__ __forceinline__ float safe_inv(float d)
{
    const float tiny = 1e-30f;
    if (fabsf(d) < tiny) d = (d < 0.0f || (d == 0.0f && signbit(d))) ? -tiny : tiny;
    return 1.0f / d;
}

// (t, tri) lexicographic "a sorts before b"
__device__ __forceinline__ bool hit_less(float ta, int ia, float tb, int ib) { return ta < tb || (ta == tb && ia < ib); }

// Four consecutive list entries as ONE memory request.  A ray's list starts at ray * K entries, 4-byte aligned only
// (K = 25 is the default everywhere), and gfx9+ global memory takes dwordx4 accesses at dword alignment: these types
// make the compiler emit them.  The kernels that walk [ray][K] lists lane = ray are bound by the number of scattered
// per-lane requests (measured: ~4.75 us per million), so a row costs K / 4 of them instead of K.
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));
typedef int i32x4u __attribute__((ext_vector_type(4), aligned(4)));

// A hit as one 64-bit key: t > 0, so its bit pattern orders like its value, and the triangle id breaks ties --
// key order IS the (t, tri) order of the contract.
__device__ __forceinline__ uint64_t hit_key(float t, int id) { return ((uint64_t)__float_as_uint(t) << 32) | (uint32_t)id; }
__device__ __forceinline__ float key_t(uint64_t k) { return __uint_as_float((uint32_t)(k >> 32)); }
__device__ __forceinline__ int key_id(uint64_t k) { return (int)(uint32_t)k; }

// A lane's hit list (cnt <= 32 entries, contiguous in LDS) sorted ascending in t (kTri = false) or (t, tri) (kTri = true)
// THROUGH REGISTERS: a 32-key bitonic network, every index a compile-time constant, 240 compare-exchanges with no
// memory in between.  The per-lane insertion sort it replaces walked the row in LDS, one dependent read-modify-write per
// shift: ~18 us of a tile wave's ~40 us, which is what a row band of a frame sharded over 8 GPUs (one wave per SIMD,
// nothing to overlap with) waited for.  Same order: t > 0, so the bit pattern of t orders like its value, +inf pads the
// tail; hits with equal (t, tri) do not exist (a ray meets a triangle once), equal t alone are interchangeable samples.
template <bool kTri>
__device__ __forceinline__ void sort_row_32(float *row_t, int32_t *row_i, int cnt)
{
    if (kTri) {
        uint64_t key[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) key[k] = k < cnt ? hit_key(row_t[k], row_i[k]) : ~0ull;
#pragma unroll
        for (int k = 2; k <= 32; k <<= 1) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int l = i ^ (k - 1);
                if (l > i) { const uint64_t a = key[i], b = key[l]; key[i] = a < b ? a : b; key[l] = a < b ? b : a; }
            }
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int l = i ^ j;
                    if (l > i) { const uint64_t a = key[i], b = key[l]; key[i] = a < b ? a : b; key[l] = a < b ? b : a; }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < cnt) { row_t[k] = key_t(key[k]); row_i[k] = key_id(key[k]); }
    } else {
        float key[32];
#pragma unroll
        for (int k = 0; k < 32; ++k) key[k] = k < cnt ? row_t[k] : INFINITY;
#pragma unroll
        for (int k = 2; k <= 32; k <<= 1) {
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                const int l = i ^ (k - 1);
                if (l > i) { const float a = key[i], b = key[l]; key[i] = fminf(a, b); key[l] = fmaxf(a, b); }
            }
#pragma unroll
            for (int j = k >> 2; j > 0; j >>= 1) {
#pragma unroll
                for (int i = 0; i < 32; ++i) {
                    const int l = i ^ j;
                    if (l > i) { const float a = key[i], b = key[l]; key[i] = fminf(a, b); key[l] = fmaxf(a, b); }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 32; ++k)
            if (k < cnt) row_t[k] = key[k];
    }
}

}  // namespace
