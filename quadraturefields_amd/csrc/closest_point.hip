// The closest point on a mesh (include/qf_closest_point.h states the rule in full; restated in
// numpy in tests/closest_point_reference.py): a best-first walk of the 8-wide BVH, EIGHT LANES PER QUERY like the ray
// traversal of bvh_traverse.hip.  Lane j of a query's octet takes child j's box of a node (the squared distance from
// the query to the box, fp64 from the fp32 box) or triangle j of a leaf (the fp64 region walk).  The nearest child that
// can still matter is taken next (DPP minimum over the octet), the others go to the octet's stack in LDS together with
// their box distance (fp32, rounded TOWARD ZERO: never above the fp64 value), so that an entry is dropped when it is
// popped if the best distance has passed it meanwhile.  The capacity of the stack is the tree's exact bound
// (qf_bvh::max_stack8): at most (children - 1) entries are pushed per visited node, as in the ray traversal.
//
// Why pruning is exact.  A subtree is skipped only when its box distance is STRICTLY greater than the bound (the best
// dist2 found so far, at first max_distance^2).  Every box holds its triangles' boxes (the builders and the refit
// inflate by eps >= 0), the point of rule 3 lies in its triangle's box coordinate by coordinate, and subtraction,
// squaring and the three-term sum are monotone under rounding: so a triangle's computed dist2 is never below the
// computed distance to any box above it, and a skipped subtree holds no triangle with dist2 <= bound.  Equality is
// visited, so of several triangles at the same dist2 the lowest id is found whatever the order of the walk.
//
// Each lane keeps the best (dist2, id, v, w) of the triangles IT tested; the octet shares only the bound (one 64-bit
// DPP minimum per leaf) and picks the winner once at the end.  Every floating-point operation of the result is written
// out below in the order of the header; the file is compiled with -ffp-contract=off.
#include "bvh.h"
#include "qf_closest_point.h"
#include "qf_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kOctQueries = 32;                 // queries per workgroup: 256 threads = 4 waves x 8 octets
constexpr int kCpThreads = kOctQueries * 8;
constexpr int kDone = (int)0x80000000;          // == QF_BVH8_EMPTY; no leaf token takes this value (n_tri < 2^28)

// The octet primitives of bvh_traverse.hip (which keeps its own in its anonymous namespace and is left as it is), with
// the 64-bit minimum this walk needs
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
template <int kCtrl>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v)
{
    const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)v, kCtrl, 0xf, 0xf, true);
    const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(v >> 32), kCtrl, 0xf, 0xf, true);
    return ((uint64_t)hi << 32) | lo;
}
__device__ __forceinline__ uint64_t oct_min_u64(uint64_t v)
{
    uint64_t o = dpp_u64<QF_DPP_QUAD_1032>(v); v = o < v ? o : v;
    o = dpp_u64<QF_DPP_QUAD_2301>(v); v = o < v ? o : v;
    o = dpp_u64<QF_DPP_HALF_MIRROR>(v); v = o < v ? o : v;
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

__device__ __forceinline__ double dot3(double ux, double uy, double uz, double vx, double vy, double vz)
{
    return (ux * vx + uy * vy) + uz * vz;
}
__device__ __forceinline__ double ratio(double num, double den) { return den > 0.0 ? num / den : 0.0; }

// One triangle against one query: rules 1 to 3 of the header
struct TriQuery {
    double qx, qy, qz;
    double ax, ay, az, bx, by, bz, cx, cy, cz;
    double abx, aby, abz, acx, acy, acz;
    double lox, loy, loz, hix, hiy, hiz;

    __device__ __forceinline__ double coord(double a, double b, double c, double ab, double ac, double lo, double hi, double v,
                                            double w) const
    {
        double p = (a + v * ab) + w * ac;
        p = p < lo ? lo : p;
        p = p > hi ? hi : p;
        return v == 1.0 ? b : (w == 1.0 ? c : p);
    }
    __device__ __forceinline__ double dist2(double v, double w) const
    {
        const double ex = qx - coord(ax, bx, cx, abx, acx, lox, hix, v, w);
        const double ey = qy - coord(ay, by, cy, aby, acy, loy, hiy, v, w);
        const double ez = qz - coord(az, bz, cz, abz, acz, loz, hiz, v, w);
        return (ex * ex + ey * ey) + ez * ez;
    }
};

__device__ __forceinline__ double min3(double a, double b, double c)
{
    double lo = b < a ? b : a;
    return c < lo ? c : lo;
}
__device__ __forceinline__ double max3(double a, double b, double c)
{
    double hi = b > a ? b : a;
    return c > hi ? c : hi;
}

__device__ __forceinline__ void tri_closest(double qx, double qy, double qz, const float4 A, const float4 B, const float4 C,
                                            double *v_out, double *w_out, double *d2_out)
{
    TriQuery t;
    t.qx = qx; t.qy = qy; t.qz = qz;
    t.ax = (double)A.x; t.ay = (double)A.y; t.az = (double)A.z;
    t.bx = (double)B.x; t.by = (double)B.y; t.bz = (double)B.z;
    t.cx = (double)C.x; t.cy = (double)C.y; t.cz = (double)C.z;
    t.abx = t.bx - t.ax; t.aby = t.by - t.ay; t.abz = t.bz - t.az;
    t.acx = t.cx - t.ax; t.acy = t.cy - t.ay; t.acz = t.cz - t.az;
    t.lox = min3(t.ax, t.bx, t.cx); t.loy = min3(t.ay, t.by, t.cy); t.loz = min3(t.az, t.bz, t.cz);
    t.hix = max3(t.ax, t.bx, t.cx); t.hiy = max3(t.ay, t.by, t.cy); t.hiz = max3(t.az, t.bz, t.cz);
    const double apx = qx - t.ax, apy = qy - t.ay, apz = qz - t.az;
    const double d1 = dot3(t.abx, t.aby, t.abz, apx, apy, apz), d2 = dot3(t.acx, t.acy, t.acz, apx, apy, apz);
    const double bpx = qx - t.bx, bpy = qy - t.by, bpz = qz - t.bz;
    const double d3 = dot3(t.abx, t.aby, t.abz, bpx, bpy, bpz), d4 = dot3(t.acx, t.acy, t.acz, bpx, bpy, bpz);
    const double cpx = qx - t.cx, cpy = qy - t.cy, cpz = qz - t.cz;
    const double d5 = dot3(t.abx, t.aby, t.abz, cpx, cpy, cpz), d6 = dot3(t.acx, t.acy, t.acz, cpx, cpy, cpz);
    const double vc = d1 * d4 - d3 * d2;
    const double vb = d5 * d2 - d1 * d6;
    const double va = d3 * d6 - d5 * d4;
    const double den_ab = d1 - d3, den_ac = d2 - d6;
    const double n_bc = d4 - d3, m_bc = d5 - d6;
    const double den_bc = n_bc + m_bc;
    double v, w;
    if (d1 <= 0.0 && d2 <= 0.0) {                                                   // A
        v = 0.0; w = 0.0;
    } else if (d3 >= 0.0 && d4 <= d3) {                                             // B
        v = 1.0; w = 0.0;
    } else if (vc <= 0.0 && d1 >= 0.0 && d3 <= 0.0 && den_ab > 0.0) {               // AB
        v = d1 / den_ab; w = 0.0;
    } else if (d6 >= 0.0 && d5 <= d6) {                                             // C
        v = 0.0; w = 1.0;
    } else if (vb <= 0.0 && d2 >= 0.0 && d6 <= 0.0 && den_ac > 0.0) {               // AC
        v = 0.0; w = d2 / den_ac;
    } else if (va <= 0.0 && n_bc >= 0.0 && m_bc >= 0.0 && den_bc > 0.0) {           // BC
        w = n_bc / den_bc; v = 1.0 - w;
    } else {                                                                        // the end of the walk (rule 2)
        const double s_ab = d1 <= 0.0 ? 0.0 : (d3 >= 0.0 ? 1.0 : ratio(d1, den_ab));
        const double s_ac = d2 <= 0.0 ? 0.0 : (d6 >= 0.0 ? 1.0 : ratio(d2, den_ac));
        const double s_bc = n_bc <= 0.0 ? 0.0 : (m_bc <= 0.0 ? 1.0 : ratio(n_bc, den_bc));
        v = s_ab; w = 0.0;
        double ed = t.dist2(v, w);
        double kd = t.dist2(0.0, s_ac);
        if (kd < ed) { v = 0.0; w = s_ac; ed = kd; }
        const double kv = 1.0 - s_bc;
        kd = t.dist2(kv, s_bc);
        if (kd < ed) { v = kv; w = s_bc; ed = kd; }
        if (va > 0.0 && vb > 0.0 && vc > 0.0) {
            const double r = 1.0 / ((va + vb) + vc);
            const double iv = vb * r, iw = vc * r;
            if (!(ed < t.dist2(iv, iw))) { v = iv; w = iw; }
        }
    }
    *v_out = v;
    *w_out = w;
    *d2_out = t.dist2(v, w);
}

struct CpArgs {
    const float4 *nodes, *tris;
    const double *points;
    int64_t n_points;
    double max2;
    int root_is_valid, stack_cap, n_blocks, blocks_per_xcd;
    int32_t *tri;
    double *bary, *dist2;
    unsigned long long *counts;
};

// LDS of a workgroup: [kOctQueries][stack_cap] entries = (fp32 bits of the box distance, rounded toward zero) << 32 | token
extern __shared__ uint64_t cp_lds[];

__global__ __launch_bounds__(kCpThreads) void closest_point_kernel(CpArgs a)
{
    __shared__ int s_counts[QF_CLOSEST_POINT_COUNTS];
    const int tid = threadIdx.x, j = tid & 7, q = tid >> 3;
    const int oct_base = (tid & 63) & 56;               // first lane of this octet within its wave
    if (tid < QF_CLOSEST_POINT_COUNTS) s_counts[tid] = 0;
    __syncthreads();
    // XCD x walks the x-th contiguous eighth of the blocks: its L2 holds the part of the tree that slice of the queries
    // meets (bvh_traverse.hip: xcd_block)
    const int block = (int)(blockIdx.x & 7) * a.blocks_per_xcd + (int)(blockIdx.x >> 3);
    const int64_t query = (int64_t)block * kOctQueries + q;
    if (block < a.n_blocks && query < a.n_points) {
        const double qx = a.points[query * 3], qy = a.points[query * 3 + 1], qz = a.points[query * 3 + 2];
        const double inf = __builtin_huge_val();
        const bool finite = fabs(qx) < inf && fabs(qy) < inf && fabs(qz) < inf;          // false for NaN
        double best_d2 = inf, best_v = 0.0, best_w = 0.0;       // of the triangles THIS lane tested
        int best_id = -1;
        if (finite) {
            const float4 *__restrict__ nodes = a.nodes;
            const float4 *__restrict__ tris = a.tris;
            uint64_t *stack = cp_lds + (size_t)q * a.stack_cap;
            const double max2 = a.max2;
            double bound = max2;                                // octet-uniform: a box beyond it cannot hold the answer
            int sp = 0;
            int cur = a.root_is_valid ? 0 : kDone;
            while (cur != kDone) {
                while (cur >= 0) {
                    const float4 *np = nodes + (size_t)cur * 16 + j * 2;
                    const float4 lo = np[0];                    // lo.xyz, hi.x
                    const float4 hi = np[1];                    // hi.yz, token, 0
                    const double ex = fmax(fmax((double)lo.x - qx, qx - (double)lo.w), 0.0);
                    const double ey = fmax(fmax((double)lo.y - qy, qy - (double)hi.x), 0.0);
                    const double ez = fmax(fmax((double)lo.z - qz, qz - (double)hi.y), 0.0);
                    const double bd = (ex * ex + ey * ey) + ez * ez;
                    const int tok = __float_as_int(hi.z);
                    const bool hit = tok != kDone && !(bd > bound);         // equality is visited; NaN counts as a hit
                    const unsigned m8 = (unsigned)(__ballot(hit) >> oct_base) & 0xffu;
                    if (m8 == 0) {
                        cur = kDone;
                        while (sp > 0) {
                            const uint64_t e = stack[--sp];
                            if (!((double)__uint_as_float((unsigned)(e >> 32)) > bound)) { cur = (int)(unsigned)e; break; }
                        }
                        continue;
                    }
                    const uint64_t key = hit ? (((uint64_t)__double_as_longlong(bd) & ~7ull) | (uint64_t)j) : ~0ull;
                    const int nearest = (int)(oct_min_u64(key) & 7ull);
                    if (hit && j != nearest) {
                        const unsigned others = m8 & ~(1u << nearest);
                        stack[sp + __popc(others & ((1u << j) - 1u))] =
                            ((uint64_t)__float_as_uint(__double2float_rz(bd)) << 32) | (uint64_t)(unsigned)tok;
                    }
                    sp += __popc(m8) - 1;
                    cur = oct_bcast(tok, oct_base, nearest);
                    oct_lds_sync();
                }
                if (cur == kDone) break;
                {
                    const int packed = ~cur;
                    const int first = packed >> 3, cnt = (packed & 7) + 1;
                    if (j < cnt) {
                        const float4 A = tris[(size_t)(first + j) * 3 + 0];
                        const float4 B = tris[(size_t)(first + j) * 3 + 1];
                        const float4 C = tris[(size_t)(first + j) * 3 + 2];
                        const int id = __float_as_int(A.w);
                        double v, w, d2;
                        tri_closest(qx, qy, qz, A, B, C, &v, &w, &d2);
                        if (d2 <= max2 && (d2 < best_d2 || best_id < 0 || (d2 == best_d2 && id < best_id))) {
                            best_d2 = d2; best_v = v; best_w = w; best_id = id;
                        }
                    }
                    const uint64_t m = oct_min_u64(best_id >= 0 ? (uint64_t)__double_as_longlong(best_d2) : ~0ull);
                    if (m != ~0ull) bound = __longlong_as_double((long long)m);       // dist2 >= +0: its bits order as it does
                }
                cur = kDone;
                while (sp > 0) {
                    const uint64_t e = stack[--sp];
                    if (!((double)__uint_as_float((unsigned)(e >> 32)) > bound)) { cur = (int)(unsigned)e; break; }
                }
            }
        }
        // the octet's winner: the smallest (dist2, id) of its lanes' bests
        const uint64_t mine = best_id >= 0 ? (uint64_t)__double_as_longlong(best_d2) : ~0ull;
        const uint64_t m = oct_min_u64(mine);
        const unsigned win = oct_min_u32(best_id >= 0 && mine == m ? (unsigned)best_id : 0xffffffffu);
        if (win == 0xffffffffu) {
            if (j == 0) {
                a.tri[query] = -1;
                a.bary[query * 3] = 0.0; a.bary[query * 3 + 1] = 0.0; a.bary[query * 3 + 2] = 0.0;
                a.dist2[query] = inf;
                atomicAdd(&s_counts[finite ? 1 : 0], 1);
            }
        } else if (best_id >= 0 && (unsigned)best_id == win && mine == m) {
            a.tri[query] = best_id;
            a.bary[query * 3] = (1.0 - best_v) - best_w; a.bary[query * 3 + 1] = best_v; a.bary[query * 3 + 2] = best_w;
            a.dist2[query] = best_d2;
        }
    }
    __syncthreads();
    if (tid < QF_CLOSEST_POINT_COUNTS && s_counts[tid] != 0) atomicAdd(&a.counts[tid], (unsigned long long)s_counts[tid]);
}

QfLdsAttr g_cp_lds_attr;

}  // namespace

extern "C" int qf_bvh_closest_points(const qf_bvh *bvh, const double *points, int64_t n_points, double max_distance,
                                     int32_t *tri, double *bary, double *dist2, int64_t *counts, void *stream)
{
    if (!bvh || !counts || n_points < 0 || !(max_distance >= 0.0)) return QF_ERR_INVALID_ARGUMENT;
    if (n_points > 0 && (!points || !tri || !bary || !dist2)) return QF_ERR_INVALID_ARGUMENT;
    if (bvh->n_tri >= (1 << 28)) return QF_ERR_UNSUPPORTED;      // leaf tokens pack (first, count)
    const int stack_cap = (bvh->max_stack8 < 2 ? 2 : bvh->max_stack8) | 1;       // odd row stride
    const size_t lds = (size_t)kOctQueries * (size_t)stack_cap * 8;
    if (lds > 160 * 1024 - 2048) return QF_ERR_UNSUPPORTED;
    const int64_t n_blocks = qf_div_up(n_points, kOctQueries);
    const int64_t per_xcd = qf_div_up(n_blocks, 8);
    if (per_xcd * 8 > 0x7fffffff) return QF_ERR_UNSUPPORTED;
    if (lds > 48 * 1024)
        QF_HIP_TRY(qf_ensure_dynamic_lds(g_cp_lds_attr, reinterpret_cast<const void *>(closest_point_kernel), 160 * 1024 - 2048));
    QF_HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * QF_CLOSEST_POINT_COUNTS, qf_stream(stream)));
    if (n_points == 0) return QF_OK;
    CpArgs a;
    a.nodes = reinterpret_cast<const float4 *>(bvh->d_nodes8);
    a.tris = reinterpret_cast<const float4 *>(bvh->d_tris);
    a.points = points; a.n_points = n_points;
    a.max2 = max_distance * max_distance;
    a.root_is_valid = (bvh->n_tri > 0 && bvh->d_nodes8 && bvh->d_tris) ? 1 : 0;
    a.stack_cap = stack_cap; a.n_blocks = (int)n_blocks; a.blocks_per_xcd = (int)per_xcd;
    a.tri = tri; a.bary = bary; a.dist2 = dist2;
    a.counts = reinterpret_cast<unsigned long long *>(counts);
    hipLaunchKernelGGL(closest_point_kernel, dim3((unsigned)(per_xcd * 8)), dim3(kCpThreads), lds, qf_stream(stream), a);
    QF_LAUNCH_CHECK();
    return QF_OK;
}
