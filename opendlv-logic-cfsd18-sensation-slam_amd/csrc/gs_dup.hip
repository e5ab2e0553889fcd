// gs_dup.hip — map twins (include/graphslam.h, "map twins"; gfx950, wave64): duplicate cones found among all pairs of a map, fused, and the
// map compacted.
//   k_dup_nearest   a thread per cone i, workgroups of 256; the map walks through LDS in tiles of 256 cones (xy, the floored covariance, the
//                   type: 11 KB), every thread reading the same entry (a broadcast), eight entries at a look; the key (d2, j), the
//                   runner-up and the count stay in registers.  The map is read n / 256 times from memory, not n times
//   k_dup_fuse      a thread per cone: the mutual test, the fusion for keepers, the keep flag as the cone's rank among the kept of its
//                   block (ballots and prefix counts across the four waves), the block's counts
//   k_dup_scan      one workgroup: the exclusive scan of the blocks' kept counts (four blocks a thread), and gs_dup_info
//   k_dup_scatter   a thread per cone: a kept cone goes to blk_off[block] + rank of the second buffer; remap for all; the entries behind
//                   the consolidated map become free cones
// No atomics, no spin, no cross-workgroup wait.  Every floating-point expression is under contract(off): the header's order of operations.
#include "gs_dup.hpp"
#include "gs_dup_host.hpp"
#include <hip/hip_ext.h>

namespace gs {

namespace {

static_assert(DUP_MAP_MAX == GS_DUP_MAP_MAX && DUP_BLOCK == 256 && DUP_BLOCKS_MAX == 4 * 256, "a tile of 256 cones; the scan takes four blocks a thread");

static constexpr int DUP_LOOK = 8;                                             // tile entries the search looks at together
static_assert(DUP_BLOCK % DUP_LOOK == 0, "the search walks a tile in whole groups");

struct DupCone { double x, y, c00, c01, c11; };                               // the covariance floored: A of the header
__device__ __forceinline__ DupCone dup_cone(const DupMap &m, int j, double s2) {
#pragma clang fp contract(off)
    const double2 xy = reinterpret_cast<const double2 *>(m.xy)[j];
    DupCone c{xy.x, xy.y, 0.0, 0.0, 0.0};
    if (m.cov) { const double4 cv = reinterpret_cast<const double4 *>(m.cov)[j]; c.c00 = cv.x; c.c01 = cv.y; c.c11 = cv.w; }
    c.c00 = c.c00 + s2; c.c11 = c.c11 + s2;
    return c;
}

__global__ void __launch_bounds__(256) k_dup_nearest(DupMap m, DupDev p, int32_t *__restrict__ out_twin, double *__restrict__ out_d2,
                                                     double *__restrict__ out_second, int32_t *__restrict__ out_nadm) {
#pragma clang fp contract(off)
    __shared__ double2 s_xy[DUP_BLOCK];
    __shared__ double s_c00[DUP_BLOCK], s_c01[DUP_BLOCK], s_c11[DUP_BLOCK];
    __shared__ int s_ty[DUP_BLOCK];
    const int tid = threadIdx.x, i = blockIdx.x * DUP_BLOCK + tid;
    const bool live = i < m.n;
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    DupCone me{nan, nan, 0.0, 0.0, 0.0}; int ti = 0;
    if (live) { me = dup_cone(m, i, p.s2); ti = m.type[i]; }
    double best = inf, second = inf; int bj = -1, cnt = 0;
    for (int t0 = 0; t0 < m.n; t0 += DUP_BLOCK) {                              // (uniform: every thread meets every barrier)
        __syncthreads();                                                       // the tile before has been read by all
        { const int j = t0 + tid;
          DupCone c{nan, nan, 0.0, 0.0, 0.0}; int ty = 0;
          if (j < m.n) { c = dup_cone(m, j, p.s2); ty = m.type[j]; }
          s_xy[tid] = make_double2(c.x, c.y); s_c00[tid] = c.c00; s_c01[tid] = c.c01; s_c11[tid] = c.c11; s_ty[tid] = ty; }
        __syncthreads();
        if (!live) continue;
        // eight entries at a time (the tile's entries beyond the map are NaN): their loads in flight together, a first look without a branch —
        // (n0 n0) + (n1 n1) has the same bits for either order of the pair — and the rule itself only for the few that are near
        for (int e0 = 0; e0 < DUP_BLOCK; e0 += DUP_LOOK) {
            bool near[DUP_LOOK]; bool any = false;
#pragma unroll
            for (int k = 0; k < DUP_LOOK; ++k) {
                const double2 q = s_xy[e0 + k];
                const double a0 = q.x - me.x, a1 = q.y - me.y;
                near[k] = a0 * a0 + a1 * a1 < p.md2_hi;                        // false: far (or a NaN), the tests below cannot hold
                any = any || near[k];
            }
            if (!any) continue;
#pragma unroll
            for (int k = 0; k < DUP_LOOK; ++k) {
                const int e = e0 + k, j = t0 + e;
                if (!near[k] || j == i) continue;
                if (p.same_type && s_ty[e] != ti) continue;
                const double2 q = s_xy[e];
                const bool up = j > i;                                         // the pair is formed from a = min(i, j), b = max(i, j)
                const double n0 = up ? q.x - me.x : me.x - q.x, n1 = up ? q.y - me.y : me.y - q.y;
                if (!(sqrt(n0 * n0 + n1 * n1) < p.max_distance)) continue;
                const double s00 = up ? me.c00 + s_c00[e] : s_c00[e] + me.c00, s01 = up ? me.c01 + s_c01[e] : s_c01[e] + me.c01,
                             s11 = up ? me.c11 + s_c11[e] : s_c11[e] + me.c11;
                const double det = s00 * s11 - s01 * s01;
                const double d2 = (((s11 * n0) * n0 - ((2.0 * s01) * n0) * n1) + (s00 * n1) * n1) / det;
                if (!(det > 0.0 && s00 > 0.0 && d2 < p.gate_chi2)) continue;
                cnt += 1;
                if (d2 < best) { second = best; best = d2; bj = j; }           // j ascends: an exact tie stays with the lower index
                else if (d2 < second) second = d2;
            }
        }
    }
    if (!live) return;
    out_twin[i] = bj;
    if (out_d2) out_d2[i] = best;
    if (out_second) out_second[i] = second;
    if (out_nadm) out_nadm[i] = cnt;
}

__global__ void __launch_bounds__(256) k_dup_fuse(DupMap m, DupDev p, DupWork W) {
#pragma clang fp contract(off)
    __shared__ int s_keep[4], s_pair[4], s_amb[4];
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63, i = blockIdx.x * DUP_BLOCK + tid;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    const bool live = i < m.n;
    int t = -1, na = 0; bool mutual = false;
    if (live) {
        t = W.twin[i]; na = W.nadm[i];
        if (t >= 0 && t < m.n && t != i) { mutual = W.twin[t] == i; if (p.exclusive) mutual = mutual && na == 1 && W.nadm[t] == 1; }
    }
    const bool keeper = mutual && i < t, keep = live && !(mutual && i > t), amb = live && na > 1;
    if (keep) {
        double2 xy = reinterpret_cast<const double2 *>(m.xy)[i];
        double4 cv = make_double4(0.0, 0.0, 0.0, 0.0);
        if (m.cov) cv = reinterpret_cast<const double4 *>(m.cov)[i];
        if (keeper) {                                                          // a = i, b = t
            const DupCone a = dup_cone(m, i, p.s2), b = dup_cone(m, t, p.s2);
            const double s00 = a.c00 + b.c00, s01 = a.c01 + b.c01, s11 = a.c11 + b.c11;
            const double det = s00 * s11 - s01 * s01;
            const double n0 = b.x - a.x, n1 = b.y - a.y;
            const double k00 = ((a.c00 * s11) - (a.c01 * s01)) / det, k01 = ((a.c01 * s00) - (a.c00 * s01)) / det;
            const double k10 = ((a.c01 * s11) - (a.c11 * s01)) / det, k11 = ((a.c11 * s00) - (a.c01 * s01)) / det;
            xy.x = a.x + ((k00 * n0) + (k01 * n1)); xy.y = a.y + ((k10 * n0) + (k11 * n1));
            const double f00 = (k00 * b.c00) + (k01 * b.c01), f01 = (k00 * b.c01) + (k01 * b.c11), f11 = (k10 * b.c01) + (k11 * b.c11);
            cv = make_double4(f00, f01, f01, f11);
        }
        reinterpret_cast<double2 *>(W.f_xy)[i] = xy;
        if (m.cov) reinterpret_cast<double4 *>(W.f_cov)[i] = cv;
    }
    const unsigned long long m_keep = __ballot(keep);
    const int n_pair = __popcll(__ballot(keeper)), n_amb = __popcll(__ballot(amb));
    if (lane == 0) { s_keep[w] = __popcll(m_keep); s_pair[w] = n_pair; s_amb[w] = n_amb; }
    __syncthreads();
    const int lower = (w > 0 ? s_keep[0] : 0) + (w > 1 ? s_keep[1] : 0) + (w > 2 ? s_keep[2] : 0);
    if (live) W.slot[i] = keep ? lower + __popcll(m_keep & below) : -1;
    if (tid == 0) {
        const int nb = gridDim.x, b = blockIdx.x;
        W.blk[b] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
        W.blk[nb + b] = s_pair[0] + s_pair[1] + s_pair[2] + s_pair[3];
        W.blk[2 * nb + b] = s_amb[0] + s_amb[1] + s_amb[2] + s_amb[3];
    }
}

__global__ void __launch_bounds__(256) k_dup_scan(int n, int nb, DupWork W) {
    __shared__ int s_k[256], s_p[256], s_a[256];
    const int tid = threadIdx.x;
    int k[4], sum = 0, pr = 0, am = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int b = 4 * tid + e;
        k[e] = 0;
        if (b < nb) { k[e] = W.blk[b]; pr += W.blk[nb + b]; am += W.blk[2 * nb + b]; }
        sum += k[e];
    }
    s_k[tid] = sum; s_p[tid] = pr; s_a[tid] = am;
    __syncthreads();
    int base = 0;
    for (int u = 0; u < tid; ++u) base += s_k[u];
#pragma unroll
    for (int e = 0; e < 4; ++e) { const int b = 4 * tid + e; if (b < nb) { W.blk_off[b] = base; base += k[e]; } }
    if (tid == 0) {
        int kept = 0, pairs = 0, ambiguous = 0;
        for (int u = 0; u < 256; ++u) { kept += s_k[u]; pairs += s_p[u]; ambiguous += s_a[u]; }
        W.info->n_in = n; W.info->n_out = kept; W.info->n_pairs = pairs; W.info->n_ambiguous = ambiguous;
    }
}

__global__ void __launch_bounds__(256) k_dup_scatter(DupMap m, DupWork W) {
    const int i = blockIdx.x * DUP_BLOCK + threadIdx.x;
    if (i >= m.n) return;
    if (i >= W.info->n_out) {                                                  // behind the consolidated map: free cones (no kept cone lands here)
        const double nan = __builtin_nan("");
        reinterpret_cast<double2 *>(W.out_xy)[i] = make_double2(nan, nan);
        W.out_type[i] = 0;
        if (W.out_cov) reinterpret_cast<double4 *>(W.out_cov)[i] = make_double4(0.0, 0.0, 0.0, 0.0);
    }
    const int s = W.slot[i];
    if (s >= 0) {
        const int to = W.blk_off[i >> 8] + s;                                  // (to <= i: nothing lands beyond the map's size)
        reinterpret_cast<double2 *>(W.out_xy)[to] = reinterpret_cast<const double2 *>(W.f_xy)[i];
        W.out_type[to] = m.type[i];
        if (W.out_cov) reinterpret_cast<double4 *>(W.out_cov)[to] = reinterpret_cast<const double4 *>(W.f_cov)[i];
        W.remap[i] = to;
    } else {
        const int a = W.twin[i];                                               // dropped: the keeper's place (k_dup_fuse dropped i for a twin in range)
        W.remap[i] = W.blk_off[a >> 8] + W.slot[a];
    }
}

}  // namespace

void launch_dup_nearest(const DupMap &m, const DupDev &p, int32_t *twin, double *d2, double *second, int32_t *nadm, hipStream_t st, hipEvent_t start,
                        hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_dup_nearest, dim3(dup_blocks(m.n)), dim3(DUP_BLOCK), 0, st, start, stop, 0, m, p, twin, d2, second, nadm);
}
void launch_dup_fuse(const DupMap &m, const DupDev &p, const DupWork &w, hipStream_t st) {
    hipLaunchKernelGGL(k_dup_fuse, dim3(dup_blocks(m.n)), dim3(DUP_BLOCK), 0, st, m, p, w);
}
void launch_dup_scan(int n, const DupWork &w, hipStream_t st) {
    hipLaunchKernelGGL(k_dup_scan, dim3(1), dim3(256), 0, st, n, dup_blocks(n), w);
}
void launch_dup_scatter(const DupMap &m, const DupWork &w, hipStream_t st, hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_dup_scatter, dim3(dup_blocks(m.n)), dim3(DUP_BLOCK), 0, st, nullptr, stop, 0, m, w);
}

}  // namespace gs
