// gs_reloc.hip — relocalisation (gfx950 / CDNA4, wave64): from one frame and the map alone the rigid pose under which the most observations
// land on type-compatible cones, and the best count at a clearly different pose (include/graphslam.h, "relocalisation").
//
//   k_reloc_seed   a workgroup per (frame, slice of cones p).  It rebuilds the frame in LDS (z by the A0 function, the seed observations by
//                  rank, the table of kept seed pairs), then every WAVE streams its share of the cones q against the slice's p on its own:
//                  a lane holds one q, p is wave-uniform.  Two rings in LDS per wave, filled by ballot compaction and drained 64 at a time,
//                  keep the lanes full where the work thins out:
//                    (p, q) whose length can match SOME table entry (a conservative band on M2: it never drops a match)  -> candidate ring
//                    candidate x table entry that passes the type and length tests of the rule                           -> seed ring
//                    a lane per seed: c, s, t, the existence test, the score over the frame's observations in ascending i -> the lane's best key
//                  No barrier inside the loop (a wave's rings are its own), no atomics on results, no list that could overflow: a ring holds
//                  at most 63 + 64 entries.  The workgroup's best key and its seed count go into ONE record.
//   k_reloc_pick   a workgroup per frame: the smallest key of the frame's records, the sum of their seed counts, the winner scored once more
//                  a lane per observation (index, e2), the frame's record; the winner is kept for the second pass.
//   Runner-up: k_reloc_seed again, skipping the seeds near the kept winner, then k_reloc_pick again for second_count / second_pose.
//
// The key (-count, cost, u, v, p, q) is strict and total and every seed's score is formed by one lane in ascending i, so the result does not
// depend on the slices, on the order the rings fill in or on which search scores: the hashed grid (cell edge from inlier_radius: every cone
// inside the radius sits in the nine cells around w) and the walk over the whole map take the same minimum over (e2, j) below the radius.
#include "gs_assoc_dev.hpp"

#include <algorithm>

namespace gs {

static constexpr int RL_NONE = 0x7fffffff;
static constexpr int RL_FRAME = NN_FRAME_MAX;
static constexpr int RL_SEEDS = 16;                                            // GS_RELOC_SEED_MAX
static constexpr int RL_PAIRS = RL_SEEDS * (RL_SEEDS - 1) / 2;                 // 120
static constexpr int RL_RING = 128;                                            // > 63 + 64: a ring is drained as soon as it holds 64

struct RlFrame { double zx[RL_FRAME], zy[RL_FRAME], ty[RL_FRAME], r2[RL_FRAME]; int32_t valid[RL_FRAME]; };       // 9 KB
struct RlTable { double dzx[RL_PAIRS], dzy[RL_PAIRS], L2[RL_PAIRS], L[RL_PAIRS], tyu[RL_PAIRS], tyv[RL_PAIRS], mzx[RL_PAIRS], mzy[RL_PAIRS];
                 int32_t u[RL_PAIRS], v[RL_PAIRS]; double lo2, hi2; int32_t n; };                                    // 8.7 KB
struct RlMap { int n_map; const double *xy; const int32_t *type; GridParams g; const int32_t *cell_start, *cell_items; };
struct RlArgs { int n; const double *obs; int n_frames; const int32_t *frame_start; double lidar; RlMap m; RlDev p; int slice, n_slices; RlRec *rec; int excl; };
struct RlBest { int count; double cost; int u, v, p, q; double c, s, tx, ty; };

__device__ __forceinline__ int rl_below(unsigned long long m) {               // the set bits of m below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}
// the key (-count, cost, u, v, p, q): is a strictly before b?  (count < 0: no seed; costs are finite sums)
__device__ __forceinline__ bool rl_before(int count, double cost, int u, int v, int p, int q, const RlBest &b) {
    if (count != b.count) return count > b.count;
    if (cost != b.cost) return cost < b.cost;
    if (u != b.u) return u < b.u;
    if (v != b.v) return v < b.v;
    if (p != b.p) return p < b.p;
    return q < b.q;
}
__device__ __forceinline__ void rl_merge(RlBest &b, const RlBest &o) { if (o.count >= 0 && rl_before(o.count, o.cost, o.u, o.v, o.p, o.q, b)) b = o; }
__device__ __forceinline__ RlBest rl_shfl_xor(const RlBest &b, int off) {
    RlBest o;
    o.count = __shfl_xor(b.count, off, 64); o.cost = __shfl_xor(b.cost, off, 64);
    o.u = __shfl_xor(b.u, off, 64); o.v = __shfl_xor(b.v, off, 64); o.p = __shfl_xor(b.p, off, 64); o.q = __shfl_xor(b.q, off, 64);
    o.c = __shfl_xor(b.c, off, 64); o.s = __shfl_xor(b.s, off, 64); o.tx = __shfl_xor(b.tx, off, 64); o.ty = __shfl_xor(b.ty, off, 64);
    return o;
}
__device__ __forceinline__ RlBest rl_of(const RlRec &r) { return RlBest{r.count, r.cost, r.u, r.v, r.p, r.q, r.c, r.s, r.tx, r.ty}; }
__device__ __forceinline__ RlRec rl_rec(const RlBest &b, long long n_seeds) { return RlRec{b.cost, b.c, b.s, b.tx, b.ty, n_seeds, b.count, b.u, b.v, b.p, b.q, 0}; }
// the workgroup's smallest key and the sum of its seed counts, in every thread; red: four entries of LDS
__device__ __forceinline__ void rl_reduce(RlBest &b, long long &n_seeds, RlRec *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const RlBest o = rl_shfl_xor(b, off); rl_merge(b, o); n_seeds += __shfl_xor(n_seeds, off, 64); }
    __syncthreads();                                                           // (red may still be read from a reduction before)
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = rl_rec(b, n_seeds);
    __syncthreads();
    b = rl_of(red[0]); n_seeds = red[0].n_seeds;
#pragma unroll
    for (int w = 1; w < 4; ++w) { rl_merge(b, rl_of(red[w])); n_seeds += red[w].n_seeds; }
}

// observation a + t of the frame into slot t (t < k), an invalid slot beyond: z by the A0 function, r2, the type
__device__ __forceinline__ void rl_load(RlFrame &F, int t, int a, int k, const double *__restrict__ obs, double lidar) {
#pragma clang fp contract(off)
    double zx = 0.0, zy = 0.0, ty = 0.0, r2 = 0.0; int valid = 0;
    if (t < k) {
        const double4 o4 = reinterpret_cast<const double4 *>(obs)[a + t];     // (az, zen, dist, type) in one 32-byte load
        const double2 z = nn_polar(o4.x, o4.y, o4.z, lidar);
        zx = z.x; zy = z.y; ty = o4.w; r2 = zx * zx + zy * zy;
        valid = isfinite(zx) && isfinite(zy) && r2 > 0.0;
    }
    F.zx[t] = zx; F.zy[t] = zy; F.ty[t] = ty; F.r2[t] = r2; F.valid[t] = valid;
}

// the type-compatible cone of smallest (e2, j) with e2 < r2max around w, or RL_NONE
template <bool GRID>
__device__ __forceinline__ void rl_nearest(const RlMap &M, double type_tol, double r2max, double wx, double wy, double ty, int &bj, double &be) {
#pragma clang fp contract(off)
    bj = RL_NONE; be = __builtin_inf();
    auto offer = [&](int j) {
        if (!(fabs((double)M.type[j] - ty) < type_tol)) return;
        const double2 l = reinterpret_cast<const double2 *>(M.xy)[j];
        const double ex = l.x - wx, ey = l.y - wy, e2 = ex * ex + ey * ey;
        if (e2 < r2max && (e2 < be || (e2 == be && j < bj))) { be = e2; bj = j; }
    };
    map_walk<GRID>(M.n_map, M.g, M.cell_start, M.cell_items, wx, wy, offer);
}
// the score of (c, s, t): the frame's valid observations in ascending i
template <bool GRID>
__device__ __forceinline__ void rl_score(const RlFrame &F, int k, const RlMap &M, const RlDev &P, double c, double s, double tx, double ty, int &count, double &cost) {
#pragma clang fp contract(off)
    count = 0; cost = 0.0;
    for (int i = 0; i < k; ++i) {
        if (!F.valid[i]) continue;                                             // (uniform: every lane reads the same slot)
        const double zx = F.zx[i], zy = F.zy[i];
        const double wx = (c * zx - s * zy) + tx, wy = (s * zx + c * zy) + ty;
        int bj; double be; rl_nearest<GRID>(M, P.type_tol, P.inlier_r2, wx, wy, F.ty[i], bj, be);
        if (bj != RL_NONE) { ++count; cost += be; }
    }
}
// the seed of table entry t and the ordered cone pair (p, q): false when it does not exist
__device__ __forceinline__ bool rl_seed(const RlTable &T, int t, double2 lp, double2 lq, double &c, double &s, double &tx, double &ty) {
#pragma clang fp contract(off)
    const double dlx = lq.x - lp.x, dly = lq.y - lp.y, M2 = dlx * dlx + dly * dly;
    const double dzx = T.dzx[t], dzy = T.dzy[t], den = sqrt(T.L2[t] * M2);
    c = (dzx * dlx + dzy * dly) / den;
    s = (dzx * dly - dzy * dlx) / den;
    const double mlx = 0.5 * (lp.x + lq.x), mly = 0.5 * (lp.y + lq.y), mzx = T.mzx[t], mzy = T.mzy[t];
    tx = mlx - (c * mzx - s * mzy);
    ty = mly - (s * mzx + c * mzy);
    return den > 0.0 && isfinite(c) && isfinite(s) && isfinite(tx) && isfinite(ty);
}

template <bool GRID>
__global__ void __launch_bounds__(256) k_reloc_seed(RlArgs A) {
#pragma clang fp contract(off)
    __shared__ RlFrame F;
    __shared__ RlTable T;
    __shared__ int32_t s_sel[RL_FRAME], s_seed[RL_SEEDS];
    __shared__ int32_t s_cand[4][RL_RING][2], s_sq[4][RL_RING][3];            // a wave's rings: (p, q) and (p, q, table entry)
    __shared__ RlRec s_red[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int f = blockIdx.x / A.n_slices, sl = blockIdx.x - f * A.n_slices;
    int a, b;
    if (frame_bounds(A.frame_start, A.n, f, a, b) != FRAME_OK) return;         // not a frame of this call, or refused: the pick kernel reads no record of it
    const RlRec *win = A.rec + (size_t)A.n_frames * A.n_slices + f;
    if (A.excl && win->count < 0) return;                                      // second pass without a winner: likewise
    const int k = b - a;
    rl_load(F, tid, a, k, A.obs, A.lidar);
    __syncthreads();
    // the seed observations: the seed_obs smallest (r2, index) among the valid, then in ascending index
    int sel = 0;
    if (F.valid[tid]) { const double mine = F.r2[tid]; int r = 0;
        for (int j = 0; j < k; ++j) r += F.valid[j] && (F.r2[j] < mine || (F.r2[j] == mine && j < tid));
        sel = r < A.p.seed_obs; }
    s_sel[tid] = sel;
    if (tid == 0) T.n = 0;
    __syncthreads();
    int ns = 0, pos = 0;
    for (int j = 0; j < k; ++j) { ns += s_sel[j]; pos += j < tid ? s_sel[j] : 0; }
    if (sel) s_seed[pos] = tid;
    __syncthreads();
    // the table of kept pairs (u < v): its order is whatever the slots were taken in; no result depends on it
    if (tid < ns * (ns - 1) / 2) {
        int ia = 0, rem = tid;
        while (rem >= ns - 1 - ia) { rem -= ns - 1 - ia; ++ia; }
        const int u = s_seed[ia], v = s_seed[ia + 1 + rem];
        const double dzx = F.zx[v] - F.zx[u], dzy = F.zy[v] - F.zy[u], L2 = dzx * dzx + dzy * dzy, L = sqrt(L2);
        if (L >= A.p.min_baseline) { const int t = atomicAdd(&T.n, 1);
            T.dzx[t] = dzx; T.dzy[t] = dzy; T.L2[t] = L2; T.L[t] = L; T.tyu[t] = F.ty[u]; T.tyv[t] = F.ty[v];
            T.mzx[t] = 0.5 * (F.zx[u] + F.zx[v]); T.mzy[t] = 0.5 * (F.zy[u] + F.zy[v]); T.u[t] = a + u; T.v[t] = a + v; }
    }
    __syncthreads();
    if (tid == 0) {
        // a band on M2 outside which |M - L| <= length_tol holds for no entry: M = fl(sqrt(M2)) inside [Lmin - tol', Lmax + tol'] with
        // tol' = 1.000001 tol (which covers the rounding of M - L), squared with a margin of 1e-9 (which covers that of the square root)
        double lmin = __builtin_inf(), lmax = 0.0;
        for (int t = 0; t < T.n; ++t) { lmin = fmin(lmin, T.L[t]); lmax = fmax(lmax, T.L[t]); }
        const double m = 1.000001 * A.p.length_tol, lo = lmin - m, hi = lmax + m;
        T.lo2 = lo > 0.0 ? (lo * lo) * (1.0 - 1e-9) : -1.0; T.hi2 = (hi * hi) * (1.0 + 1e-9);
    }
    __syncthreads();

    RlBest best{-1, 0.0, 0, 0, 0, 0, 0.0, 0.0, 0.0, 0.0}; long long n_seeds = 0;
    const int nt = T.n;
    if (nt > 0) {
        const double lo2 = T.lo2, hi2 = T.hi2;
        RlBest wn = best;
        if (A.excl) wn = rl_of(*win);
        int chead = 0, ccnt = 0, shead = 0, scnt = 0;                          // wave-uniform: the two rings' heads and fills
        int32_t (*cq)[2] = s_cand[w]; int32_t (*sq)[3] = s_sq[w];
        // a lane per seed of the ring's first m entries
        auto score_batch = [&](int m) {
            wave_sync();
            if (lane < m) {
                const int e = (shead + lane) & (RL_RING - 1), p = sq[e][0], q = sq[e][1], t = sq[e][2];
                const double2 lp = reinterpret_cast<const double2 *>(A.m.xy)[p], lq = reinterpret_cast<const double2 *>(A.m.xy)[q];
                double c, s, tx, ty;
                if (rl_seed(T, t, lp, lq, c, s, tx, ty)) {
                    bool near = false;
                    if (A.excl) { const double dx = tx - wn.tx, dy = ty - wn.ty; near = (dx * dx + dy * dy) < A.p.distinct_d2 && (c * wn.c + s * wn.s) > A.p.distinct_cos; }
                    else ++n_seeds;
                    if (!near) {
                        int count; double cost; rl_score<GRID>(F, k, A.m, A.p, c, s, tx, ty, count, cost);
                        if (rl_before(count, cost, T.u[t], T.v[t], p, q, best)) best = RlBest{count, cost, T.u[t], T.v[t], p, q, c, s, tx, ty};
                    }
                }
            }
            shead = (shead + m) & (RL_RING - 1); scnt -= m;
        };
        // a lane per candidate of the ring's first m entries, against every table entry
        auto match_batch = [&](int m) {
            wave_sync();
            const bool act = lane < m; int p = 0, q = 0; double M = 0.0, tp = 0.0, tq = 0.0;
            if (act) {
                const int e = (chead + lane) & (RL_RING - 1); p = cq[e][0]; q = cq[e][1];
                const double2 lp = reinterpret_cast<const double2 *>(A.m.xy)[p], lq = reinterpret_cast<const double2 *>(A.m.xy)[q];
                const double dlx = lq.x - lp.x, dly = lq.y - lp.y;
                M = sqrt(dlx * dlx + dly * dly); tp = (double)A.m.type[p]; tq = (double)A.m.type[q];
            }
            chead = (chead + m) & (RL_RING - 1); ccnt -= m;
            for (int t = 0; t < nt; ++t) {
                const bool hit = act && fabs(tp - T.tyu[t]) < A.p.type_tol && fabs(tq - T.tyv[t]) < A.p.type_tol && fabs(M - T.L[t]) <= A.p.length_tol;
                const unsigned long long mm = __ballot(hit);
                if (mm == 0) continue;
                if (hit) { const int e = (shead + scnt + rl_below(mm)) & (RL_RING - 1); sq[e][0] = p; sq[e][1] = q; sq[e][2] = t; }
                scnt += __popcll(mm);
                if (scnt >= 64) score_batch(64);
            }
        };
        const int p0 = sl * A.slice, p1 = min(A.m.n_map, p0 + A.slice);
        for (int qb = w * 64; qb < A.m.n_map; qb += 256) {
            const int q = qb + lane; const bool hq = q < A.m.n_map;
            const double2 lq = hq ? reinterpret_cast<const double2 *>(A.m.xy)[q] : make_double2(0.0, 0.0);
            for (int p = p0; p < p1; ++p) {
                const double2 lp = reinterpret_cast<const double2 *>(A.m.xy)[p];
                const double dlx = lq.x - lp.x, dly = lq.y - lp.y, M2 = dlx * dlx + dly * dly;
                const bool pass = hq && q != p && M2 >= lo2 && M2 <= hi2;
                const unsigned long long mm = __ballot(pass);
                if (mm == 0) continue;
                if (pass) { const int e = (chead + ccnt + rl_below(mm)) & (RL_RING - 1); cq[e][0] = p; cq[e][1] = q; }
                ccnt += __popcll(mm);
                if (ccnt >= 64) match_batch(64);
            }
        }
        if (ccnt > 0) match_batch(ccnt);                                       // what is left in the rings: fewer than 64 each
        if (scnt > 0) score_batch(scnt);
    }
    rl_reduce(best, n_seeds, s_red);
    if (tid == 0) A.rec[(size_t)f * A.n_slices + sl] = rl_rec(best, n_seeds);
}

template <bool GRID>
__global__ void __launch_bounds__(256) k_reloc_pick(RlArgs A, RlOut O, double *chain_pose, int32_t *chain_frame_end) {
#pragma clang fp contract(off)
    __shared__ RlRec s_red[4];
    const int tid = threadIdx.x, f = blockIdx.x;
    int a, b; const FrameKind kind = frame_bounds(A.frame_start, A.n, f, a, b);
    if (kind == FRAME_NONE) return;                                            // not a frame of this call: nothing read, nothing written
    RlRec *win = A.rec + (size_t)A.n_frames * A.n_slices + f;
    const bool refused = kind == FRAME_LARGE;
    RlBest best{-1, 0.0, -1, -1, -1, -1, 0.0, 0.0, 0.0, 0.0}; long long n_seeds = 0;
    if (!refused && !(A.excl && win->count < 0))
        for (int s = tid; s < A.n_slices; s += 256) { const RlRec r = A.rec[(size_t)f * A.n_slices + s]; n_seeds += r.n_seeds; rl_merge(best, rl_of(r)); }
    rl_reduce(best, n_seeds, s_red);
    const bool found = best.count >= 0;
    if (A.excl) {                                                              // the second pass: the runner-up's count and pose
        if (tid == 0) {
            if (O.second_count) O.second_count[f] = found ? best.count : 0;
            if (O.second_pose) { O.second_pose[3 * f] = found ? best.tx : 0.0; O.second_pose[3 * f + 1] = found ? best.ty : 0.0;
                                 O.second_pose[3 * f + 2] = found ? atan2(best.s, best.c) : 0.0; }
        }
        return;
    }
    // the winner once more, a lane per observation: its cone and e2 (the count and the cost are the seed kernel's)
    for (int i = a + tid; i < b; i += 256) {                                   // (more than one round only in a refused frame)
        int j = -1; double e2 = __builtin_inf();
        if (found) {
            const double4 o4 = reinterpret_cast<const double4 *>(A.obs)[i];
            const double2 z = nn_polar(o4.x, o4.y, o4.z, A.lidar);
            const double r2 = z.x * z.x + z.y * z.y;
            if (isfinite(z.x) && isfinite(z.y) && r2 > 0.0) {
                const double wx = (best.c * z.x - best.s * z.y) + best.tx, wy = (best.s * z.x + best.c * z.y) + best.ty;
                int bj; double be; rl_nearest<GRID>(A.m, A.p.type_tol, A.p.inlier_r2, wx, wy, o4.w, bj, be);
                if (bj != RL_NONE) { j = bj; e2 = be; }
            }
        }
        if (O.index) O.index[i] = j;
        if (O.e2) O.e2[i] = e2;
    }
    if (tid == 0) {
        const int status = refused ? 4 : !found ? 2 : best.count >= A.p.min_inliers ? 0 : 1;
        const double th = found ? atan2(best.s, best.c) : 0.0, px = found ? best.tx : 0.0, py = found ? best.ty : 0.0;
        if (O.pose) { O.pose[3 * f] = px; O.pose[3 * f + 1] = py; O.pose[3 * f + 2] = th; }
        if (O.count) O.count[f] = found ? best.count : 0;
        if (O.cost) O.cost[f] = found ? best.cost : __builtin_inf();
        if (O.seed) { O.seed[4 * f] = best.u; O.seed[4 * f + 1] = best.v; O.seed[4 * f + 2] = best.p; O.seed[4 * f + 3] = best.q; }
        if (O.n_seeds) O.n_seeds[f] = n_seeds;
        if (O.status) O.status[f] = status;
        *win = rl_rec(best, n_seeds);
        if (chain_pose) { chain_pose[0] = px; chain_pose[1] = py; chain_pose[2] = th;
            if (status >= 2) *chain_frame_end = 0; }                           // the chain behind finds an empty frame
    }
}

int reloc_slices(int n_frames, int n_map, int forced, int &slice) {
    // enough workgroups to fill the device whatever the number of frames (about 2048), a slice of at least 16 cones; speed only
    const int want = std::max(1, (2048 + std::max(n_frames, 1) - 1) / std::max(n_frames, 1));
    slice = forced > 0 ? forced : std::max(16, (n_map + want - 1) / want);
    return std::max(1, (n_map + slice - 1) / slice);
}

void launch_relocalize(const ObsRef &o, const MapRef &m, double lidar, RlDev p, int slice, int n_slices, RlRec *rec, const RlOut &out, double *chain_pose,
                       int32_t *chain_frame_end, Launch L) {
    if (o.n_frames <= 0) return;
    RlArgs A{o.n, o.obs, o.n_frames, o.frame_start, lidar,
             RlMap{m.n, m.xy, m.type, m.cell_start ? grid_params_of(p.inlier_radius, m.buckets) : GridParams{}, m.cell_start, m.cell_items}, p, slice, n_slices, rec, 0};
    const dim3 sg((unsigned)o.n_frames * (unsigned)n_slices), pg(o.n_frames), blk(256);
    const bool second = out.second_count || out.second_pose;
    for (int pass = 0; pass < (second ? 2 : 1); ++pass) {                      // start on the first dispatch, stop on the last
        A.excl = pass;
        hipEvent_t e0 = pass == 0 ? L.start : nullptr, e1 = pass == (second ? 1 : 0) ? L.stop : nullptr;
        if (m.cell_start) { hipExtLaunchKernelGGL(k_reloc_seed<true>, sg, blk, 0, L.st, e0, nullptr, 0, A);
                            hipExtLaunchKernelGGL(k_reloc_pick<true>, pg, blk, 0, L.st, nullptr, e1, 0, A, out, pass == 0 ? chain_pose : nullptr, pass == 0 ? chain_frame_end : nullptr); }
        else { hipExtLaunchKernelGGL(k_reloc_seed<false>, sg, blk, 0, L.st, e0, nullptr, 0, A);
               hipExtLaunchKernelGGL(k_reloc_pick<false>, pg, blk, 0, L.st, nullptr, e1, 0, A, out, pass == 0 ? chain_pose : nullptr, pass == 0 ? chain_frame_end : nullptr); }
    }
}

}  // namespace gs
