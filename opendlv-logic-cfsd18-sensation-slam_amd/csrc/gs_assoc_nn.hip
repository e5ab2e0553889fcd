// gs_assoc_nn.hip — covariance-gated association (gfx950 / CDNA4, wave64): for every observation the map cone with the smallest
// Mahalanobis distance d2 inside a chi-square gate, its d2, and the runner-up's d2 (include/graphslam.h, "covariance-gated association").
//
//   k_assoc_nn        a thread per observation, the map (xy, covariance, type) streamed through LDS in tiles of 1024
//   k_assoc_nn_grid   a thread per observation, the nine buckets of the hashed grid around it (cell edge from max_distance)
//   k_frame_nn        one frame in one launch: a workgroup per observation, its 256 threads stride over the map
//   k_map_cov_gather  map covariances out of the gathered marginals (gs_map_set_cov_from_marginals)
//   k_assign_nn       the one-to-one association inside frames (gs_assign_nn_*, gs_frame_frontend_assign)
//   k_assign_opt      the minimum-cost association inside frames (gs_assign_opt_*), k_assign_opt_big for frames above 64 observations
//   k_joint_compat    the joint test of a frame's hypothesis (gs_joint_compat_*, gs_frame_frontend_jc), k_joint_compat_big likewise
//   k_localize        the iterated pose refinement of a frame against the map (gs_localize_*, gs_frame_frontend_localize), k_localize_big likewise
// The last four have their own text further down.  What the kernels share is in gs_assoc_dev.hpp, once: the query and the candidate, the walk
// over the map, the wave sync, the frame kernels' scaffold (argument block, lane split, frame defences, the two drivers, the launcher) and
// the ten pair terms of the joint test and the localisation.
//
// The three association kernels return IDENTICAL bits: the query's side (z, g, Q + P) is nn_query, one candidate's side (S, det, d2 and
// the five tests) is nn_pair, both without contraction, the A0 conversion is ONE out-of-line function (polar_to_xy compiled once, not
// once per inlining context), heading cos / sin come from sincos everywhere, and the winner is a minimum over (d2, index) — which does
// not depend on the order the candidates arrive in; the frame kernel reduces it in a fixed order all the same.
#include "gs_assoc_dev.hpp"
#include "gs_edge_dev.hpp"      // normalize_theta
#include <hip/hip_ext.h>

namespace gs {

static constexpr int NN_TILE = 1024;

struct NnBest { double d2; int j; double second; };

__device__ __forceinline__ void nn_take(NnBest &b, double d2, int j) {
    if (d2 < b.d2 || (d2 == b.d2 && j < b.j)) { b.second = b.d2; b.d2 = d2; b.j = j; }
    else if (d2 < b.second) b.second = d2;
}
// b <- the best and the runner-up of the union of b's and o's candidates
__device__ __forceinline__ void nn_merge(NnBest &b, double od2, int oj, double osecond) {
    if (od2 < b.d2 || (od2 == b.d2 && oj < b.j)) { b.second = fmin(b.d2, osecond); b.d2 = od2; b.j = oj; }
    else b.second = fmin(b.second, od2);
}
__device__ __forceinline__ void nn_store(int i, const NnBest &b, int32_t *out_idx, double *out_d2, double *out_second) {
    out_idx[i] = b.j == NN_NONE ? -1 : b.j;
    if (out_d2) out_d2[i] = b.d2;
    if (out_second) out_second[i] = b.second;
}

__global__ void __launch_bounds__(256) k_assoc_nn(int n, const double *__restrict__ poses, int n_poses, const int32_t *__restrict__ pose_of_obs,
        const double *__restrict__ obs, double lidar, int n_map, const double *__restrict__ map_xy, const int32_t *__restrict__ map_type,
        const double *__restrict__ map_cov, const double *__restrict__ pose_cov, NnDev p,
        int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    __shared__ double sx[NN_TILE], sy[NN_TILE], s00[NN_TILE], s01[NN_TILE], s11[NN_TILE];      // 44 KB with the types: three workgroups per CU
    __shared__ int32_t st[NN_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const NnQuery q = nn_query_of(i, n, poses, n_poses, pose_of_obs, obs, pose_cov, lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    for (int base = 0; base < n_map; base += NN_TILE) {
        const int cnt = min(NN_TILE, n_map - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const double2 xy = reinterpret_cast<const double2 *>(map_xy)[base + t];
            sx[t] = xy.x; sy[t] = xy.y; st[t] = map_type[base + t];
            if (map_cov) { const double4 cv = reinterpret_cast<const double4 *>(map_cov)[base + t]; s00[t] = cv.x; s01[t] = cv.y; s11[t] = cv.w; }
            else { s00[t] = 0.0; s01[t] = 0.0; s11[t] = 0.0; }
        }
        __syncthreads();
        if (q.valid)
            for (int t = 0; t < cnt; ++t) { double d2;                         // every thread reads the same LDS word: a broadcast
                if (nn_pair(q, p, sx[t], sy[t], s00[t], s01[t], s11[t], st[t], d2)) nn_take(b, d2, base + t); }
    }
    if (i < n) nn_store(i, b, out_idx, out_d2, out_second);
}

__global__ void __launch_bounds__(256) k_assoc_nn_grid(int n, const double *__restrict__ poses, int n_poses, const int32_t *__restrict__ pose_of_obs,
        const double *__restrict__ obs, double lidar, const double *__restrict__ map_xy, const int32_t *__restrict__ map_type,
        const double *__restrict__ map_cov, const double *__restrict__ pose_cov, NnDev p, GridParams g,
        const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_items,
        int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const NnQuery q = nn_query_of(i, n, poses, n_poses, pose_of_obs, obs, pose_cov, lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    const NnMap map{map_xy, map_type, map_cov};
    if (q.valid)
        grid_walk9(g, cell_start, cell_items, q.gx, q.gy, [&](int j) __attribute__((always_inline)) {
            double d2; if (nn_candidate(map, j, q, p, d2)) nn_take(b, d2, j); });
    nn_store(i, b, out_idx, out_d2, out_second);
}

__global__ void __launch_bounds__(256) k_frame_nn(int k, const double *__restrict__ in, int has_pose_cov, double lidar, int n_map,
        const double *__restrict__ map_xy, const int32_t *__restrict__ map_type, const double *__restrict__ map_cov, NnDev p,
        double *__restrict__ out_z, double *__restrict__ out_g, int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    __shared__ double rd[4], rs[4]; __shared__ int rj[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *ob = in + 12 + 4 * (size_t)i;
    const NnQuery q = nn_query(in, has_pose_cov ? in + 3 : nullptr, ob[0], ob[1], ob[2], ob[3], lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    const NnMap map{map_xy, map_type, map_cov};
    if (q.valid)
        for (int j = tid; j < n_map; j += 256) { double d2; if (nn_candidate(map, j, q, p, d2)) nn_take(b, d2, j); }
    // fixed order: lanes by halving distance inside a wave, then waves 0 .. 3
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(b.d2, off, 64), os = __shfl_down(b.second, off, 64); const int oj = __shfl_down(b.j, off, 64);
        nn_merge(b, od, oj, os);
    }
    if ((tid & 63) == 0) { rd[tid >> 6] = b.d2; rs[tid >> 6] = b.second; rj[tid >> 6] = b.j; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) nn_merge(b, rd[w], rj[w], rs[w]);
        nn_store(i, b, out_idx, out_d2, out_second);
        out_z[2 * i] = q.zx; out_z[2 * i + 1] = q.zy; out_g[2 * i] = q.gx; out_g[2 * i + 1] = q.gy;
    }
}

__global__ void __launch_bounds__(256) k_map_cov_gather(int n, const int64_t *__restrict__ src, const double *__restrict__ values, double *__restrict__ dst) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t s = src[k];
    double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
    if (s >= 0) v = make_double4(values[s], values[s + 1], values[s + 2], values[s + 3]);
    dst[4 * (size_t)k] = v.x; dst[4 * (size_t)k + 1] = v.y; dst[4 * (size_t)k + 2] = v.z; dst[4 * (size_t)k + 3] = v.w;
}

// ---- one-to-one association inside a frame (include/graphslam.h, "one-to-one association"): the greedy matching over the frame's admissible
// pairs in ascending (d2, observation, cone).  A wave owns fpw consecutive frames (1, 2, 4 or 8: the host's guess from the mean frame size,
// which decides speed only) and gives each W lanes, W = 64 / fpw or the power of two that holds the wave's largest frame: 64 / W frames run
// side by side, the rest in further passes — a frame of 8 keeps 8 lanes busy, not 64.  With W = 64 lane l owns observations l, l + 64,
// l + 128, l + 192 of the one frame.  No barrier between waves (their round counts differ).  Per observation the wave keeps its PROPOSAL —
// the best admissible cone by (d2, j) that no observation of the frame has taken — in LDS (12 bytes), and each frame's taken cones in an
// open-addressed table (512 words of LDS a wave, shared out among its frames: always at least two words per observation).
// A round: (1) observations without a proposal search (all of them in the first round, afterwards only those whose
// proposed cone was just taken; the query is recomputed by nn_query, the same bits, rather than kept for 256 observations), (2) the minimum
// of the open proposals by (d2, i, j) over the wave, (3) that pair is taken.  The minimum open proposal IS the frame's smallest open pair —
// every open observation proposes its own smallest open pair — so the pairs are taken in exactly the greedy's order, one per round; the
// mutual-best contest of the rule's text would take several per round at k pair evaluations per observation, which costs more than the
// 24 shuffles of a round here.  d2 and "admissible" are nn_query / nn_pair: nothing about a pair differs from the kernels above.
static constexpr int AS_NEED = -3, AS_DONE = -2;                               // an observation's state where it holds no proposal
static constexpr int AS_TABLE = 512;                                           // >= 2 x GS_NN_FRAME_MAX: a probe always meets an empty word
static constexpr int AS_SLOTS = 4;                                             // GS_NN_FRAME_MAX / 64
static constexpr int AS_PACKED_TABLE = 128;                                    // the wave's table words in use when groups share it (64 / W groups of 2 W words)

// a frame's taken cones: its words of the wave's table in LDS (-1 = empty), mask + 1 of them, at least twice the frame's observations
struct AsTaken { int32_t *t; uint32_t mask; };
__device__ __forceinline__ uint32_t as_hash(int j, uint32_t mask) { return (((uint32_t)j * 2654435761u) >> 23) & mask; }
__device__ __forceinline__ bool as_taken(const AsTaken &tk, int j) {
    for (uint32_t h = as_hash(j, tk.mask);; h = (h + 1) & tk.mask) { const int v = tk.t[h]; if (v == j) return true; if (v < 0) return false; }
}
__device__ __forceinline__ void as_take(const AsTaken &tk, int j) {
    uint32_t h = as_hash(j, tk.mask); while (tk.t[h] >= 0) h = (h + 1) & tk.mask;
    tk.t[h] = j;
}
// the proposal's order (d2, j); a taken cone is looked up only when it would win
__device__ __forceinline__ void as_offer(double &bd, int &bj, double d2, int j, const AsTaken &tk) {
    if ((d2 < bd || (d2 == bd && j < bj)) && !as_taken(tk, j)) { bd = d2; bj = j; }
}
template <bool GRID>
__global__ void __launch_bounds__(256) k_assign_nn(int n, const double *__restrict__ poses, int n_poses, const int32_t *__restrict__ pose_of_obs,
        const double *__restrict__ obs, int n_frames, const int32_t *__restrict__ frame_start, int fpw, double lidar, int n_map,
        const double *__restrict__ map_xy, const int32_t *__restrict__ map_type, const double *__restrict__ map_cov,
        const double *__restrict__ pose_cov, NnDev p, GridParams g, const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_items,
        int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_z, double *__restrict__ out_g) {
    __shared__ double s_d2[4][AS_SLOTS * 64];                                  // 8 + 4 + 8 = 20 KB a workgroup
    __shared__ int32_t s_j[4][AS_SLOTS * 64];
    __shared__ int32_t s_taken[4][AS_TABLE];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f0 = (blockIdx.x * 4 + w) * fpw;                                 // this wave's frames: [f0, f0 + fpw), fpw in {1, 2, 4, 8}
    if (f0 >= n_frames) return;
    const FrameLanes l = frame_lanes(frame_start, f0, fpw, n_frames, n, NN_FRAME_MAX, lane);
    const int W = l.W, gp = l.gp, gi = l.gi, lg = l.lg;
    const NnMap map{map_xy, map_type, map_cov};
    const int tsz = W == 64 ? AS_TABLE : 2 * W;
    double *pd = s_d2[w]; int32_t *pj = s_j[w]; const AsTaken tk{s_taken[w] + gi * tsz, (uint32_t)tsz - 1};
    for (int ps = 0; ps * gp < fpw; ++ps) {                                    // 64 / W frames side by side, pass after pass
        int a = 0, b = 0;
        const int f = f0 + ps * gp + gi;
        if (ps * gp + gi < fpw && f < n_frames) {
            const FrameKind kind = frame_bounds(frame_start, n, f, a, b);
            if (kind == FRAME_LARGE) for (int i = a + lg; i < b; i += W) { out_idx[i] = -1; if (out_d2) out_d2[i] = __builtin_inf(); }
            if (kind != FRAME_OK) a = b = 0;
        }
        const int slots = (b - a + 63) >> 6;                                   // of this lane's frame: 0 (none), 1, or up to 4 when W == 64
        for (int t = lane; t < (W == 64 ? AS_TABLE : AS_PACKED_TABLE); t += 64) s_taken[w][t] = -1;
        for (int s = 0; s < slots; ++s) pj[s * 64 + lane] = a + s * 64 + lg < b ? AS_NEED : AS_DONE;
        wave_sync();
        for (bool first = true;; first = false) {
            // (1) the search
            for (int s = 0; s < slots; ++s) {
                const int e = s * 64 + lane, i = a + s * 64 + lg;
                if (pj[e] != AS_NEED) continue;
                const NnQuery q = nn_query_of(i, n, poses, n_poses, pose_of_obs, obs, pose_cov, lidar, p);
                if (first && out_z) { out_z[2 * i] = q.zx; out_z[2 * i + 1] = q.zy; out_g[2 * i] = q.gx; out_g[2 * i + 1] = q.gy; }
                double bd = __builtin_inf(); int bj = NN_NONE;
                if (q.valid) map_walk<GRID>(n_map, g, cell_start, cell_items, q.gx, q.gy, [&](int j) __attribute__((always_inline)) {
                    double d2; if (nn_candidate(map, j, q, p, d2)) as_offer(bd, bj, d2, j, tk); });
                if (bj == NN_NONE) { out_idx[i] = -1; if (out_d2) out_d2[i] = __builtin_inf(); pj[e] = AS_DONE; }      // no open cone left: final
                else { pd[e] = bd; pj[e] = bj; }
            }
            // (2) the smallest open pair by (d2, i): a lane's slots ascend in i, then the frame's lanes by butterfly (every lane ends with the result)
            double md = __builtin_inf(); int mi = NN_NONE, mj = NN_NONE;
            for (int s = 0; s < slots; ++s) { const int e = s * 64 + lane, j = pj[e];
                if (j >= 0) { const double d = pd[e]; if (mi == NN_NONE || d < md) { md = d; mi = a + s * 64 + lg; mj = j; } } }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                if (off >= W) continue;                                        // (wave-uniform) the butterfly stays inside the frame's W lanes
                const double od = __shfl_xor(md, off, 64); const int oi = __shfl_xor(mi, off, 64), oj = __shfl_xor(mj, off, 64);
                if (oi != NN_NONE && (mi == NN_NONE || od < md || (od == md && oi < mi))) { md = od; mi = oi; mj = oj; }
            }
            // (3) the pair is taken; whoever proposed its cone searches again.  A frame without an open proposal is finished (its lanes idle)
            if (mi != NN_NONE) {
                if (lg == 0) as_take(tk, mj);
                for (int s = 0; s < slots; ++s) { const int e = s * 64 + lane;
                    if (a + s * 64 + lg == mi) { out_idx[mi] = mj; if (out_d2) out_d2[mi] = md; pj[e] = AS_DONE; }
                    else if (pj[e] == mj) pj[e] = AS_NEED; }
            }
            wave_sync();
            if (__ballot(mi != NN_NONE) == 0) break;                           // wave-uniform: every frame of the pass is finished
        }
    }
}

// ---- minimum-cost association inside a frame (include/graphslam.h, "minimum-cost association"): among the matchings over every observation's
// AO_CAND admissible cones of smallest (d2, j), one of largest total gain sum(gate_chi2 - d2).  Three phases per frame:
//   COLLECT   an observation's admissible count and its AO_CAND smallest (d2, j), kept sorted in registers by compare-and-swap (a minimum
//             over (d2, j) does not depend on the order the cones arrive in), then in LDS, candidate-major ([t][row]: no bank conflicts).
//   SHORTCUT  every observation claims its first candidate in the frame's open-addressed table (an LDS compare-and-swap); no claim met
//             another one: the first candidates are the answer (each observation has its own smallest d2: no matching has a smaller sum).
//   SOLVE     successive shortest augmenting paths (Jonker-Volgenant) over the lists, rows = the frame's observations in ascending order,
//             a private dummy column of cost gate_chi2 per row, duals in fp64.  The search tree of a row is kept PER ROW, not per column
//             (a row has at most AO_CAND + 1 edges): a tree row holds the distance rd it was reached at and how (pred); a column is scanned
//             iff its matched row is in the tree; a step takes the minimum over the tree rows' unscanned edges of
//             ((rd + d2) - u[row]) - v[column] by (value, row, slot) — the solve is a function of the lists alone.  v is nonzero only for
//             matched columns and is stored with the matched row (vm), the table maps a matched cone to its row (matched columns stay
//             matched, so the table only grows); unmatched and dummy columns have v = 0.  A step either adds a row to the tree or ends
//             the path: at most rows + 1 steps per row, and every loop below is bounded by the frame's rows, AO_CAND, or the table size.
// Lanes: frames_small / frames_big, wave-scope syncs only.  k_assign_opt runs four waves of 64 rows each (9.5 KB of LDS a wave);
// k_assign_opt_big is ONE wave of 256 rows (38 KB).
static constexpr int AO_CAND = 8;                                              // GS_ASSIGN_CAND_MAX
static constexpr int AO_DUMMY = 8, AO_NOMATE = 9;                              // a row's mate: a slot of its list, its dummy column, or nothing yet

template <int SLOTS> struct AoLds {
    static constexpr int ROWS = 64 * SLOTS, TAB = 2 * ROWS;
    double cd[AO_CAND][ROWS];                                                  // the lists: d2 and cone, sorted by (d2, j)
    int32_t cj[AO_CAND][ROWS];
    double u[ROWS], vm[ROWS], rd[ROWS];                                        // row dual; the dual of the row's matched column; tree distance
    int32_t tkey[TAB], tval[TAB];                                              // matched cone -> row (-1 = empty)
    int32_t cnt[ROWS], mate[ROWS], stamp[ROWS], pred[ROWS];                    // candidates; mate; the root whose tree holds the row; 16 * row + slot it was reached by
};
struct AoArgs : FrameArgs {
    const int32_t *map_type; GridParams g; const int32_t *cell_start, *cell_items; int32_t *out_idx; double *out_d2; int32_t *out_na; double *out_z, *out_g;
};
__device__ __forceinline__ uint32_t ao_hash(int j, uint32_t mask) { return (((uint32_t)j * 2654435761u) >> 21) & mask; }
// the row matched to cone j, or -1
__device__ __forceinline__ int ao_find(const int32_t *tkey, const int32_t *tval, uint32_t mask, int j) {
    uint32_t h = ao_hash(j, mask);
    for (uint32_t pr = 0; pr <= mask; ++pr, h = (h + 1) & mask) { const int v = tkey[h]; if (v == j) return tval[h]; if (v < 0) return -1; }
    return -1;
}
__device__ __forceinline__ void ao_put(int32_t *tkey, int32_t *tval, uint32_t mask, int j, int row) {
    uint32_t h = ao_hash(j, mask);
    for (uint32_t pr = 0; pr <= mask; ++pr, h = (h + 1) & mask) { const int v = tkey[h]; if (v == j || v < 0) { tkey[h] = j; tval[h] = row; return; } }
}
// false when another observation of the frame has claimed cone j already
__device__ __forceinline__ bool ao_claim(int32_t *tkey, uint32_t mask, int j) {
    uint32_t h = ao_hash(j, mask);
    for (uint32_t pr = 0; pr <= mask; ++pr, h = (h + 1) & mask) { const int v = atomicCAS(&tkey[h], -1, j); if (v == -1) return true; if (v == j) return false; }
    return false;
}
// (d2, j) into the sorted list: static indices only, so the list stays in registers
__device__ __forceinline__ void ao_insert(double (&bd)[AO_CAND], int (&bj)[AO_CAND], double d2, int j) {
#pragma unroll
    for (int t = 0; t < AO_CAND; ++t)
        if (d2 < bd[t] || (d2 == bd[t] && j < bj[t])) { const double td = bd[t]; const int tj = bj[t]; bd[t] = d2; bj[t] = j; d2 = td; j = tj; }
}
// one pass of a wave: lane group gi (W lanes, lane lg of it) solves the frame [a, b) (a == b: none), b - a <= W (W < 64) or <= 64 * SLOTS
template <bool GRID, int SLOTS>
__device__ __forceinline__ void ao_pass(AoLds<SLOTS> &L, const AoArgs &A, int a, int b, int W, int gi, int lg, int lane) {
    const int k = b - a, eb = gi * W, slots = (k + 63) >> 6;                   // rows; the LDS row of the frame's row 0; rows per lane
    const int tsz = W == 64 ? AoLds<SLOTS>::TAB : 2 * W;                        // the frame's table: at least two words per row
    int32_t *tkey = L.tkey + gi * tsz, *tval = L.tval + gi * tsz; const uint32_t mask = (uint32_t)tsz - 1;
    const double gate = A.p.gate_chi2; const NnMap map{A.map_xy, A.map_type, A.map_cov};
    // COLLECT
    for (int t = lane; t < AoLds<SLOTS>::TAB; t += 64) L.tkey[t] = -1;
    for (int s = 0; s < slots; ++s) {
        const int rl = s * 64 + lg, e = eb + rl; int c = 0;
        if (rl < k) {
            const int i = a + rl;
            const NnQuery q = nn_query_of(i, A.n, A.poses, A.n_poses, A.pose_of_obs, A.obs, A.pose_cov, A.lidar, A.p);
            if (A.out_z) { A.out_z[2 * i] = q.zx; A.out_z[2 * i + 1] = q.zy; A.out_g[2 * i] = q.gx; A.out_g[2 * i + 1] = q.gy; }
            double bd[AO_CAND]; int bj[AO_CAND]; int na = 0;
#pragma unroll
            for (int t = 0; t < AO_CAND; ++t) { bd[t] = __builtin_inf(); bj[t] = NN_NONE; }
            if (q.valid) map_walk<GRID>(A.n_map, A.g, A.cell_start, A.cell_items, q.gx, q.gy, [&](int j) __attribute__((always_inline)) {
                double d2; if (nn_candidate(map, j, q, A.p, d2)) { ++na; ao_insert(bd, bj, d2, j); } });
            if (A.out_na) A.out_na[i] = na;
            c = na < AO_CAND ? na : AO_CAND;
#pragma unroll
            for (int t = 0; t < AO_CAND; ++t) { L.cd[t][e] = bd[t]; L.cj[t][e] = bj[t]; }
        }
        L.cnt[e] = c; L.mate[e] = AO_NOMATE; L.stamp[e] = -1;
    }
    wave_sync();
    // SHORTCUT
    bool dup = false;
    for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg, e = eb + rl;
        if (rl < k && L.cnt[e] > 0 && !ao_claim(tkey, mask, L.cj[0][e])) dup = true; }
    const unsigned long long gm = W == 64 ? ~0ull : ((1ull << W) - 1) << eb;
    const bool contested = (__ballot(dup) & gm) != 0;                          // (uniform over the frame's lanes)
    wave_sync();
    if (!contested) {
        for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg, e = eb + rl;
            if (rl < k) { const bool m = L.cnt[e] > 0; A.out_idx[a + rl] = m ? L.cj[0][e] : -1; if (A.out_d2) A.out_d2[a + rl] = m ? L.cd[0][e] : __builtin_inf(); } }
    } else
        for (int t = lg; t < tsz; t += W) tkey[t] = -1;
    // SOLVE: `root` is the row being added (k: the frame is finished); rows without a candidate are passed over
    int root = k;
    if (contested) { root = 0; while (root < k && L.cnt[eb + root] == 0) ++root;
        if (lg == 0 && root < k) { L.stamp[eb + root] = root; L.rd[eb + root] = 0.0; L.u[eb + root] = 0.0; } }
    wave_sync();
    const int cap = W == 64 ? 64 * SLOTS : W, maxit = (cap + 2) * (cap + 2);  // rows * (rows + 1) steps at the most: a hard stop all the same
    for (int it = 0; it < maxit; ++it) {
        const bool act = root < k;
        if (__ballot(act) == 0) break;                                         // wave-uniform: every frame of the pass is finished
        // (1) the smallest unscanned edge of this lane's tree rows; (row, slot) ascend, so < keeps the first
        double mk = __builtin_inf(); int mr = NN_NONE, ms = 0;
        if (act)
            for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg, e = eb + rl;
                if (rl >= k || L.stamp[e] != root) continue;
                const double rdv = L.rd[e], uv = L.u[e]; const int c = L.cnt[e];
                for (int t = 0; t < c; ++t) {
                    const int r = ao_find(tkey, tval, mask, L.cj[t][e]);
                    if (r >= 0 && L.stamp[eb + r] == root) continue;           // the column is scanned
                    const double key = ((rdv + L.cd[t][e]) - uv) - (r >= 0 ? L.vm[eb + r] : 0.0);
                    if (mr == NN_NONE || key < mk) { mk = key; mr = rl; ms = t; }
                }
                if (L.mate[e] != AO_DUMMY) { const double key = (rdv + gate) - uv;
                    if (mr == NN_NONE || key < mk) { mk = key; mr = rl; ms = AO_DUMMY; } }
            }
        // (2) over the frame's lanes by butterfly, by (value, row, slot): every lane ends with the result
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            if (off >= W) continue;
            const double od = __shfl_xor(mk, off, 64); const int orw = __shfl_xor(mr, off, 64), os = __shfl_xor(ms, off, 64);
            if (orw != NN_NONE && (mr == NN_NONE || od < mk || (od == mk && (orw < mr || (orw == mr && os < ms))))) { mk = od; mr = orw; ms = os; }
        }
        // (3) a matched column: its row joins the tree.  A free or a dummy column: the path ends — duals, then the flip along pred
        int r = -1; bool term = false;
        if (act) {
            if (mr == NN_NONE) root = k;                                       // (cannot happen: the root's dummy column is always free)
            else { if (ms != AO_DUMMY) r = ao_find(tkey, tval, mask, L.cj[ms][eb + mr]);
                term = r < 0;
                if (!term && lg == 0) { L.stamp[eb + r] = root; L.rd[eb + r] = mk; L.pred[eb + r] = 16 * mr + ms; } }
        }
        if (term)
            for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg, e = eb + rl;
                if (rl < k && L.stamp[e] == root) { const double dl = mk - L.rd[e]; L.u[e] += dl; if (rl != root) L.vm[e] -= dl; } }
        wave_sync();
        if (term) {
            if (lg == 0) {
                int row = mr, slot = ms; double cv = 0.0;
                for (int nn = 0; nn <= k; ++nn) {
                    const int e = eb + row; const double ov = L.vm[e]; const int pd = L.pred[e];
                    L.mate[e] = slot; L.vm[e] = cv;
                    if (slot != AO_DUMMY) ao_put(tkey, tval, mask, L.cj[slot][e], row);
                    if (row == root) break;
                    cv = ov; row = pd >> 4; slot = pd & 15;                    // the row's old column goes to the row it was reached from
                }
            }
            ++root; while (root < k && L.cnt[eb + root] == 0) ++root;
            if (lg == 0 && root < k) { L.stamp[eb + root] = root; L.rd[eb + root] = 0.0; L.u[eb + root] = 0.0; }
        }
        wave_sync();
    }
    if (contested)
        for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg, e = eb + rl;
            if (rl < k) { const int m = L.mate[e]; A.out_idx[a + rl] = m < AO_CAND ? L.cj[m][e] : -1;
                if (A.out_d2) A.out_d2[a + rl] = m < AO_CAND ? L.cd[m][e] : __builtin_inf(); } }
    wave_sync();                                                                 // the next pass fills the same LDS
}
template <bool GRID>
__global__ void __launch_bounds__(256) k_assign_opt(AoArgs A) {
    __shared__ AoLds<1> Ls[4];
    frames_small(A, [&](int, int a, int b, const FrameLanes &l, int lane) __attribute__((always_inline)) {
        ao_pass<GRID, 1>(Ls[threadIdx.x >> 6], A, a, b, l.W, l.gi, l.lg, lane); });
}
template <bool GRID>
__global__ void __launch_bounds__(64) k_assign_opt_big(AoArgs A) {
    __shared__ AoLds<4> L;
    frames_big(A, [&](int, int a, int b, int lane) __attribute__((always_inline)) {      // refused: -1 / +inf / 0
                   for (int i = a + lane; i < b; i += 64) { A.out_idx[i] = -1; if (A.out_d2) A.out_d2[i] = __builtin_inf(); if (A.out_na) A.out_na[i] = 0; } },
               [&](int, int a, int b, const FrameLanes &l, int lane) __attribute__((always_inline)) {
                   if (b > a) ao_pass<GRID, 4>(L, A, a, b, l.W, l.gi, l.lg, lane); });
}

// ---- joint compatibility of a frame's hypothesis (include/graphslam.h, "joint compatibility"): the pairs (i, in_idx[i]) of a frame share ONE
// pose error, so their joint innovation covariance is blockdiag(D_i) + G Sigma_p G^T and Woodbury turns nu^T S^-1 nu into sums of per-pair
// terms and one 3x3 solve:  J = a - c^T delta,  delta = Sigma_p (I + M Sigma_p)^-1 c.  No map search: l_j and Sigma_j are gathered through
// in_idx, so the batch, the resident and the frame call run the one function below.
//   PAIRS   a row's ten terms (a, c[3], M[6]) once, into LDS term-major ([t][row]: no bank conflicts); only the lane that wrote a row reads it
//   ROUND   the sums over the kept rows in a FIXED order — a lane's rows ascending from +0, then the wave's 64 lanes by butterfly at distance
//           32, 16 .. 1 (fp64 addition commutes, so every lane holds the same bits; a lane without a kept row adds +0, which changes nothing:
//           the bits do not depend on how many lanes W the frame was given) — and the 3x3 solve, on every lane.  J < gate[kept]: finished.
//           Otherwise every kept row solves for (sums - its own terms) and the row of smallest (J, row) leaves.  The sums are recomputed from
//           the kept rows in every round, never carried: a round's error does not depend on the rounds before it.
// Lanes as frames_small / frames_big give them, W per frame and 64 / W frames side by side, but through this section's own copy of the two
// drivers, and jc_pass finds the frame's pose and sums the rows in its own text (lo_pass repeats both): with the shared drivers and a shared
// pose search and sum k_joint_compat measured 1.0 .. 1.4 % slower than before on an MI355X (profiles/assoc_scaffold_time.txt), with its own
// it does not.  At most rows + 1 rounds; no barrier, no scratch, no wait.
template <int SLOTS> struct JcLds { double t[JC_TERMS][64 * SLOTS]; int32_t kj[64 * SLOTS]; };       // kj: the row's cone while it is kept, else -1
struct JcArgs : FrameArgs {
    const int32_t *in_idx; int32_t *out_idx; double *out_j; int32_t *out_kept, *out_dropped, *out_untestable; double *out_delta; JcGate gate;
};
// (the solve in three pieces, so that lo_pass below runs the same operations.)  P = Sigma_p's upper triangle (p00 p01 p02 p11 p12 p22)
// K = the nine cofactors of A = I + M Sigma_p (K[3 r + s] = C_rs) and det A, from the sums' M (S[4 .. 9])
__device__ __forceinline__ double jc_cofactors(const double (&S)[JC_TERMS], const double (&P)[6], double (&K)[9]) {
#pragma clang fp contract(off)
    const double m00 = S[4], m01 = S[5], m02 = S[6], m11 = S[7], m12 = S[8], m22 = S[9];
    const double p00 = P[0], p01 = P[1], p02 = P[2], p11 = P[3], p12 = P[4], p22 = P[5];
    // A = I + M Sigma_p
    const double a00 = 1.0 + ((m00 * p00 + m01 * p01) + m02 * p02), a01 = (m00 * p01 + m01 * p11) + m02 * p12, a02 = (m00 * p02 + m01 * p12) + m02 * p22;
    const double a10 = (m01 * p00 + m11 * p01) + m12 * p02, a11 = 1.0 + ((m01 * p01 + m11 * p11) + m12 * p12), a12 = (m01 * p02 + m11 * p12) + m12 * p22;
    const double a20 = (m02 * p00 + m12 * p01) + m22 * p02, a21 = (m02 * p01 + m12 * p11) + m22 * p12, a22 = 1.0 + ((m02 * p02 + m12 * p12) + m22 * p22);
    // cofactors C[r][s] of A; x = adj(A) c / det = C^T c / det
    const double k00 = a11 * a22 - a12 * a21, k01 = a12 * a20 - a10 * a22, k02 = a10 * a21 - a11 * a20;
    const double k10 = a02 * a21 - a01 * a22, k11 = a00 * a22 - a02 * a20, k12 = a01 * a20 - a00 * a21;
    const double k20 = a01 * a12 - a02 * a11, k21 = a02 * a10 - a00 * a12, k22 = a00 * a11 - a01 * a10;
    K[0] = k00; K[1] = k01; K[2] = k02; K[3] = k10; K[4] = k11; K[5] = k12; K[6] = k20; K[7] = k21; K[8] = k22;
    return (a00 * k00 + a01 * k01) + a02 * k02;
}
// x = C^T c / det A and dl = Sigma_p x, c = S[1 .. 3]; returns det A
__device__ __forceinline__ double jc_step(const double (&S)[JC_TERMS], const double (&P)[6], double (&x)[3], double (&dl)[3]) {
#pragma clang fp contract(off)
    double K[9];
    const double det = jc_cofactors(S, P, K);
    const double c0 = S[1], c1 = S[2], c2 = S[3];
    const double p00 = P[0], p01 = P[1], p02 = P[2], p11 = P[3], p12 = P[4], p22 = P[5];
    const double k00 = K[0], k01 = K[1], k02 = K[2], k10 = K[3], k11 = K[4], k12 = K[5], k20 = K[6], k21 = K[7], k22 = K[8];
    const double x0 = ((k00 * c0 + k10 * c1) + k20 * c2) / det, x1 = ((k01 * c0 + k11 * c1) + k21 * c2) / det, x2 = ((k02 * c0 + k12 * c1) + k22 * c2) / det;
    x[0] = x0; x[1] = x1; x[2] = x2;
    dl[0] = (p00 * x0 + p01 * x1) + p02 * x2; dl[1] = (p01 * x0 + p11 * x1) + p12 * x2; dl[2] = (p02 * x0 + p12 * x1) + p22 * x2;
    return det;
}
// J and delta of the sums S; has_p false: Sigma_p = 0, delta = 0 and J = a
__device__ __forceinline__ double jc_solve(const double (&S)[JC_TERMS], const double (&P)[6], bool has_p, double (&dl)[3]) {
#pragma clang fp contract(off)
    dl[0] = dl[1] = dl[2] = 0.0;
    if (!has_p) return S[0];
    double x[3];
    jc_step(S, P, x, dl);
    return S[0] - ((S[1] * dl[0] + S[2] * dl[1]) + S[3] * dl[2]);
}
// one pass of a wave: lane group gi (W lanes, lane lg of it) tests the frame fw = [a, b) (fw < 0: none), b - a <= W (W < 64) or <= 64 * SLOTS.
// Row rl of the frame sits at LDS row (rl / 64) * 64 + lane: lane == eb + lg with W < 64, lane == rl % 64 with W == 64.
template <int SLOTS>
__device__ __forceinline__ void jc_pass(JcLds<SLOTS> &L, const JcArgs &A, int fw, int a, int b, int W, int lg, int lane) {
#pragma clang fp contract(off)
    const int k = fw < 0 ? 0 : b - a, slots = (k + 63) >> 6;
    // the frame's pose: the one index inside [0, n_poses) its observations name; two different ones: the frame is refused as a whole
    int plo = NN_NONE, phi = -1;
    for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg;
        if (rl < k) { const int pi = A.pose_of_obs[a + rl]; if (pi >= 0 && pi < A.n_poses) { plo = min(plo, pi); phi = max(phi, pi); } } }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if (off >= W) continue;                                                // (wave-uniform) the butterfly stays inside the frame's W lanes
        plo = min(plo, __shfl_xor(plo, off, 64)); phi = max(phi, __shfl_xor(phi, off, 64));
    }
    const bool mixed = phi >= 0 && plo != phi;
    const bool has_p = A.pose_cov != nullptr && phi >= 0 && !mixed;
    double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (has_p) { const double *pc = A.pose_cov + 9 * (size_t)plo; P[0] = pc[0]; P[1] = pc[1]; P[2] = pc[2]; P[3] = pc[4]; P[4] = pc[5]; P[5] = pc[8]; }
    // PAIRS
    int nun = 0;                                                               // this lane's untestable rows
    for (int s = 0; s < slots; ++s) {
        const int rl = s * 64 + lg, e = s * 64 + lane; int keep = -1;
        if (rl < k && !mixed) {
            const int i = a + rl, j = A.in_idx[i];
            if (j != -1) {
                const NnQuery q = nn_query_of(i, A.n, A.poses, A.n_poses, A.pose_of_obs, A.obs, nullptr, A.lidar, A.p);      // a = Q alone
                bool ok = q.valid && j >= 0 && j < A.n_map;
                if (ok) {
                    const PairNu v = pair_nu(q, nn_cone(A.map_xy, A.map_cov, j));
                    ok = v.det > 0.0 && v.d00 > 0.0;
                    if (ok) {
                        double sn, cs, T[JC_TERMS]; sincos(A.poses[3 * (size_t)plo + 2], &sn, &cs);
                        pair_terms(q, v, sn, cs, T);
#pragma unroll
                        for (int t = 0; t < JC_TERMS; ++t) L.t[t][e] = T[t];
                        keep = j;
                    }
                }
                if (!ok) ++nun;
            }
        }
        L.kj[e] = keep;
    }
    // ROUNDS
    double J = 0.0, dl[3] = {0.0, 0.0, 0.0}; int kept = 0, dropped = 0; bool open = fw >= 0 && !mixed;
    for (int round = 0; round <= 64 * SLOTS; ++round) {                        // a round that does not finish the frame removes a row: rows + 1 at the most
        double S[JC_TERMS]; int cnt = 0;
#pragma unroll
        for (int t = 0; t < JC_TERMS; ++t) S[t] = 0.0;
        for (int s = 0; s < slots; ++s) { const int e = s * 64 + lane;
            if (L.kj[e] >= 0) { ++cnt;
#pragma unroll
                for (int t = 0; t < JC_TERMS; ++t) S[t] += L.t[t][e]; } }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            if (off >= W) continue;
            cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
            for (int t = 0; t < JC_TERMS; ++t) S[t] += __shfl_xor(S[t], off, 64);
        }
        if (open) { J = jc_solve(S, P, has_p, dl); kept = cnt; open = !(cnt == 0 || J < A.gate.g[cnt]); }
        if (__ballot(open) == 0) break;                                        // wave-uniform: every frame of the pass is finished
        // the row whose removal leaves the smallest J, by (J, row): a lane's rows ascend, so < keeps the first
        double mk = __builtin_inf(); int mr = NN_NONE;
        if (open)
            for (int s = 0; s < slots; ++s) { const int e = s * 64 + lane;
                if (L.kj[e] < 0) continue;
                double R[JC_TERMS], du[3];
#pragma unroll
                for (int t = 0; t < JC_TERMS; ++t) R[t] = S[t] - L.t[t][e];
                const double jr = jc_solve(R, P, has_p, du);
                if (mr == NN_NONE || jr < mk) { mk = jr; mr = s * 64 + lg; } }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            if (off >= W) continue;
            const double od = __shfl_xor(mk, off, 64); const int orw = __shfl_xor(mr, off, 64);
            if (orw != NN_NONE && (mr == NN_NONE || od < mk || (od == mk && orw < mr))) { mk = od; mr = orw; }
        }
        if (open && mr != NN_NONE) { ++dropped; if ((mr & 63) == lg) L.kj[(mr & ~63) + lane] = -1; }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { if (off >= W) continue; nun += __shfl_xor(nun, off, 64); }
    if (fw < 0) return;
    if (mixed) { J = __builtin_inf(); kept = dropped = 0; }
    for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg; if (rl < k) A.out_idx[a + rl] = L.kj[s * 64 + lane]; }
    if (lg == 0) {
        if (A.out_j) A.out_j[fw] = J;
        if (A.out_kept) A.out_kept[fw] = kept;
        if (A.out_dropped) A.out_dropped[fw] = dropped;
        if (A.out_untestable) A.out_untestable[fw] = mixed ? 0 : nun;
        if (A.out_delta) { A.out_delta[3 * (size_t)fw] = dl[0]; A.out_delta[3 * (size_t)fw + 1] = dl[1]; A.out_delta[3 * (size_t)fw + 2] = dl[2]; }
    }
}
// frame f of the call: its bounds, and whether it is one (bounds outside 0 <= a <= b <= n: not a frame, nothing read or written).  Above
// GS_NN_FRAME_MAX (when `refuse`): -1 per observation, +inf, counts and delta 0, and not a frame for the pass
__device__ __forceinline__ bool jc_frame(const JcArgs &A, int f, bool refuse, int lg, int W, int &a, int &b) {
    a = A.frame_start[f]; b = A.frame_start[f + 1];
    if (a < 0 || b < a || b > A.n) return false;
    if (b - a <= 256) return true;
    if (refuse) {
        for (int i = a + lg; i < b; i += W) A.out_idx[i] = -1;
        if (lg == 0) {
            if (A.out_j) A.out_j[f] = __builtin_inf();
            if (A.out_kept) A.out_kept[f] = 0;
            if (A.out_dropped) A.out_dropped[f] = 0;
            if (A.out_untestable) A.out_untestable[f] = 0;
            if (A.out_delta) { A.out_delta[3 * (size_t)f] = 0.0; A.out_delta[3 * (size_t)f + 1] = 0.0; A.out_delta[3 * (size_t)f + 2] = 0.0; }
        }
    }
    return false;
}
__global__ void __launch_bounds__(256) k_joint_compat(JcArgs A) {
    __shared__ JcLds<1> Ls[4];                                                 // 5.25 KB a wave
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f0 = (blockIdx.x * 4 + w) * A.fpw;                               // this wave's frames: [f0, f0 + fpw), fpw in {2, 4, 8}
    if (f0 >= A.n_frames) return;
    int W = 64 / A.fpw;                                                        // (frame_lanes' text) frames above 64 are k_joint_compat_big's
    for (int t = 0; t < A.fpw && f0 + t < A.n_frames; ++t) { const int a = A.frame_start[f0 + t], b = A.frame_start[f0 + t + 1];
        if (a >= 0 && b >= a && b <= A.n && b - a <= 64) while (W < 64 && W < b - a) W <<= 1; }
    const int gp = 64 / W, gi = lane >> __builtin_ctz(W), lg = lane & (W - 1);
    for (int ps = 0; ps * gp < A.fpw; ++ps) {
        int a = 0, b = 0, fw = -1; const int f = f0 + ps * gp + gi;
        if (ps * gp + gi < A.fpw && f < A.n_frames && jc_frame(A, f, false, lg, W, a, b) && b - a <= 64) fw = f;
        jc_pass<1>(Ls[w], A, fw, a, b, W, lg, lane);
    }
}
__global__ void __launch_bounds__(64) k_joint_compat_big(JcArgs A) {
    __shared__ JcLds<4> L;                                                     // 21 KB
    const int lane = threadIdx.x, f0 = blockIdx.x * A.fpw;
    for (int t = 0; t < A.fpw && f0 + t < A.n_frames; ++t) {
        int a, b;
        if (!jc_frame(A, f0 + t, true, lane, 64, a, b) || (A.only_large && b - a <= 64)) continue;      // (wave-uniform)
        jc_pass<4>(L, A, f0 + t, a, b, 64, lane, lane);
    }
}

// ---- frame localisation (include/graphslam.h, "frame localisation"): the maximum-a-posteriori pose under the prior (x0, Sigma_p) and the
// frame's pairs (i, in_idx[i]), by iterated relinearisation — the joint test's sums and solve at the moving pose x_k = x0 + d_k, with the
// right-hand side c + M d_k, so that d_{k+1} = (Sigma_p^-1 + M)^-1 (c + M d_k) without inverting Sigma_p — then one more pass at the last pose for
// the posterior covariance Sigma_p (I + M Sigma_p)^-1 and chi2.
//   FETCH   what no iteration changes, once: z (the A0 conversion), l_j, Sigma_j — seven doubles a row, in registers for frames up to 64
//           (a row per lane), in LDS term-major for the large form (only the lane that wrote a row reads it); a row that can never count
//           (no pair, an index outside the map, a pose index out of range) is left out by a bit of `live`
//   ITERATE the pair terms at x_k (nn_query_at without a pose covariance, then pair_nu and pair_terms), the sums of c, M and the count in
//           the joint test's fixed order, the 3x3 solve on every lane (jc_step), the stop tests; a __ballot over the frames still open ends
//           the loop, max_iterations bounds it
//   FINAL   the pair terms with a (nn_pair's d2), the sums, the cofactors of A once more (jc_cofactors), Sigma+ and chi2
// Lanes: frames_small / frames_big; no barrier, no scratch, no wait, nothing written per observation.
static constexpr int LO_FIXED = 7;                                             // zx zy lx ly c00 c01 c11
template <int SLOTS> struct LoRows;
template <> struct LoRows<1> {                                                 // a row per lane: registers
    double r[LO_FIXED];
    __device__ __forceinline__ void put(int, int, const double (&v)[LO_FIXED]) {
#pragma unroll
        for (int t = 0; t < LO_FIXED; ++t) r[t] = v[t]; }
    __device__ __forceinline__ void get(int, int, double (&v)[LO_FIXED]) const {
#pragma unroll
        for (int t = 0; t < LO_FIXED; ++t) v[t] = r[t]; }
};
struct LoLds { double f[LO_FIXED][256]; };                                     // 14 KB
template <> struct LoRows<4> {                                                 // four rows per lane: LDS, row s * 64 + lane
    LoLds *L;
    __device__ __forceinline__ void put(int s, int lane, const double (&v)[LO_FIXED]) {
#pragma unroll
        for (int t = 0; t < LO_FIXED; ++t) L->f[t][s * 64 + lane] = v[t]; }
    __device__ __forceinline__ void get(int s, int lane, double (&v)[LO_FIXED]) const {
#pragma unroll
        for (int t = 0; t < LO_FIXED; ++t) v[t] = L->f[t][s * 64 + lane]; }
};
struct LoArgs : FrameArgs {
    const int32_t *in_idx; int max_it; double tol_xy, tol_th;
    double *out_pose, *out_cov, *out_chi2; int32_t *out_pairs, *out_iters, *out_status; double *out_step;
};
// one row's terms at the pose (sn, cs: its heading's sin / cos) ADDED to S (a, c[3], M[6]: jc_solve's layout) when the pair counts; FINAL: a
// and M, else c and M (the terms not added are never computed: everything here is inlined)
template <bool FINAL>
__device__ __forceinline__ bool lo_row(const double (&v)[LO_FIXED], const double (&pose)[3], double sn, double cs, const NnDev &p, double (&S)[JC_TERMS]) {
#pragma clang fp contract(off)
    const NnQuery q = nn_query_at(pose, nullptr, make_double2(v[0], v[1]), sn, cs, 0.0, p);
    if (!q.valid) return false;
    const PairNu nu = pair_nu(q, NnCone{v[2], v[3], v[4], v[5], v[6]});
    if (!(nu.det > 0.0 && nu.d00 > 0.0 && isfinite(nu.n0) && isfinite(nu.n1))) return false;     // (a non-finite cone position never counts)
    double T[JC_TERMS]; pair_terms(q, nu, sn, cs, T);
    if (FINAL) S[0] += T[0];
    else { S[1] += T[1]; S[2] += T[2]; S[3] += T[3]; }
#pragma unroll
    for (int t = 4; t < JC_TERMS; ++t) S[t] += T[t];
    return true;
}
// the sums of the frame's live rows at the pose, in the fixed order of jc_pass: a lane's rows ascending from +0, then the butterfly inside the W lanes
template <int SLOTS, bool FINAL>
__device__ __forceinline__ int lo_sums(const LoRows<SLOTS> &R, const LoArgs &A, int live, int slots, int W, int lane, const double (&pose)[3], double (&S)[JC_TERMS]) {
    double sn, cs; sincos(pose[2], &sn, &cs);
    int cnt = 0;
#pragma unroll
    for (int t = 0; t < JC_TERMS; ++t) S[t] = 0.0;
    for (int s = 0; s < slots; ++s)
        if (live >> s & 1) { double v[LO_FIXED]; R.get(s, lane, v); cnt += lo_row<FINAL>(v, pose, sn, cs, A.p, S) ? 1 : 0; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if (off >= W) continue;                                                // (wave-uniform) the butterfly stays inside the frame's W lanes
        cnt += __shfl_xor(cnt, off, 64);
#pragma unroll
        for (int t = 0; t < JC_TERMS; ++t) S[t] += __shfl_xor(S[t], off, 64);
    }
    return cnt;
}
// a frame's record.  Status 4 (a refused frame): zeros, chi2 +inf
__device__ __forceinline__ void lo_write(const LoArgs &A, int f, const double (&pose)[3], const double (&cv)[6], double chi2, int pairs, int iters, int status,
                                         const double (&d)[3]) {
    if (A.out_pose) { double *o = A.out_pose + 3 * (size_t)f; o[0] = pose[0]; o[1] = pose[1]; o[2] = pose[2]; }
    if (A.out_cov) { double *o = A.out_cov + 9 * (size_t)f;                    // the upper triangle, mirrored
        o[0] = cv[0]; o[1] = cv[1]; o[2] = cv[2]; o[3] = cv[1]; o[4] = cv[3]; o[5] = cv[4]; o[6] = cv[2]; o[7] = cv[4]; o[8] = cv[5]; }
    if (A.out_chi2) A.out_chi2[f] = chi2;
    if (A.out_pairs) A.out_pairs[f] = pairs;
    if (A.out_iters) A.out_iters[f] = iters;
    if (A.out_status) A.out_status[f] = status;
    if (A.out_step) { double *o = A.out_step + 3 * (size_t)f; o[0] = d[0]; o[1] = d[1]; o[2] = d[2]; }
}
// one pass of a wave: lane group gi (W lanes, lane lg of it) localises the frame fw = [a, b) (fw < 0: none), b - a <= W (W < 64) or <= 64 * SLOTS
template <int SLOTS>
__device__ __forceinline__ void lo_pass(LoRows<SLOTS> &R, const LoArgs &A, int fw, int a, int b, int W, int lg, int lane) {
#pragma clang fp contract(off)
    const int k = fw < 0 ? 0 : b - a, slots = (k + 63) >> 6;
    // the frame's pose, found as in jc_pass
    int plo = NN_NONE, phi = -1;
    for (int s = 0; s < slots; ++s) { const int rl = s * 64 + lg;
        if (rl < k) { const int pi = A.pose_of_obs[a + rl]; if (pi >= 0 && pi < A.n_poses) { plo = min(plo, pi); phi = max(phi, pi); } } }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        if (off >= W) continue;
        plo = min(plo, __shfl_xor(plo, off, 64)); phi = max(phi, __shfl_xor(phi, off, 64));
    }
    const bool mixed = phi >= 0 && plo != phi, posed = phi >= 0 && !mixed;
    const bool has_p = A.pose_cov != nullptr && posed;
    double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, x0[3] = {0.0, 0.0, 0.0};
    if (posed) { const double *ps = A.poses + 3 * (size_t)plo; x0[0] = ps[0]; x0[1] = ps[1]; x0[2] = ps[2]; }
    if (has_p) { const double *pc = A.pose_cov + 9 * (size_t)plo; P[0] = pc[0]; P[1] = pc[1]; P[2] = pc[2]; P[3] = pc[4]; P[4] = pc[5]; P[5] = pc[8]; }
    // FETCH
    int live = 0;
    for (int s = 0; s < slots; ++s) {
        const int rl = s * 64 + lg;
        if (rl < k && posed) {
            const int i = a + rl, j = A.in_idx[i], pi = A.pose_of_obs[i];
            if (j >= 0 && j < A.n_map && pi >= 0 && pi < A.n_poses) {
                const double4 o4 = reinterpret_cast<const double4 *>(A.obs)[i];
                const double2 z = nn_polar(o4.x, o4.y, o4.z, A.lidar); const NnCone c = nn_cone(A.map_xy, A.map_cov, j);
                const double v[LO_FIXED] = {z.x, z.y, c.x, c.y, c.c00, c.c01, c.c11};
                R.put(s, lane, v); live |= 1 << s;
            }
        }
    }
    // ITERATE
    double d[3] = {0.0, 0.0, 0.0}, x[3] = {0.0, 0.0, 0.0}, S[JC_TERMS];
    int iters = 0, status = has_p ? 1 : posed ? 0 : 2; bool open = fw >= 0 && has_p;
    for (int it = 0; it < A.max_it; ++it) {
        if (__ballot(open) == 0) break;                                        // wave-uniform: every frame of the pass has stopped
        double xk[3] = {x0[0], x0[1], x0[2]};
        if (it > 0) { xk[0] = x0[0] + d[0]; xk[1] = x0[1] + d[1]; xk[2] = x0[2] + d[2]; }      // not normalised: sincos is periodic
        const int cnt = lo_sums<SLOTS, false>(R, A, live, slots, W, lane, xk, S);
        if (open && it == 0 && cnt == 0) { status = 2; open = false; }
        if (open) {
            if (it > 0) {                                                      // b = c + M d
                const double b0 = S[1] + ((S[4] * d[0] + S[5] * d[1]) + S[6] * d[2]), b1 = S[2] + ((S[5] * d[0] + S[7] * d[1]) + S[8] * d[2]),
                             b2 = S[3] + ((S[6] * d[0] + S[8] * d[1]) + S[9] * d[2]);
                S[1] = b0; S[2] = b1; S[3] = b2; }
            double xn[3], dn[3];
            const double det = jc_step(S, P, xn, dn); ++iters;
            if (!(isfinite(det) && isfinite(dn[0]) && isfinite(dn[1]) && isfinite(dn[2]))) { status = 3; open = false; }
            else {
                const bool conv = fabs(dn[0] - d[0]) <= A.tol_xy && fabs(dn[1] - d[1]) <= A.tol_xy && fabs(dn[2] - d[2]) <= A.tol_th;
                d[0] = dn[0]; d[1] = dn[1]; d[2] = dn[2]; x[0] = xn[0]; x[1] = xn[1]; x[2] = xn[2];
                if (conv) { status = 0; open = false; }
            }
        }
    }
    // FINAL
    double xf[3] = {x0[0], x0[1], x0[2]};
    if (iters > 0) { xf[0] = x0[0] + d[0]; xf[1] = x0[1] + d[1]; xf[2] = x0[2] + d[2]; }
    const int pairs = lo_sums<SLOTS, true>(R, A, live, slots, W, lane, xf, S);
    if (fw < 0 || lg != 0) return;
    const double zero3[3] = {0.0, 0.0, 0.0}, zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (mixed) { lo_write(A, fw, zero3, zero6, __builtin_inf(), 0, 0, 4, zero3); return; }
    if (status == 2) { lo_write(A, fw, x0, P, 0.0, 0, 0, 2, zero3); return; }  // (a frame without a pose: x0 and P are zeros)
    double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, chi2 = S[0];
    if (has_p && status != 3) {
        double K[9];
        const double det = jc_cofactors(S, P, K);
        if (!isfinite(det)) status = 3;
        // Sigma+ = Sigma_p adj(A) / det A: entry (r, s) = sum_t P_rt C_st / det
        cv[0] = ((P[0] * K[0] + P[1] * K[1]) + P[2] * K[2]) / det; cv[1] = ((P[0] * K[3] + P[1] * K[4]) + P[2] * K[5]) / det;
        cv[2] = ((P[0] * K[6] + P[1] * K[7]) + P[2] * K[8]) / det; cv[3] = ((P[1] * K[3] + P[3] * K[4]) + P[4] * K[5]) / det;
        cv[4] = ((P[1] * K[6] + P[3] * K[7]) + P[4] * K[8]) / det; cv[5] = ((P[2] * K[6] + P[4] * K[7]) + P[5] * K[8]) / det;
        chi2 = S[0] + ((x[0] * d[0] + x[1] * d[1]) + x[2] * d[2]);
    }
    if (status == 3) { lo_write(A, fw, x0, P, __builtin_inf(), 0, iters, 3, zero3); return; }
    xf[2] = normalize_theta(xf[2]);                                         // k_update's addition and normalisation
    lo_write(A, fw, xf, cv, chi2, pairs, iters, status, d);
}
__global__ void __launch_bounds__(256) k_localize(LoArgs A) {
    frames_small(A, [&](int fw, int a, int b, const FrameLanes &l, int lane) __attribute__((always_inline)) {
        LoRows<1> R;
        lo_pass<1>(R, A, fw, a, b, l.W, l.lg, lane); });
}
__global__ void __launch_bounds__(64) k_localize_big(LoArgs A) {
    __shared__ LoLds L;
    LoRows<4> R{&L};
    frames_big(A, [&](int f, int, int, int lane) __attribute__((always_inline)) {         // refused: the record of status 4
                   const double zero3[3] = {0.0, 0.0, 0.0}, zero6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                   if (lane == 0) lo_write(A, f, zero3, zero6, __builtin_inf(), 0, 0, 4, zero3); },
               [&](int f, int a, int b, const FrameLanes &l, int lane) __attribute__((always_inline)) { lo_pass<4>(R, A, f, a, b, l.W, l.lg, lane); });
}

void launch_assoc_nn(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, double *out_second, Launch L) {
    if (o.n <= 0) return;
    const dim3 grid((o.n + 255) / 256), block(256);
    if (m.cell_start) hipExtLaunchKernelGGL(k_assoc_nn_grid, grid, block, 0, L.st, L.start, L.stop, 0, o.n, o.poses, o.n_poses, o.pose_of_obs, o.obs, lidar,
                                            m.xy, m.type, m.cov, o.pose_cov, p, grid_params_of(p.max_distance, m.buckets), m.cell_start, m.cell_items,
                                            out_idx, out_d2, out_second);
    else hipExtLaunchKernelGGL(k_assoc_nn, grid, block, 0, L.st, L.start, L.stop, 0, o.n, o.poses, o.n_poses, o.pose_of_obs, o.obs, lidar, m.n,
                               m.xy, m.type, m.cov, o.pose_cov, p, out_idx, out_d2, out_second);
}
void launch_frame_nn(int k, const double *in, int has_pose_cov, const MapRef &m, double lidar, NnDev p, double *out_z, double *out_g, int32_t *out_idx,
                     double *out_d2, double *out_second, hipStream_t st) {
    if (k > 0) hipLaunchKernelGGL(k_frame_nn, dim3(k), dim3(256), 0, st, k, in, has_pose_cov, lidar, m.n, m.xy, m.type, m.cov, p,
                                  out_z, out_g, out_idx, out_d2, out_second);
}
void launch_map_cov_gather(int n, const int64_t *src, const double *values, double *map_cov_first, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_map_cov_gather, dim3((n + 255) / 256), dim3(256), 0, st, n, src, values, map_cov_first);
}
void launch_assign_nn(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, double *out_z, double *out_g, Launch L) {
    if (o.n <= 0 || o.n_frames <= 0) return;
    const int fpw = frames_per_wave(mean_frame(o.n, o.n_frames));
    const dim3 grid((o.n_frames + 4 * fpw - 1) / (4 * fpw)), block(256);
    if (m.cell_start) hipExtLaunchKernelGGL(k_assign_nn<true>, grid, block, 0, L.st, L.start, L.stop, 0, o.n, o.poses, o.n_poses, o.pose_of_obs, o.obs, o.n_frames,
                                            o.frame_start, fpw, lidar, m.n, m.xy, m.type, m.cov, o.pose_cov, p, grid_params_of(p.max_distance, m.buckets),
                                            m.cell_start, m.cell_items, out_idx, out_d2, out_z, out_g);
    else hipExtLaunchKernelGGL(k_assign_nn<false>, grid, block, 0, L.st, L.start, L.stop, 0, o.n, o.poses, o.n_poses, o.pose_of_obs, o.obs, o.n_frames,
                               o.frame_start, fpw, lidar, m.n, m.xy, m.type, m.cov, o.pose_cov, p, GridParams{}, m.cell_start, m.cell_items,
                               out_idx, out_d2, out_z, out_g);
}
// what the three two-kernel launchers put first in their argument block (fpw and only_large: launch_small_then_big's to set)
static FrameArgs frame_args(const ObsRef &o, const MapRef &m, double lidar, NnDev p) {
    return FrameArgs{o.n, o.poses, o.n_poses, o.pose_of_obs, o.obs, o.n_frames, o.frame_start, 1, 0, lidar, m.n, m.xy, m.cov, o.pose_cov, p};
}
void launch_assign_opt(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, int32_t *out_na, double *out_z, double *out_g,
                       Launch L) {
    if (o.n <= 0 || o.n_frames <= 0) return;
    const AoArgs A{frame_args(o, m, lidar, p), m.type, m.cell_start ? grid_params_of(p.max_distance, m.buckets) : GridParams{}, m.cell_start, m.cell_items,
                   out_idx, out_d2, out_na, out_z, out_g};
    if (m.cell_start) launch_small_then_big(A, -1, k_assign_opt<true>, k_assign_opt_big<true>, L.st, L.start, L.stop);
    else launch_small_then_big(A, -1, k_assign_opt<false>, k_assign_opt_big<false>, L.st, L.start, L.stop);
}
void launch_joint_compat(const ObsRef &o, const MapRef &m, double lidar, NnDev p, const JcGate &gate, const int32_t *in_idx, int32_t *out_idx, double *out_j,
                         int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable, double *out_delta, Launch L) {
    if (o.n_frames <= 0) return;
    const JcArgs A{frame_args(o, m, lidar, p), in_idx, out_idx, out_j, out_kept, out_dropped, out_untestable, out_delta, gate};
    launch_small_then_big(A, -1, k_joint_compat, k_joint_compat_big, L.st, L.start, L.stop);
}
// kernel 0 / 1 (gs_debug_localize) forces k_localize (with k_localize_big behind it for the frames above 64) / k_localize_big alone
void launch_localize(const ObsRef &o, const MapRef &m, double lidar, NnDev p, const LoParams &lp, const int32_t *in_idx, const LoOut &out, int kernel, Launch L) {
    if (o.n_frames <= 0) return;
    const LoArgs A{frame_args(o, m, lidar, p), in_idx, lp.max_iterations, lp.tol_xy, lp.tol_theta, out.pose, out.cov, out.chi2, out.n_pairs, out.iterations,
                   out.status, out.step};
    launch_small_then_big(A, kernel, k_localize, k_localize_big, L.st, L.start, L.stop);
}

}  // namespace gs
