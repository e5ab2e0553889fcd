// gs_cand.hip — cone candidates (include/graphslam.h, "cone candidates"; gfx950, wave64): the two dispatches a step adds around the
// minimum-cost association of gs_assoc_nn.hip, and the one that sets a table up.
//   k_cand_init     a thread per four slots copies the loaded records into the table's map form and records, frees the rest, and finds
//                   next_id, t and n_live
//   k_cand_stage    a thread per observation copies the frame with the explained observations' azimuth replaced by NaN
//   k_cand_update   one workgroup of 256: a lane per observation classifies and fuses; a thread per four consecutive slots does visibility,
//                   retirement and confirmation; spawners are ranked by ballots and prefix counts across the four waves, free slots
//                   likewise, and rank r meets the r-th free slot through LDS; the counters are sums of ballots
// No atomics, no spin, no cross-workgroup wait.  Every floating-point expression is under contract(off): the header's order of operations.
#include "gs_cand.hpp"
#include "gs_cand_host.hpp"
#include "gs_assoc_dev.hpp"
#include <hip/hip_ext.h>

namespace gs {

namespace {

static_assert(sizeof(gs_cand) == CAND_REC_BYTES && sizeof(gs_cand_step) == CAND_STEP_BYTES, "gs_cand_host.hpp restates the record sizes");
static_assert(CAND_MAX == GS_CAND_MAX && CAND_MAX == 4 * 256 && CAND_FRAME_MAX == NN_FRAME_MAX, "four slots a thread, a lane per observation");

// the step's frame: true and k = its size when it is a frame of this call
__device__ __forceinline__ bool cd_frame(const CdArgs &A, int &a, int &k) {
    a = A.fs[0]; const int b = A.fs[1];
    const bool ok = a >= 0 && b >= a && b <= A.n && b - a <= A.cap && b - a <= CAND_FRAME_MAX;
    k = ok ? b - a : 0;
    return ok;
}
__device__ __forceinline__ void cd_free_slot(const CdTable &T, int slot) {
    const double nan = __builtin_nan("");
    T.xy[2 * slot] = nan; T.xy[2 * slot + 1] = nan; T.type[slot] = 0;
    gs_cand &r = T.rec[slot];
    r.xy[0] = nan; r.xy[1] = nan; r.type = 0; r.id = -1; r.state = 0; r.hits = 0; r.misses = 0; r.first_step = 0; r.last_step = 0; r.confirm_step = -1;
#pragma unroll
    for (int e = 0; e < 4; ++e) { T.cov[4 * slot + e] = 0.0; r.cov[e] = 0.0; }
}
// xy and cov of a slot, in the map form and in its record
__device__ __forceinline__ void cd_store_cone(const CdTable &T, int slot, double x, double y, double c00, double c01, double c11) {
    T.xy[2 * slot] = x; T.xy[2 * slot + 1] = y;
    double *cv = T.cov + 4 * slot; cv[0] = c00; cv[1] = c01; cv[2] = c01; cv[3] = c11;
    gs_cand &r = T.rec[slot];
    r.xy[0] = x; r.xy[1] = y; r.cov[0] = c00; r.cov[1] = c01; r.cov[2] = c01; r.cov[3] = c11;
}
// the sum of a per-wave count over the workgroup's four waves, and over the waves below w
__device__ __forceinline__ int cd_sum4(const int (&s)[4]) { return s[0] + s[1] + s[2] + s[3]; }
__device__ __forceinline__ int cd_below(const int (&s)[4], int w) { return (w > 0 ? s[0] : 0) + (w > 1 ? s[1] : 0) + (w > 2 ? s[2] : 0); }

__global__ void __launch_bounds__(256) k_cand_init(int n_in, const gs_cand *in, CdTable T) {
    __shared__ int s_id[256], s_last[256], s_live[256];
    const int tid = threadIdx.x;
    int mid = -1, mlast = -1, live = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int slot = 4 * tid + e;
        bool take = false; gs_cand r;
        if (slot < n_in) { r = in[slot]; take = r.state == 1 || r.state == 2; }
        if (!take) { cd_free_slot(T, slot); continue; }
        T.rec[slot] = r;
        T.xy[2 * slot] = r.xy[0]; T.xy[2 * slot + 1] = r.xy[1]; T.type[slot] = r.type;
#pragma unroll
        for (int c = 0; c < 4; ++c) T.cov[4 * slot + c] = r.cov[c];
        mid = max(mid, r.id); mlast = max(mlast, r.last_step); live += 1;
    }
    s_id[tid] = mid; s_last[tid] = mlast; s_live[tid] = live;
    __syncthreads();
    if (tid == 0) {
        for (int j = 1; j < 256; ++j) { mid = max(mid, s_id[j]); mlast = max(mlast, s_last[j]); live += s_live[j]; }
        T.meta[0] = live > 0 ? mid + 1 : 0; T.meta[1] = live > 0 ? mlast + 1 : 0; T.meta[2] = live; T.meta[3] = 0;
    }
}

__global__ void __launch_bounds__(256) k_cand_stage(CdArgs A) {
    int a, k; const bool ok = cd_frame(A, a, k);
    const int i = threadIdx.x;
    if (i == 0) { A.st_fs[0] = 0; A.st_fs[1] = k; }                            // empty for a step that is no frame
    if (!ok || i >= k) return;
    double4 o = reinterpret_cast<const double4 *>(A.obs)[a + i];
    if (A.in_idx && A.in_idx[a + i] >= 0) o.x = __builtin_nan("");            // explained: an invalid query, -1 from the association
    reinterpret_cast<double4 *>(A.st_obs)[i] = o;
    A.st_pose_of_obs[i] = 0;
}

__global__ void __launch_bounds__(256) k_cand_update(CdArgs A) {
#pragma clang fp contract(off)
    __shared__ int s_fused[CAND_MAX];                                          // slot -> fused in this step
    __shared__ int s_slot_of_rank[256];                                        // r -> the r-th slot that was free at the start
    __shared__ int s_unexpl[4], s_nfuse[4], s_ncont[4], s_nfar[4], s_nspawn[4];               // per wave, over observations
    __shared__ int s_free[4], s_missed[4], s_retired[4], s_confirmed[4], s_live[4];           // per wave, over slots
    int a, k; if (!cd_frame(A, a, k)) return;                                  // (uniform)
    const CdTable &T = A.tab;
    const int tid = threadIdx.x, w = tid >> 6, lane = tid & 63;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int e = 0; e < 4; ++e) s_fused[4 * tid + e] = 0;
    s_slot_of_rank[tid] = -1;
    const int next_id = T.meta[0], t = T.meta[1];
    __syncthreads();

    // ---- a lane per observation: what it is, and the fusion's values (written once every slot has been looked at)
    const int i = tid;
    bool in_u = false, fuse = false, contested = false, far = false, spawn = false;
    int c = -1, cid = -1;
    NnQuery q; q.valid = false; q.ty = 0; q.gx = q.gy = q.zx = q.zy = q.a00 = q.a01 = q.a11 = 0;
    double fx = 0.0, fy = 0.0, f00 = 0.0, f01 = 0.0, f11 = 0.0;
    if (i < k) {
        in_u = !A.in_idx || A.in_idx[a + i] < 0;
        if (in_u) q = nn_query_of(i, k, A.pose, 1, A.st_pose_of_obs, A.st_obs, A.pose_cov, A.lidar, A.p);
        if (in_u && q.valid) {
            const int ci = A.as_idx[i], na = A.as_na[i];
            if (ci >= 0 && ci < CAND_MAX) {
                fuse = true; c = ci; cid = T.rec[c].id; s_fused[c] = 1;
                const NnCone cn = nn_cone(T.xy, T.cov, c);
                const double s00 = cn.c00 + q.a00, s01 = cn.c01 + q.a01, s11 = cn.c11 + q.a11;
                const double det = (s00 * s11) - (s01 * s01);
                const double n0 = q.gx - cn.x, n1 = q.gy - cn.y;
                const double k00 = ((cn.c00 * s11) - (cn.c01 * s01)) / det, k01 = ((cn.c01 * s00) - (cn.c00 * s01)) / det;
                const double k10 = ((cn.c01 * s11) - (cn.c11 * s01)) / det, k11 = ((cn.c11 * s00) - (cn.c01 * s01)) / det;
                fx = cn.x + ((k00 * n0) + (k01 * n1)); fy = cn.y + ((k10 * n0) + (k11 * n1));
                f00 = (k00 * q.a00) + (k01 * q.a01); f01 = (k00 * q.a01) + (k01 * q.a11); f11 = (k10 * q.a01) + (k11 * q.a11);
            } else if (na > 0) contested = true;
            else if (A.st_obs[4 * i + 2] < A.spawn_range) spawn = true;
            else far = true;
        }
    }
    const unsigned long long m_spawn = __ballot(spawn);
    const int rank_in_wave = __popcll(m_spawn & below);
    {
        const int nu = __popcll(__ballot(in_u)), nf = __popcll(__ballot(fuse)), nc = __popcll(__ballot(contested)), nr = __popcll(__ballot(far));
        if (lane == 0) { s_unexpl[w] = nu; s_nfuse[w] = nf; s_ncont[w] = nc; s_nfar[w] = nr; s_nspawn[w] = __popcll(m_spawn); }
    }
    __syncthreads();

    // ---- a thread per four consecutive slots: counters of the fused, visibility of the others, retirement, confirmation
    double sn, cs; sincos(A.pose[2], &sn, &cs);
    const double tx = A.pose[0], ty = A.pose[1];
    int free_wave = 0, n_missed = 0, n_retired = 0, n_confirmed = 0, n_live = 0;
    bool was_free[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int slot = 4 * tid + e;
        gs_cand &r = T.rec[slot];
        int state = r.state;
        was_free[e] = state == 0;
        bool missed = false, retired = false, confirmed = false;
        if (state != 0) {
            int hits = r.hits;
            if (s_fused[slot]) { hits += 1; r.hits = hits; r.misses = 0; r.last_step = t; }
            else {
                const double ex = T.xy[2 * slot] - tx, ey = T.xy[2 * slot + 1] - ty;
                const double dx = (cs * ex) + (sn * ey), dy = (cs * ey) - (sn * ex);
                const double r2 = (dx * dx) + (dy * dy);
                if (r2 < A.view2 && dx >= A.view_cos * sqrt(r2)) {
                    missed = true;
                    const int misses = r.misses + 1;
                    if (state == 1 && misses >= A.max_misses) { retired = true; state = 0; cd_free_slot(T, slot); }
                    else r.misses = misses;
                }
            }
            if (state == 1 && hits >= A.confirm_hits) { confirmed = true; r.state = 2; r.confirm_step = t; }
        }
        free_wave += __popcll(__ballot(was_free[e]));
        n_missed += __popcll(__ballot(missed)); n_retired += __popcll(__ballot(retired)); n_confirmed += __popcll(__ballot(confirmed));
        n_live += __popcll(__ballot(!was_free[e]));
    }
    if (lane == 0) { s_free[w] = free_wave; s_missed[w] = n_missed; s_retired[w] = n_retired; s_confirmed[w] = n_confirmed; s_live[w] = n_live; }
    __syncthreads();
    // the slots that were free at the start, in ascending slot index: a thread's four are consecutive, so they rank by (wave, lane, e)
    {
        int mine = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) mine += was_free[e] ? 1 : 0;
        int lower = 0;                                                         // the free slots of the lanes below: a ballot per count 1 .. 4
#pragma unroll
        for (int v = 1; v <= 4; ++v) lower += v * __popcll(__ballot(mine == v) & below);
        int ord = cd_below(s_free, w) + lower;
#pragma unroll
        for (int e = 0; e < 4; ++e) if (was_free[e]) { if (ord < 256) s_slot_of_rank[ord] = 4 * tid + e; ord += 1; }
    }
    __syncthreads();

    // ---- the lanes again: the fused write their values, rank r takes the r-th free slot
    const int n_free = cd_sum4(s_free), n_spawn = cd_sum4(s_nspawn);
    const int taken = min(n_spawn, n_free);
    int out_id = -1, out_slot = -1;
    if (fuse) { cd_store_cone(T, c, fx, fy, f00, f01, f11); out_id = cid; out_slot = c; }
    if (spawn) {
        const int rank = cd_below(s_nspawn, w) + rank_in_wave;
        if (rank < n_free) {
            const int slot = s_slot_of_rank[rank];
            cd_store_cone(T, slot, q.gx, q.gy, q.a00, q.a01, q.a11);
            T.type[slot] = (int)q.ty;
            gs_cand &r = T.rec[slot];
            const bool now = A.confirm_hits <= 1;
            r.type = (int)q.ty; r.id = next_id + rank; r.state = now ? 2 : 1; r.hits = 1; r.misses = 0; r.first_step = t; r.last_step = t;
            r.confirm_step = now ? t : -1;
            out_id = next_id + rank; out_slot = slot;
        }
    }
    if (i < k) { if (A.out_id) A.out_id[a + i] = out_id; if (A.out_slot) A.out_slot[a + i] = out_slot; }
    if (tid == 0) {
        const int live = cd_sum4(s_live) - cd_sum4(s_retired) + taken;
        if (A.rec) { gs_cand_step &o = *A.rec;
            o.step = t; o.n_unexplained = cd_sum4(s_unexpl); o.n_fused = cd_sum4(s_nfuse); o.n_spawned = taken; o.n_contested = cd_sum4(s_ncont);
            o.n_far = cd_sum4(s_nfar); o.n_dropped = n_spawn - taken; o.n_missed = cd_sum4(s_missed); o.n_retired = cd_sum4(s_retired);
            o.n_confirmed = cd_sum4(s_confirmed) + (A.confirm_hits <= 1 ? taken : 0); o.n_live = live; o.reserved = 0; }
        T.meta[0] = next_id + taken; T.meta[1] = t + 1; T.meta[2] = live; T.meta[3] = 0;
    }
}

}  // namespace

void launch_cand_init(int n_in, const gs_cand *in, const CdTable &tab, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_cand_init, dim3(1), dim3(256), 0, st, start, stop, 0, n_in, in, tab);
}
void launch_cand_stage(const CdArgs &A, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_cand_stage, dim3(1), dim3(256), 0, st, start, stop, 0, A);
}
void launch_cand_update(const CdArgs &A, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_cand_update, dim3(1), dim3(256), 0, st, start, stop, 0, A);
}

}  // namespace gs
