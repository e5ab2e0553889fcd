// gs_trial_dev.hpp — what the vertex-parallel kernels (gs_lm.hip, gs_dogleg.hip, gs_hmul.hip) share.  Device code only.
// The geometry: thread v < NP = N + tN is pose v (a grown plan's tail poses follow the base ones in every per-pose array), thread NP + l
// is landmark l < ML = M + tM; 256 threads per workgroup, lm_grid() workgroups.  Every sum is two-stage in a fixed order — lanes by
// shuffle, waves in wave order, then the workgroups' partials in index order — so no value depends on the solver's launch mode.
#pragma once
#include <hip/hip_runtime.h>

#include "gs_device.hpp"
#include "gs_trial.hpp"

namespace gs {

// fixed-order sum / max over the 256 threads, the result in EVERY thread (red: 5 doubles of LDS)
template <bool MAX> __device__ __forceinline__ double lm_block_reduce(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { const double o = __shfl_down(v, off, 64); v = MAX ? fmax(v, o) : v + o; }
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) red[4] = MAX ? fmax(fmax(red[0], red[1]), fmax(red[2], red[3])) : ((red[0] + red[1]) + red[2]) + red[3];
    __syncthreads();
    const double r = red[4];
    __syncthreads();
    return r;
}
__device__ __forceinline__ double lm_block_sum(double v, double *red) { return lm_block_reduce<false>(v, red); }
__device__ __forceinline__ double lm_block_max(double v, double *red) { return lm_block_reduce<true>(v, red); }
// the total of n per-workgroup partials in index order, the same bits in every thread of every workgroup
__device__ __forceinline__ double part_total(const double *part, int n, double *red) {
    double s = 0.0;
    for (int k = threadIdx.x; k < n; k += 256) s += part[k];
    return lm_block_sum(s, red);
}

// pose p's first plane of a packed per-pose array (diagonal block, right-hand side) and the stride of its planes: base or tail arena
template <class T> __device__ __forceinline__ T *pose_plane(const DevGraph &d, T *base, T *tail, int p, int64_t &S) {
    S = p < d.N ? d.N : d.tcapN;
    return p < d.N ? base + p : tail + (p - d.N);
}
// entries e[0..K) of base landmark l on the fused path: its run of lm_part slots summed q ascending from lm_grp_start[l], as
// k_linearize_finalize and the fronts do (the tail's shares, the priors and an LM lambda sit in the first slot)
template <int K> __device__ __forceinline__ void lm_slot_sum(const DevGraph &d, int l, const int (&e)[K], double (&s)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k) s[k] = 0.0;
    for (int q = d.lm_grp_start[l]; q < d.lm_grp_start[l + 1]; ++q) { const double *r = d.lm_part + (int64_t)q * LM_REC;
#pragma unroll
        for (int k = 0; k < K; ++k) s[k] += r[e[k]]; }
}
// two scalars of landmark l on any path: planes 0 and `plane` of the tail arena (l >= M) or of the gather path's array, entries e0 and
// e1 of the slots on the fused path
__device__ __forceinline__ void lm_pair(const DevGraph &d, int l, const double *tail, const double *gather, int plane, int e0, int e1, double &a, double &b) {
    if (l >= d.M) { const int o = l - d.M; a = tail[o]; b = tail[plane * (int64_t)d.tcapM + o]; }
    else if (d.n_wtiles > 0) { double s[2]; lm_slot_sum(d, l, {e0, e1}, s); a = s[0]; b = s[1]; }
    else { a = gather[l]; b = gather[plane * (int64_t)d.M + l]; }
}
// the diagonal scalars H00, H11 and the right-hand side of landmark l, as the fronts see them
__device__ __forceinline__ void lm_diag_pair(const DevGraph &d, int l, double &h00, double &h11) { lm_pair(d, l, d.t_Hll_diag, d.Hll_diag, 2, 0, 2, h00, h11); }
__device__ __forceinline__ void lm_rhs_pair(const DevGraph &d, int l, double &b0, double &b1) { lm_pair(d, l, d.t_b_lm, d.b_lm, 1, 3, 4, b0, b1); }

// thread v's share of the base copy of the estimates (a trial starts at the accepted point) or of putting it back, bit for bit
__device__ __forceinline__ void copy_vertex(const DevGraph &d, int v, double *pose, double *cs, double *lm, const double *pose0, const double *cs0, const double *lm0) {
    const int NP = d.N + d.tN, ML = d.M + d.tM;
    if (v < NP) {
#pragma unroll
        for (int c = 0; c < 3; ++c) pose[3 * (int64_t)v + c] = pose0[3 * (int64_t)v + c];
        cs[2 * (int64_t)v] = cs0[2 * (int64_t)v]; cs[2 * (int64_t)v + 1] = cs0[2 * (int64_t)v + 1];
    } else if (v < NP + ML) { const int l = v - NP;
        lm[2 * (int64_t)l] = lm0[2 * (int64_t)l]; lm[2 * (int64_t)l + 1] = lm0[2 * (int64_t)l + 1]; }
}
__device__ __forceinline__ void save_base(const DevGraph &d, const TrialDev &w, int v) { copy_vertex(d, v, w.base_pose, w.base_cs, w.base_lm, d.pose_est, d.pose_cs, d.lm_est); }
__device__ __forceinline__ void restore_base(const DevGraph &d, const TrialDev &w, int v) { copy_vertex(d, v, d.pose_est, d.pose_cs, d.lm_est, w.base_pose, w.base_cs, w.base_lm); }

// Behind the update, before the chi2 pass, by one thread (fields no workgroup of that launch reads): chi2[0] is still the total at the
// linearisation point (k_update / k_reduce_chi2 filed it); fail[0] is final for this trial (only the solver kernels raise it)
__device__ __forceinline__ void trial_file(const DevGraph &d, TrialState &S) { S.chi_old = d.chi2[0]; S.failcode = d.fail[0]; }
// The method-independent half of the verdict of an ACTIVE trial, by the one thread that writes the next record T (a copy of S on entry):
// the history slot, the counters, "terminate" after max_trials rejections in a row, done when the budget is used up.
//   done: fail[2] = this trial's iteration number makes k_update skip every later enqueued trial (the rule of gs_optimize_until).
__device__ __forceinline__ void trial_verdict(const DevGraph &d, const TrialDev &w, const TrialState &S, TrialState &T, bool accept, double chi_new) {
    const int it = S.iterations;
    if (S.trials == 0) T.chi_base = S.chi_old;
    if (it < 64) { w.hist_chi2[it] = S.chi_old; w.hist_trials[it] = S.trials_iter + 1; }
    T.trials = S.trials + 1;
    if (accept) {
        T.iterations = it + 1; T.trials_iter = 0; T.chi_base = chi_new;
        if (T.iterations >= S.budget) T.done = 1;
    } else {
        T.rejected = S.rejected + 1; T.trials_iter = S.trials_iter + 1;
        if (T.trials_iter >= S.max_trials) { T.terminated = 1; T.done = 1; }
    }
    if (T.done) d.fail[2] = d.iter;
}

}  // namespace gs
