// gs_lm.hip — the kernels gs_optimize_lm adds around the Gauss-Newton launches (gfx950, wave64).  See gs_lm.hpp for the trial
// sequence and the double-buffered state record.  A translation unit of its own: the kernels of gs_kernels.hip are not touched,
// not re-instantiated, and DevGraph is what it was.
//
// All four kernels are vertex-parallel with the geometry of gs_trial_dev.hpp, which also holds what they share with gs_dogleg.hip and
// gs_hmul.hip: the fixed-order reductions, a vertex's diagonal and right-hand side on any path, the base copy of the estimates and the
// method-independent half of the verdict.  One writer per address, no atomics.
//
// Where lambda goes (wherever the front assembly reads the diagonal scalar from):
//   free pose p < N          Hpp_diag planes xx, yy, tt (0, 3, 5)
//   free tail pose           t_Hpp_diag, the same planes with stride tcapN
//   free landmark l < M      gather path: Hll_diag planes 00, 11 (0, 2); fused path: entries 0 and 2 of the landmark's FIRST lm_part
//                            slot (the fronts sum the landmark's run of slots; k_linearize_tail adds there too)
//   free tail landmark       t_Hll_diag planes 0, 2 with stride tcapM
#include "gs_lm.hpp"
#include "gs_trial_dev.hpp"

#include <algorithm>
#include <cmath>

namespace gs {

__global__ void __launch_bounds__(256) k_lm_maxdiag(DevGraph d, LmDev lm) {
    __shared__ double red[5];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    double m = 0.0;
    if (v < NP) { const int p = v;
        if (d.pose_gidx[p] >= 0) {
            int64_t S; const double *H = pose_plane<const double>(d, d.Hpp_diag, d.t_Hpp_diag, p, S);
            m = fmax(fabs(H[0]), fmax(fabs(H[3 * S]), fabs(H[5 * S]))); }
    } else if (v < NP + ML) { const int l = v - NP;
        if (d.lm_gidx[l] >= 0) { double a, b; lm_diag_pair(d, l, a, b); m = fmax(fabs(a), fabs(b)); } }
    m = lm_block_max(m, red);
    if (threadIdx.x == 0) lm.t.part[blockIdx.x] = m;
}

// base copy of the estimates (the trial starts at the accepted point) + lambda on the free diagonal scalars.
// init: the first trial of a call without a lambda — every workgroup reduces the max-diagonal partials itself (a max does not depend
// on the order), workgroup 0 files the value.  A trial enqueued behind the end of the call (done) re-applies the last trial's lambda:
// its linearisation ran at the same estimates, so the system in HBM stays the last trial's as it was factorised.
__global__ void __launch_bounds__(256) k_lm_damp(DevGraph d, LmDev lm, int par, int init) {
    __shared__ double red[5];
    LmState &S = lm.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    const bool first = init != 0 && S.need_lambda != 0, done = S.t.done != 0;
    double lam;
    if (first) { double m = 0.0;
        for (int k = threadIdx.x; k < lm.t.n_part; k += 256) m = fmax(m, lm.t.part[k]);
        lam = S.tau * lm_block_max(m, red);
    } else lam = done ? S.lambda_last : S.lambda;
    save_base(d, lm.t, v);
    if (v < NP) { const int p = v;
        if (d.pose_gidx[p] >= 0) {
            int64_t St; double *H = pose_plane(d, d.Hpp_diag, d.t_Hpp_diag, p, St);
            H[0] += lam; H[3 * St] += lam; H[5 * St] += lam; }
    } else if (v < NP + ML) { const int l = v - NP;
        if (d.lm_gidx[l] >= 0) {
            if (l >= d.M) { const int o = l - d.M; d.t_Hll_diag[o] += lam; d.t_Hll_diag[2 * (int64_t)d.tcapM + o] += lam; }
            // (fused path: a free base landmark always has a slot — the plan gives every landmark with an observation edge in the layout one
            // per wave tile that sees it, and a growth step that would touch a landmark without one is refused, gs_plan.cpp grow_plan
            // "landmark without a partial-sum slot".  A free landmark with no observation edge at all has no slot and no place the fronts
            // would read a lambda from: its diagonal is assembled as 0, H + lambda I stays singular there, and the zero pivot makes every
            // trial a rejected one — the call terminates instead of moving a vertex no measurement holds.  The guard keeps the store in bounds.)
            else if (d.n_wtiles > 0) { const int q = d.lm_grp_start[l];
                if (q < d.lm_grp_start[l + 1]) { d.lm_part[(int64_t)q * LM_REC] += lam; d.lm_part[(int64_t)q * LM_REC + 2] += lam; } }
            else { d.Hll_diag[l] += lam; d.Hll_diag[2 * (int64_t)d.M + l] += lam; } } }
    if (blockIdx.x == 0 && threadIdx.x == 0 && !done) {             // (fields no other workgroup of this launch reads)
        S.lambda_last = lam;
        if (first) { S.lambda = lam; S.lambda_initial = lam; } }
}

// scale = sum_j D_j (lambda D_j + b_j) over the free scalars, g2o's computeScale: one partial per workgroup.  Runs BEHIND the update
// (dpose / dlm are the increment) and before the chi2 pass (which reads the new estimates and writes nothing of H or b).
__global__ void __launch_bounds__(256) k_lm_scale(DevGraph d, LmDev lm, int par) {
    __shared__ double red[5];
    LmState &S = lm.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    const double lam = S.lambda_last;
    double s = 0.0;
    if (v < NP) { const int p = v;
        if (d.pose_gidx[p] >= 0) {
            int64_t St; const double *b = pose_plane<const double>(d, d.b_pose, d.t_b_pose, p, St);
#pragma unroll
            for (int c = 0; c < 3; ++c) { const double dx = d.dpose[3 * (int64_t)p + c]; s += dx * (lam * dx + b[c * St]); } }
    } else if (v < NP + ML) { const int l = v - NP;
        if (d.lm_gidx[l] >= 0) {
            double b0, b1; lm_rhs_pair(d, l, b0, b1);
            const double d0 = d.dlm[2 * (int64_t)l], d1 = d.dlm[2 * (int64_t)l + 1];
            s += d0 * (lam * d0 + b0); s += d1 * (lam * d1 + b1); } }
    s = lm_block_sum(s, red);
    if (threadIdx.x == 0) lm.t.part[blockIdx.x] = s;
    if (blockIdx.x == 0 && threadIdx.x == 0) trial_file(d, S.t);
}

// The verdict.  Every workgroup forms it from the same read-only inputs — state[par], the scale partials in index order, chi2[0] of
// the chi2 pass — and restores its share of the estimates on a rejection; workgroup 0 writes the next record, the history and the flags
// (trial_verdict), and what is LM's own here: lambda, nu, and
//   fail[0] == 1 (zero pivot in this trial's factorisation; k_update applied nothing): a rejected trial, the code is cleared.
//   fail[0] >= 2 (a whole-tree launch gave up on a flag, ...): nothing moves, the host repairs it and runs the trial again.
__global__ void __launch_bounds__(256) k_lm_step(DevGraph d, LmDev lm, int par) {
    __shared__ double red[5];
    const LmState S = lm.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const double scale = part_total(lm.t.part, lm.t.n_part, red) + 1e-3;
    const double chi_new = d.chi2[0];
    const bool active = S.t.done == 0 && (S.t.failcode == 0 || S.t.failcode == 1);
    const double rho = (S.t.chi_old - chi_new) / scale;
    const bool accept = active && S.t.failcode == 0 && rho > 0.0 && isfinite(chi_new);
    if (active && !accept) restore_base(d, lm.t, v);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    LmState T = S;
    T.t.failcode = 0;
    if (active) {
        if (S.t.iterations < 64) lm.hist_lambda[S.t.iterations] = S.lambda_last;
        T.need_lambda = 0;
        if (accept) {
            const double t = 2.0 * rho - 1.0;
            double alpha = 1.0 - t * t * t;
            alpha = fmin(alpha, 2.0 / 3.0);
            T.lambda = S.lambda_last * fmax(1.0 / 3.0, alpha); T.nu = 2.0;
        } else {
            T.lambda = S.lambda_last * S.nu; T.nu = 2.0 * S.nu;
            if (S.t.failcode == 1) d.fail[0] = 0;
        }
        trial_verdict(d, lm.t, S.t, T.t, accept, chi_new);
    } else if (S.t.done != 0 && S.t.failcode == 1) d.fail[0] = 0;  // a no-op trial behind the end of the call factorised the last trial's system again: its zero pivot is that trial's, already counted
    lm.state[par ^ 1] = T;
}

int lm_grid(const DevGraph &d) { return std::max(1, (d.N + d.tN + d.M + d.tM + 255) / 256); }
void launch_lm_maxdiag(const DevGraph &d, const LmDev &lm, hipStream_t st) { hipLaunchKernelGGL(k_lm_maxdiag, dim3(lm_grid(d)), dim3(256), 0, st, d, lm); }
void launch_lm_damp(const DevGraph &d, const LmDev &lm, int par, int init, hipStream_t st) { hipLaunchKernelGGL(k_lm_damp, dim3(lm_grid(d)), dim3(256), 0, st, d, lm, par, init); }
void launch_lm_scale(const DevGraph &d, const LmDev &lm, int par, hipStream_t st) { hipLaunchKernelGGL(k_lm_scale, dim3(lm_grid(d)), dim3(256), 0, st, d, lm, par); }
void launch_lm_step(const DevGraph &d, const LmDev &lm, int par, hipStream_t st) { hipLaunchKernelGGL(k_lm_step, dim3(lm_grid(d)), dim3(256), 0, st, d, lm, par); }

}  // namespace gs
