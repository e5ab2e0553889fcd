// gs_lm.hpp — device state and launchers of gs_optimize_lm (Levenberg-Marquardt around the Gauss-Newton launches).
//
// A trial is   linearise (+ tail) -> DAMP -> factor -> back-solve -> update -> SCALE -> chi2 at x_try -> STEP
// where the upper-case steps are the kernels of gs_lm.hip and the others are the launches of gs_iterate, unchanged (DevGraph and
// gs_kernels.hip do not know about LM: everything below travels in LmDev, a kernel argument of the new kernels only).
// No host decision inside a trial: lambda, nu, the counters and the accept / reject verdict live in LmState on the device.  The
// record is double-buffered — trial number q (counted by the host as it enqueues) reads state[q & 1] and its step kernel writes
// state[(q + 1) & 1] — so that every workgroup of a launch sees the same record whatever the timing.  The record and LmDev begin with
// the parts every step-control method has (gs_trial.hpp); the host's trial loop is run_trials (gs_solve.cpp).
#pragma once
#include "gs_device.hpp"
#include "gs_trial.hpp"

namespace gs {

struct LmState {
    TrialState t;               // (gs_trial.hpp; failcode 1, a zero pivot, is a rejected trial here; 2 ..: the host's business)
    double lambda;              // of the next trial (need_lambda: not known yet, the first damp kernel computes tau * max |H_jj|)
    double nu;                  // rejection factor, 2 after every accepted step
    double lambda_initial, lambda_last;     // first lambda of the call; lambda of the last trial that ran
    double tau;
    int32_t need_lambda, pad;
};

struct LmDev {
    TrialDev t;                                                     // history, base copy, partials (max |H_jj|, then scale)
    LmState *state = nullptr;                                       // [2]
    double *hist_lambda = nullptr;                                  // [64] per ITERATION: lambda of its accepted (or last) trial
};

int  lm_grid(const DevGraph &d);                                    // workgroups of the vertex-parallel kernels (= n_part)
void launch_lm_maxdiag(const DevGraph &d, const LmDev &lm, hipStream_t st);             // first iteration, no lambda given: per-workgroup max |H_jj| over the free scalars
void launch_lm_damp(const DevGraph &d, const LmDev &lm, int par, int init, hipStream_t st);    // base copy of the estimates + lambda on every free diagonal scalar
void launch_lm_scale(const DevGraph &d, const LmDev &lm, int par, hipStream_t st);      // partials of sum_j D_j (lambda D_j + b_j); files chi_old and the failure code
void launch_lm_step(const DevGraph &d, const LmDev &lm, int par, hipStream_t st);       // rho, accept / reject (+ restore), lambda, nu, counters, history, flags

}  // namespace gs
