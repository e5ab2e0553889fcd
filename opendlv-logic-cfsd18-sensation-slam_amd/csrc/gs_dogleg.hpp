// gs_dogleg.hpp — device state and launchers of gs_optimize_dogleg (Powell's dogleg around the Gauss-Newton launches), and the vectors
// gs_multiply_hessian stages its operand and result in.
//
// A trial is   linearise (+ tail + side passes) -> BEGIN -> H b -> DOT -> factor -> back-solve -> NORMS -> BLEND -> H h_dl -> update
//              -> GAIN -> chi2 at x_try -> STEP
// where the upper-case steps are the kernels of gs_dogleg.hip, the two products are launch_hmul (gs_hmul.hpp) and the others are the
// launches of gs_iterate, unchanged (DevGraph and gs_kernels.hip do not know about the dogleg: everything below travels in DlDev).
// No host decision inside a trial: the trust radius, the counters and the verdict live in DlState on the device, double-buffered as
// LmState is — trial q reads state[q & 1], its step kernel writes state[(q + 1) & 1]; both begin with TrialState (gs_trial.hpp).
//   BEGIN  base copy of the estimates; b in vertex order (zeros on fixed vertices)
//   DOT    partials of b.b and b.(H b)
//   NORMS  alpha = b.b / b.Hb (0 unless b.Hb is finite and > 0); with h_gn out of xe, h_sd = alpha b, a = h_gn - h_sd: partials of
//          |h_gn|^2, |h_sd|^2, h_sd.a, |a|^2
//   BLEND  the kind of step from the totals and delta; h_dl into xe (elimination order, what k_update applies) and in vertex order
//   GAIN   behind the update (chi2[0] is the total at the linearisation point by then), before the chi2 pass: partials of h_dl.(H h_dl),
//          b.h_dl, |h_dl|^2; files chi_old and the failure code
//   STEP   gain, rho, accept / reject (+ restore), delta, counters, history, flags
// Every sum is two-stage in a fixed order (gs_trial_dev.hpp: lm_block_sum, then the workgroups' partials in index order).
#pragma once
#include "gs_device.hpp"
#include "gs_trial.hpp"

namespace gs {

enum { DL_GN = 0, DL_SD = 1, DL_DL = 2 };                            // == GS_DOGLEG_* of include/graphslam.h
enum { DL_BB = 0, DL_BHB, DL_GG, DL_SS, DL_C, DL_Q, DL_HHH, DL_BH, DL_HH, DL_NPART };   // the partial arrays of DlDev::part

struct DlState {
    TrialState t;               // (gs_trial.hpp; any failcode: nothing moves, the host ends or repairs the call)
    double delta;               // trust radius of the next trial
    double delta_initial;
    int32_t kind;               // of the trial that ran last (filed by the blend kernel)
    int32_t n_kind[3];          // accepted steps by kind
};

struct DlDev {
    TrialDev t;                                                     // history, base copy, DL_NPART arrays of one partial per workgroup
    DlState *state = nullptr;                                       // [2]
    double *hist_delta = nullptr; int32_t *hist_kind = nullptr;     // [64] per ITERATION: delta and kind of its accepted (or last) trial
    double *b_pose = nullptr, *b_lm = nullptr, *Hb_pose = nullptr, *Hb_lm = nullptr;    // vertex order: b, H b  (gs_multiply_hessian: v, H v)
    double *h_pose = nullptr, *h_lm = nullptr, *Hh_pose = nullptr, *Hh_lm = nullptr;    // h_dl, H h_dl
    int32_t part_stride = 0;                                        // doubles between two partial arrays of t.part
};

void launch_dl_begin(const DevGraph &d, const DlDev &dl, hipStream_t st);
void launch_dl_dot(const DevGraph &d, const DlDev &dl, hipStream_t st);
void launch_dl_norms(const DevGraph &d, const DlDev &dl, hipStream_t st);
void launch_dl_blend(const DevGraph &d, const DlDev &dl, int par, hipStream_t st);
void launch_dl_gain(const DevGraph &d, const DlDev &dl, int par, hipStream_t st);
void launch_dl_step(const DevGraph &d, const DlDev &dl, int par, hipStream_t st);

}  // namespace gs
