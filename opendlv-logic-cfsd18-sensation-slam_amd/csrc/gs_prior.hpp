// gs_prior.hpp — device tables and launchers of the prior edges (unary edges: g2o's EdgeSE2Prior, EdgeSE2XYPrior, EdgeXYPrior).
//
// A prior adds no off-diagonal block: the plan, the fronts, the schedule and the linearisation kernels do not know about it.  It adds
// J^T Omega J to the diagonal block and -J^T Omega e to the right-hand side of ONE vertex, and e^T Omega e to chi2, in a pass of its own
//     linearise (+ tail) -> PRIORS -> (LM damp) -> factor ...
// that ADDS where the front assembly reads (the address cases of k_lm_damp, gs_lm.hip).  DevGraph and gs_kernels.hip are what they were:
// the tables travel in PriorDev, a kernel argument of the kernels of gs_prior.hip only.  A handle without priors launches nothing.
// Table formats: gs_prior_host.hpp.
#pragma once
#include "gs_device.hpp"
#include "gs_prior_host.hpp"

namespace gs {

struct PriorDev {
    int32_t n_pv = 0, n_lv = 0;                                   // listed vertices: free poses / free landmarks with at least one prior
    int32_t n_pr = 0, n_lr = 0;                                   // records = plane strides
    const int32_t *pv_id = nullptr, *pv_start = nullptr;          // [n_pv], [n_pv + 1]
    const int32_t *lv_id = nullptr, *lv_start = nullptr;          // [n_lv], [n_lv + 1]
    const double *pr = nullptr, *lr = nullptr;                    // [PRIOR_POSE_REC][n_pr], [PRIOR_LM_REC][n_lr]
    double *part = nullptr;                                       // one chi2 partial per workgroup of the pass
};

int  prior_grid(const PriorDev &pd);                              // workgroups of the pass (0: no priors)
// H, b and chi2 of every listed vertex's priors; the prior total is then ADDED to *chi_target by one thread, from the workgroups'
// partials summed in a fixed order (one launch when the pass is a single workgroup, else a second launch of one workgroup).
// apply = false: the chi2 total alone (behind launch_chi2_only)
void launch_prior_pass(const DevGraph &d, const PriorDev &pd, bool apply, double *chi_target, hipStream_t st);
// gs_get_prior_chi2: a thread per record of `rec` ([per][n] planes, any order), vertex index in vert[n]; out[n] = e^T Omega e
void launch_prior_chi2_each(const DevGraph &d, int kind, int n, const int32_t *vert, const double *rec, double *out, hipStream_t st);

}  // namespace gs
