// gs_polar.hpp — device tables and launchers of the polar observation edges (range-bearing, bearing-only; g2o's EdgeSE2PointXYBearing
// is the bearing-only one).
//
// A polar edge joins the same two vertices as a Cartesian observation edge, and it is carried by one (z = 0, information +0.0): the
// plan, the fronts, the schedule and the linearisation kernels do not know about it and add exact zeros for it.  Its blocks are written
// in a pass of its own
//     linearise (+ tail) -> priors -> POLAR -> (LM damp) -> factor ...
// that STORES the edge's H_pl block at the carrier's location and ADDS the diagonal shares and right-hand sides where the front assembly
// reads them (the address cases of k_prior_pass).  DevGraph and gs_kernels.hip are what they were: the tables travel in PolarDev, a
// kernel argument of the kernels of gs_polar.hip only.  A handle without polar edges launches nothing.  Table formats: gs_polar_host.hpp.
#pragma once
#include "gs_device.hpp"
#include "gs_polar_host.hpp"

namespace gs {

struct PolarDev {
    int32_t n_rec = 0, n_pv = 0, n_lv = 0;                        // records (= plane stride); listed poses / landmarks
    const int32_t *pv_id = nullptr, *pv_start = nullptr;          // [n_pv], [n_pv + 1]
    const int32_t *lv_id = nullptr, *lv_start = nullptr;          // [n_lv], [n_lv + 1]
    const int32_t *rec_pose = nullptr, *rec_lm = nullptr, *rec_src = nullptr;   // [n_rec], pose-sorted
    const int32_t *lm_order = nullptr;                            // [n_rec] record indices sorted by landmark
    const double *planes = nullptr;                               // [POLAR_REC][n_rec]
    double *part = nullptr;                                       // one chi2 partial per workgroup of the pose side
};

int  polar_grid(const PolarDev &pd);                              // workgroups of the pose side (0: no polar edges)
// H_pl blocks, diagonal shares, b and chi2 of every polar edge; the total of rho(s) is then ADDED to *chi_target by one thread, from
// the workgroups' partials summed in a fixed order (no second launch when the pose side is a single workgroup).
// apply = false: the chi2 total alone, nothing stored (behind launch_chi2_only)
void launch_polar_pass(const DevGraph &d, const PolarDev &pd, bool apply, double *chi_target, hipStream_t st);
// gs_get_edge_chi2: a thread per polar edge; tab [n_pol][3] {observation index, pose, landmark}, vals [n_pol][POLAR_REC] with the edge's
// OWN Omega, act [n_pol] (0: inactive -> weight 0).  Overwrites out[obs] = s and out[n + obs] = weight of out [2][n]
void launch_polar_edge_chi2(const DevGraph &d, int n_pol, const int32_t *tab, const double *vals, const uint8_t *act, int n, double *out, hipStream_t st);

}  // namespace gs
