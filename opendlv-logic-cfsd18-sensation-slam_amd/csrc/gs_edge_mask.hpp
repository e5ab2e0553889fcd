// gs_edge_mask.hpp — device side of edge deactivation (gs_set_edge_active ... gs_deactivate_edges_above; host side: gs_edge_mask_host.hpp).
//
// An inactive edge is an edge whose information on the device is exactly +0.0: the linearisation, factor and LM kernels then add
// exact zeros to H, b and chi2 (s = 0: both robust kernels give weight 1 and rho 0) and are what they were — DevGraph and gs_kernels.hip
// do not know about flags.  The pattern only shrinks, so plan, fronts and schedule stay valid: no structure phase.  The information
// lives in three arrays: ell_w (observation edges of the linearisation layout), t_pl_w (a grown plan's tail), pp_info (odometry edges,
// tail included).  k_edge_mask_apply rewrites the entries of the edges whose flag changed, behind any upload of the edge values and
// before the first launch of the call (edge_mask_sync, gs_edge_mask_api.cpp).  A handle that never had an inactive edge launches nothing.
#pragma once
#include "gs_device.hpp"
#include "gs_edge_mask_host.hpp"

namespace gs {

// One thread per listed edge of the kind (0 odometry, 1 observation).  loc[t]: odometry: the edge's insertion index = its record in
// pp_info; observation: src >= 0 its ELL index, src < 0 tail slot -(src + 1) (the table of gs_get_edge_chi2).  orig [n][6 | 3]: the
// edges' own information (host graph), act[t]: the flag.  Writes act ? orig : +0.0.  An edge is listed once: one writer per address.
void launch_edge_mask_apply(const DevGraph &d, int kind, int n, const int32_t *loc, const double *orig, const uint8_t *act, hipStream_t st);

// One thread per edge of the kind, insertion order.  tab: the table of launch_edge_chi2 ([n][2] {i, j} / [n][3] {pose, landmark, src});
// info [n][6 | 3]: every edge's OWN information (not the device arrays, which hold zeros for inactive edges); act [n] (null: all active).
// s = e^T Omega e at the current estimates by the expressions of quad_pl / pp_incidence.  Outputs, each may be null:
//   out_sw [2][n]   s, then the weight rho'(s) of the kind's kernel — 0 for an inactive edge
//   cand [n]        1 where the edge is active and s > threshold, else 0
//   wg_count        candidates per workgroup ([edge_select_grid(n)]; summed by the host in index order)
int  edge_select_grid(int n);
void launch_edge_select(const DevGraph &d, int kind, int n, const int32_t *tab, const double *info, const uint8_t *act, double threshold,
                        double *out_sw, uint8_t *cand, int32_t *wg_count, hipStream_t st);

}  // namespace gs
