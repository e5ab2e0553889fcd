// gs_side_dev.hpp — device functions the three side passes share (gs_prior.hip, gs_edge_mask.hip, gs_polar.hip; gfx950, wave64).
// Residuals, squared errors, robust weight and angle normalisation are those of the main path: gs_edge_dev.hpp.  Every workgroup of a
// side pass has 256 threads.
#pragma once
#include "gs_device.hpp"
#include "gs_edge_dev.hpp"

namespace gs {

// fixed-order sum over the 256 threads, the result in thread 0 (red: 4 doubles of LDS)
__device__ __forceinline__ double side_block_sum(double v, double *red) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// chi2 of a pass: the workgroup's sum is ADDED to *chi_target when the pass is this one workgroup (no second launch), else it is the
// workgroup's partial and launch_side_total follows.  (+=: the slot holds the total, or one of the partials, of the linearisation /
// chi2 launches and of the passes EARLIER ON THIS STREAM, or zero from enqueue_linearize when no wave tile is swept; a pass must stay
// behind them)
__device__ __forceinline__ void side_chi2_finish(double chi, double *red, double *__restrict__ part, double *__restrict__ chi_target) {
    const double tot = side_block_sum(chi, red);
    if (threadIdx.x == 0) {
        if (gridDim.x == 1) *chi_target += tot;
        else part[blockIdx.x] = tot; }
}
// k_side_total (gs_prior.hip): the n_part partials by ONE workgroup in a fixed order, ADDED to *chi_target by one thread
void launch_side_total(const double *part, int n_part, double *chi_target, hipStream_t st);

// Where an observation edge lives: src >= 0 its index in the ELL planes (stride ell_len), src < 0 tail slot -(src + 1) (the table of
// gs_get_edge_chi2).  Neither holds for a src outside the plan's counts — the caller then touches nothing
__device__ __forceinline__ bool side_pl_in_ell(const DevGraph &d, int src) { return src >= 0 && (int64_t)src < d.ell_len; }
__device__ __forceinline__ bool side_pl_in_tail(const DevGraph &d, int src, int &e) { e = -(src + 1); return src < 0 && e >= 0 && e < d.tEpl && e < d.tcapEpl; }

// ADD a block and a right-hand side where the front assembly reads them (the address cases of k_lm_damp / k_lm_scale, gs_lm.hip).
// The caller has checked 0 <= p < N + tN / 0 <= l < M + tM; the guards here keep every store in bounds whatever the tables say.
//   pose p < N              Hpp_diag planes 0 .. 5, b_pose planes 0 .. 2 (stride N)
//   tail pose               t_Hpp_diag, t_b_pose (stride tcapN), slot p - N
__device__ __forceinline__ void side_add_pose(const DevGraph &d, int p, const double H[6], const double b[3]) {
    if (!(p < d.N || (p - d.N) < d.tcapN)) return;
    double *Hd = p < d.N ? d.Hpp_diag + p : d.t_Hpp_diag + (p - d.N), *bd = p < d.N ? d.b_pose + p : d.t_b_pose + (p - d.N);
    const int64_t St = p < d.N ? d.N : d.tcapN;
#pragma unroll
    for (int c = 0; c < 6; ++c) Hd[c * St] += H[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) bd[c * St] += b[c];
}
//   landmark l < M          gather path: Hll_diag planes 0 .. 2, b_lm planes 0, 1 (stride M); fused path: entries 0 .. 4 of the landmark's
//                           FIRST lm_part slot (the fronts and k_linearize_finalize sum the landmark's run of slots).  A landmark
//                           without a slot has no observation edge in the layout: the host refuses it before anything is uploaded
//   tail landmark           t_Hll_diag, t_b_lm (stride tcapM), slot l - M
__device__ __forceinline__ void side_add_lm(const DevGraph &d, int l, const double H[3], const double b[2]) {
    if (l >= d.M) { const int o = l - d.M; const int64_t St = d.tcapM;
        if (o < d.tcapM && d.t_Hll_diag) {
            d.t_Hll_diag[o] += H[0]; d.t_Hll_diag[St + o] += H[1]; d.t_Hll_diag[2 * St + o] += H[2]; d.t_b_lm[o] += b[0]; d.t_b_lm[St + o] += b[1]; } }
    else if (d.n_wtiles > 0) { const int q0 = d.lm_grp_start[l];
        if (q0 >= 0 && q0 < d.lm_grp_start[l + 1] && q0 < d.n_groups) { double *s = d.lm_part + (int64_t)q0 * LM_REC;
            s[0] += H[0]; s[1] += H[1]; s[2] += H[2]; s[3] += b[0]; s[4] += b[1]; } }
    else { const int64_t St = d.M;
        d.Hll_diag[l] += H[0]; d.Hll_diag[St + l] += H[1]; d.Hll_diag[2 * St + l] += H[2]; d.b_lm[l] += b[0]; d.b_lm[St + l] += b[1]; }
}

}  // namespace gs
