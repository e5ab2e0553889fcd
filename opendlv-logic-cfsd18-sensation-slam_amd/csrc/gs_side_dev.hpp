// gs_side_dev.hpp — device functions the three side passes share (gs_prior.hip, gs_edge_mask.hip, gs_polar.hip; gfx950, wave64).
// Included by those three files only: gs_kernels.hip and gs_lm.hip keep their own copies of the expressions restated here, so the main
// path's code objects do not depend on this header.  Every workgroup of a side pass has 256 threads.
#pragma once
#include "gs_device.hpp"

namespace gs {

static constexpr int SIDE_LM_PART = 8;       // doubles per lm_part record (gs_kernels.hip)
static constexpr double kSidePi = 3.14159265358979323846;

__device__ __forceinline__ double side_normalize_theta(double th) {      // g2o normalize_theta, as in gs_kernels.hip
#pragma clang fp contract(off)
    if (th >= -kSidePi && th < kSidePi) return th;
    const double m = floor(th / (2.0 * kSidePi));
    th = th - m * 2.0 * kSidePi;
    if (th >= kSidePi) th -= 2.0 * kSidePi;
    if (th < -kSidePi) th += 2.0 * kSidePi;
    return th;
}
// rho(s) and w = rho'(s) of robust_rho (gs_kernels.hip): w exactly 1 where the kernel does not act
__device__ __forceinline__ double side_robust_rho(int kernel, double delta, double s, double &w) {
#pragma clang fp contract(off)
    w = 1.0;
    if (kernel == 1) { const double d2 = delta * delta;
        if (s > d2) { const double r = sqrt(s); w = delta / r; return 2.0 * r * delta - d2; }
        return s; }
    if (kernel == 2) { const double d2 = delta * delta, aux = 1.0 + s / d2; w = 1.0 / aux; return d2 * log(aux); }
    return s;
}
// d = x_p^-1 * l, the landmark in the pose frame, by the expressions of edge_pl (GS_G2O_ORDER: inverse, then compose, every product
// rounded on its own); c, s: the pose's cached cos / sin
__device__ __forceinline__ void side_lm_in_pose_frame(double px, double py, double c, double s, double lx, double ly, double &dx, double &dy) {
#pragma clang fp contract(off)
    const double ix = -(c * px + s * py), iy = s * px - c * py;
    dx = (c * lx + s * ly) + ix;
    dy = (c * ly - s * lx) + iy;
}

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
        if (q0 >= 0 && q0 < d.lm_grp_start[l + 1] && q0 < d.n_groups) { double *s = d.lm_part + (int64_t)q0 * SIDE_LM_PART;
            s[0] += H[0]; s[1] += H[1]; s[2] += H[2]; s[3] += b[0]; s[4] += b[1]; } }
    else { const int64_t St = d.M;
        d.Hll_diag[l] += H[0]; d.Hll_diag[St + l] += H[1]; d.Hll_diag[2 * St + l] += H[2]; d.b_lm[l] += b[0]; d.b_lm[St + l] += b[1]; }
}

}  // namespace gs
