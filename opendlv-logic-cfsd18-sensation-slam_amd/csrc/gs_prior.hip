// gs_prior.hip — the device pass of the prior edges (gfx950, wave64).  See gs_prior.hpp for where the pass runs and gs_prior_host.hpp for
// the tables.  A translation unit of its own, like gs_lm.hip: the kernels of gs_kernels.hip are not touched and DevGraph is what it was.
//
// Semantics, restated from g2o's published text (g2o is not part of this project's checkers: nothing here is pinned against a g2o build):
//   pose prior (EdgeSE2Prior)       e = vec(z^-1 o x): e_t = R_z^T (t - t_z), e_theta = normalize(theta - z_theta);  J = diag(R_z^T, 1)
//   pose XY prior (EdgeSE2XYPrior)  e = t - z: the pose prior with z_theta = 0 and Omega in the upper-left 2 x 2, stored as such
//   landmark prior (EdgeXYPrior)    e = l - z;  J = I
// with the additive update of k_update.  The error is formed the way the odometry residual is (pp_error, gs_edge_dev.hpp): the stored
// inverse measurement composed with the estimate, every product rounded on its own.
//
// k_prior_pass: thread v < n_pv is listed pose v, thread n_pv + j listed landmark j; 256 threads per workgroup.  The thread walks its
// vertex's run of records in order, sums J^T Omega J (packed symmetric), -J^T Omega e and e^T Omega e, and ADDS block and right-hand
// side where the front assembly reads them (side_add_pose / side_add_lm, gs_side_dev.hpp).  One writer per address (a vertex is listed
// once), no atomics.  chi2: one partial per workgroup, lanes -> waves in a fixed order; the total of the partials, summed by one
// workgroup in a fixed order, is ADDED to *chi_target by one thread (k_side_total, or the pass itself when it is one workgroup).
#include "gs_prior.hpp"
#include "gs_side_dev.hpp"

namespace gs {

// one pose-prior record (plane stride S, record r) at the estimate x: adds to H (xx xy xt yy yt tt) and b, returns e^T Omega e
template <bool APPLY>
__device__ __forceinline__ double prior_pose_record(const double *__restrict__ rec, int64_t S, int r, const double x[3], double H[6], double b[3]) {
#pragma clang fp contract(off)
    double v[PRIOR_POSE_REC];
#pragma unroll
    for (int k = 0; k < PRIOR_POSE_REC; ++k) v[k] = rec[(int64_t)k * S + r];
    const double cz = v[3], sz = v[4];
    const double e0 = v[0] + (cz * x[0] - sz * x[1]), e1 = v[1] + (sz * x[0] + cz * x[1]);
    const double e2 = normalize_theta(v[2] + normalize_theta(x[2]));
    const double w00 = v[5], w01 = v[6], w02 = v[7], w11 = v[8], w12 = v[9], w22 = v[10];
    const double We0 = w00 * e0 + w01 * e1 + w02 * e2, We1 = w01 * e0 + w11 * e1 + w12 * e2, We2 = w02 * e0 + w12 * e1 + w22 * e2;
    if (APPLY) {
        // J = [[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]];  WJ = Omega J (rows 0, 1 are all that the packed J^T (Omega J) needs beside Omega's last column)
        const double wj00 = w00 * cz + w01 * sz, wj01 = w01 * cz - w00 * sz;
        const double wj10 = w01 * cz + w11 * sz, wj11 = w11 * cz - w01 * sz;
        H[0] += cz * wj00 + sz * wj10; H[1] += cz * wj01 + sz * wj11; H[2] += cz * w02 + sz * w12;
        H[3] += cz * wj11 - sz * wj01; H[4] += cz * w12 - sz * w02; H[5] += w22;
        b[0] -= cz * We0 + sz * We1; b[1] -= cz * We1 - sz * We0; b[2] -= We2;
    }
    return e0 * We0 + e1 * We1 + e2 * We2;
}
template <bool APPLY>
__device__ __forceinline__ double prior_lm_record(const double *__restrict__ rec, int64_t S, int r, const double x[2], double H[3], double b[2]) {
#pragma clang fp contract(off)
    double v[PRIOR_LM_REC];
#pragma unroll
    for (int k = 0; k < PRIOR_LM_REC; ++k) v[k] = rec[(int64_t)k * S + r];
    const double e0 = x[0] - v[0], e1 = x[1] - v[1];
    const double We0 = v[2] * e0 + v[3] * e1, We1 = v[3] * e0 + v[4] * e1;
    if (APPLY) { H[0] += v[2]; H[1] += v[3]; H[2] += v[4]; b[0] -= We0; b[1] -= We1; }
    return e0 * We0 + e1 * We1;
}

template <bool APPLY>
__global__ void __launch_bounds__(256) k_prior_pass(DevGraph d, PriorDev pd, double *__restrict__ chi_target) {
    __shared__ double red[4];
    const int v = blockIdx.x * 256 + threadIdx.x;
    double chi = 0.0;
    if (v < pd.n_pv) {
        const int p = pd.pv_id[v];
        if (p >= 0 && p < d.N + d.tN) {                                  // (the host builds the list from this plan's graph; the guard keeps every store in bounds)
            double x[3], H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
#pragma unroll
            for (int c = 0; c < 3; ++c) x[c] = d.pose_est[3 * (int64_t)p + c];
            for (int r = pd.pv_start[v]; r < pd.pv_start[v + 1]; ++r) chi += prior_pose_record<APPLY>(pd.pr, pd.n_pr, r, x, H, b);
            if (APPLY) side_add_pose(d, p, H, b); }
    } else if (v < pd.n_pv + pd.n_lv) {
        const int j = v - pd.n_pv, l = pd.lv_id[j];
        if (l >= 0 && l < d.M + d.tM) {
            double x[2] = {d.lm_est[2 * (int64_t)l], d.lm_est[2 * (int64_t)l + 1]}, H[3] = {0, 0, 0}, b[2] = {0, 0};
            for (int r = pd.lv_start[j]; r < pd.lv_start[j + 1]; ++r) chi += prior_lm_record<APPLY>(pd.lr, pd.n_lr, r, x, H, b);
            if (APPLY) side_add_lm(d, l, H, b); }
    }
    side_chi2_finish(chi, red, pd.part, chi_target);
}
// the workgroups' partials by ONE workgroup in a fixed order, as k_reduce_chi2 sums the linearisation's: thread t takes partials t, t + 256, ...
// in index order, then lanes -> waves; thread 0 writes.  (One thread walking all of them is a chain of dependent adds: 391 at cfg4 with a
// prior on every pose.)
__global__ void __launch_bounds__(256) k_side_total(const double *__restrict__ part, int n_part, double *__restrict__ chi_target) {
    __shared__ double red[4];
    double s = 0.0;
    for (int k = threadIdx.x; k < n_part; k += 256) s += part[k];
    const double tot = side_block_sum(s, red);
    if (threadIdx.x == 0) *chi_target += tot;
}
void launch_side_total(const double *part, int n_part, double *chi_target, hipStream_t st) {
    hipLaunchKernelGGL(k_side_total, dim3(1), dim3(256), 0, st, part, n_part, chi_target);
}

// gs_get_prior_chi2: e^T Omega e per record, fixed vertices too (the same expressions as the pass)
__global__ void __launch_bounds__(256) k_prior_chi2_each(DevGraph d, int kind, int n, const int32_t *__restrict__ vert, const double *__restrict__ rec, double *__restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int v = vert[k];
    double s = 0.0;
    if (kind == 0) { if (v >= 0 && v < d.N + d.tN) { double x[3] = {d.pose_est[3 * (int64_t)v], d.pose_est[3 * (int64_t)v + 1], d.pose_est[3 * (int64_t)v + 2]};
        s = prior_pose_record<false>(rec, n, k, x, nullptr, nullptr); } }
    else if (v >= 0 && v < d.M + d.tM) { double x[2] = {d.lm_est[2 * (int64_t)v], d.lm_est[2 * (int64_t)v + 1]};
        s = prior_lm_record<false>(rec, n, k, x, nullptr, nullptr); }
    out[k] = s;
}

int prior_grid(const PriorDev &pd) { return (pd.n_pv + pd.n_lv + 255) / 256; }
void launch_prior_pass(const DevGraph &d, const PriorDev &pd, bool apply, double *chi_target, hipStream_t st) {
    const int grid = prior_grid(pd);
    if (grid <= 0) return;
    if (apply) hipLaunchKernelGGL(k_prior_pass<true>, dim3(grid), dim3(256), 0, st, d, pd, chi_target);
    else hipLaunchKernelGGL(k_prior_pass<false>, dim3(grid), dim3(256), 0, st, d, pd, chi_target);
    if (grid > 1) launch_side_total(pd.part, grid, chi_target, st);
}
void launch_prior_chi2_each(const DevGraph &d, int kind, int n, const int32_t *vert, const double *rec, double *out, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_prior_chi2_each, dim3((n + 255) / 256), dim3(256), 0, st, d, kind, n, vert, rec, out);
}

}  // namespace gs
