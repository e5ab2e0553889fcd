// gs_polar.hip — the device pass of the polar observation edges (gfx950, wave64).  See gs_polar.hpp for where the pass runs and
// gs_polar_host.hpp for the tables.  A translation unit of its own, like gs_prior.hip: the kernels of gs_kernels.hip are not touched and
// DevGraph is what it was.
//
// Semantics.  d = x_p^-1 * l, the landmark in the pose frame, by lm_in_pose_frame (gs_edge_dev.hpp: inverse, then compose, every
// product rounded on its own; the pose's cached cos / sin); r = sqrt(dx^2 + dy^2), beta = atan2(dy, dx).
//   range-bearing   e = (r - z_r, normalize_theta(beta - z_beta)), Omega 2 x 2 in (range, bearing)
//   bearing-only    the range-bearing edge with z_r = 0 and Omega = [[0, 0], [0, w]], stored as such
// g2o's EdgeSE2PointXYBearing takes z - beta: the sign changes neither H, b nor chi2.  (g2o is not part of this project's checkers:
// nothing here is pinned against a g2o build.)  Jacobians, analytic, for the additive update of k_update:
//   Jd = d(r, beta)/dd = [[dx/r, dy/r], [-dy/r^2, dx/r^2]],  B = Jd R^T,  A = Jd [-R^T | (dy, -dx)^T] = [-B | (0, -1)^T] exactly.
// s = e^T Omega e; w and rho from the OBSERVATION kind's robust kernel (rk_pl, rd_pl; w = 1, rho = s without one).  The edge gives
// w A^T Omega A, w A^T Omega B, w B^T Omega B, -w A^T Omega e, -w B^T Omega e and rho(s).  r^2 == 0 exactly: nothing, s = 0.
//
// k_polar_pose: thread v < n_pv is listed pose v; 256 threads per workgroup.  It walks the pose's run of records in order: the H_pl block
// is STORED at the record's location (Hpl planes, stride ell_len, or t_Hpl, stride tcapEpl: the carrier's block, which the linearisation
// wrote as zeros), A^T Omega A and -A^T Omega e are summed in registers and ADDED to Hpp_diag / b_pose (t_Hpp_diag / t_b_pose for a tail
// pose), rho(s) is summed for chi2.  k_polar_lm: thread j < n_lv is listed landmark j; it walks the landmark's run (the second index),
// recomputes B^T Omega B and -B^T Omega e by the same expressions and ADDS them where the front assembly reads the landmark
// (side_add_lm, gs_side_dev.hpp).
// Fixed vertices as in the main kernels: a fixed endpoint stays out of H (its diagonal share is not added, the H_pl block is zero), an
// edge between two fixed vertices stays out of chi2.  One writer per address (a vertex is listed once, an edge has one location), no
// floating-point atomics, every index checked against the plan's counts, plain vector stores.  chi2: one partial per workgroup, lanes ->
// waves in a fixed order; the total of the partials, summed by one workgroup in a fixed order, is ADDED to *chi_target by one thread
// (k_side_total, or the pose side itself when it is one workgroup).
#include "gs_polar.hpp"
#include "gs_side_dev.hpp"

namespace gs {

// everything one polar edge produces, packed as PlQuad of gs_kernels.hip: Hp = A^T W A (xx xy xt yy yt tt), bp = -A^T W e,
// W6 = A^T W B (3 x 2 row-major), Hl = B^T W B (00 01 11), bl = -B^T W e with W = w Omega; s = e^T Omega e, chi = rho(s), wr = w
struct PolarQuad { double Hp[6], bp[3], W6[6], Hl[3], bl[2], s, chi, wr; };

// false: r^2 == 0 exactly (the edge contributes nothing; q.s = q.chi = 0, q.wr = 1)
__device__ __forceinline__ bool polar_quad(double px, double py, double c, double s, double lx, double ly, double zr, double zb,
                                           double w00, double w01, double w11, int rk, double rd, PolarQuad &q) {
    double dx, dy;
    lm_in_pose_frame(px, py, c, s, lx, ly, dx, dy);
    const double r2 = dx * dx + dy * dy;
    q.s = 0.0; q.chi = 0.0; q.wr = 1.0;
    if (!(r2 > 0.0)) return false;
    const double r = sqrt(r2), beta = atan2(dy, dx);
    const double e0 = r - zr, e1 = normalize_theta(beta - zb);
    const double j00 = dx / r, j01 = dy / r, j10 = -dy / r2, j11 = dx / r2;
    // B = Jd R^T, R^T rows (c, s), (-s, c)
    const double B0[2] = {j00 * c - j01 * s, j00 * s + j01 * c}, B1[2] = {j10 * c - j11 * s, j10 * s + j11 * c};
    const double A0[3] = {-B0[0], -B0[1], 0.0}, A1[3] = {-B1[0], -B1[1], -1.0};
    double We0 = w00 * e0 + w01 * e1, We1 = w01 * e0 + w11 * e1;
    q.s = e0 * We0 + e1 * We1;
    q.chi = robust_rho(rk, rd, q.s, q.wr);
    w00 *= q.wr; w01 *= q.wr; w11 *= q.wr; We0 *= q.wr; We1 *= q.wr;
    double WA0[3], WA1[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { WA0[k] = w00 * A0[k] + w01 * A1[k]; WA1[k] = w01 * A0[k] + w11 * A1[k]; }
    q.Hp[0] = A0[0] * WA0[0] + A1[0] * WA1[0]; q.Hp[1] = A0[0] * WA0[1] + A1[0] * WA1[1]; q.Hp[2] = A0[0] * WA0[2] + A1[0] * WA1[2];
    q.Hp[3] = A0[1] * WA0[1] + A1[1] * WA1[1]; q.Hp[4] = A0[1] * WA0[2] + A1[1] * WA1[2]; q.Hp[5] = A0[2] * WA0[2] + A1[2] * WA1[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) q.bp[k] = -(A0[k] * We0 + A1[k] * We1);
    const double WB0[2] = {w00 * B0[0] + w01 * B1[0], w00 * B0[1] + w01 * B1[1]};
    const double WB1[2] = {w01 * B0[0] + w11 * B1[0], w01 * B0[1] + w11 * B1[1]};
#pragma unroll
    for (int k = 0; k < 3; ++k) { q.W6[2 * k] = A0[k] * WB0[0] + A1[k] * WB1[0]; q.W6[2 * k + 1] = A0[k] * WB0[1] + A1[k] * WB1[1]; }
    q.Hl[0] = B0[0] * WB0[0] + B1[0] * WB1[0]; q.Hl[1] = B0[0] * WB0[1] + B1[0] * WB1[1]; q.Hl[2] = B0[1] * WB0[1] + B1[1] * WB1[1];
    q.bl[0] = -(B0[0] * We0 + B1[0] * We1); q.bl[1] = -(B0[1] * We0 + B1[1] * We1);
    return true;
}
// record r of the planes (stride S) at pose p / landmark l; the caller has checked p, l and r
__device__ __forceinline__ bool polar_record(const DevGraph &d, const PolarDev &pd, int r, int p, int l, PolarQuad &q) {
    const int64_t S = pd.n_rec;
    const double2 cs = reinterpret_cast<const double2 *>(d.pose_cs)[p];
    return polar_quad(d.pose_est[3 * (int64_t)p], d.pose_est[3 * (int64_t)p + 1], cs.x, cs.y, d.lm_est[2 * (int64_t)l], d.lm_est[2 * (int64_t)l + 1],
                      pd.planes[r], pd.planes[S + r], pd.planes[2 * S + r], pd.planes[3 * S + r], pd.planes[4 * S + r], d.rk_pl, d.rd_pl, q);
}

template <bool APPLY>
__global__ void __launch_bounds__(256) k_polar_pose(DevGraph d, PolarDev pd, double *__restrict__ chi_target) {
    __shared__ double red[4];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const int NP = d.N + d.tN, NL = d.M + d.tM;
    double chi = 0.0;
    if (v < pd.n_pv) {
        const int p = pd.pv_id[v];
        if (p >= 0 && p < NP) {                                          // (the host builds the lists from this plan's graph; the guards keep every access in bounds)
            const bool fp = d.pose_fixed[p] != 0;
            double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0};
            int r0 = pd.pv_start[v], r1 = pd.pv_start[v + 1];
            if (r0 < 0) r0 = 0;
            if (r1 > pd.n_rec) r1 = pd.n_rec;
            for (int r = r0; r < r1; ++r) {
                const int l = pd.rec_lm[r];
                if (l < 0 || l >= NL) continue;
                const bool fl = d.lm_fixed[l] != 0;
                PolarQuad q;
                if (!polar_record(d, pd, r, p, l, q)) continue;          // r^2 == 0: the carrier's zeros stay
                if (!(fp && fl)) chi += q.chi;
                if (APPLY) {
                    const bool both = !fp && !fl;
                    const int src = pd.rec_src[r]; int e;
                    if (side_pl_in_ell(d, src)) { const int64_t L = d.ell_len;
                        if (d.Hpl) {
#pragma unroll
                            for (int k = 0; k < 6; ++k) d.Hpl[k * L + src] = both ? q.W6[k] : 0.0; } }
                    else if (side_pl_in_tail(d, src, e) && d.t_Hpl) { const int64_t St = d.tcapEpl;
#pragma unroll
                        for (int k = 0; k < 6; ++k) d.t_Hpl[k * St + e] = both ? q.W6[k] : 0.0; }
#pragma unroll
                    for (int k = 0; k < 6; ++k) H[k] += q.Hp[k];
#pragma unroll
                    for (int k = 0; k < 3; ++k) b[k] += q.bp[k];
                }
            }
            if (APPLY && !fp) side_add_pose(d, p, H, b);
        }
    }
    side_chi2_finish(chi, red, pd.part, chi_target);
}

__global__ void __launch_bounds__(256) k_polar_lm(DevGraph d, PolarDev pd) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= pd.n_lv) return;
    const int NP = d.N + d.tN, NL = d.M + d.tM;
    const int l = pd.lv_id[j];
    if (l < 0 || l >= NL || d.lm_fixed[l]) return;
    double H[3] = {0, 0, 0}, b[2] = {0, 0};
    int t0 = pd.lv_start[j], t1 = pd.lv_start[j + 1];
    if (t0 < 0) t0 = 0;
    if (t1 > pd.n_rec) t1 = pd.n_rec;
    for (int t = t0; t < t1; ++t) {
        const int r = pd.lm_order[t];
        if (r < 0 || r >= pd.n_rec) continue;
        const int p = pd.rec_pose[r];
        if (p < 0 || p >= NP) continue;
        PolarQuad q;
        if (!polar_record(d, pd, r, p, l, q)) continue;
        H[0] += q.Hl[0]; H[1] += q.Hl[1]; H[2] += q.Hl[2]; b[0] += q.bl[0]; b[1] += q.bl[1];
    }
    side_add_lm(d, l, H, b);
}

// gs_get_edge_chi2: s and weight of the polar edges over what the per-edge kernel wrote for their carriers (fixed vertices do not matter here)
__global__ void __launch_bounds__(256) k_polar_edge_chi2(DevGraph d, int n_pol, const int32_t *__restrict__ tab, const double *__restrict__ vals,
                                                         const uint8_t *__restrict__ act, int n, double *__restrict__ out) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n_pol) return;
    const int o = tab[3 * (int64_t)k], p = tab[3 * (int64_t)k + 1], l = tab[3 * (int64_t)k + 2];
    if (o < 0 || o >= n || p < 0 || p >= d.N + d.tN || l < 0 || l >= d.M + d.tM) return;
    const double *v = vals + (int64_t)POLAR_REC * k;
    const double2 cs = reinterpret_cast<const double2 *>(d.pose_cs)[p];
    PolarQuad q;
    polar_quad(d.pose_est[3 * (int64_t)p], d.pose_est[3 * (int64_t)p + 1], cs.x, cs.y, d.lm_est[2 * (int64_t)l], d.lm_est[2 * (int64_t)l + 1],
               v[0], v[1], v[2], v[3], v[4], d.rk_pl, d.rd_pl, q);
    out[o] = q.s; out[(int64_t)n + o] = act[k] ? q.wr : 0.0;
}

int polar_grid(const PolarDev &pd) { return pd.n_rec > 0 ? (pd.n_pv + 255) / 256 : 0; }
void launch_polar_pass(const DevGraph &d, const PolarDev &pd, bool apply, double *chi_target, hipStream_t st) {
    const int grid = polar_grid(pd);
    if (grid <= 0) return;
    if (apply) hipLaunchKernelGGL(k_polar_pose<true>, dim3(grid), dim3(256), 0, st, d, pd, chi_target);
    else hipLaunchKernelGGL(k_polar_pose<false>, dim3(grid), dim3(256), 0, st, d, pd, chi_target);
    if (grid > 1) launch_side_total(pd.part, grid, chi_target, st);
    if (apply && pd.n_lv > 0) hipLaunchKernelGGL(k_polar_lm, dim3((pd.n_lv + 255) / 256), dim3(256), 0, st, d, pd);
}
void launch_polar_edge_chi2(const DevGraph &d, int n_pol, const int32_t *tab, const double *vals, const uint8_t *act, int n, double *out, hipStream_t st) {
    if (n_pol > 0) hipLaunchKernelGGL(k_polar_edge_chi2, dim3((n_pol + 255) / 256), dim3(256), 0, st, d, n_pol, tab, vals, act, n, out);
}

}  // namespace gs
