// gs_edge_dev.hpp — how an edge is evaluated on the device, once (gfx950): the angle normalisation, the robust weight, the residuals of
// EdgeSE2PointXY and EdgeSE2 with their squared errors.  Device code only, everything inlined.  Every pass that evaluates an edge includes
// this text (gs_kernels.hip, the side passes through gs_side_dev.hpp, gs_assoc_nn.hip, gs_follow.hip): their values agree bit for bit
// because they are the same expressions, in g2o's operation order and without fused multiply-adds where the comments below say so.
#pragma once
#include <hip/hip_runtime.h>

namespace gs {

// (kDeg2Rad, kRad2Deg, kPiF: gs_frontend_dev.hpp)
__device__ static constexpr double kPi = 3.14159265358979323846;

// g2o normalize_theta
__device__ __forceinline__ double normalize_theta(double th) {
#pragma clang fp contract(off)                                      // m * 2 pi is rounded before the subtraction, as on the CPU path
    if (th >= -kPi && th < kPi) return th;
    double m = floor(th / (2.0 * kPi));
    th = th - m * 2.0 * kPi;
    if (th >= kPi) th -= 2.0 * kPi;
    if (th < -kPi) th += 2.0 * kPi;
    return th;
}

// Robust kernels (g2o RobustKernelHuber / RobustKernelCauchy, restated): for the squared error s = e^T W e of an edge returns rho(s)
// and sets w = rho'(s).  kernel: GS_ROBUST_* of include/graphslam.h (0 none, 1 Huber, 2 Cauchy).  IEEE sqrt / log / division, every
// product rounded on its own, so that a weight is a function of s alone wherever it is computed.  w is EXACTLY 1.0 where the kernel
// does not act (none; Huber with s <= delta^2): scaling by it changes no bit.
__device__ __forceinline__ double robust_rho(int kernel, double delta, double s, double &w) {
#pragma clang fp contract(off)
    w = 1.0;
    if (kernel == 1) { const double d2 = delta * delta;
        if (s > d2) { const double r = sqrt(s); w = delta / r; return 2.0 * r * delta - d2; }
        return s; }
    if (kernel == 2) { const double d2 = delta * delta, aux = 1.0 + s / d2; w = 1.0 / aux; return d2 * log(aux); }
    return s;
}

// ---- EdgeSE2PointXY (c, s: the pose's cos / sin)
// e = (x_p^-1 * l) - z
__device__ __forceinline__ void pl_error(double px, double py, double c, double s, double lx, double ly, double zx, double zy, double &ex, double &ey) {
    // g2o EdgeSE2PointXY::computeError: (x_p^-1 * l) - z with SE2::inverse() = (R^T (-t), -theta) and SE2 * point =
    // R p + t, in g2o's operation order and without fused multiply-adds: at kilometre coordinates the two products
    // cancel to the metre-sized residual and HOW they are rounded is 1e-12 m of it — the CPU path's rounding is the bar
#pragma clang fp contract(off)
    const double ix = -(c * px + s * py), iy = s * px - c * py;
    ex = ((c * lx + s * ly) + ix) - zx;
    ey = ((c * ly - s * lx) + iy) - zy;
}
// d = x_p^-1 * l, the landmark in the pose frame: the residual against z = 0 (x - 0.0 is x, bit for bit)
__device__ __forceinline__ void lm_in_pose_frame(double px, double py, double c, double s, double lx, double ly, double &dx, double &dy) {
    pl_error(px, py, c, s, lx, ly, 0.0, 0.0, dx, dy);
}
// error and Jacobian rows A0 / A1 (2 x 3) of the pose; B = R(theta)^T
__device__ __forceinline__ void edge_pl(double px, double py, double c, double s, double lx, double ly, double zx, double zy,
                                        double &ex, double &ey, double A0[3], double A1[3]) {
    pl_error(px, py, c, s, lx, ly, zx, zy, ex, ey);
    A0[0] = -c; A0[1] = -s; A1[0] = s;  A1[1] = -c;
    {   // g2o EdgeSE2PointXY::linearizeOplus writes the lever-arm entries as  a1 y2 - a1 y1 - a3 x2 + a3 x1  and
        // -a3 y2 + a3 y1 - a1 x2 + a1 x1  (a1 = cos, a3 = sin; left to right, every product rounded): at kilometre coordinates that
        // is 1e-13 of relative rounding in H_pp and H_pl which "differences first" does not have — and cond(H) ~ 1e13 on a 25 km lap
        // turns exactly that 1e-13 into the per-cent of the first increment by which the GPU path stood apart from every CPU path
        // (measured: profiles/r03_parity_spread_cfg4*.json).  The reference's numbers are the bar: same order, no contraction.
#pragma clang fp contract(off)
        A0[2] = ((c * ly - c * py) - s * lx) + s * px;
        A1[2] = (((-s) * ly + s * py) - c * lx) + c * px;
    }
}
// W e (W: 00 01 11), and the squared error s = e^T W e from it
__device__ __forceinline__ void pl_info_error(double ex, double ey, double w00, double w01, double w11, double &We0, double &We1) {
    We0 = w00 * ex + w01 * ey; We1 = w01 * ex + w11 * ey;
}
__device__ __forceinline__ double pl_sq_error(double ex, double ey, double We0, double We1) { return ex * We0 + ey * We1; }
// s of the edge at the estimates
__device__ __forceinline__ double pl_sq_error(double px, double py, double c, double s, double lx, double ly, double zx, double zy,
                                              double w00, double w01, double w11) {
    double ex, ey, We0, We1;
    pl_error(px, py, c, s, lx, ly, zx, zy, ex, ey);
    pl_info_error(ex, ey, w00, w01, w11, We0, We1);
    return pl_sq_error(ex, ey, We0, We1);
}

// ---- EdgeSE2 (ci, si: cos / sin of x_i's heading; zinv5 = z^-1 as {x, y, theta, cos theta, sin theta})
// e = vec(z^-1 * (x_i^-1 * x_j))
__device__ __forceinline__ void pp_error(const double xi[3], const double xj[3], double ci, double si, const double zinv5[5],
                                         double &e0, double &e1, double &e2) {
    const double rth = normalize_theta(normalize_theta(-xi[2]) + xj[2]);
    const double cz = zinv5[3], sz = zinv5[4];
    {   // g2o EdgeSE2::computeError: z^-1 * (x_i^-1 * x_j) as inverse-then-compose (SE2::inverse = (R^T (-t), -theta), SE2 * SE2 =
        // (R_a t_b + t_a, theta_a + theta_b)), every product rounded on its own (no fused multiply-add): at the reference's
        // initial point these residuals are zero in exact arithmetic and what is computed IS the rounding — follow the CPU path's
#pragma clang fp contract(off)
        const double ix = -(ci * xi[0] + si * xi[1]), iy = si * xi[0] - ci * xi[1];
        const double qx = ix + (ci * xj[0] + si * xj[1]), qy = iy + (ci * xj[1] - si * xj[0]);
        e0 = zinv5[0] + (cz * qx - sz * qy); e1 = zinv5[1] + (sz * qx + cz * qy);
    }
    e2 = normalize_theta(zinv5[2] + rth);
}
// W e (w: 00 01 02 11 12 22), and the squared error s = e^T W e from it
__device__ __forceinline__ void pp_info_error(double e0, double e1, double e2, const double w[6], double &We0, double &We1, double &We2) {
    We0 = w[0] * e0 + w[1] * e1 + w[2] * e2; We1 = w[1] * e0 + w[3] * e1 + w[4] * e2; We2 = w[2] * e0 + w[4] * e1 + w[5] * e2;
}
__device__ __forceinline__ double pp_sq_error(double e0, double e1, double e2, double We0, double We1, double We2) { return e0 * We0 + e1 * We1 + e2 * We2; }
// s of the edge at the estimates
__device__ __forceinline__ double pp_sq_error(const double xi[3], const double xj[3], double ci, double si, const double zinv5[5], const double w[6]) {
    double e0, e1, e2, We0, We1, We2;
    pp_error(xi, xj, ci, si, zinv5, e0, e1, e2);
    pp_info_error(e0, e1, e2, w, We0, We1, We2);
    return pp_sq_error(e0, e1, e2, We0, We1, We2);
}

}  // namespace gs
