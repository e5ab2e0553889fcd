// gs_frontend_dev.hpp — device helpers of the front end that more than one unit needs: the A0 conversion (polar -> CoG-frame XY -> global
// XY) and the hashed uniform grid's cell arithmetic.  gs_kernels.hip (A0, the Euclidean A1) and gs_assoc_nn.hip (the covariance-gated A1)
// include it; the text below is what gs_kernels.hip held, unchanged.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gs {

// constants exactly as the reference declares them (src/slam.hpp:134-136; PI is a FLOAT literal)
__device__ static constexpr double kDeg2Rad = 0.017453292522222;
__device__ static constexpr double kRad2Deg = 57.295779513082325;
__device__ static constexpr double kPiF = (double)3.14159265f;

// ------------------------------------------------------------------ A0
__device__ __forceinline__ void polar_to_xy(double az, double zen, double dist, double lidar, double &x, double &y) {
    // transformConeToCoG: sign is NaN at az == 0 (kept)
    double sign = az / fabs(az);
    double ang = kPiF - fabs(az * kDeg2Rad);
    double sa, ca; sincos(ang, &sa, &ca);                           // (one range reduction for the pair: the batched association is bound by these calls)
    double dnew = sqrt(lidar * lidar + dist * dist - 2.0 * lidar * dist * ca);
    double anew = asin((sa * dist) / dnew) * kRad2Deg;
    double az2 = anew * sign;
    // Spherical2Cartesian
    double cz = cos(zen * kDeg2Rad);
    double s2, c2; sincos(az2 * kDeg2Rad, &s2, &c2);
    x = dnew * cz * c2;
    y = dnew * cz * s2;
}

__device__ __forceinline__ void cone_to_global_cs(double px, double py, double c, double s, const double *obs, double lidar, double &gx, double &gy) {
    double x, y; polar_to_xy(obs[0], obs[1], obs[2], lidar, x, y);
    gx = (x * c - y * s) + px;
    gy = (x * s + y * c) + py;
}

// ------------------------------------------------------------------ the hashed uniform grid of A1 (built by launch_grid_build, gs_kernels.hip)
struct GridParams { double inv_cell; uint32_t mask; int pad; };
__device__ __forceinline__ long long grid_coord(double v, double inv_cell) { return (long long)fmin(fmax(floor(v * inv_cell), -4.0e15), 4.0e15); }   // (finite input; clamped: no overflow of the cast)
__device__ __forceinline__ uint32_t grid_bucket(long long cx, long long cy, uint32_t mask) {
    return (((uint32_t)cx * 73856093u) ^ ((uint32_t)cy * 19349663u)) & mask;
}
static inline GridParams grid_params_of(double thr, long long buckets) { GridParams g; g.inv_cell = 1.0 / (thr * (1.0 + 1e-9)); g.mask = (uint32_t)(buckets - 1); g.pad = 0; return g; }

}  // namespace gs
