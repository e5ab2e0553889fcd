// gs_assoc_nn.hip — covariance-gated association (gfx950 / CDNA4, wave64): for every observation the map cone with the smallest
// Mahalanobis distance d2 inside a chi-square gate, its d2, and the runner-up's d2 (include/graphslam.h, "covariance-gated association").
//
//   k_assoc_nn        a thread per observation, the map (xy, covariance, type) streamed through LDS in tiles of 1024
//   k_assoc_nn_grid   a thread per observation, the nine buckets of the hashed grid around it (cell edge from max_distance)
//   k_frame_nn        one frame in one launch: a workgroup per observation, its 256 threads stride over the map
//   k_map_cov_gather  map covariances out of the gathered marginals (gs_map_set_cov_from_marginals)
//
// The three association kernels return IDENTICAL bits: the query's side (z, g, Q + P) is nn_query, one candidate's side (S, det, d2 and
// the five tests) is nn_pair, both without contraction, the A0 conversion is ONE out-of-line function (polar_to_xy compiled once, not
// once per inlining context), heading cos / sin come from sincos everywhere, and the winner is a minimum over (d2, index) — which does
// not depend on the order the candidates arrive in; the frame kernel reduces it in a fixed order all the same.
#include "gs_assoc_nn.hpp"
#include "gs_frontend_dev.hpp"
#include <hip/hip_ext.h>

namespace gs {

static constexpr int NN_TILE = 1024;
static constexpr int NN_NONE = 0x7fffffff;

struct NnQuery { double zx, zy, gx, gy, a00, a01, a11, ty; bool valid; };      // a = Q + P, once per observation
struct NnBest { double d2; int j; double second; };

__device__ __noinline__ double2 nn_polar(double az, double zen, double dist, double lidar) {
    double x, y; polar_to_xy(az, zen, dist, lidar, x, y);
    return make_double2(x, y);
}

// pose = (t, theta), pc = the pose's 3x3 covariance (row-major, upper triangle read) or null
__device__ __forceinline__ NnQuery nn_query(const double *pose, const double *pc, double az, double zen, double dist, double ty, double lidar, const NnDev &p) {
#pragma clang fp contract(off)
    NnQuery q;
    const double2 z = nn_polar(az, zen, dist, lidar);
    double s, c; sincos(pose[2], &s, &c);
    const double wx = z.x * c - z.y * s, wy = z.x * s + z.y * c;               // w = R(theta) z
    q.zx = z.x; q.zy = z.y; q.gx = wx + pose[0]; q.gy = wy + pose[1]; q.ty = ty;
    const double r2 = z.x * z.x + z.y * z.y;
    const double k = (p.sigma_range * p.sigma_range) / r2, sb2 = p.sigma_bearing * p.sigma_bearing, sx2 = p.sigma_xy * p.sigma_xy;
    // Q = (sigma_r^2 / r^2) w w^T + sigma_b^2 wp wp^T + sigma_xy^2 I,  wp = (-wy, wx)
    q.a00 = ((k * wx) * wx + (sb2 * wy) * wy) + sx2;
    q.a01 = (k * wx) * wy - (sb2 * wx) * wy;
    q.a11 = ((k * wy) * wy + (sb2 * wx) * wx) + sx2;
    if (pc) {                                                                 // P = G Sigma_p G^T, G = [I | wp]
        const double ux = -wy, uy = wx;
        q.a00 += (pc[0] + (2.0 * pc[2]) * ux) + (pc[8] * ux) * ux;
        q.a01 += ((pc[1] + pc[2] * uy) + pc[5] * ux) + (pc[8] * ux) * uy;
        q.a11 += (pc[4] + (2.0 * pc[5]) * uy) + (pc[8] * uy) * uy;
    }
    q.valid = isfinite(q.gx) && isfinite(q.gy) && r2 > 0.0;
    return q;
}

// one candidate: true and d2 when it is admissible (all tests positive: any NaN skips it)
__device__ __forceinline__ bool nn_pair(const NnQuery &q, const NnDev &p, double lx, double ly, double c00, double c01, double c11, int32_t type, double &d2) {
#pragma clang fp contract(off)
    if (!(fabs((double)type - q.ty) < p.type_tol)) return false;
    const double n0 = lx - q.gx, n1 = ly - q.gy;
    if (!(sqrt(n0 * n0 + n1 * n1) < p.max_distance)) return false;
    const double s00 = c00 + q.a00, s01 = c01 + q.a01, s11 = c11 + q.a11;
    const double det = s00 * s11 - s01 * s01;
    d2 = (((s11 * n0) * n0 - ((2.0 * s01) * n0) * n1) + (s00 * n1) * n1) / det;
    return det > 0.0 && s00 > 0.0 && d2 < p.gate_chi2;
}
__device__ __forceinline__ void nn_take(NnBest &b, double d2, int j) {
    if (d2 < b.d2 || (d2 == b.d2 && j < b.j)) { b.second = b.d2; b.d2 = d2; b.j = j; }
    else if (d2 < b.second) b.second = d2;
}
// b <- the best and the runner-up of the union of b's and o's candidates
__device__ __forceinline__ void nn_merge(NnBest &b, double od2, int oj, double osecond) {
    if (od2 < b.d2 || (od2 == b.d2 && oj < b.j)) { b.second = fmin(b.d2, osecond); b.d2 = od2; b.j = oj; }
    else b.second = fmin(b.second, od2);
}
__device__ __forceinline__ void nn_store(int i, const NnBest &b, int32_t *out_idx, double *out_d2, double *out_second) {
    out_idx[i] = b.j == NN_NONE ? -1 : b.j;
    if (out_d2) out_d2[i] = b.d2;
    if (out_second) out_second[i] = b.second;
}

// the observation's query, or an invalid one: i beyond n, or a pose index outside [0, n_poses) (nothing is read through it)
__device__ __forceinline__ NnQuery nn_query_of(int i, int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs,
                                               const double *pose_cov, double lidar, const NnDev &p) {
    NnQuery q; q.valid = false; q.ty = 0; q.gx = q.gy = q.zx = q.zy = q.a00 = q.a01 = q.a11 = 0;
    if (i >= n) return q;
    const int pi = pose_of_obs[i];
    if (pi < 0 || pi >= n_poses) return q;
    const double4 o4 = reinterpret_cast<const double4 *>(obs)[i];              // (az, zen, dist, type) in one 32-byte load
    return nn_query(poses + 3 * (size_t)pi, pose_cov ? pose_cov + 9 * (size_t)pi : nullptr, o4.x, o4.y, o4.z, o4.w, lidar, p);
}

__global__ void __launch_bounds__(256) k_assoc_nn(int n, const double *__restrict__ poses, int n_poses, const int32_t *__restrict__ pose_of_obs,
        const double *__restrict__ obs, double lidar, int n_map, const double *__restrict__ map_xy, const int32_t *__restrict__ map_type,
        const double *__restrict__ map_cov, const double *__restrict__ pose_cov, NnDev p,
        int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    __shared__ double sx[NN_TILE], sy[NN_TILE], s00[NN_TILE], s01[NN_TILE], s11[NN_TILE];      // 44 KB with the types: three workgroups per CU
    __shared__ int32_t st[NN_TILE];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const NnQuery q = nn_query_of(i, n, poses, n_poses, pose_of_obs, obs, pose_cov, lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    for (int base = 0; base < n_map; base += NN_TILE) {
        const int cnt = min(NN_TILE, n_map - base);
        __syncthreads();
        for (int t = threadIdx.x; t < cnt; t += 256) {
            const double2 xy = reinterpret_cast<const double2 *>(map_xy)[base + t];
            sx[t] = xy.x; sy[t] = xy.y; st[t] = map_type[base + t];
            if (map_cov) { const double4 cv = reinterpret_cast<const double4 *>(map_cov)[base + t]; s00[t] = cv.x; s01[t] = cv.y; s11[t] = cv.w; }
            else { s00[t] = 0.0; s01[t] = 0.0; s11[t] = 0.0; }
        }
        __syncthreads();
        if (q.valid)
            for (int t = 0; t < cnt; ++t) { double d2;                         // every thread reads the same LDS word: a broadcast
                if (nn_pair(q, p, sx[t], sy[t], s00[t], s01[t], s11[t], st[t], d2)) nn_take(b, d2, base + t); }
    }
    if (i < n) nn_store(i, b, out_idx, out_d2, out_second);
}

__global__ void __launch_bounds__(256) k_assoc_nn_grid(int n, const double *__restrict__ poses, int n_poses, const int32_t *__restrict__ pose_of_obs,
        const double *__restrict__ obs, double lidar, const double *__restrict__ map_xy, const int32_t *__restrict__ map_type,
        const double *__restrict__ map_cov, const double *__restrict__ pose_cov, NnDev p, GridParams g,
        const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_items,
        int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const NnQuery q = nn_query_of(i, n, poses, n_poses, pose_of_obs, obs, pose_cov, lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    if (q.valid) {
        const long long cx = grid_coord(q.gx, g.inv_cell), cy = grid_coord(q.gy, g.inv_cell);
        uint32_t bk[9]; int s0[9], s1[9];                                      // the nine buckets' ranges first: independent loads
#pragma unroll
        for (int k = 0; k < 9; ++k) { bk[k] = grid_bucket(cx + (k % 3) - 1, cy + (k / 3) - 1, g.mask); s0[k] = cell_start[bk[k]]; s1[k] = cell_start[bk[k] + 1]; }
#pragma unroll
        for (int k = 1; k < 9; ++k)                                            // two of the nine cells in ONE bucket: its cones are candidates once
            for (int m = 0; m < k; ++m) if (bk[m] == bk[k]) s1[k] = s0[k];     // (a second visit would make a cone its own runner-up)
#pragma unroll
        for (int k = 0; k < 9; ++k)
            for (int t = s0[k]; t < s1[k]; ++t) { const int j = cell_items[t];
                const double2 xy = reinterpret_cast<const double2 *>(map_xy)[j];
                double c00 = 0.0, c01 = 0.0, c11 = 0.0;
                if (map_cov) { const double4 cv = reinterpret_cast<const double4 *>(map_cov)[j]; c00 = cv.x; c01 = cv.y; c11 = cv.w; }
                double d2;
                if (nn_pair(q, p, xy.x, xy.y, c00, c01, c11, map_type[j], d2)) nn_take(b, d2, j); }
    }
    nn_store(i, b, out_idx, out_d2, out_second);
}

__global__ void __launch_bounds__(256) k_frame_nn(int k, const double *__restrict__ in, int has_pose_cov, double lidar, int n_map,
        const double *__restrict__ map_xy, const int32_t *__restrict__ map_type, const double *__restrict__ map_cov, NnDev p,
        double *__restrict__ out_z, double *__restrict__ out_g, int32_t *__restrict__ out_idx, double *__restrict__ out_d2, double *__restrict__ out_second) {
    __shared__ double rd[4], rs[4]; __shared__ int rj[4];
    const int i = blockIdx.x, tid = threadIdx.x;
    const double *ob = in + 12 + 4 * (size_t)i;
    const NnQuery q = nn_query(in, has_pose_cov ? in + 3 : nullptr, ob[0], ob[1], ob[2], ob[3], lidar, p);
    NnBest b{__builtin_inf(), NN_NONE, __builtin_inf()};
    if (q.valid)
        for (int j = tid; j < n_map; j += 256) {
            const double2 xy = reinterpret_cast<const double2 *>(map_xy)[j];
            double c00 = 0.0, c01 = 0.0, c11 = 0.0;
            if (map_cov) { const double4 cv = reinterpret_cast<const double4 *>(map_cov)[j]; c00 = cv.x; c01 = cv.y; c11 = cv.w; }
            double d2;
            if (nn_pair(q, p, xy.x, xy.y, c00, c01, c11, map_type[j], d2)) nn_take(b, d2, j);
        }
    // fixed order: lanes by halving distance inside a wave, then waves 0 .. 3
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double od = __shfl_down(b.d2, off, 64), os = __shfl_down(b.second, off, 64); const int oj = __shfl_down(b.j, off, 64);
        nn_merge(b, od, oj, os);
    }
    if ((tid & 63) == 0) { rd[tid >> 6] = b.d2; rs[tid >> 6] = b.second; rj[tid >> 6] = b.j; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < 4; ++w) nn_merge(b, rd[w], rj[w], rs[w]);
        nn_store(i, b, out_idx, out_d2, out_second);
        out_z[2 * i] = q.zx; out_z[2 * i + 1] = q.zy; out_g[2 * i] = q.gx; out_g[2 * i + 1] = q.gy;
    }
}

__global__ void __launch_bounds__(256) k_map_cov_gather(int n, const int64_t *__restrict__ src, const double *__restrict__ values, double *__restrict__ dst) {
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= n) return;
    const int64_t s = src[k];
    double4 v = make_double4(0.0, 0.0, 0.0, 0.0);
    if (s >= 0) v = make_double4(values[s], values[s + 1], values[s + 2], values[s + 3]);
    dst[4 * (size_t)k] = v.x; dst[4 * (size_t)k + 1] = v.y; dst[4 * (size_t)k + 2] = v.z; dst[4 * (size_t)k + 3] = v.w;
}

void launch_assoc_nn(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, double lidar, int n_map,
                     const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                     int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    if (n <= 0) return;
    hipExtLaunchKernelGGL(k_assoc_nn, dim3((n + 255) / 256), dim3(256), 0, st, start, stop, 0, n, poses, n_poses, pose_of_obs, obs, lidar, n_map,
                          map_xy, map_type, map_cov, pose_cov, p, out_idx, out_d2, out_second);
}
void launch_assoc_nn_grid(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, double lidar,
                          const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                          long long buckets, const int32_t *cell_start, const int32_t *cell_items,
                          int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    if (n <= 0) return;
    hipExtLaunchKernelGGL(k_assoc_nn_grid, dim3((n + 255) / 256), dim3(256), 0, st, start, stop, 0, n, poses, n_poses, pose_of_obs, obs, lidar,
                          map_xy, map_type, map_cov, pose_cov, p, grid_params_of(p.max_distance, buckets), cell_start, cell_items, out_idx, out_d2, out_second);
}
void launch_frame_nn(int k, const double *in, int has_pose_cov, double lidar, int n_map, const double *map_xy, const int32_t *map_type,
                     const double *map_cov, NnDev p, double *out_z, double *out_g, int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st) {
    if (k > 0) hipLaunchKernelGGL(k_frame_nn, dim3(k), dim3(256), 0, st, k, in, has_pose_cov, lidar, n_map, map_xy, map_type, map_cov, p,
                                  out_z, out_g, out_idx, out_d2, out_second);
}
void launch_map_cov_gather(int n, const int64_t *src, const double *values, double *map_cov_first, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_map_cov_gather, dim3((n + 255) / 256), dim3(256), 0, st, n, src, values, map_cov_first);
}

}  // namespace gs
