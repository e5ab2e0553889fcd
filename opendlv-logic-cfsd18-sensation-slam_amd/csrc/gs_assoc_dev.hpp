// gs_assoc_dev.hpp — what the kernels of the covariance-gated family (gs_assoc_nn.hip, gs_reloc.hip) share, each piece ONCE, because each is
// something their bit-for-bit promise rests on: the out-of-line A0 conversion, the walk over the map (the nine buckets of the hashed grid or
// every cone), a query and one candidate's d2, the wave-scope sync, the scaffold of the kernels that give a frame W lanes of a wave (the
// argument block, the lane split, the frame defences, the two drivers, the launcher) and the ten pair terms of the joint test.
// Every function that holds a floating-point expression carries its own contract-off pragma: the pragma is scoped to the function.
#pragma once
#include "gs_assoc_nn.hpp"
#include "gs_frontend_dev.hpp"
#include <hip/hip_ext.h>

#include <algorithm>

namespace gs {

static constexpr int NN_NONE = 0x7fffffff;
static constexpr int NN_FRAME_MAX = 256;                                       // GS_NN_FRAME_MAX

// the A0 conversion out of line: polar_to_xy compiled once per unit, not once per inlining context (its roundings depend on the context)
__device__ __noinline__ double2 nn_polar(double az, double zen, double dist, double lidar) {
    double x, y; polar_to_xy(az, zen, dist, lidar, x, y);
    return make_double2(x, y);
}
__device__ __forceinline__ void wave_sync() {                                  // what a lane wrote to LDS before, every lane of the wave reads after
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// ---- the walk over the map
// f(j) for every cone of the nine buckets around (x, y), each cone once.  The nine ranges are loaded first (independent loads), a bucket that
// two of the nine cells share is emptied at its second meeting (a second visit would make a cone its own runner-up), then c = 0 .. 8, t ascending
template <class F>
__device__ __forceinline__ void grid_walk9(const GridParams &g, const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_items, double x, double y, F &&f) {
    const long long cx = grid_coord(x, g.inv_cell), cy = grid_coord(y, g.inv_cell);
    uint32_t bk[9]; int s0[9], s1[9];
#pragma unroll
    for (int c = 0; c < 9; ++c) { bk[c] = grid_bucket(cx + (c % 3) - 1, cy + (c / 3) - 1, g.mask); s0[c] = cell_start[bk[c]]; s1[c] = cell_start[bk[c] + 1]; }
#pragma unroll
    for (int c = 1; c < 9; ++c)
        for (int m = 0; m < c; ++m) if (bk[m] == bk[c]) s1[c] = s0[c];
#pragma unroll
    for (int c = 0; c < 9; ++c)
        for (int t = s0[c]; t < s1[c]; ++t) f(cell_items[t]);
}
// the grid walk, or j = 0 .. n_map - 1
template <bool GRID, class F>
__device__ __forceinline__ void map_walk(int n_map, const GridParams &g, const int32_t *__restrict__ cell_start, const int32_t *__restrict__ cell_items, double x, double y, F &&f) {
    if (GRID) grid_walk9(g, cell_start, cell_items, x, y, f);
    else for (int j = 0; j < n_map; ++j) f(j);
}

// ---- a query and a candidate
struct NnQuery { double zx, zy, gx, gy, a00, a01, a11, ty; bool valid; };      // a = Q + P, once per observation
struct NnMap { const double *xy; const int32_t *type; const double *cov; };    // cov may be null: zeros
struct NnCone { double x, y, c00, c01, c11; };
__device__ __forceinline__ NnCone nn_cone(const double *__restrict__ map_xy, const double *__restrict__ map_cov, int j) {
    const double2 xy = reinterpret_cast<const double2 *>(map_xy)[j];
    NnCone c{xy.x, xy.y, 0.0, 0.0, 0.0};
    if (map_cov) { const double4 cv = reinterpret_cast<const double4 *>(map_cov)[j]; c.c00 = cv.x; c.c01 = cv.y; c.c11 = cv.w; }
    return c;
}

// pose = (t, theta), pc = the pose's 3x3 covariance (row-major, upper triangle read) or null
// (nn_query_at: the same from z and the heading's sin / cos, for a caller that moves the pose under a fixed z — lo_pass)
__device__ __forceinline__ NnQuery nn_query_at(const double *pose, const double *pc, double2 z, double s, double c, double ty, const NnDev &p) {
#pragma clang fp contract(off)
    NnQuery q;
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
__device__ __forceinline__ NnQuery nn_query(const double *pose, const double *pc, double az, double zen, double dist, double ty, double lidar, const NnDev &p) {
    const double2 z = nn_polar(az, zen, dist, lidar);
    double s, c; sincos(pose[2], &s, &c);
    return nn_query_at(pose, pc, z, s, c, ty, p);
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
// cone j of the map against the query
__device__ __forceinline__ bool nn_candidate(const NnMap &m, int j, const NnQuery &q, const NnDev &p, double &d2) {
    const NnCone c = nn_cone(m.xy, m.cov, j);
    return nn_pair(q, p, c.x, c.y, c.c00, c.c01, c.c11, m.type[j], d2);
}

// ---- the frame scaffold: a wave owns fpw consecutive frames and gives each W lanes, 64 / W frames side by side, the rest in further passes
// what every frame kernel is given first (the kernels' own argument blocks extend it)
struct FrameArgs {
    int n; const double *poses; int n_poses; const int32_t *pose_of_obs; const double *obs; int n_frames; const int32_t *frame_start; int fpw, only_large;
    double lidar; int n_map; const double *map_xy, *map_cov, *pose_cov; NnDev p;
};
// W lanes per frame: 64 / fpw when every frame of the wave fits, else the next power of two that holds the largest frame within `limit`
// (wave-uniform); gp frames per pass, this lane's group gi and its place lg in it
struct FrameLanes { int W, gp, gi, lg; };
__device__ __forceinline__ FrameLanes frame_lanes(const int32_t *frame_start, int f0, int fpw, int n_frames, int n, int limit, int lane) {
    int W = 64 / fpw;
    for (int t = 0; t < fpw && f0 + t < n_frames; ++t) { const int a = frame_start[f0 + t], b = frame_start[f0 + t + 1];
        if (a >= 0 && b >= a && b <= n && b - a <= limit) while (W < 64 && W < b - a) W <<= 1; }
    return FrameLanes{W, 64 / W, lane >> __builtin_ctz(W), lane & (W - 1)};
}
// frame f's bounds.  Outside 0 <= a <= b <= n it is no frame of this call: nothing is read or written for it.  Above GS_NN_FRAME_MAX it is
// refused as a whole: the caller writes its feature's refusal record and leaves it out
enum FrameKind { FRAME_NONE, FRAME_OK, FRAME_LARGE };
__device__ __forceinline__ FrameKind frame_bounds(const int32_t *frame_start, int n, int f, int &a, int &b) {
    a = frame_start[f]; b = frame_start[f + 1];
    return a < 0 || b < a || b > n ? FRAME_NONE : b - a > NN_FRAME_MAX ? FRAME_LARGE : FRAME_OK;
}
// the body of a kernel of four waves for frames of up to 64 observations (2 .. 8 a wave): pass(fw, a, b, lanes, lane) for every pass of the
// wave, fw = the frame [a, b) of this lane's group, or -1 (then a == b == 0): none, not a frame, or one above 64, which frames_big takes
template <class Args, class Pass>
__device__ __forceinline__ void frames_small(const Args &A, Pass &&pass) {
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f0 = (blockIdx.x * 4 + w) * A.fpw;                               // this wave's frames: [f0, f0 + fpw)
    if (f0 >= A.n_frames) return;
    const FrameLanes l = frame_lanes(A.frame_start, f0, A.fpw, A.n_frames, A.n, 64, lane);
    for (int ps = 0; ps * l.gp < A.fpw; ++ps) {
        int a = 0, b = 0, fw = -1; const int f = f0 + ps * l.gp + l.gi;
        if (ps * l.gp + l.gi < A.fpw && f < A.n_frames && frame_bounds(A.frame_start, A.n, f, a, b) == FRAME_OK && b - a <= 64) fw = f;
        else a = b = 0;
        pass(fw, a, b, l, lane);
    }
}
// the body of a kernel of ONE wave that gives a frame all 64 lanes (up to four rows a lane): pass(f, a, b, lanes, lane) for each of the
// workgroup's fpw frames in turn — every frame, or with only_large those above 64 that frames_small left out — and refuse(f, a, b, lane) for
// a frame above GS_NN_FRAME_MAX
template <class Args, class Refuse, class Pass>
__device__ __forceinline__ void frames_big(const Args &A, Refuse &&refuse, Pass &&pass) {
    const int lane = threadIdx.x, f0 = blockIdx.x * A.fpw;
    for (int t = 0; t < A.fpw && f0 + t < A.n_frames; ++t) {
        int a, b; const FrameKind kind = frame_bounds(A.frame_start, A.n, f0 + t, a, b);
        if (kind == FRAME_LARGE) refuse(f0 + t, a, b, lane);
        if (kind != FRAME_OK || (A.only_large && b - a <= 64)) continue;       // (wave-uniform)
        pass(f0 + t, a, b, FrameLanes{64, 1, 0, lane}, lane);
    }
}

// ---- the pair terms of the joint test and of the localisation
static constexpr int JC_TERMS = 10;                                            // a, c0 c1 c2, m00 m01 m02 m11 m12 m22
// the pair's innovation n and its covariance D = Sigma_j + Q (the query's a without a pose covariance); the callers test det, d00 (and n) themselves
struct PairNu { double n0, n1, d00, d01, d11, det; };
__device__ __forceinline__ PairNu pair_nu(const NnQuery &q, const NnCone &c) {
#pragma clang fp contract(off)
    PairNu v{c.x - q.gx, c.y - q.gy, c.c00 + q.a00, c.c01 + q.a01, c.c11 + q.a11, 0.0};
    v.det = v.d00 * v.d11 - v.d01 * v.d01;
    return v;
}
// T = the ten terms of an admissible pair at a pose whose heading has sin / cos (sn, cs): d2, y = D^-1 n, wp . y, D^-1, D^-1 wp, wp . D^-1 wp
__device__ __forceinline__ void pair_terms(const NnQuery &q, const PairNu &v, double sn, double cs, double (&T)[JC_TERMS]) {
#pragma clang fp contract(off)
    const double n0 = v.n0, n1 = v.n1, d00 = v.d00, d01 = v.d01, d11 = v.d11, det = v.det;
    const double ux = -(q.zx * sn + q.zy * cs), uy = q.zx * cs - q.zy * sn;  // wp = (-w_y, w_x), w as nn_query forms it
    const double y0 = (d11 * n0 - d01 * n1) / det, y1 = (d00 * n1 - d01 * n0) / det;
    const double e00 = d11 / det, e01 = -(d01 / det), e11 = d00 / det;       // D^-1
    const double h0 = e00 * ux + e01 * uy, h1 = e01 * ux + e11 * uy;         // D^-1 wp
    T[0] = (((d11 * n0) * n0 - ((2.0 * d01) * n0) * n1) + (d00 * n1) * n1) / det;      // nn_pair's d2
    T[1] = y0; T[2] = y1; T[3] = ux * y0 + uy * y1;
    T[4] = e00; T[5] = e01; T[6] = h0; T[7] = e11; T[8] = h1; T[9] = ux * h0 + uy * h1;
}
// ---- host side: the launchers' shared choices.  The MEAN frame size decides them (the host does not see a resident call's offsets): a
// guess that costs time when it is wrong — the kernel widens W to its largest frame and runs passes — and never changes a result
static inline long long mean_frame(int n, int n_frames) { return ((long long)n + n_frames - 1) / n_frames; }
static inline int frames_per_wave(long long mean) { return mean <= 8 ? 8 : mean <= 16 ? 4 : mean <= 32 ? 2 : 1; }
// a mean of up to 32 (or force == 0): `small` (frames_small: 2 .. 8 frames a wave), then `big` (frames_big) over groups of 64 frames for
// those above 64 (its waves find none as a rule).  Above (or force == 1): `big` alone, a wave per frame.  force < 0: by the mean.
// start sits on the first dispatch, stop on the last
template <class Args>
static inline void launch_small_then_big(Args A, int force, void (*small)(Args), void (*big)(Args), hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    const long long mean = mean_frame(A.n, A.n_frames);
    A.fpw = 1; A.only_large = 0;
    if (force == 0 || (force < 0 && mean <= 32)) {
        A.fpw = std::max(2, frames_per_wave(mean));
        hipExtLaunchKernelGGL(small, dim3((A.n_frames + 4 * A.fpw - 1) / (4 * A.fpw)), dim3(256), 0, st, start, nullptr, 0, A);
        A.fpw = 64; A.only_large = 1; start = nullptr;
    }
    hipExtLaunchKernelGGL(big, dim3((A.n_frames + A.fpw - 1) / A.fpw), dim3(64), 0, st, start, stop, 0, A);
}

}  // namespace gs
