// gs_follow.hip — frame following (include/graphslam.h, "frame following"; gfx950, wave64): the two dispatches a step adds around the
// chain of gs_assoc_nn.hip, and the one that starts a resident run.
//   k_follow_stage    wave 0 of workgroup 0 predicts (a lane per hypothesis) and writes the chain's poses, covariances and frame bounds;
//                     every thread of the grid copies observation records, so that the chain sees n_hyp ordinary frames
//   k_follow_update   wave 0 decides (a lane per hypothesis): accept / reject, counters, the duplicate pass in ascending h through
//                     ballots, best by a scan of broadcasts; then the workgroup's 256 threads copy the pruned index
// No atomics, no spin, no cross-workgroup wait.  Every floating-point expression is under contract(off): the header's order of operations.
#include "gs_follow.hpp"
#include "gs_edge_dev.hpp"      // normalize_theta
#include <hip/hip_ext.h>

#include <algorithm>

namespace gs {

namespace {

// lane `src`'s value in every lane; src is wave-uniform (a loop counter): two v_readlane, no LDS traffic
__device__ __forceinline__ int fo_bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }
__device__ __forceinline__ double fo_bcast(double v, int src) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), src), __builtin_amdgcn_readlane(__double2loint(v), src));
}
// the step's frame: true and k = its size when it is a frame of this call
__device__ __forceinline__ bool fo_frame(const FoArgs &A, int &a, int &k) {
    a = A.fs[0]; const int b = A.fs[1];
    const bool ok = a >= 0 && b >= a && b <= A.n && b - a <= A.cap;
    k = ok ? b - a : 0;
    return ok;
}
// x-, Sigma- of a tracking hypothesis from (x, P) and the motion record u, Qu (null: zeros); P, S: 00 01 02 11 12 22
__device__ __forceinline__ void fo_predict(const double *u, const double *qu, double (&x)[3], double (&P)[6]) {
#pragma clang fp contract(off)
    double s, c; sincos(x[2], &s, &c);
    const double p = (c * u[0]) - (s * u[1]), q = (s * u[0]) + (c * u[1]);
    x[0] = x[0] + p; x[1] = x[1] + q; x[2] = normalize_theta(x[2] + u[2]);
    const double a = -q, b = p;
    const double P00 = P[0], P01 = P[1], P02 = P[2], P11 = P[3], P12 = P[4], P22 = P[5];
    double S[6];
    S[0] = (P00 + a * P02) + a * (P02 + a * P22);
    S[1] = (P01 + a * P12) + b * (P02 + a * P22);
    S[2] = P02 + a * P22;
    S[3] = (P11 + b * P12) + b * (P12 + b * P22);
    S[4] = P12 + b * P22;
    S[5] = P22;
    double N[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (qu) {
        const double q00 = qu[0], q01 = qu[1], q02 = qu[2], q11 = qu[4], q12 = qu[5], q22 = qu[8];
        N[0] = c * (c * q00 - s * q01) - s * (c * q01 - s * q11);
        N[1] = s * (c * q00 - s * q01) + c * (c * q01 - s * q11);
        N[3] = s * (s * q00 + c * q01) + c * (s * q01 + c * q11);
        N[2] = c * q02 - s * q12;
        N[4] = s * q02 + c * q12;
        N[5] = q22;
    }
#pragma unroll
    for (int e = 0; e < 6; ++e) P[e] = S[e] + N[e];
}
__device__ __forceinline__ void fo_store9(double *o, const double (&P)[6]) {  // the upper triangle, mirrored
    o[0] = P[0]; o[1] = P[1]; o[2] = P[2]; o[3] = P[1]; o[4] = P[3]; o[5] = P[4]; o[6] = P[2]; o[7] = P[4]; o[8] = P[5];
}
__device__ __forceinline__ void fo_load6(const double *c, double (&P)[6]) { P[0] = c[0]; P[1] = c[1]; P[2] = c[2]; P[3] = c[4]; P[4] = c[5]; P[5] = c[8]; }

__global__ void __launch_bounds__(64) k_follow_init(int n_hyp, const double *poses, const double *covs, gs_follow_state *state, int32_t *best2) {
    const int h = threadIdx.x;
    if (h == 0) { best2[0] = 0; best2[1] = n_hyp; }
    if (h >= n_hyp) return;
    gs_follow_state &s = state[h];
    double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (covs) fo_load6(covs + 9 * (size_t)h, P);
    s.pose[0] = poses[3 * h]; s.pose[1] = poses[3 * h + 1]; s.pose[2] = poses[3 * h + 2];
    fo_store9(s.cov, P);
    s.sum_chi2 = 0.0; s.hits = 0; s.frames_hit = 0; s.frames_missed = 0; s.misses = 0; s.state = 0; s.state_step = -1; s.duplicate_of = -1; s.reserved = 0;
}

__global__ void __launch_bounds__(256) k_follow_stage(FoArgs A) {
    int a, k; const bool ok = fo_frame(A, a, k);
    if (blockIdx.x == 0 && threadIdx.x < 64) {
        const int h = threadIdx.x;
        if (h < A.n_hyp) A.st_frame_start[h] = h * k;                          // n_hyp + 1 bounds; all zero for a step that is no frame
        if (h == 0) A.st_frame_start[A.n_hyp] = A.n_hyp * k;                   // (the 65th of 64 hypotheses has no lane of its own)
        if (ok && h < A.n_hyp) {
            const gs_follow_state &s = A.state[h];
            double x[3] = {s.pose[0], s.pose[1], s.pose[2]}, P[6]; fo_load6(s.cov, P);
            if (s.state == 0 && A.motion) fo_predict(A.motion, A.motion_cov, x, P);       // a retired hypothesis is frozen
            double *sp = A.st_pose + 3 * h; sp[0] = x[0]; sp[1] = x[1]; sp[2] = x[2];
            fo_store9(A.st_cov + 9 * h, P);
        }
    }
    if (!ok) return;
    const int total = A.n_hyp * k;                                             // <= 64 * 256
    for (int i = blockIdx.x * 256 + threadIdx.x; i < total; i += gridDim.x * 256) {
        const int h = i / k, r = i - h * k;
        reinterpret_cast<double4 *>(A.st_obs)[i] = reinterpret_cast<const double4 *>(A.obs)[a + r];
        A.st_pose_of_obs[i] = h;
    }
}

struct FoUpdateArgs { FoArgs A; JcGate gate; };

__global__ void __launch_bounds__(256) k_follow_update(FoUpdateArgs U) {
#pragma clang fp contract(off)
    const FoArgs &A = U.A;
    __shared__ int s_was[64];
    int a, k; if (!fo_frame(A, a, k)) return;                                  // (uniform)
    if (threadIdx.x < 64) {
        const int h = threadIdx.x; const bool active = h < A.n_hyp;
        gs_follow_state s; s.pose[0] = s.pose[1] = s.pose[2] = 0.0; s.sum_chi2 = 0.0;
        s.hits = s.frames_hit = s.frames_missed = s.misses = 0; s.state = 1; s.state_step = -1; s.duplicate_of = -1; s.reserved = 0;
        double P[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (active) { const gs_follow_state &g = A.state[h];
            s.pose[0] = g.pose[0]; s.pose[1] = g.pose[1]; s.pose[2] = g.pose[2]; fo_load6(g.cov, P); s.sum_chi2 = g.sum_chi2;
            s.hits = g.hits; s.frames_hit = g.frames_hit; s.frames_missed = g.frames_missed; s.misses = g.misses; s.state = g.state;
            s.state_step = g.state_step; s.duplicate_of = g.duplicate_of; }
        const bool was = active && s.state == 0;
        s_was[h] = was ? 1 : 0;
        // the step's record: the prior the chain was given, and what it found (an empty frame: no launch, the record of no pair)
        double pr[3] = {s.pose[0], s.pose[1], s.pose[2]}, PR[6] = {P[0], P[1], P[2], P[3], P[4], P[5]};
        double po[3] = {pr[0], pr[1], pr[2]}, PO[6] = {P[0], P[1], P[2], P[3], P[4], P[5]}, chi2 = 0.0;
        int pairs = 0, iters = 0, status = -1, kept = 0, accepted = 0;
        if (was) {
            const double *sp = A.st_pose + 3 * h; pr[0] = sp[0]; pr[1] = sp[1]; pr[2] = sp[2]; fo_load6(A.st_cov + 9 * h, PR);
            po[0] = pr[0]; po[1] = pr[1]; po[2] = pr[2];
#pragma unroll
            for (int e = 0; e < 6; ++e) PO[e] = PR[e];
            status = 2;
            if (k > 0) {
                const double *lp = A.lo_pose + 3 * h; po[0] = lp[0]; po[1] = lp[1]; po[2] = lp[2]; fo_load6(A.lo_cov + 9 * h, PO);
                chi2 = A.lo_chi2[h]; pairs = A.lo_pairs[h]; iters = A.lo_iters[h]; status = A.lo_status[h]; kept = A.jc_kept[h];
            }
            bool acc = status <= 1 && pairs >= A.min_pairs && pairs >= 0 && pairs <= 256;
            if (acc) acc = chi2 <= U.gate.g[pairs];
            if (acc) {
                accepted = 1;
                s.pose[0] = po[0]; s.pose[1] = po[1]; s.pose[2] = po[2];
#pragma unroll
                for (int e = 0; e < 6; ++e) P[e] = PO[e];
                s.hits += pairs; s.sum_chi2 = s.sum_chi2 + chi2; s.frames_hit += 1; s.misses = 0;
            } else {
                s.pose[0] = pr[0]; s.pose[1] = pr[1]; s.pose[2] = pr[2];
#pragma unroll
                for (int e = 0; e < 6; ++e) P[e] = PR[e];
                s.frames_missed += 1; s.misses += 1;
                if (s.misses >= A.max_misses) { s.state = 1; s.state_step = A.t; }
            }
        }
        // duplicates, h ascending: the lanes d < hh that still track answer, the lowest of them is the one hh folds into
        int alive = active && s.state == 0 ? 1 : 0;
        for (int hh = 1; hh < A.n_hyp; ++hh) {
            const int alive_h = fo_bcast(alive, hh);
            if (!alive_h) continue;                                            // (wave-uniform) a retired hypothesis is compared with nobody
            const double xh = fo_bcast(s.pose[0], hh), yh = fo_bcast(s.pose[1], hh), th = fo_bcast(s.pose[2], hh);
            const double dx = xh - s.pose[0], dy = yh - s.pose[1], dth = normalize_theta(th - s.pose[2]);
            const bool near = alive && h < hh && ((dx * dx) + (dy * dy)) < A.merge2 && fabs(dth) < A.merge_theta;
            const unsigned long long m = __ballot(near);
            if (m != 0ull && h == hh) { alive = 0; s.state = 2; s.duplicate_of = __builtin_ctzll(m); s.state_step = A.t; }
        }
        // best: the smallest (-hits, sum_chi2, h) among the tracking
        int best = -1, best_hits = 0; double best_chi = 0.0;
        for (int hh = 0; hh < A.n_hyp; ++hh) {
            const int al = fo_bcast(alive, hh), hi = fo_bcast(s.hits, hh); const double ch = fo_bcast(s.sum_chi2, hh);
            if (al && (best < 0 || hi > best_hits || (hi == best_hits && ch < best_chi))) { best = hh; best_hits = hi; best_chi = ch; }
        }
        const int n_tracking = __popcll(__ballot(alive != 0));
        if (h == 0) { A.best2[0] = best; A.best2[1] = n_tracking; }
        if (active) {
            if (was) {                                                         // a hypothesis retired before this step is frozen: nothing to write
                gs_follow_state &g = A.state[h];
                g.pose[0] = s.pose[0]; g.pose[1] = s.pose[1]; g.pose[2] = s.pose[2]; fo_store9(g.cov, P); g.sum_chi2 = s.sum_chi2;
                g.hits = s.hits; g.frames_hit = s.frames_hit; g.frames_missed = s.frames_missed; g.misses = s.misses; g.state = s.state;
                g.state_step = s.state_step; g.duplicate_of = s.duplicate_of;
            }
            if (A.rec) { gs_follow_step &r = A.rec[h];
                r.prior_pose[0] = pr[0]; r.prior_pose[1] = pr[1]; r.prior_pose[2] = pr[2]; fo_store9(r.prior_cov, PR);
                r.pose[0] = po[0]; r.pose[1] = po[1]; r.pose[2] = po[2]; fo_store9(r.cov, PO);
                r.chi2 = chi2; r.n_pairs = pairs; r.iterations = iters; r.status = status; r.n_kept = kept; r.accepted = accepted; r.state = s.state; }
        }
    }
    __syncthreads();
    if (!A.out_index) return;
    const int total = A.n_hyp * k;
    for (int i = threadIdx.x; i < total; i += 256) {
        const int h = i / k, r = i - h * k;
        A.out_index[(size_t)h * A.n + a + r] = s_was[h] ? A.jc_idx[i] : -1;
    }
}

}  // namespace

void launch_follow_init(int n_hyp, const double *poses, const double *covs, gs_follow_state *state, int32_t *best2, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    hipExtLaunchKernelGGL(k_follow_init, dim3(1), dim3(64), 0, st, start, stop, 0, n_hyp, poses, covs, state, best2);
}
void launch_follow_stage(const FoArgs &A, int k_max, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    const long long total = (long long)A.n_hyp * k_max;
    const int blocks = (int)std::max<long long>(1, std::min<long long>(64, (total + 255) / 256));
    hipExtLaunchKernelGGL(k_follow_stage, dim3(blocks), dim3(256), 0, st, start, stop, 0, A);
}
void launch_follow_update(const FoArgs &A, const JcGate &gate, hipStream_t st, hipEvent_t start, hipEvent_t stop) {
    FoUpdateArgs U; U.A = A; U.gate = gate;
    hipExtLaunchKernelGGL(k_follow_update, dim3(1), dim3(256), 0, st, start, stop, 0, U);
}

}  // namespace gs
