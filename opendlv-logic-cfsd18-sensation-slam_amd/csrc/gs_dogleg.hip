// gs_dogleg.hip — the kernels gs_optimize_dogleg adds around the Gauss-Newton launches (gfx950, wave64).  See gs_dogleg.hpp for the
// trial sequence and the double-buffered state record.  A translation unit of its own, like gs_lm.hip: the kernels of gs_kernels.hip
// are not touched and DevGraph is what it was.
//
// All six kernels are vertex-parallel with the geometry of gs_trial_dev.hpp, which holds what they share with gs_lm.hip (reductions, b on
// any path, base copy, the method-independent half of the verdict).  A total is formed by EVERY workgroup that needs it from the same
// partials in index order, so all of them take the same branch; one writer per address, no atomics.
//
// Free vertices are told by pose_gidx / lm_gidx alone.  k_update also asks pose_known / lm_known, which differ from "every vertex" only
// on pose-window shards; gs_optimize_dogleg refuses sharded handles, so on the handles that get here the two agree.  A port to shards
// must add the same gate to the kernels below that read and rewrite xe (norms, blend), or they touch rows k_update ignores.
//
// xe.  The factor fronts reset their rows of xe to the "not written yet" pattern and the whole-tree back-solve polls them; both happen
// inside the factor / back-solve launches of ONE iteration.  The blend kernel runs behind the back-solve and in front of k_update: it
// overwrites every free scalar of xe with h_dl by plain stores, which is the state k_update expects (values), and the next trial's
// factor launch resets the rows again before anything polls them.
#include "gs_dogleg.hpp"
#include "gs_trial_dev.hpp"
#include "gs_lm.hpp"                    // lm_grid: the geometry the vertex-parallel kernels share

#include <cmath>

namespace gs {

// the total of partial array `which`, the same bits in every thread of every workgroup
__device__ __forceinline__ double dl_total(const DlDev &dl, int which, double *red) { return part_total(dl.t.part + (int64_t)which * dl.part_stride, dl.t.n_part, red); }
__device__ __forceinline__ void dl_put(const DlDev &dl, int which, double v, double *red) {
    v = lm_block_sum(v, red);
    if (threadIdx.x == 0) dl.t.part[(int64_t)which * dl.part_stride + blockIdx.x] = v;
}
__device__ __forceinline__ double dl_alpha(double bb, double bHb) { return (isfinite(bHb) && bHb > 0.0) ? bb / bHb : 0.0; }

__global__ void __launch_bounds__(256) k_dl_begin(DevGraph d, DlDev dl) {
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    save_base(d, dl.t, v);
    if (v < NP) { const int p = v;
        const bool fr = d.pose_gidx[p] >= 0;
        int64_t St; const double *b = pose_plane<const double>(d, d.b_pose, d.t_b_pose, p, St);
#pragma unroll
        for (int c = 0; c < 3; ++c) dl.b_pose[3 * (int64_t)p + c] = fr ? b[c * St] : 0.0;
    } else if (v < NP + ML) { const int l = v - NP;
        double b0 = 0.0, b1 = 0.0;
        if (d.lm_gidx[l] >= 0) lm_rhs_pair(d, l, b0, b1);
        dl.b_lm[2 * (int64_t)l] = b0; dl.b_lm[2 * (int64_t)l + 1] = b1; }
}

__global__ void __launch_bounds__(256) k_dl_dot(DevGraph d, DlDev dl) {
    __shared__ double red[5];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    double bb = 0.0, bHb = 0.0;
    if (v < NP) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { const double b = dl.b_pose[3 * (int64_t)v + c]; bb += b * b; bHb += b * dl.Hb_pose[3 * (int64_t)v + c]; }
    } else if (v < NP + ML) { const int l = v - NP;
#pragma unroll
        for (int c = 0; c < 2; ++c) { const double b = dl.b_lm[2 * (int64_t)l + c]; bb += b * b; bHb += b * dl.Hb_lm[2 * (int64_t)l + c]; } }
    dl_put(dl, DL_BB, bb, red); dl_put(dl, DL_BHB, bHb, red);
}

__global__ void __launch_bounds__(256) k_dl_norms(DevGraph d, DlDev dl) {
    __shared__ double red[5];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    const double bb = dl_total(dl, DL_BB, red), bHb = dl_total(dl, DL_BHB, red);
    const double alpha = dl_alpha(bb, bHb);
    double gg = 0.0, ss = 0.0, cc = 0.0, qq = 0.0;
    auto term = [&](double hg, double b) { const double hs = alpha * b, a = hg - hs; gg += hg * hg; ss += hs * hs; cc += hs * a; qq += a * a; };
    if (v < NP) { const int g = d.pose_gidx[v];
        if (g >= 0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) term(d.xe[g + c], dl.b_pose[3 * (int64_t)v + c]); }
    } else if (v < NP + ML) { const int l = v - NP, g = d.lm_gidx[l];
        if (g >= 0) {
#pragma unroll
            for (int c = 0; c < 2; ++c) term(d.xe[g + c], dl.b_lm[2 * (int64_t)l + c]); } }
    dl_put(dl, DL_GG, gg, red); dl_put(dl, DL_SS, ss, red); dl_put(dl, DL_C, cc, red); dl_put(dl, DL_Q, qq, red);
}

__global__ void __launch_bounds__(256) k_dl_blend(DevGraph d, DlDev dl, int par) {
    __shared__ double red[5];
    DlState &S = dl.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    const double bb = dl_total(dl, DL_BB, red), bHb = dl_total(dl, DL_BHB, red);
    const double gg = dl_total(dl, DL_GG, red), ss = dl_total(dl, DL_SS, red), cc = dl_total(dl, DL_C, red), qq = dl_total(dl, DL_Q, red);
    const double alpha = dl_alpha(bb, bHb), delta = S.delta, gn = sqrt(gg), sd = sqrt(ss);
    // h_dl = wg h_gn + ws h_sd (GN, SD) or h_sd + beta (h_gn - h_sd) (DL)
    int kind; double beta = 0.0, scale = 1.0;
    if (gn < delta) kind = DL_GN;
    else if (sd > delta) { kind = DL_SD; scale = delta / sd; }
    else { kind = DL_DL;
        const double m = delta * delta - ss, disc = sqrt(cc * cc + qq * m);
        beta = qq > 0.0 ? (cc <= 0.0 ? (-cc + disc) / qq : m / (cc + disc)) : 0.0; }
    auto blend = [&](double hg, double b) { const double hs = alpha * b;
        return kind == DL_GN ? hg : (kind == DL_SD ? scale * hs : hs + beta * (hg - hs)); };
    if (v < NP) { const int g = d.pose_gidx[v];
#pragma unroll
        for (int c = 0; c < 3; ++c) { double h = 0.0;
            if (g >= 0) { h = blend(d.xe[g + c], dl.b_pose[3 * (int64_t)v + c]); d.xe[g + c] = h; }
            dl.h_pose[3 * (int64_t)v + c] = h; }
    } else if (v < NP + ML) { const int l = v - NP, g = d.lm_gidx[l];
#pragma unroll
        for (int c = 0; c < 2; ++c) { double h = 0.0;
            if (g >= 0) { h = blend(d.xe[g + c], dl.b_lm[2 * (int64_t)l + c]); d.xe[g + c] = h; }
            dl.h_lm[2 * (int64_t)l + c] = h; } }
    if (blockIdx.x == 0 && threadIdx.x == 0) S.kind = kind;        // (a field no workgroup of this launch reads)
}

__global__ void __launch_bounds__(256) k_dl_gain(DevGraph d, DlDev dl, int par) {
    __shared__ double red[5];
    DlState &S = dl.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x, NP = d.N + d.tN, ML = d.M + d.tM;
    double hHh = 0.0, bh = 0.0, hh = 0.0;
    if (v < NP) {
#pragma unroll
        for (int c = 0; c < 3; ++c) { const double h = dl.h_pose[3 * (int64_t)v + c]; hHh += h * dl.Hh_pose[3 * (int64_t)v + c]; bh += dl.b_pose[3 * (int64_t)v + c] * h; hh += h * h; }
    } else if (v < NP + ML) { const int l = v - NP;
#pragma unroll
        for (int c = 0; c < 2; ++c) { const double h = dl.h_lm[2 * (int64_t)l + c]; hHh += h * dl.Hh_lm[2 * (int64_t)l + c]; bh += dl.b_lm[2 * (int64_t)l + c] * h; hh += h * h; } }
    dl_put(dl, DL_HHH, hHh, red); dl_put(dl, DL_BH, bh, red); dl_put(dl, DL_HH, hh, red);
    if (blockIdx.x == 0 && threadIdx.x == 0) trial_file(d, S.t);
}

// The verdict.  Every workgroup forms it from the same read-only inputs and restores its share of the estimates on a rejection;
// workgroup 0 writes the next record, the history and the flags (trial_verdict) and what is the dogleg's own: delta and the kinds.  Any
// failure code (a zero pivot is g2o's "Fail" here, not a rejected trial): k_update applied nothing, nothing moves, the host ends the
// call or — a flag timeout — repairs it and runs the trial again.
__global__ void __launch_bounds__(256) k_dl_step(DevGraph d, DlDev dl, int par) {
    __shared__ double red[5];
    const DlState S = dl.state[par];
    const int v = blockIdx.x * 256 + threadIdx.x;
    const double hHh = dl_total(dl, DL_HHH, red), bh = dl_total(dl, DL_BH, red), hh = dl_total(dl, DL_HH, red);
    double gain = -hHh + 2.0 * bh;
    if (fabs(gain) < 1e-12) gain = 1e-12;
    const double chi_new = d.chi2[0];
    const bool active = S.t.done == 0 && S.t.failcode == 0;
    const double rho = (S.t.chi_old - chi_new) / gain;
    const bool accept = active && rho > 0.0 && isfinite(chi_new);
    if (active && !accept) restore_base(d, dl.t, v);
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    DlState T = S;
    T.t.failcode = 0;
    if (active) {
        if (S.t.iterations < 64) { dl.hist_delta[S.t.iterations] = S.delta; dl.hist_kind[S.t.iterations] = S.kind; }
        if (rho > 0.75) T.delta = fmax(S.delta, 3.0 * sqrt(hh));
        else if (rho < 0.25) T.delta = 0.5 * S.delta;
        if (accept) { T.n_kind[DL_GN] += S.kind == DL_GN; T.n_kind[DL_SD] += S.kind == DL_SD; T.n_kind[DL_DL] += S.kind == DL_DL; }      // (constant indices: the record stays in registers)
        trial_verdict(d, dl.t, S.t, T.t, accept, chi_new);
    }
    dl.state[par ^ 1] = T;
}

void launch_dl_begin(const DevGraph &d, const DlDev &dl, hipStream_t st) { hipLaunchKernelGGL(k_dl_begin, dim3(lm_grid(d)), dim3(256), 0, st, d, dl); }
void launch_dl_dot(const DevGraph &d, const DlDev &dl, hipStream_t st) { hipLaunchKernelGGL(k_dl_dot, dim3(lm_grid(d)), dim3(256), 0, st, d, dl); }
void launch_dl_norms(const DevGraph &d, const DlDev &dl, hipStream_t st) { hipLaunchKernelGGL(k_dl_norms, dim3(lm_grid(d)), dim3(256), 0, st, d, dl); }
void launch_dl_blend(const DevGraph &d, const DlDev &dl, int par, hipStream_t st) { hipLaunchKernelGGL(k_dl_blend, dim3(lm_grid(d)), dim3(256), 0, st, d, dl, par); }
void launch_dl_gain(const DevGraph &d, const DlDev &dl, int par, hipStream_t st) { hipLaunchKernelGGL(k_dl_gain, dim3(lm_grid(d)), dim3(256), 0, st, d, dl, par); }
void launch_dl_step(const DevGraph &d, const DlDev &dl, int par, hipStream_t st) { hipLaunchKernelGGL(k_dl_step, dim3(lm_grid(d)), dim3(256), 0, st, d, dl, par); }

}  // namespace gs
