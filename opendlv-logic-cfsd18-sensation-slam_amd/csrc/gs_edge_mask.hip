// gs_edge_mask.hip — the device kernels of edge deactivation (gfx950, wave64).  See gs_edge_mask.hpp for what an inactive edge is on the
// device and gs_edge_mask_host.hpp for the flags.  A translation unit of its own, like gs_prior.hip: the kernels of gs_kernels.hip are
// not touched and DevGraph is what it was.
//
// Semantics, restated from g2o's published text (g2o is not part of this project's checkers: nothing here is pinned against a g2o build):
// OptimizableGraph::Edge::setLevel(1) + initializeOptimization(0) leave the edge out of the active set — out of H, b and activeChi2.
//
// k_edge_mask_apply   a thread per edge whose flag changed: active ? the edge's own information : +0.0 into the three planes of ell_w,
//                     the three entries of t_pl_w, or the six entries of pp_info.  Every index is checked against the plan's counts on
//                     the device; plain vector stores, one writer per address (an edge is listed once).
// k_edge_select       a thread per edge of one kind: s = e^T Omega e with the edge's OWN information at the current estimates — the
//                     residuals and squared errors of the linearisation (pl_sq_error / pp_sq_error, gs_edge_dev.hpp), the poses' cached cos / sin —, the weight of the kind's robust kernel (0 for an inactive edge), a candidate
//                     byte (active and s > threshold) and the candidates per workgroup (waves by ballot, then the four waves' counts
//                     in index order: integers, no floating-point atomics, nothing order-dependent).
#include "gs_edge_mask.hpp"
#include "gs_side_dev.hpp"

namespace gs {

__global__ void __launch_bounds__(256) k_edge_mask_apply(DevGraph d, int kind, int n, const int32_t *__restrict__ loc, const double *__restrict__ orig,
                                                         const uint8_t *__restrict__ act) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    const bool on = act[t] != 0;
    if (kind == 0) {
        const int k = loc[t];
        if (k < 0 || k >= d.Epp + d.tEpp || !d.pp_info) return;         // (the host lists edges of this plan; the guard keeps every store in bounds)
        double *w = d.pp_info + 6 * (int64_t)k;
#pragma unroll
        for (int c = 0; c < 6; ++c) w[c] = on ? orig[6 * (int64_t)t + c] : 0.0;
    } else {
        const int src = loc[t]; int e;
        if (side_pl_in_ell(d, src)) { const int64_t L = d.ell_len;
            if (!d.ell_w) return;
#pragma unroll
            for (int c = 0; c < 3; ++c) d.ell_w[c * L + src] = on ? orig[3 * (int64_t)t + c] : 0.0;
        } else if (side_pl_in_tail(d, src, e) && d.t_pl_w) {
#pragma unroll
            for (int c = 0; c < 3; ++c) d.t_pl_w[3 * e + c] = on ? orig[3 * (int64_t)t + c] : 0.0;
        }
    }
}

__global__ void __launch_bounds__(256) k_edge_select(DevGraph d, int kind, int n, const int32_t *__restrict__ tab, const double *__restrict__ info,
                                                     const uint8_t *__restrict__ act, double threshold, double *__restrict__ out_sw,
                                                     uint8_t *__restrict__ cand, int32_t *__restrict__ wg_count) {
    __shared__ int32_t wave_cnt[4];
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int NP = d.N + d.tN, NL = d.M + d.tM;
    bool in = k < n, ok = false, on = false;
    double s = 0.0, w = 0.0;
    if (in) {
        on = !act || act[k] != 0;
        if (kind == 0) {
            const int i = tab[2 * (int64_t)k], j = tab[2 * (int64_t)k + 1];
            if (i >= 0 && i < NP && j >= 0 && j < NP && k < d.Epp + d.tEpp) {
                double xi[3], xj[3], z5[5], wi[6];
#pragma unroll
                for (int c = 0; c < 3; ++c) { xi[c] = d.pose_est[3 * (int64_t)i + c]; xj[c] = d.pose_est[3 * (int64_t)j + c]; }
#pragma unroll
                for (int c = 0; c < 5; ++c) z5[c] = d.pp_zinv[5 * (int64_t)k + c];
#pragma unroll
                for (int c = 0; c < 6; ++c) wi[c] = info[6 * (int64_t)k + c];
                const double2 ci = reinterpret_cast<const double2 *>(d.pose_cs)[i];
                s = pp_sq_error(xi, xj, ci.x, ci.y, z5, wi);
                if (on) robust_rho(d.rk_pp, d.rd_pp, s, w);
                ok = true; }
        } else {
            const int p = tab[3 * (int64_t)k], l = tab[3 * (int64_t)k + 1], src = tab[3 * (int64_t)k + 2];
            double zx = 0.0, zy = 0.0; bool have = false; int e;
            if (side_pl_in_ell(d, src)) { if (d.ell_z) { zx = d.ell_z[src]; zy = d.ell_z[d.ell_len + src]; have = true; } }
            else if (side_pl_in_tail(d, src, e) && d.t_pl_z) { zx = d.t_pl_z[2 * e]; zy = d.t_pl_z[2 * e + 1]; have = true; }
            if (have && p >= 0 && p < NP && l >= 0 && l < NL) {
                const double2 cs = reinterpret_cast<const double2 *>(d.pose_cs)[p];
                s = pl_sq_error(d.pose_est[3 * (int64_t)p], d.pose_est[3 * (int64_t)p + 1], cs.x, cs.y, d.lm_est[2 * (int64_t)l], d.lm_est[2 * (int64_t)l + 1],
                                zx, zy, info[3 * (int64_t)k], info[3 * (int64_t)k + 1], info[3 * (int64_t)k + 2]);
                if (on) robust_rho(d.rk_pl, d.rd_pl, s, w);
                ok = true; }
        }
    }
    const bool is_cand = in && ok && on && s > threshold;
    if (in) {
        if (out_sw) { out_sw[k] = s; out_sw[(int64_t)n + k] = w; }
        if (cand) cand[k] = is_cand ? 1 : 0; }
    const unsigned long long m = __ballot(is_cand);
    if ((threadIdx.x & 63) == 0) wave_cnt[threadIdx.x >> 6] = __popcll(m);
    __syncthreads();
    if (threadIdx.x == 0 && wg_count) wg_count[blockIdx.x] = ((wave_cnt[0] + wave_cnt[1]) + wave_cnt[2]) + wave_cnt[3];
}

void launch_edge_mask_apply(const DevGraph &d, int kind, int n, const int32_t *loc, const double *orig, const uint8_t *act, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_edge_mask_apply, dim3((n + 255) / 256), dim3(256), 0, st, d, kind, n, loc, orig, act);
}
int edge_select_grid(int n) { return (n + 255) / 256; }
void launch_edge_select(const DevGraph &d, int kind, int n, const int32_t *tab, const double *info, const uint8_t *act, double threshold,
                        double *out_sw, uint8_t *cand, int32_t *wg_count, hipStream_t st) {
    if (n > 0) hipLaunchKernelGGL(k_edge_select, dim3(edge_select_grid(n)), dim3(256), 0, st, d, kind, n, tab, info, act, threshold, out_sw, cand, wg_count);
}

}  // namespace gs
