// gs_hmul.hip — y = H v over the blocks the last linearisation left behind (gfx950, wave64).  See gs_hmul.hpp for the vector layout.
// A translation unit of its own: nothing of gs_kernels.hip is touched or re-instantiated, DevGraph is what it was, and every access
// to the H arena here is a load.
//
// Vertex-parallel gather, one writer per address, no atomics, every sum in a fixed order that does not depend on the solver's launch
// mode.  k_hmul: thread t < N is base pose t, thread N + l base landmark l < M.
//   a pose sums      1. its diagonal block (Hpp_diag planes xx xy xt yy yt tt, stride N)
//                    2. its odometry incidences in record order (ppadj_start / ppinc): the block Hpp_off[k] = A^T W B of edge k (rows of
//                       the i endpoint) when the pose is the edge's i endpoint (role bit 0), its transpose when it is the j endpoint
//                    3. its observation slots in slot order (ELL index of slot s: (s / T) (T np) + T (p - p0) + s % T), block Hpl [3 x 2]
//   a landmark sums  1. its diagonal block — fused path (n_wtiles > 0): the landmark's run of lm_part slots summed in slot order, as
//                       k_linearize_finalize and the fronts do (the tail's shares, the priors and an LM lambda sit in the first slot);
//                       gather path: Hll_diag
//                    2. the transposed Hpl blocks of its edges in table order.
// Landmark side tables.  BOTH linearisation paths: lm_start / lm_edges, landmark -> the ELL indices of its edges; every single-device
// plan uploads them (the gather kernels walk them, the fused path keeps them), so nothing is built here.  The pose of an ELL index e
// is p0 + (e mod (T np)) / T.  The tail's landmark side: t_lt_id / t_lt_start / t_lt_edges (touched landmark -> its tail edges) and
// t_pl (edge -> {pose, landmark}).
//
// k_hmul_tail (a grown plan only, ONE workgroup behind k_hmul, like k_linearize_tail):
//   wave 0        a lane per tail pose: t_Hpp_diag, then the tail odometry edges that touch it in edge order (t_pp_ij, t_Hpp_off),
//                 then its tail observation edges in edge order (t_pose_start / t_pose_edges, t_Hpl)
//   wave 1        lane 0 walks the tail odometry edges in order and ADDS each edge's product to its OLD endpoints' rows (behind the
//                 sums k_hmul stored there: "tail edges last")
//   waves 2, 3    a lane per landmark the tail touches: the transposed t_Hpl blocks of its tail edges in edge order — a tail landmark
//                 (all of its edges are tail edges) stores t_Hll_diag v + that sum, an old one adds the sum to its row.
// The old vertices' diagonal shares that come from tail edges are where k_linearize_tail added them: Hpp_diag and the first lm_part slot.
#include "gs_hmul.hpp"
#include "gs_trial_dev.hpp"             // lm_slot_sum: a landmark's run of lm_part slots, summed in slot order

#include <algorithm>

namespace gs {

// y += O u (tr == false) or O^T u (tr == true), O a 3 x 3 row-major block in planes of stride S
__device__ __forceinline__ void hm_add33(const double *O, int64_t S, bool tr, const double *u, double &y0, double &y1, double &y2) {
    const double o0 = O[0], o1 = O[S], o2 = O[2 * S], o3 = O[3 * S], o4 = O[4 * S], o5 = O[5 * S], o6 = O[6 * S], o7 = O[7 * S], o8 = O[8 * S];
    if (!tr) { y0 += o0 * u[0] + o1 * u[1] + o2 * u[2]; y1 += o3 * u[0] + o4 * u[1] + o5 * u[2]; y2 += o6 * u[0] + o7 * u[1] + o8 * u[2]; }
    else     { y0 += o0 * u[0] + o3 * u[1] + o6 * u[2]; y1 += o1 * u[0] + o4 * u[1] + o7 * u[2]; y2 += o2 * u[0] + o5 * u[1] + o8 * u[2]; }
}
// the symmetric diagonal blocks, packed: 3 x 3 in planes xx xy xt yy yt tt, 2 x 2 as three values 00 01 11
__device__ __forceinline__ void hm_diag3(const double *H, int64_t S, const double *v, double &y0, double &y1, double &y2) {
    const double h0 = H[0], h1 = H[S], h2 = H[2 * S], h3 = H[3 * S], h4 = H[4 * S], h5 = H[5 * S];
    y0 = h0 * v[0] + h1 * v[1] + h2 * v[2]; y1 = h1 * v[0] + h3 * v[1] + h4 * v[2]; y2 = h2 * v[0] + h4 * v[1] + h5 * v[2];
}

__global__ void __launch_bounds__(256) k_hmul(DevGraph d, const double *__restrict__ vp, const double *__restrict__ vl,
                                              double *__restrict__ yp, double *__restrict__ yl) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t < d.N) { const int p = t;
        double y0 = 0.0, y1 = 0.0, y2 = 0.0;
        if (d.pose_gidx[p] >= 0) {
            hm_diag3(d.Hpp_diag + p, d.N, vp + 3 * (int64_t)p, y0, y1, y2);
            for (int q = d.ppadj_start[p]; q < d.ppadj_start[p + 1]; ++q) {
                const int2 inc = reinterpret_cast<const int2 *>(d.ppinc)[q];
                const int k = inc.x, role = (int)((uint32_t)inc.y >> 31), other = inc.y & 0x7fffffff;
                if (k < 0 || k >= d.Epp) continue;                   // (a record without an edge on this device)
                hm_add33(d.Hpp_off + k, d.Epp, role != 0, vp + 3 * (int64_t)other, y0, y1, y2); }
            const int64_t L = d.ell_len, S = (int64_t)d.ell_T * d.ell_np;
            const bool laid_out = p >= d.ell_p0 && p < d.ell_p0 + d.ell_np;
            for (int sl = 0; laid_out && sl < d.ell_R * d.ell_T; ++sl) {
                const int64_t e = (int64_t)(sl / d.ell_T) * S + (int64_t)d.ell_T * (p - d.ell_p0) + (sl % d.ell_T);
                const int l = d.ell_l[e];
                if (l < 0) continue;
                const double *W = d.Hpl + e; const double w0 = vl[2 * (int64_t)l], w1 = vl[2 * (int64_t)l + 1];
                y0 += W[0] * w0 + W[L] * w1; y1 += W[2 * L] * w0 + W[3 * L] * w1; y2 += W[4 * L] * w0 + W[5 * L] * w1; } }
        yp[3 * (int64_t)p] = y0; yp[3 * (int64_t)p + 1] = y1; yp[3 * (int64_t)p + 2] = y2;
    } else if (t < d.N + d.M) { const int l = t - d.N;
        double y0 = 0.0, y1 = 0.0;
        if (d.lm_gidx[l] >= 0) {
            double a[3];
            if (d.n_wtiles > 0) lm_slot_sum(d, l, {0, 1, 2}, a);
            else { a[0] = d.Hll_diag[l]; a[1] = d.Hll_diag[(int64_t)d.M + l]; a[2] = d.Hll_diag[2 * (int64_t)d.M + l]; }
            const double v0 = vl[2 * (int64_t)l], v1 = vl[2 * (int64_t)l + 1];
            y0 = a[0] * v0 + a[1] * v1; y1 = a[1] * v0 + a[2] * v1;
            const int64_t L = d.ell_len, S = (int64_t)d.ell_T * d.ell_np;
            for (int q = d.lm_start[l]; q < d.lm_start[l + 1]; ++q) {
                const int64_t e = d.lm_edges[q];
                const int p = d.ell_p0 + (int)((e % S) / d.ell_T);
                const double *W = d.Hpl + e; const double *u = vp + 3 * (int64_t)p;
                y0 += W[0] * u[0] + W[2 * L] * u[1] + W[4 * L] * u[2]; y1 += W[L] * u[0] + W[3 * L] * u[1] + W[5 * L] * u[2]; } }
        yl[2 * (int64_t)l] = y0; yl[2 * (int64_t)l + 1] = y1;
    }
}

__global__ void __launch_bounds__(256) k_hmul_tail(DevGraph d, const double *__restrict__ vp, const double *__restrict__ vl,
                                                   double *__restrict__ yp, double *__restrict__ yl) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    for (int o = tid; o < d.tM; o += 256) { yl[2 * (int64_t)(d.M + o)] = 0.0; yl[2 * (int64_t)(d.M + o) + 1] = 0.0; }     // (a tail landmark no tail edge touches, or a fixed one)
    __syncthreads();
    if (wave == 0) {
        for (int t = lane; t < d.tN; t += 64) { const int p = d.N + t;
            double y0 = 0.0, y1 = 0.0, y2 = 0.0;
            if (d.pose_gidx[p] >= 0) {
                hm_diag3(d.t_Hpp_diag + t, d.tcapN, vp + 3 * (int64_t)p, y0, y1, y2);
                for (int kk = 0; kk < d.tEpp; ++kk) { const int i = d.t_pp_ij[2 * kk], j = d.t_pp_ij[2 * kk + 1];
                    if (i == p) hm_add33(d.t_Hpp_off + kk, d.tcapEpp, false, vp + 3 * (int64_t)j, y0, y1, y2);
                    if (j == p) hm_add33(d.t_Hpp_off + kk, d.tcapEpp, true, vp + 3 * (int64_t)i, y0, y1, y2); }
                const int64_t St = d.tcapEpl;
                for (int q = d.t_pose_start[t]; q < d.t_pose_start[t + 1]; ++q) { const int e = d.t_pose_edges[q], l = d.t_pl[2 * e + 1];
                    const double *W = d.t_Hpl + e; const double w0 = vl[2 * (int64_t)l], w1 = vl[2 * (int64_t)l + 1];
                    y0 += W[0] * w0 + W[St] * w1; y1 += W[2 * St] * w0 + W[3 * St] * w1; y2 += W[4 * St] * w0 + W[5 * St] * w1; } }
            yp[3 * (int64_t)p] = y0; yp[3 * (int64_t)p + 1] = y1; yp[3 * (int64_t)p + 2] = y2; }
    } else if (wave == 1) {
        if (lane == 0) for (int kk = 0; kk < d.tEpp; ++kk) { const int i = d.t_pp_ij[2 * kk], j = d.t_pp_ij[2 * kk + 1];
            for (int side = 0; side < 2; ++side) { const int v = side ? j : i, u = side ? i : j;
                if (v >= d.N || d.pose_gidx[v] < 0) continue;        // a tail endpoint is wave 0's; a fixed row stays zero
                double y0 = yp[3 * (int64_t)v], y1 = yp[3 * (int64_t)v + 1], y2 = yp[3 * (int64_t)v + 2];
                hm_add33(d.t_Hpp_off + kk, d.tcapEpp, side != 0, vp + 3 * (int64_t)u, y0, y1, y2);
                yp[3 * (int64_t)v] = y0; yp[3 * (int64_t)v + 1] = y1; yp[3 * (int64_t)v + 2] = y2; } }
    } else {
        const int64_t St = d.tcapEpl;
        for (int j = tid - 128; j < d.tLt; j += 128) { const int l = d.t_lt_id[j];
            if (d.lm_gidx[l] < 0) continue;
            double s0 = 0.0, s1 = 0.0;
            for (int q = d.t_lt_start[j]; q < d.t_lt_start[j + 1]; ++q) { const int e = d.t_lt_edges[q], p = d.t_pl[2 * e];
                const double *W = d.t_Hpl + e; const double *u = vp + 3 * (int64_t)p;
                s0 += W[0] * u[0] + W[2 * St] * u[1] + W[4 * St] * u[2]; s1 += W[St] * u[0] + W[3 * St] * u[1] + W[5 * St] * u[2]; }
            if (l >= d.M) { const int o = l - d.M; const int64_t Sm = d.tcapM;
                const double a0 = d.t_Hll_diag[o], a1 = d.t_Hll_diag[Sm + o], a2 = d.t_Hll_diag[2 * Sm + o];
                const double v0 = vl[2 * (int64_t)l], v1 = vl[2 * (int64_t)l + 1];
                yl[2 * (int64_t)l] = (a0 * v0 + a1 * v1) + s0; yl[2 * (int64_t)l + 1] = (a1 * v0 + a2 * v1) + s1; }
            else { yl[2 * (int64_t)l] += s0; yl[2 * (int64_t)l + 1] += s1; } }
    }
}

void launch_hmul(const DevGraph &d, const double *v_pose, const double *v_lm, double *y_pose, double *y_lm, hipStream_t st) {
    const int n = d.N + d.M;
    if (n > 0) hipLaunchKernelGGL(k_hmul, dim3((n + 255) / 256), dim3(256), 0, st, d, v_pose, v_lm, y_pose, y_lm);
    if (d.tN > 0 || d.tM > 0) hipLaunchKernelGGL(k_hmul_tail, dim3(1), dim3(256), 0, st, d, v_pose, v_lm, y_pose, y_lm);
}

}  // namespace gs
