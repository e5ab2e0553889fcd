// gs_export_host.hpp — device layout -> export layout of gs_export_system, on host copies of the device arrays.  The device keeps H and b
// structure-of-arrays in planes (plane stride = the array's count; the tail arenas of a grown plan: the tail CAPACITIES tcap*) with the
// diagonal blocks packed symmetric; the export is array-of-blocks, full and row-major, base entries first and the tail's behind them:
//   pose p < N            Hpp_diag / b_pose planes, stride N          pose N + t, t < tN        t_Hpp_diag / t_b_pose, stride tcapN
//   landmark l < M        Hll_diag / b_lm planes, stride M            landmark M + t, t < tM    t_Hll_diag / t_b_lm, stride tcapM
//   odometry edge k < Epp Hpp_off planes, stride Epp                  edge Epp + t, t < tEpp    t_Hpp_off, stride tcapEpp
//   observation edge k (insertion order), e = ell_of_ins[k]: e < 0 zeros (outside the layout); e < L the Hpl planes, stride L;
//                         otherwise slot e - L < tEpl of t_Hpl, stride tcapEpl (grow_plan numbers the tail's edges behind the layout)
// The shares the tail adds to OLD vertices are already in the base arrays (k_linearize_tail adds them there): nothing is summed here.
// No HIP in here: tests/export_layout_san.cpp compiles it with the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gs {

struct ExportCounts { int64_t N, M, Epp, L, Epl;                      // base: poses, landmarks, odometry edges, layout length (ell_len), observation edges by insertion (base + tail)
                      int64_t tN, tM, tEpp, tEpl;                     // the tail's counts
                      int64_t tcapN, tcapM, tcapEpp, tcapEpl; };      // ... and the plane strides of its arenas
struct ExportSrc { const double *Hpp_diag, *Hll_diag, *Hpp_off, *Hpl, *b_pose, *b_lm;           // [6][N] [3][M] [9][Epp] [6][L] [3][N] [2][M]
                   const double *t_Hpp_diag, *t_Hll_diag, *t_Hpp_off, *t_Hpl, *t_b_pose, *t_b_lm;   // [6][tcapN] [3][tcapM] [9][tcapEpp] [6][tcapEpl] [3][tcapN] [2][tcapM] (unread when the tail count is 0)
                   const int32_t *ell_of_ins; };                      // [Epl]
struct ExportDst { double *Hpp_diag, *Hll_diag, *Hpp_off, *Hpl, *b_pose, *b_lm; };               // [(N+tN)*9] [(M+tM)*4] [(Epp+tEpp)*9] [Epl*6] [(N+tN)*3] [(M+tM)*2]; any may be null

inline void export_layout(const ExportCounts &c, const ExportSrc &s, const ExportDst &o) {
    static const int sym3[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}}, sym2[2][2] = {{0, 1}, {1, 2}};
    // n blocks of planes [*][stride] -> dst blocks from `first` on
    auto sym_blocks3 = [&](double *dst, int64_t first, const double *src, int64_t n, int64_t stride) {
        for (int64_t p = 0; p < n; ++p) for (int r = 0; r < 3; ++r) for (int q = 0; q < 3; ++q) dst[9 * (first + p) + 3 * r + q] = src[sym3[r][q] * stride + p]; };
    auto sym_blocks2 = [&](double *dst, int64_t first, const double *src, int64_t n, int64_t stride) {
        for (int64_t l = 0; l < n; ++l) for (int r = 0; r < 2; ++r) for (int q = 0; q < 2; ++q) dst[4 * (first + l) + 2 * r + q] = src[sym2[r][q] * stride + l]; };
    auto planes = [&](double *dst, int64_t first, const double *src, int64_t n, int64_t stride, int comps) {
        for (int64_t k = 0; k < n; ++k) for (int q = 0; q < comps; ++q) dst[comps * (first + k) + q] = src[q * stride + k]; };
    if (o.Hpp_diag) { sym_blocks3(o.Hpp_diag, 0, s.Hpp_diag, c.N, c.N); sym_blocks3(o.Hpp_diag, c.N, s.t_Hpp_diag, c.tN, c.tcapN); }
    if (o.Hll_diag) { sym_blocks2(o.Hll_diag, 0, s.Hll_diag, c.M, c.M); sym_blocks2(o.Hll_diag, c.M, s.t_Hll_diag, c.tM, c.tcapM); }
    if (o.Hpp_off) { planes(o.Hpp_off, 0, s.Hpp_off, c.Epp, c.Epp, 9); planes(o.Hpp_off, c.Epp, s.t_Hpp_off, c.tEpp, c.tcapEpp, 9); }
    if (o.Hpl) for (int64_t k = 0; k < c.Epl; ++k) { const int64_t e = s.ell_of_ins[k];                 // insertion order
        const bool tail = e >= c.L && e - c.L < c.tEpl;
        for (int q = 0; q < 6; ++q) o.Hpl[6 * k + q] = e < 0 ? 0.0 : e < c.L ? s.Hpl[q * c.L + e] : tail ? s.t_Hpl[q * c.tcapEpl + (e - c.L)] : 0.0; }
    if (o.b_pose) { planes(o.b_pose, 0, s.b_pose, c.N, c.N, 3); planes(o.b_pose, c.N, s.t_b_pose, c.tN, c.tcapN, 3); }
    if (o.b_lm) { planes(o.b_lm, 0, s.b_lm, c.M, c.M, 2); planes(o.b_lm, c.M, s.t_b_lm, c.tM, c.tcapM, 2); }
}

}  // namespace gs
