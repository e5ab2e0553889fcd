// gs_upload_host.hpp — the tables that the upload of a plan (gs_upload.cpp: upload_graph) and its append-only growth (upload_growth)
// send to the device, each built by ONE pure function of the HostGraph / Plan: growth rebuilds, for the changed fronts only, exactly the
// rows the full upload builds for all of them.  No HIP in here: tests/upload_tables_san.cpp compiles it with the host sanitizers.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <utility>
#include <vector>

#include "gs_host.hpp"
#include "gs_layout.hpp"
#include "gs_side_host.hpp"      // normalize_theta

namespace gs {

inline DevFront dev_front(const Front &F) {
    DevFront o;
    o.npiv = F.npiv; o.nbnd = F.nbnd; o.piv0 = F.piv0; o.parent = F.parent; o.asm_off = F.asm_off; o.asm_cnt = F.asm_cnt;
    o.asm_dup = F.asm_dup; o.child_off = F.child_off; o.child_cnt = F.child_cnt; o.owner = F.owner; o.level = F.level; o.pad0 = 0;
    o.bnd_off = F.bnd_off; o.map_off = F.map_off; o.L_off = F.L_off; o.U_off = F.U_off;
    return o;
}

// What k_build_sc3 expands a front's unique block records into: ns scalar records {offset in H_arena, offset in the staging image} —
// padded per front to a multiple of 64 — and nl fused landmark records (landmark diagonals of the fused linearisation go to lm3)
struct RecCount { int32_t ns = 0, nl = 0; int32_t padded() const { return (ns + 63) & ~63; } };
inline RecCount front_record_count(const Plan &P, const Front &F, bool fused) {
    RecCount c;
    for (int t = F.asm_off; t < F.asm_off + F.asm_cnt - F.asm_dup; ++t) { const int k = P.asm_recs[t].kind;
        if (k == ASM_POSE_DIAG) c.ns += 9; else if (k == ASM_LM_DIAG) { if (fused) ++c.nl; else c.ns += 5; } else if (k <= ASM_PP_T) c.ns += 9;
        else if (k == ASM_LM_DIAG_TAIL) c.ns += 5; else c.ns += 6; }
    return c;
}

// update matrices, packed: row r' (0 .. nbnd, the last = rhs) of the boundary block holds columns 0 .. min(r', nbnd - 1) at
// r'(r'+1)/2; then one double that stays zero (clamped gathers land on it) and one that collects clamped stores; slots even-aligned
inline int32_t u3_slot_size(int nbnd) { return (nbnd * (nbnd + 1)) / 2 + nbnd; }
inline int64_t u3_slot_advance(int32_t size) { return (size + 2 + 1) & ~1; }

// the bf row of a front: {first block record, unique block records, f, first scalar record, scalar records (padded), first landmark
// record, landmark records, 0}
constexpr int BF_INTS = 8;
inline void bf_row(const Front &F, RecCount c, int64_t sc_off, int64_t lm_off, int32_t *r) {
    r[0] = F.asm_off; r[1] = F.asm_cnt - F.asm_dup; r[2] = F.npiv + F.nbnd; r[3] = (int32_t)sc_off; r[4] = c.padded(); r[5] = (int32_t)lm_off; r[6] = c.nl; r[7] = 0;
}

// growth: the patch record of front s (slots: gs_layout.hpp) — its rows of the compact tables, the update matrix and the scalar records
// at the offsets growth found behind the used room; the landmark records stay where they are (growth adds none)
inline void patch_record(const Plan &P, int s, bool fused, int64_t u_off, int64_t sc_off, int32_t lm_off, int32_t *r) {
    const Front &F = P.fronts[s]; const DevFront o = dev_front(F);
    r[PATCH_FRONT] = s; std::memcpy(r + PATCH_DEVFRONT, &o, sizeof(o));
    r[PATCH_U3_OFF] = (int32_t)u_off; r[PATCH_U3_SIZE] = u3_slot_size(F.nbnd);
    bf_row(F, front_record_count(P, F, fused), sc_off, lm_off, r + PATCH_BF);
    r[PATCH_SPARE] = 0;
}

// the record of an odometry measurement on the device: z^-1 (g2o keeps _inverseMeasurement) as x y theta, then cos and sin of that theta
inline void zinv5(const double *z, double *o) {
    const double th = normalize_theta(-z[2]), c = std::cos(th), s = std::sin(th);
    o[0] = c * (-z[0]) - s * (-z[1]); o[1] = s * (-z[0]) + c * (-z[1]); o[2] = th; o[3] = c; o[4] = s;
}

// incidence records, 8 bytes each: {edge, other endpoint | role << 31}; the pose that holds the record is known to the kernel; an edge
// another rank evaluates: edge = -1
inline std::vector<int32_t> incidence_records(const Plan &P) {
    const size_t Q = P.ppinc.size() / 4;
    std::vector<int32_t> inc(2 * Q);
    for (size_t q = 0; q < Q; ++q) { const int32_t k = P.ppinc[4 * q], role = P.ppinc[4 * q + 1], other = role ? P.ppinc[4 * q + 2] : P.ppinc[4 * q + 3];
        inc[2 * q] = (P.world > 1 && P.pp_rank[k] != P.rank) ? -1 : k; inc[2 * q + 1] = (int32_t)((uint32_t)other | ((uint32_t)role << 31)); }
    return inc;
}

// per landmark group of this rank's wave tiles {first | end << 16 of its tile-local positions, partial-sum slot}
inline std::vector<int32_t> group_table(const Plan &P) {
    const size_t Gn = P.grp_slot.size(); std::vector<int32_t> gt(2 * Gn + 2, 0);
    for (int w = P.wt_lo; w < P.wt_hi; ++w) { const int ga = P.wt_desc[4 * (size_t)w], gn = P.wt_desc[4 * (size_t)w + 1], pos_off = P.wt_desc[4 * (size_t)w + 2];
        for (int q = ga; q < ga + gn; ++q) { gt[2 * (size_t)q] = (P.grp_pos_start[q] - pos_off) | ((P.grp_pos_start[q + 1] - pos_off) << 16); gt[2 * (size_t)q + 1] = P.grp_slot[q]; } }
    return gt;
}

// [children][4] child front, npiv | nbnd << 16, owner, map offset
inline std::vector<int32_t> child_desc(const Plan &P) {
    std::vector<int32_t> cd(P.children.size() * 4);
    for (size_t q = 0; q < P.children.size(); ++q) { const Front &C = P.fronts[P.children[q]];
        cd[4 * q] = P.children[q]; cd[4 * q + 1] = C.npiv | (C.nbnd << 16); cd[4 * q + 2] = C.owner; cd[4 * q + 3] = (int32_t)C.map_off; }
    return cd;
}

// level lists on the device: this rank's own fronts, then the shared top (empty when world == 1); front -> its position in that list
inline std::vector<int32_t> level_list(const Plan &P) {
    std::vector<int32_t> lf = P.level_fronts_owned;
    lf.insert(lf.end(), P.level_fronts_shared.begin(), P.level_fronts_shared.end());
    return lf;
}
inline std::vector<int32_t> pos_of_front(const Plan &P, const std::vector<int32_t> &lf) {
    std::vector<int32_t> pos(P.fronts.size(), -1);
    for (size_t q = 0; q < lf.size(); ++q) pos[lf[q]] = (int32_t)q;
    return pos;
}

// a child's row table in f3_x: 64 entries + 8 header ints, or 160 + 8 when the plan holds a front of more than 63 scalars; xrow = the
// first int of every level position's children tables ([positions + 1]).  false: beyond 2^30 ints
inline int32_t f3x_stride(const Plan &P) { return P.max_front > 63 ? 168 : 72; }
inline bool children_row_offsets(const Plan &P, const std::vector<int32_t> &lf, std::vector<int32_t> &xrow) {
    const int32_t stride = f3x_stride(P);
    xrow.assign(lf.size() + 1, 0);
    for (size_t q = 0; q < lf.size(); ++q) { xrow[q + 1] = xrow[q] + stride * P.fronts[lf[q]].child_cnt;
        if (xrow[q + 1] >= (1 << 30)) return false; }
    return true;
}

// the tail's observation edges (the whole tail: [base_Epl, planned_Epl)) grouped by tail pose and by touched landmark, edge order
// inside a group (the order of the sums in k_linearize_tail); fixed cones are left out of the second: nothing is summed for them
struct TailGroups { std::vector<int32_t> pose_start, pose_edges, lt_id, lt_start, lt_edges; };
inline void tail_groups(const HostGraph &h, const Plan &P, TailGroups &T) {
    const int tN = P.planned_N - P.base_N, tE = P.planned_Epl - P.base_Epl;
    T.pose_start.assign((size_t)tN + 1, 0); T.pose_edges.resize((size_t)tE); T.lt_id.clear(); T.lt_start.clear(); T.lt_edges.clear();
    for (int e = 0; e < tE; ++e) T.pose_start[(size_t)(h.pl_p[P.base_Epl + e] - P.base_N) + 1]++;
    for (int t = 0; t < tN; ++t) T.pose_start[(size_t)t + 1] += T.pose_start[(size_t)t];
    { std::vector<int32_t> fill(T.pose_start.begin(), T.pose_start.end() - 1);
      for (int e = 0; e < tE; ++e) T.pose_edges[(size_t)fill[(size_t)(h.pl_p[P.base_Epl + e] - P.base_N)]++] = e; }
    std::vector<std::pair<int32_t, int32_t>> le; le.reserve((size_t)tE);        // (landmark, edge)
    for (int e = 0; e < tE; ++e) { const int l = h.pl_l[P.base_Epl + e]; if (!h.lm_fixed[l]) le.emplace_back(l, e); }
    std::sort(le.begin(), le.end());
    T.lt_start.push_back(0);
    for (size_t q = 0; q < le.size(); ++q) { if (q == 0 || le[q].first != le[q - 1].first) { if (q) T.lt_start.push_back((int32_t)q); T.lt_id.push_back(le[q].first); }
        T.lt_edges.push_back(le[q].second); }
    if (!le.empty()) T.lt_start.push_back((int32_t)le.size());
}

// Room behind the plan's arrays: a growth step re-writes the runs of the fronts it changes there.  Sized with the plan, within bounds (a
// lap-sized graph must not pay for a 100k-pose graph's room with extra device chunks); entries of the array in question
inline size_t room_of(size_t n, size_t lo, size_t hi) { return std::min(hi, std::max(lo, n / 2)); }
inline size_t room_rows(const Plan &P) { return room_of(P.bnd_rows.size(), 8 * 1024, 64 * 1024); }            // bnd_rows, child_map
inline size_t room_recs(const Plan &P) { return room_of(P.asm_recs.size(), 12 * 1024, 96 * 1024); }           // asm_recs, asm3
inline int64_t room_U(const Plan &P, int64_t used) { return (int64_t)room_of((size_t)used, (size_t)128 << 10, (size_t)(P.max_front > 63 ? 4 : 1) << 20); }   // update matrices of fronts a growth step enlarges
inline int64_t room_sc(const Plan &P, int64_t used) { return (int64_t)room_of((size_t)used, (size_t)64 << 10, (size_t)(P.max_front > 63 ? 4 : 1) << 19); }   // scalar records of the fronts it rebuilds
inline int64_t room_L(const Plan &P) { return (int64_t)room_of((size_t)P.l_doubles, (size_t)256 << 10, (size_t)(P.max_front > 63 ? 8 : 2) << 20); }          // L panels of the fronts it enlarges

}  // namespace gs
