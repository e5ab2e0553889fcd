// gs_prior_host.hpp — host side of the prior edges (gs_add_pose_prior, gs_add_pose_xy_prior, gs_add_landmark_prior): the priors as
// they were added, and the tables the device pass reads (gs_prior.hpp).  No HIP in here: tests/prior_tables_san.cpp compiles this header
// alone with the host sanitizers.
//
// One pose-prior record format: the measurement INVERTED with the cos / sin of the inverse's angle, taken when the prior is added
// (g2o's EdgeSE2Prior keeps _inverseMeasurement; the odometry records, pp_zinv, are kept the same way), and the six distinct entries
// of Omega.  An XY prior is the record of (zx, zy, 0) with Omega in the upper-left 2 x 2 and zeros elsewhere.
//   pose record      zi_x zi_y zi_theta cos sin | w_xx w_xy w_xt w_yy w_yt w_tt        (11 doubles)
//   landmark record  z_x z_y | w_00 w_01 w_11                                          (5 doubles)
// Tables: the priors of FREE vertices grouped by vertex — a compact list of the vertices that carry one (ascending vertex index), the
// start offset of each vertex's run, and the records as structure-of-arrays planes (plane k of record r at k * n_records + r), sorted by
// vertex, insertion order within a vertex.  A prior on a fixed vertex stays out of the tables (g2o: an edge whose vertices are all
// fixed is inactive); gs_get_prior_chi2 reads the store.
#pragma once
#include <string>

#include "gs_side_host.hpp"

namespace gs {

constexpr int PRIOR_POSE_REC = 11, PRIOR_LM_REC = 5;

struct PriorStore {                                  // insertion order, vertex INDICES (not ids)
    std::vector<int32_t> pose_v, lm_v;
    std::vector<double> pose_rec, lm_rec;            // [n][PRIOR_POSE_REC], [n][PRIOR_LM_REC]
    uint64_t version = 0;                            // bumped by every add / clear: what the device copy is compared with
    int n_pose() const { return (int)pose_v.size(); }
    int n_lm() const { return (int)lm_v.size(); }
    bool empty() const { return pose_v.empty() && lm_v.empty(); }
    void clear() { if (!empty()) ++version; pose_v.clear(); lm_v.clear(); pose_rec.clear(); lm_rec.clear(); }
    // z = (x, y, theta), w = the six distinct entries of Omega (xx xy xt yy yt tt)
    void add_pose(int32_t v, const double z[3], const double w[6]) {
        const double th = normalize_theta(-z[2]), c = std::cos(th), s = std::sin(th);
        const double r[PRIOR_POSE_REC] = {c * (-z[0]) - s * (-z[1]), s * (-z[0]) + c * (-z[1]), th, c, s, w[0], w[1], w[2], w[3], w[4], w[5]};
        pose_v.push_back(v); pose_rec.insert(pose_rec.end(), r, r + PRIOR_POSE_REC); ++version;
    }
    void add_lm(int32_t v, const double z[2], const double w[3]) {
        const double r[PRIOR_LM_REC] = {z[0], z[1], w[0], w[1], w[2]};
        lm_v.push_back(v); lm_rec.insert(lm_rec.end(), r, r + PRIOR_LM_REC); ++version;
    }
};

struct PriorTables {
    std::vector<int32_t> pv_id, pv_start, lv_id, lv_start;      // listed vertices; [n + 1] run starts (pv_start.size() == pv_id.size() + 1)
    std::vector<double> pr, lr;                                 // [PRIOR_POSE_REC][n_pr], [PRIOR_LM_REC][n_lr]
    int32_t n_pr = 0, n_lr = 0;
    int n_vertices() const { return (int)(pv_id.size() + lv_id.size()); }
};

// one kind: the priors of free vertices v < n_vertex grouped by vertex (group_by_key: insertion order within a vertex)
inline bool prior_group(const std::vector<int32_t> &vert, const std::vector<double> &rec, int per, const uint8_t *fixed, int n_vertex,
                        std::vector<int32_t> &ids, std::vector<int32_t> &start, std::vector<double> &planes, int32_t &n_rec, std::string &err) {
    ids.clear(); start.clear(); planes.clear(); n_rec = 0;
    std::vector<uint8_t> skip(vert.size());
    for (size_t k = 0; k < vert.size(); ++k) {
        const int32_t v = vert[k];
        if (v < 0 || v >= n_vertex) { err = "prior on a vertex that is not in the graph"; return false; }
        skip[k] = fixed[v]; }
    std::vector<int32_t> order;
    group_by_key(vert, n_vertex, skip.data(), ids, start, order);
    n_rec = (int32_t)order.size();
    planes.resize((size_t)per * (size_t)n_rec);
    for (size_t r = 0; r < order.size(); ++r) for (int c = 0; c < per; ++c) planes[(size_t)c * (size_t)n_rec + r] = rec[(size_t)order[r] * (size_t)per + (size_t)c];
    return true;
}

// lm_obs[l]: observation edges of landmark l.  A free landmark whose only measurement is a prior is refused: the fused linearisation
// gives it no partial-sum slot, so there is no address the fronts would read its block from (NOT DONE, include/graphslam.h)
inline bool build_prior_tables(const PriorStore &S, const uint8_t *pose_fixed, int N, const uint8_t *lm_fixed, int M, const int32_t *lm_obs,
                               PriorTables &T, std::string &err) {
    if (!prior_group(S.pose_v, S.pose_rec, PRIOR_POSE_REC, pose_fixed, N, T.pv_id, T.pv_start, T.pr, T.n_pr, err)) return false;
    if (!prior_group(S.lm_v, S.lm_rec, PRIOR_LM_REC, lm_fixed, M, T.lv_id, T.lv_start, T.lr, T.n_lr, err)) return false;
    for (int32_t l : T.lv_id) if (lm_obs[l] <= 0) { err = "a free landmark whose only measurement is a prior is not supported (it needs an observation edge)"; return false; }
    return true;
}

// What the device holds against what the handle holds: the tables go up again (whole: they are small) when the priors changed or
// when another plan came (fixed flags, vertex counts and the tail may differ)
using PriorSync = SyncStamp<2>;                     // the store's version, the plan's version

}  // namespace gs
