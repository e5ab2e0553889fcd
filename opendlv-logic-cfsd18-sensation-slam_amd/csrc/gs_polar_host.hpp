// gs_polar_host.hpp — host side of the polar observation edges (gs_add_range_bearing_edge, gs_add_bearing_edge): the measurements as
// they were added, and the tables the device pass reads (gs_polar.hpp).  No HIP in here: tests/polar_tables_san.cpp compiles this header
// alone with the host sanitizers.
//
// A polar edge IS an observation edge: the add call appends a carrier (z = (0, 0), information +0.0) to the host graph, so the structure
// phase, the ELL layout, growth, the fronts and the schedule see an ordinary edge, and records the measurement here under the carrier's
// observation index.  One record format: a bearing-only edge is the range-bearing record with z_r = 0 and Omega = [[0, 0], [0, w]].
//   record   z_r z_beta | w_rr w_rb w_bb                                                 (5 doubles)
// Tables (structure-of-arrays planes, plane k of record r at k * n_rec + r; uploaded whole):
//   pose side      records sorted by pose, insertion order within a pose; pv_id = the poses that carry one (ascending), pv_start = run starts
//   landmark side  lm_order = the SAME records' indices sorted by landmark (insertion order within a landmark); lv_id / lv_start alike
//   per record     rec_pose, rec_lm (vertex indices), rec_src = where its H_pl block lives, in the encoding of gs_get_edge_chi2's table:
//                  src >= 0 the ELL index, src < 0 tail slot -(src + 1)
// An inactive edge (gs_set_edge_active) goes up with Omega = 0: exact zeros in H, b and chi2, as the carrier gives.
// Fixed vertices stay listed: the kernels read the device's fixed flags (a fixed pose's edges still count in chi2 and zero their H_pl block).
#pragma once
#include <string>

#include "gs_side_host.hpp"

namespace gs {

constexpr int POLAR_REC = 5;

struct PolarStore {                                  // insertion order; vertex INDICES (not ids)
    std::vector<int32_t> obs, model, pose_v, lm_v;   // obs: the carrier's observation-edge index; model: GS_OBS_RANGE_BEARING / GS_OBS_BEARING
    std::vector<double> rec;                         // [n][POLAR_REC]
    uint64_t version = 0;                            // bumped by every add / clear: what the device copy is compared with
    int n() const { return (int)obs.size(); }
    bool empty() const { return obs.empty(); }
    void clear() { if (!empty()) ++version; obs.clear(); model.clear(); pose_v.clear(); lm_v.clear(); rec.clear(); }
    // w = (w_rr, w_rb, w_bb); z_beta is normalised when stored
    void add(int32_t obs_index, int32_t mdl, int32_t p, int32_t l, double z_r, double z_beta, const double w[3]) {
        const double r[POLAR_REC] = {z_r, normalize_theta(z_beta), w[0], w[1], w[2]};
        obs.push_back(obs_index); model.push_back(mdl); pose_v.push_back(p); lm_v.push_back(l);
        rec.insert(rec.end(), r, r + POLAR_REC); ++version;
    }
};

struct PolarTables {
    int32_t n_rec = 0;
    std::vector<int32_t> pv_id, pv_start, lv_id, lv_start;      // listed vertices; [n + 1] run starts
    std::vector<int32_t> rec_pose, rec_lm, rec_src, rec_obs;    // [n_rec], pose-sorted order
    std::vector<int32_t> lm_order;                              // [n_rec] record indices sorted by landmark
    std::vector<double> planes;                                 // [POLAR_REC][n_rec]
};

// N, M, Epl: the graph's counts; src_of_obs[Epl]: the location of every observation edge's H_pl block (encoding above; only the polar
// edges' entries are read); active[Epl]: 0 = switched off (nullptr: all active)
inline bool build_polar_tables(const PolarStore &S, int N, int M, int Epl, const int32_t *src_of_obs, const uint8_t *active, PolarTables &T, std::string &err) {
    T = PolarTables();
    const int n = S.n();
    for (int k = 0; k < n; ++k) {
        if (S.pose_v[(size_t)k] < 0 || S.pose_v[(size_t)k] >= N || S.lm_v[(size_t)k] < 0 || S.lm_v[(size_t)k] >= M) { err = "polar edge on a vertex that is not in the graph"; return false; }
        if (S.obs[(size_t)k] < 0 || S.obs[(size_t)k] >= Epl) { err = "polar edge without its observation edge"; return false; } }
    T.n_rec = n;
    std::vector<int32_t> by_pose;
    group_by_key(S.pose_v, N, nullptr, T.pv_id, T.pv_start, by_pose);
    T.rec_pose.resize((size_t)n); T.rec_lm.resize((size_t)n); T.rec_src.resize((size_t)n); T.rec_obs.resize((size_t)n);
    T.planes.assign((size_t)POLAR_REC * (size_t)n, 0.0);
    for (int r = 0; r < n; ++r) { const size_t k = (size_t)by_pose[(size_t)r];
        T.rec_pose[(size_t)r] = S.pose_v[k]; T.rec_lm[(size_t)r] = S.lm_v[k]; T.rec_obs[(size_t)r] = S.obs[k]; T.rec_src[(size_t)r] = src_of_obs[(size_t)S.obs[k]];
        const bool on = !active || active[(size_t)S.obs[k]] != 0;
        for (int c = 0; c < POLAR_REC; ++c) T.planes[(size_t)c * (size_t)n + (size_t)r] = (c >= 2 && !on) ? 0.0 : S.rec[k * POLAR_REC + (size_t)c]; }
    group_by_key(T.rec_lm, M, nullptr, T.lv_id, T.lv_start, T.lm_order);
    return true;
}

// What the device holds against what the handle holds: the tables go up again (whole: they are small) when the polar edges, the plan
// (locations, counts, the tail), the edge flags or the edge values on the device changed
using PolarSync = SyncStamp<4>;                     // the store's version, the plan's, the edge flags', the full uploads of the edge values

}  // namespace gs
