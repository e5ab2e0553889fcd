// gs_edge_mask_host.hpp — host side of edge deactivation (gs_set_edge_active ... gs_deactivate_edges_above): the per-edge flags, the
// scan for isolated vertices and the keep_connected rule.  No HIP in here: tests/edge_mask_san.cpp compiles this header alone with the
// host sanitizers.
//
// An edge is on level 0 (active) or level 1 (inactive) — g2o's OptimizableGraph::Edge::setLevel with initializeOptimization(0), restated.
// Flags are kept per edge KIND (0 odometry, 1 observation) by insertion index, one byte each, 1 = active.  The vectors are as long as
// the edge arrays were when a flag was last switched off; an edge beyond their end is active, and so is every edge of a store that
// never saw a deactivation (both vectors empty: the handle then does nothing new anywhere).
// A FREE vertex is isolated when it carries no prior and none of its edges is active: its diagonal block of H would be zero.
#pragma once
#include "gs_side_host.hpp"

namespace gs {

struct EdgeMaskStore {
    std::vector<uint8_t> act[2];                     // [kind][edge] 1 active, 0 inactive
    int32_t n_off[2] = {0, 0};                       // inactive edges per kind
    uint64_t version = 0;                            // bumped by every flag that changes: what the device copy is compared with
    bool empty() const { return act[0].empty() && act[1].empty(); }          // never had an inactive edge (since the last clear)
    bool any_off() const { return n_off[0] + n_off[1] > 0; }
    bool active(int kind, int64_t k) const { return k < 0 || (std::size_t)k >= act[kind].size() || act[kind][(std::size_t)k] != 0; }
    // the flag of edge k < n_edges of the kind; returns whether it changed
    bool set(int kind, int32_t k, int32_t n_edges, bool on) {
        std::vector<uint8_t> &a = act[kind];
        if (k < 0 || k >= n_edges) return false;
        if ((std::size_t)k >= a.size()) { if (on) return false; a.resize((std::size_t)n_edges, 1); }
        if ((a[(std::size_t)k] != 0) == on) return false;
        a[(std::size_t)k] = on ? 1 : 0; n_off[kind] += on ? -1 : 1; ++version;
        return true;
    }
    bool activate_all() {                            // the vectors stay: the device may still hold zeros that the next sync restores
        if (!any_off()) return false;
        for (auto &a : act) for (auto &f : a) f = 1;
        n_off[0] = n_off[1] = 0; ++version;
        return true;
    }
    void clear() { act[0].clear(); act[1].clear(); n_off[0] = n_off[1] = 0; ++version; }
};

// the graph as the scans see it (pointers into the host graph; prior flags: one byte per vertex, non-zero = carries a prior; may be null)
struct MaskGraphView {
    int32_t N = 0, M = 0, Epp = 0, Epl = 0;
    const uint8_t *pose_fixed = nullptr, *lm_fixed = nullptr;
    const int32_t *pp_i = nullptr, *pp_j = nullptr, *pl_p = nullptr, *pl_l = nullptr;
    const uint8_t *pose_prior = nullptr, *lm_prior = nullptr;
    bool pose_needs_edge(int32_t p) const { return !pose_fixed[p] && !(pose_prior && pose_prior[p]); }
    bool lm_needs_edge(int32_t l) const { return !lm_fixed[l] && !(lm_prior && lm_prior[l]); }
};

// active edges per vertex
inline void active_degrees(const MaskGraphView &v, const EdgeMaskStore &s, std::vector<int32_t> &dp, std::vector<int32_t> &dl) {
    dp.assign((std::size_t)v.N, 0); dl.assign((std::size_t)v.M, 0);
    for (int32_t k = 0; k < v.Epp; ++k) if (s.active(0, k)) { ++dp[(std::size_t)v.pp_i[k]]; ++dp[(std::size_t)v.pp_j[k]]; }
    for (int32_t k = 0; k < v.Epl; ++k) if (s.active(1, k)) { ++dp[(std::size_t)v.pl_p[k]]; ++dl[(std::size_t)v.pl_l[k]]; }
}

// the first isolated vertex: poses in insertion order, then landmarks.  kind 0 pose, 1 landmark; index = insertion index
inline bool find_isolated(const MaskGraphView &v, const EdgeMaskStore &s, int32_t &kind, int32_t &index) {
    std::vector<int32_t> dp, dl;
    active_degrees(v, s, dp, dl);
    for (int32_t p = 0; p < v.N; ++p) if (dp[(std::size_t)p] == 0 && v.pose_needs_edge(p)) { kind = 0; index = p; return true; }
    for (int32_t l = 0; l < v.M; ++l) if (dl[(std::size_t)l] == 0 && v.lm_needs_edge(l)) { kind = 1; index = l; return true; }
    return false;
}

// gs_deactivate_edges_above, host half: cand[k] != 0 marks edge k of the kind as a candidate.  Candidates are walked in insertion order;
// each ACTIVE one is switched off — except, with keep_connected, one whose removal would leave a free, prior-less endpoint without an
// active edge, given the decisions taken so far.  Returns the edges newly switched off (ascending); the store is updated.
inline std::vector<int32_t> deactivate_candidates(const MaskGraphView &v, EdgeMaskStore &s, int kind, const uint8_t *cand, bool keep_connected) {
    std::vector<int32_t> off, dp, dl;
    const int32_t n = kind == 0 ? v.Epp : v.Epl;
    if (keep_connected) active_degrees(v, s, dp, dl);
    for (int32_t k = 0; k < n; ++k) {
        if (!cand[k] || !s.active(kind, k)) continue;
        if (kind == 0) {
            const int32_t i = v.pp_i[k], j = v.pp_j[k];
            if (keep_connected) {
                const int32_t need_i = i == j ? 2 : 1;                   // (a self-edge counts twice in its vertex's degree)
                if ((v.pose_needs_edge(i) && dp[(std::size_t)i] <= need_i) || (v.pose_needs_edge(j) && dp[(std::size_t)j] <= need_i)) continue;
                --dp[(std::size_t)i]; --dp[(std::size_t)j]; }
        } else {
            const int32_t p = v.pl_p[k], l = v.pl_l[k];
            if (keep_connected) {
                if ((v.pose_needs_edge(p) && dp[(std::size_t)p] <= 1) || (v.lm_needs_edge(l) && dl[(std::size_t)l] <= 1)) continue;
                --dp[(std::size_t)p]; --dl[(std::size_t)l]; }
        }
        if (s.set(kind, k, n, false)) off.push_back(k);
    }
    return off;
}

// What the device holds against what the handle holds.  have[kind][k] = 1: the device holds edge k's own information, 0: zeros.
// A full upload of the edge values (structure phase) puts every edge's own information back: `uploads` counts them.  A growth step
// writes the appended edges only; they are beyond have[]'s end, i.e. "own information", until a sync says otherwise.
struct EdgeMaskSync {
    std::vector<uint8_t> have[2];
    SyncStamp<4> stamp;                              // the flags' version, the full uploads of the edge values, the plan's version, the priors'
    bool needed(uint64_t sv, uint64_t up, uint64_t pv, uint64_t prv) const { return stamp.needed(sv, up, pv, prv); }
    // the edges whose device values differ from what the flags ask for, per kind, ascending (after a full upload: every inactive edge)
    void changes(const EdgeMaskStore &s, const int32_t n_edges[2], uint64_t uploads_now, std::vector<int32_t> out[2]) {
        if (stamp.at[1] != uploads_now) { have[0].clear(); have[1].clear(); stamp.at[1] = uploads_now; }
        for (int kind = 0; kind < 2; ++kind) {
            out[kind].clear();
            const std::vector<uint8_t> &h = have[kind];
            for (int32_t k = 0; k < n_edges[kind]; ++k) {
                const uint8_t want = s.active(kind, k) ? 1 : 0, has = (std::size_t)k < h.size() ? h[(std::size_t)k] : 1;
                if (want != has) out[kind].push_back(k); }
        }
    }
    // the listed edges are on the device as the flags ask (after the launch that wrote them)
    void commit(const EdgeMaskStore &s, const int32_t n_edges[2], const std::vector<int32_t> list[2]) {
        for (int kind = 0; kind < 2; ++kind) {
            std::vector<uint8_t> &h = have[kind];
            if (!list[kind].empty() && h.size() < (std::size_t)n_edges[kind]) h.resize((std::size_t)n_edges[kind], 1);
            for (int32_t k : list[kind]) h[(std::size_t)k] = s.active(kind, k) ? 1 : 0; }
    }
    void done(uint64_t sv, uint64_t up, uint64_t pv, uint64_t prv) { stamp.done(sv, up, pv, prv); }
    void invalidate() { have[0].clear(); have[1].clear(); stamp = SyncStamp<4>(); }
};

}  // namespace gs
