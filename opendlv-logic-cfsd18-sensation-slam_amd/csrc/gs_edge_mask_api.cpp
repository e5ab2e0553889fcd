// gs_edge_mask_api.cpp — edge deactivation behind the C-ABI (include/graphslam.h, "edge deactivation"): the flag calls, the device
// update of the edges' information (edge_mask_sync), gs_deactivate_edges_above and the per-edge s of a handle with inactive edges.
// Host rules: gs_edge_mask_host.hpp; kernels: gs_edge_mask.hip.
// Changing a flag is NOT a structural change: no version of the host graph moves, so no structure phase and no growth step is
// triggered by it; the information of the changed edges travels with the next call that computes.
#include "../../include/graphslam.h"
#include "gs_private.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

namespace {
bool kind_ok(int32_t kind) { return kind == GS_EDGE_ODOMETRY || kind == GS_EDGE_OBSERVATION; }
int32_t n_edges_of(const gs_graph *g, int32_t kind) { return kind == GS_EDGE_ODOMETRY ? g->h.n_pp() : g->h.n_pl(); }

struct View { std::vector<uint8_t> pose_prior, lm_prior; MaskGraphView v; };
void make_view(const gs_graph *g, View &V) {
    const HostGraph &h = g->h; const PriorStore &S = g->prior.store;
    V.pose_prior.assign((size_t)h.n_poses(), 0); V.lm_prior.assign((size_t)h.n_lms(), 0);
    for (int32_t p : S.pose_v) if (p >= 0 && p < h.n_poses()) V.pose_prior[(size_t)p] = 1;
    for (int32_t l : S.lm_v) if (l >= 0 && l < h.n_lms()) V.lm_prior[(size_t)l] = 1;
    MaskGraphView &v = V.v;
    v.N = h.n_poses(); v.M = h.n_lms(); v.Epp = h.n_pp(); v.Epl = h.n_pl();
    v.pose_fixed = h.pose_fixed.data(); v.lm_fixed = h.lm_fixed.data();
    v.pp_i = h.pp_i.data(); v.pp_j = h.pp_j.data(); v.pl_p = h.pl_p.data(); v.pl_l = h.pl_l.data();
    v.pose_prior = V.pose_prior.data(); v.lm_prior = V.lm_prior.data();
}
std::string vertex_name(const gs_graph *g, int32_t kind, int32_t index) {
    return kind == 0 ? "pose " + std::to_string(g->h.pose_id[(size_t)index]) : "landmark " + std::to_string(g->h.lm_id[(size_t)index]);
}
int shard_refusal(const gs_graph *g) {
    return g->world > 1 ? fail(GS_ERR_INVALID, "inactive edges are not supported on sharded handles (gs_dist_configure with world > 1)") : GS_OK;
}
}  // namespace

static int set_flag(gs_graph *g, int32_t kind, int32_t index, bool on) {
    if (g->emask.store.set(kind, index, n_edges_of(g, kind), on)) g->marg.valid = false;
    return GS_OK;
}
extern "C" int gs_set_edge_active(gs_graph *g, int32_t kind, int32_t index, int32_t active) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!kind_ok(kind)) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    if (index < 0 || index >= n_edges_of(g, kind)) return fail(GS_ERR_INVALID, "edge index out of range");
    if (!active) { int rc = shard_refusal(g); if (rc != GS_OK) return rc; }
    return set_flag(g, kind, index, active != 0);
}
extern "C" int gs_set_edges_active(gs_graph *g, int32_t kind, int32_t count, const int32_t *indices, const uint8_t *active) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!kind_ok(kind)) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    if (count < 0 || (count > 0 && !indices)) return fail(GS_ERR_INVALID, "null argument");
    const int32_t n = n_edges_of(g, kind);
    bool any_off = false;
    for (int32_t t = 0; t < count; ++t) {                            // all or nothing
        if (indices[t] < 0 || indices[t] >= n) return fail(GS_ERR_INVALID, "edge index out of range");
        any_off = any_off || !active || !active[t]; }
    if (any_off) { int rc = shard_refusal(g); if (rc != GS_OK) return rc; }
    for (int32_t t = 0; t < count; ++t) set_flag(g, kind, indices[t], active && active[t]);
    return GS_OK;
}
extern "C" int gs_get_edges_active(gs_graph *g, int32_t kind, int32_t capacity, uint8_t *out_active) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!kind_ok(kind)) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    const int32_t n = n_edges_of(g, kind);
    if (!out_active) return n;
    if (capacity < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    for (int32_t k = 0; k < n; ++k) out_active[k] = g->emask.store.active(kind, k) ? 1 : 0;
    return n;
}
extern "C" int gs_activate_all_edges(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (g->emask.store.activate_all()) g->marg.valid = false;
    return GS_OK;
}
extern "C" int gs_num_inactive_edges(gs_graph *g, int32_t kind) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!kind_ok(kind)) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    return g->emask.store.n_off[kind];
}
extern "C" int gs_find_isolated_vertex(gs_graph *g, int32_t *out_kind, int32_t *out_id) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    View V; make_view(g, V);
    int32_t kind = 0, index = 0;
    if (!find_isolated(V.v, g->emask.store, kind, index)) return 0;
    if (out_kind) *out_kind = kind;
    if (out_id) *out_id = kind == 0 ? g->h.pose_id[(size_t)index] : g->h.lm_id[(size_t)index];
    return 1;
}

// The device arrays brought to the flags.  Called with the plan of the CURRENT graph on the device (ensure_ready, gs_iterate), behind
// any upload of the edge values and before the first launch of the call.  A handle that never had an inactive edge returns at once:
// nothing allocated, nothing launched.  A refusal (an isolated vertex) changes nothing on the device and comes back at every call
// until the cause is gone.
int edge_mask_sync(gs_graph *g) {
    auto &E = g->emask;
    if (E.store.empty()) return GS_OK;
    if (!E.sync.needed(E.store.version, g->value_uploads, g->plan_version, g->prior.store.version)) return GS_OK;
    const HostGraph &h = g->h; const DevGraph &d = g->d;
    if (E.store.any_off()) {
        if (g->world > 1 || g->plan.dist) return fail(GS_ERR_INVALID, "inactive edges are not supported on sharded plans");
        View V; make_view(g, V);
        int32_t kind = 0, index = 0;
        if (find_isolated(V.v, E.store, kind, index))
            return fail(GS_ERR_INVALID, "edge deactivation: " + vertex_name(g, kind, index) + " is free, carries no prior and has no active edge (its block of H would be zero)");
    }
    const int32_t n_edges[2] = {h.n_pp(), h.n_pl()};
    std::vector<int32_t> ch[2];
    E.sync.changes(E.store, n_edges, g->value_uploads, ch);
    const size_t n0 = ch[0].size(), n1 = ch[1].size(), n = n0 + n1;
    if (n == 0) { E.sync.done(E.store.version, g->value_uploads, g->plan_version, g->prior.store.version); return GS_OK; }
    if (g->world > 1 || g->plan.dist) return fail(GS_ERR_INVALID, "inactive edges are not supported on sharded plans");
    if (!g->dev_valid || h.n_poses() != d.N + d.tN || h.n_lms() != d.M + d.tM || h.n_pp() != d.Epp + d.tEpp || h.n_pl() != g->plan.base_Epl + d.tEpl)
        return fail(GS_ERR_NOT_INITIALIZED, "edge deactivation: the plan on the device is not the graph's");
    E.loc.resize(n); E.act.resize(n); E.orig.resize(6 * n0 + 3 * n1);
    for (size_t t = 0; t < n0; ++t) { const int32_t k = ch[0][t];
        E.loc[t] = k; E.act[t] = E.store.active(0, k) ? 1 : 0;
        std::memcpy(&E.orig[6 * t], &h.pp_info[6 * (size_t)k], 6 * sizeof(double)); }
    for (size_t t = 0; t < n1; ++t) { const int32_t k = ch[1][t]; int32_t src = -1;
        int rc = pl_location(g, k, src, ""); if (rc != GS_OK) return rc;
        E.loc[n0 + t] = src; E.act[n0 + t] = E.store.active(1, k) ? 1 : 0;
        std::memcpy(&E.orig[6 * n0 + 3 * t], &h.pl_info[3 * (size_t)k], 3 * sizeof(double)); }
    ArenaLayout lay; const size_t o_orig = lay.add(E.orig.size() * 8), o_loc = lay.add(n * 4), o_act = lay.add(n);
    int rc = arena_reserve(g, E.arena, lay.total); if (rc != GS_OK) return rc;
    char *b = E.arena.at(0);
    hipError_t e = arena_upload(g, E.arena, o_orig, E.orig.data(), E.orig.size() * 8);
    HIP_NEXT(e, arena_upload(g, E.arena, o_loc, E.loc.data(), n * 4));
    HIP_NEXT(e, arena_upload(g, E.arena, o_act, E.act.data(), n));
    if (e == hipSuccess) {
        launch_edge_mask_apply(d, 0, (int)n0, (const int32_t *)(b + o_loc), (const double *)(b + o_orig), (const uint8_t *)(b + o_act), g->stream);
        launch_edge_mask_apply(d, 1, (int)n1, (const int32_t *)(b + o_loc) + n0, (const double *)(b + o_orig) + 6 * n0, (const uint8_t *)(b + o_act) + n0, g->stream);
        e = hipGetLastError(); }
    e = sync_keep_first(e, g->stream);                               // (the staging is rebuilt in place by the next change)
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("edge deactivation: ") + hipGetErrorString(e));
    E.sync.commit(E.store, n_edges, ch);
    E.sync.done(E.store.version, g->value_uploads, g->plan_version, g->prior.store.version);
    return GS_OK;
}

// k_edge_select over every edge of the kind with the edges' own information (a query, not part of an iteration: the tables go up
// with the call, as gs_get_edge_chi2's do).  sw: [2][n] s and weight; cand: [n] candidate bytes; n_cand: their number (workgroup
// counts summed in index order)
static int eval_edges(gs_graph *g, int32_t kind, int32_t n, const std::vector<int32_t> &tab, double threshold, std::vector<double> *sw,
                      std::vector<uint8_t> *cand, int64_t *n_cand) {
    const HostGraph &h = g->h;
    const bool pp = kind == GS_EDGE_ODOMETRY; const size_t per = pp ? 6 : 3;
    const double *info = pp ? h.pp_info.data() : h.pl_info.data();
    std::vector<uint8_t> act((size_t)n);
    for (int32_t k = 0; k < n; ++k) act[(size_t)k] = g->emask.store.active(kind, k) ? 1 : 0;
    const int grid = edge_select_grid(n);
    ArenaLayout lay;
    const size_t o_info = lay.add((size_t)n * per * 8), o_sw = lay.add((size_t)n * 2 * 8), o_tab = lay.add(tab.size() * 4), o_cnt = lay.add((size_t)grid * 4),
                 o_act = lay.add((size_t)n), o_cand = lay.add((size_t)n);
    DevScratch s; HIP_TRY(s.alloc(lay.total));
    char *b = s.p;
    std::vector<int32_t> cnt((size_t)grid, 0);
    if (sw) sw->assign((size_t)n * 2, 0.0);
    if (cand) cand->assign((size_t)n, 0);
    hipError_t e = hipMemcpyAsync(b + o_info, info, (size_t)n * per * 8, hipMemcpyHostToDevice, g->stream);
    HIP_NEXT(e, hipMemcpyAsync(b + o_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, g->stream));
    HIP_NEXT(e, hipMemcpyAsync(b + o_act, act.data(), (size_t)n, hipMemcpyHostToDevice, g->stream));
    if (e == hipSuccess) { launch_edge_select(g->d, kind, n, (const int32_t *)(b + o_tab), (const double *)(b + o_info), (const uint8_t *)(b + o_act), threshold,
                                              sw ? (double *)(b + o_sw) : nullptr, cand ? (uint8_t *)(b + o_cand) : nullptr, (int32_t *)(b + o_cnt), g->stream);
        e = hipGetLastError(); }
    if (e == hipSuccess && sw && !pp && polar_edge_chi2_overwrite(g, n, (double *)(b + o_sw)) != GS_OK) { hipStreamSynchronize(g->stream); return GS_ERR_HIP; }   // (the polar edges' own s and weight; nothing without polar edges)
    if (sw) HIP_NEXT(e, hipMemcpyAsync(sw->data(), b + o_sw, (size_t)n * 2 * 8, hipMemcpyDeviceToHost, g->stream));
    if (cand) HIP_NEXT(e, hipMemcpyAsync(cand->data(), b + o_cand, (size_t)n, hipMemcpyDeviceToHost, g->stream));
    HIP_NEXT(e, hipMemcpyAsync(cnt.data(), b + o_cnt, (size_t)grid * 4, hipMemcpyDeviceToHost, g->stream));
    e = sync_keep_first(e, g->stream);
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("edge select: ") + hipGetErrorString(e));
    if (n_cand) { *n_cand = 0; for (int32_t c : cnt) *n_cand += c; }
    return GS_OK;
}

int edge_mask_edge_chi2(gs_graph *g, int32_t kind, int32_t n, const std::vector<int32_t> &tab, double *out_chi2, double *out_weight) {
    std::vector<double> sw;
    int rc = eval_edges(g, kind, n, tab, INFINITY, &sw, nullptr, nullptr); if (rc != GS_OK) return rc;
    if (out_chi2) std::memcpy(out_chi2, sw.data(), (size_t)n * sizeof(double));
    if (out_weight) std::memcpy(out_weight, sw.data() + n, (size_t)n * sizeof(double));
    return n;
}

extern "C" int gs_deactivate_edges_above(gs_graph *g, int32_t kind, double s_threshold, int32_t keep_connected, int32_t *out_deactivated) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!kind_ok(kind)) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    if (!std::isfinite(s_threshold) || s_threshold < 0) return fail(GS_ERR_INVALID, "s_threshold must be finite and >= 0");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (g->world > 1 || g->opt.force_shared_top > 0) return fail(GS_ERR_INVALID, "inactive edges are not supported on sharded handles (gs_dist_configure with world > 1)");
    rc = ensure_ready(g); if (rc != GS_OK) return rc;
    if (g->plan.dist) return fail(GS_ERR_INVALID, "inactive edges are not supported on sharded plans");
    if (out_deactivated) *out_deactivated = 0;
    const HostGraph &h = g->h;
    const int32_t n = n_edges_of(g, kind);
    if (n == 0) return GS_OK;
    std::vector<int32_t> tab;
    if (kind == GS_EDGE_ODOMETRY) {
        if (n > g->d.Epp + g->d.tEpp) return fail(GS_ERR_INVALID, "odometry edge not on the device");
        tab.resize((size_t)n * 2);
        for (int32_t k = 0; k < n; ++k) { tab[2 * (size_t)k] = h.pp_i[(size_t)k]; tab[2 * (size_t)k + 1] = h.pp_j[(size_t)k]; }
    } else {
        tab.resize((size_t)n * 3);
        for (int32_t k = 0; k < n; ++k) { int32_t src; rc = pl_location(g, k, src, ""); if (rc != GS_OK) return rc;
            tab[3 * (size_t)k] = h.pl_p[(size_t)k]; tab[3 * (size_t)k + 1] = h.pl_l[(size_t)k]; tab[3 * (size_t)k + 2] = src; }
    }
    std::vector<uint8_t> cand; int64_t n_cand = 0;
    rc = eval_edges(g, kind, n, tab, s_threshold, nullptr, &cand, &n_cand); if (rc != GS_OK) return rc;
    int64_t seen = 0; for (uint8_t c : cand) seen += c != 0;
    if (seen != n_cand) return fail(GS_ERR_HIP, "edge select: the workgroups' counts do not add up to the candidate bytes");
    View V; make_view(g, V);
    const std::vector<int32_t> off = deactivate_candidates(V.v, g->emask.store, kind, cand.data(), keep_connected != 0);
    if (!off.empty()) g->marg.valid = false;
    if (out_deactivated) *out_deactivated = (int32_t)off.size();
    return GS_OK;
}
