// gs_polar_api.cpp — polar observation edges behind the C-ABI (include/graphslam.h, "polar observation edges"): the add calls, the
// upload of the tables (polar_sync) and the per-edge values of gs_get_edge_chi2.  Host tables: gs_polar_host.hpp; device pass: gs_polar.hip.
// Adding a polar edge IS a structural change: it appends its carrier through gs_add_observation_edge, so the structure phase or a
// growth step takes it in like any observation edge, and the tables travel with the next call that computes.
#include "../../include/graphslam.h"
#include "gs_private.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

namespace {
// the checks every add shares; on GS_OK p / l are the vertex indices.  Nothing has been appended when this refuses
int polar_check(gs_graph *g, int32_t pose_id, int32_t lm_id, int32_t &p, int32_t &l) {
    if (g->world > 1) return fail(GS_ERR_INVALID, "polar observation edges are not supported on sharded handles (gs_dist_configure with world > 1)");
    auto a = g->h.pose_index.find(pose_id); auto b = g->h.lm_index.find(lm_id);
    if (a == g->h.pose_index.end() || b == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "polar observation edge references an unknown vertex");
    p = a->second; l = b->second;
    return GS_OK;
}
int polar_append(gs_graph *g, int32_t pose_id, int32_t lm_id, int32_t model, int32_t p, int32_t l, double z_r, double z_b, const double w[3]) {
    const double z0[2] = {0.0, 0.0}, info0[4] = {0.0, 0.0, 0.0, 0.0};      // the carrier: exact zeros from the main kernels
    int rc = gs_add_observation_edge(g, pose_id, lm_id, z0, info0); if (rc != GS_OK) return rc;
    g->polar.store.add(g->h.n_pl() - 1, model, p, l, z_r, z_b, w);
    g->marg.valid = false;
    return GS_OK;
}
}  // namespace

extern "C" int gs_add_range_bearing_edge(gs_graph *g, int32_t pose_id, int32_t lm_id, const double z_rb[2], const double info[4]) {
    if (!g || !z_rb || !info) return fail(GS_ERR_INVALID, "null argument");
    int32_t p, l; int rc = polar_check(g, pose_id, lm_id, p, l); if (rc != GS_OK) return rc;
    if (!std::isfinite(z_rb[0]) || !std::isfinite(z_rb[1])) return fail(GS_ERR_INVALID, "polar measurement is not finite");
    if (z_rb[0] < 0) return fail(GS_ERR_INVALID, "range measurement is negative");
    for (int k = 0; k < 4; ++k) if (!std::isfinite(info[k])) return fail(GS_ERR_INVALID, "information matrix is not finite");
    if (!sym_ok(info, 2)) return fail(GS_ERR_INVALID, "information matrix not symmetric");
    const double w[3] = {info[0], info[1], info[3]};
    return polar_append(g, pose_id, lm_id, GS_OBS_RANGE_BEARING, p, l, z_rb[0], z_rb[1], w);
}
extern "C" int gs_add_bearing_edge(gs_graph *g, int32_t pose_id, int32_t lm_id, double z_bearing, double information) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int32_t p, l; int rc = polar_check(g, pose_id, lm_id, p, l); if (rc != GS_OK) return rc;
    if (!std::isfinite(z_bearing)) return fail(GS_ERR_INVALID, "polar measurement is not finite");
    if (!std::isfinite(information) || information < 0) return fail(GS_ERR_INVALID, "bearing information must be finite and >= 0");
    const double w[3] = {0.0, 0.0, information};                        // the one record format: z_r = 0, Omega = [[0, 0], [0, w]]
    return polar_append(g, pose_id, lm_id, GS_OBS_BEARING, p, l, 0.0, z_bearing, w);
}
extern "C" int gs_add_range_bearing_edges(gs_graph *g, int32_t n, const int32_t *pose_ids, const int32_t *lm_ids, const double *z_rb, const double *info) {
    if (!g || n < 0 || (n > 0 && (!pose_ids || !lm_ids || !z_rb || !info))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_range_bearing_edge(g, pose_ids[k], lm_ids[k], z_rb + 2 * (size_t)k, info + 4 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_bearing_edges(gs_graph *g, int32_t n, const int32_t *pose_ids, const int32_t *lm_ids, const double *z_bearing, const double *info) {
    if (!g || n < 0 || (n > 0 && (!pose_ids || !lm_ids || !z_bearing || !info))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_bearing_edge(g, pose_ids[k], lm_ids[k], z_bearing[k], info[k]); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_num_polar_edges(gs_graph *g) { return g ? g->polar.store.n() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_get_polar_edges(gs_graph *g, int32_t capacity, int32_t *out_observation_index, int32_t *out_model) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    const PolarStore &S = g->polar.store; const int n = S.n();
    if ((out_observation_index || out_model) && capacity < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    if (out_observation_index && n) std::memcpy(out_observation_index, S.obs.data(), (size_t)n * sizeof(int32_t));
    if (out_model && n) std::memcpy(out_model, S.model.data(), (size_t)n * sizeof(int32_t));
    return n;
}

// The tables of the handle's polar edges to the device, whole, when the edges, the plan (a growth step included), the edge flags or the
// edge values on the device changed.  Called with the plan of the CURRENT graph on the device (ensure_ready, gs_iterate).  A handle
// without polar edges does nothing here and its dev stays empty: nothing allocated, no launch added to anything.  A refusal leaves dev
// empty and comes back at every call until the cause is gone.
int polar_sync(gs_graph *g) {
    auto &P = g->polar;
    if (P.store.empty()) { P.dev.n_rec = P.dev.n_pv = P.dev.n_lv = 0; P.sync.invalidate(); return GS_OK; }
    if (!P.sync.needed(P.store.version, g->plan_version, g->emask.store.version, g->value_uploads)) return GS_OK;
    P.dev.n_rec = P.dev.n_pv = P.dev.n_lv = 0; P.sync.invalidate();
    if (g->world > 1 || g->plan.dist) return fail(GS_ERR_INVALID, "polar observation edges are not supported on sharded plans");
    const HostGraph &h = g->h; const DevGraph &d = g->d;
    const int N = h.n_poses(), M = h.n_lms(), Epl = h.n_pl();
    if (!g->dev_valid || N != d.N + d.tN || M != d.M + d.tM || Epl != g->plan.base_Epl + d.tEpl)
        return fail(GS_ERR_NOT_INITIALIZED, "polar edges: the plan on the device is not the graph's");
    const PolarStore &S = P.store;
    std::vector<int32_t> src((size_t)Epl, -1);
    std::vector<uint8_t> act;
    for (int32_t k : S.obs) {
        if (k < 0 || k >= Epl || h.pl_info[3 * (size_t)k] != 0.0 || h.pl_info[3 * (size_t)k + 1] != 0.0 || h.pl_info[3 * (size_t)k + 2] != 0.0)
            return fail(GS_ERR_INVALID, "polar edges: a carrier is not the zero-information observation edge it was added as");
        int rc = pl_location(g, k, src[(size_t)k], "polar edges: "); if (rc != GS_OK) return rc; }
    if (g->emask.store.any_off()) { act.assign((size_t)Epl, 1); for (int32_t k : S.obs) act[(size_t)k] = g->emask.store.active(1, k) ? 1 : 0; }
    std::string err;
    if (!build_polar_tables(S, N, M, Epl, src.data(), act.empty() ? nullptr : act.data(), P.tab, err)) return fail(GS_ERR_INVALID, "polar edges: " + err);
    const PolarTables &T = P.tab;
    for (int32_t l : T.lv_id) if (lm_lacks_fused_slot(g, l))
        return fail(GS_ERR_INVALID, "polar edges: a free landmark without an observation edge in the linearisation layout cannot carry one");
    const size_t n = (size_t)T.n_rec, npv = T.pv_id.size(), nlv = T.lv_id.size();
    ArenaLayout lay;
    const size_t o_pv = lay.add(npv * 4), o_ps = lay.add((npv + 1) * 4), o_lv = lay.add(nlv * 4), o_ls = lay.add((nlv + 1) * 4), o_rp = lay.add(n * 4),
                 o_rl = lay.add(n * 4), o_rs = lay.add(n * 4), o_lo = lay.add(n * 4), o_pl = lay.add(T.planes.size() * 8), o_part = lay.add((npv + 255) / 256 * 8);
    int rc = arena_reserve(g, P.arena, lay.total); if (rc != GS_OK) return rc;
    const DevArena &A = P.arena;
    HIP_TRY(arena_upload(g, A, o_pv, T.pv_id.data(), npv * 4)); HIP_TRY(arena_upload(g, A, o_ps, T.pv_start.data(), (npv + 1) * 4));
    HIP_TRY(arena_upload(g, A, o_lv, T.lv_id.data(), nlv * 4)); HIP_TRY(arena_upload(g, A, o_ls, T.lv_start.data(), (nlv + 1) * 4));
    HIP_TRY(arena_upload(g, A, o_rp, T.rec_pose.data(), n * 4)); HIP_TRY(arena_upload(g, A, o_rl, T.rec_lm.data(), n * 4)); HIP_TRY(arena_upload(g, A, o_rs, T.rec_src.data(), n * 4));
    HIP_TRY(arena_upload(g, A, o_lo, T.lm_order.data(), n * 4)); HIP_TRY(arena_upload(g, A, o_pl, T.planes.data(), T.planes.size() * 8));
    HIP_TRY(hipStreamSynchronize(g->stream));                        // (the tables are rebuilt in place by the next change)
    PolarDev D;
    D.n_rec = T.n_rec; D.n_pv = (int32_t)npv; D.n_lv = (int32_t)nlv;
    D.pv_id = (const int32_t *)A.at(o_pv); D.pv_start = (const int32_t *)A.at(o_ps); D.lv_id = (const int32_t *)A.at(o_lv); D.lv_start = (const int32_t *)A.at(o_ls);
    D.rec_pose = (const int32_t *)A.at(o_rp); D.rec_lm = (const int32_t *)A.at(o_rl); D.rec_src = (const int32_t *)A.at(o_rs); D.lm_order = (const int32_t *)A.at(o_lo);
    D.planes = (const double *)A.at(o_pl); D.part = (double *)A.at(o_part);
    P.dev = D;
    P.sync.done(P.store.version, g->plan_version, g->emask.store.version, g->value_uploads);
    return GS_OK;
}

// gs_get_edge_chi2 (observation kind): s and weight of the polar edges over the device output [2][n] of the per-edge kernel, on the
// handle's stream behind that kernel and before the caller's copy back.  The edges' OWN Omega goes up with the call (a query, not part
// of an iteration), whatever the flags; an inactive edge reports weight 0.  Nothing without polar edges.
int polar_edge_chi2_overwrite(gs_graph *g, int32_t n, double *dev_out) {
    const PolarStore &S = g->polar.store;
    const int np = S.n();
    if (np == 0 || n <= 0 || !dev_out) return GS_OK;
    std::vector<int32_t> tab((size_t)np * 3); std::vector<uint8_t> act((size_t)np);
    for (int k = 0; k < np; ++k) { tab[3 * (size_t)k] = S.obs[(size_t)k]; tab[3 * (size_t)k + 1] = S.pose_v[(size_t)k]; tab[3 * (size_t)k + 2] = S.lm_v[(size_t)k];
        act[(size_t)k] = g->emask.store.active(1, S.obs[(size_t)k]) ? 1 : 0; }
    ArenaLayout lay; const size_t o_vals = lay.add(S.rec.size() * 8), o_tab = lay.add(tab.size() * 4), o_act = lay.add((size_t)np);
    DevScratch s; HIP_TRY(s.alloc(lay.total));
    hipError_t e = hipMemcpyAsync(s.p + o_vals, S.rec.data(), S.rec.size() * 8, hipMemcpyHostToDevice, g->stream);
    HIP_NEXT(e, hipMemcpyAsync(s.p + o_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, g->stream));
    HIP_NEXT(e, hipMemcpyAsync(s.p + o_act, act.data(), (size_t)np, hipMemcpyHostToDevice, g->stream));
    if (e == hipSuccess) { launch_polar_edge_chi2(g->d, np, (const int32_t *)(s.p + o_tab), (const double *)(s.p + o_vals), (const uint8_t *)(s.p + o_act), n, dev_out, g->stream);
        e = hipGetLastError(); }
    e = sync_keep_first(e, g->stream);
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("polar edge chi2: ") + hipGetErrorString(e));
    return GS_OK;
}
