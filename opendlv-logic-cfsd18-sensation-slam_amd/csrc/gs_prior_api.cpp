// gs_prior_api.cpp — prior edges behind the C-ABI (include/graphslam.h, "prior edges"): the gs_add_*_prior calls, the upload of the
// grouped tables (prior_sync) and gs_get_prior_chi2.  Host tables: gs_prior_host.hpp; device pass: gs_prior.hip.
// Adding or clearing priors is NOT a structural change: no version of the host graph moves, so no structure phase and no growth step
// is triggered by it, and a prior on a vertex that a growth step appends travels with the next prior_sync.
#include "../../include/graphslam.h"
#include "gs_private.hpp"

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

static int prior_common(gs_graph *g, const double *z, int nz, const double *info, int n) {
    if (!g || !z || !info) return fail(GS_ERR_INVALID, "null argument");
    if (g->world > 1) return fail(GS_ERR_INVALID, "prior edges are not supported on sharded handles (gs_dist_configure with world > 1)");
    for (int k = 0; k < nz; ++k) if (!std::isfinite(z[k])) return fail(GS_ERR_INVALID, "prior measurement is not finite");
    if (!sym_ok(info, n)) return fail(GS_ERR_INVALID, "information matrix not symmetric");
    return GS_OK;
}
extern "C" int gs_add_pose_prior(gs_graph *g, int32_t id, const double z[3], const double info[9]) {
    int rc = prior_common(g, z, 3, info, 3); if (rc != GS_OK) return rc;
    auto a = g->h.pose_index.find(id);
    if (a == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "pose prior references an unknown pose");
    const double w[6] = {info[0], info[1], info[2], info[4], info[5], info[8]};
    g->prior.store.add_pose(a->second, z, w);
    g->marg.valid = false;
    return GS_OK;
}
extern "C" int gs_add_pose_xy_prior(gs_graph *g, int32_t id, const double z[2], const double info[4]) {
    int rc = prior_common(g, z, 2, info, 2); if (rc != GS_OK) return rc;
    auto a = g->h.pose_index.find(id);
    if (a == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "pose prior references an unknown pose");
    const double z3[3] = {z[0], z[1], 0.0}, w[6] = {info[0], info[1], 0.0, info[3], 0.0, 0.0};     // the one pose-prior record format
    g->prior.store.add_pose(a->second, z3, w);
    g->marg.valid = false;
    return GS_OK;
}
extern "C" int gs_add_landmark_prior(gs_graph *g, int32_t id, const double z[2], const double info[4]) {
    int rc = prior_common(g, z, 2, info, 2); if (rc != GS_OK) return rc;
    auto a = g->h.lm_index.find(id);
    if (a == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "landmark prior references an unknown landmark");
    const double w[3] = {info[0], info[1], info[3]};
    g->prior.store.add_lm(a->second, z, w);
    g->marg.valid = false;
    return GS_OK;
}
extern "C" int gs_add_pose_priors(gs_graph *g, int32_t n, const int32_t *ids, const double *z, const double *info) {
    if (!g || (n > 0 && (!ids || !z || !info))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_pose_prior(g, ids[k], z + 3 * (size_t)k, info + 9 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_pose_xy_priors(gs_graph *g, int32_t n, const int32_t *ids, const double *z, const double *info) {
    if (!g || (n > 0 && (!ids || !z || !info))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_pose_xy_prior(g, ids[k], z + 2 * (size_t)k, info + 4 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_landmark_priors(gs_graph *g, int32_t n, const int32_t *ids, const double *z, const double *info) {
    if (!g || (n > 0 && (!ids || !z || !info))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_landmark_prior(g, ids[k], z + 2 * (size_t)k, info + 4 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_num_pose_priors(gs_graph *g) { return g ? g->prior.store.n_pose() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_num_landmark_priors(gs_graph *g) { return g ? g->prior.store.n_lm() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_clear_priors(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->prior.store.empty()) g->marg.valid = false;
    g->prior.store.clear();
    return GS_OK;
}

// The tables of the handle's priors to the device, whole, when the priors changed or another plan came (a growth step included).
// Called with the plan of the CURRENT graph on the device (ensure_ready, gs_iterate).  A handle without priors does nothing here and
// its dev stays empty: no launch is added to anything.  A refusal leaves dev empty and comes back at every call until the cause is gone.
int prior_sync(gs_graph *g) {
    auto &P = g->prior;
    if (P.store.empty()) { P.dev.n_pv = P.dev.n_lv = 0; P.sync.invalidate(); P.settled = P.store.version; return GS_OK; }
    if (!P.sync.needed(P.store.version, g->plan_version)) { P.settled = P.store.version; return GS_OK; }
    P.dev.n_pv = P.dev.n_lv = 0; P.sync.invalidate();
    if (g->world > 1 || g->plan.dist) return fail(GS_ERR_INVALID, "prior edges are not supported on sharded plans");
    const HostGraph &h = g->h; const DevGraph &d = g->d;
    const int N = h.n_poses(), M = h.n_lms();
    if (!g->dev_valid || N != d.N + d.tN || M != d.M + d.tM) return fail(GS_ERR_NOT_INITIALIZED, "priors: the plan on the device is not the graph's");
    std::vector<int32_t> lm_obs((size_t)M, 0);
    for (int32_t l : h.pl_l) ++lm_obs[(size_t)l];
    std::string err;
    if (!build_prior_tables(P.store, h.pose_fixed.data(), N, h.lm_fixed.data(), M, lm_obs.data(), P.tab, err)) return fail(GS_ERR_INVALID, "priors: " + err);
    for (int32_t l : P.tab.lv_id) if (lm_lacks_fused_slot(g, l))
        return fail(GS_ERR_INVALID, "priors: a free landmark without an observation edge in the linearisation layout cannot carry a prior");
    const PriorTables &T = P.tab;
    const size_t npv = T.pv_id.size(), nlv = T.lv_id.size();
    if (npv + nlv == 0) { P.sync.done(P.store.version, g->plan_version); P.settled = P.store.version; return GS_OK; }     // every prior sits on a fixed vertex
    ArenaLayout lay;
    const size_t o_pv = lay.add(npv * 4), o_ps = lay.add((npv + 1) * 4), o_lv = lay.add(nlv * 4), o_ls = lay.add((nlv + 1) * 4),
                 o_pr = lay.add(T.pr.size() * 8), o_lr = lay.add(T.lr.size() * 8), o_part = lay.add((npv + nlv + 255) / 256 * 8);
    int rc = arena_reserve(g, P.arena, lay.total); if (rc != GS_OK) return rc;
    const DevArena &A = P.arena;
    HIP_TRY(arena_upload(g, A, o_pv, T.pv_id.data(), npv * 4)); HIP_TRY(arena_upload(g, A, o_ps, T.pv_start.data(), (npv + 1) * 4));
    HIP_TRY(arena_upload(g, A, o_lv, T.lv_id.data(), nlv * 4)); HIP_TRY(arena_upload(g, A, o_ls, T.lv_start.data(), (nlv + 1) * 4));
    HIP_TRY(arena_upload(g, A, o_pr, T.pr.data(), T.pr.size() * 8)); HIP_TRY(arena_upload(g, A, o_lr, T.lr.data(), T.lr.size() * 8));
    HIP_TRY(hipStreamSynchronize(g->stream));                        // (the tables are rebuilt in place by the next change)
    PriorDev D;
    D.n_pv = (int32_t)npv; D.n_lv = (int32_t)nlv; D.n_pr = T.n_pr; D.n_lr = T.n_lr;
    D.pv_id = (const int32_t *)A.at(o_pv); D.pv_start = (const int32_t *)A.at(o_ps); D.lv_id = (const int32_t *)A.at(o_lv); D.lv_start = (const int32_t *)A.at(o_ls);
    D.pr = (const double *)A.at(o_pr); D.lr = (const double *)A.at(o_lr); D.part = (double *)A.at(o_part);
    P.dev = D;
    P.sync.done(P.store.version, g->plan_version); P.settled = P.store.version;     // (only now: a refused upload stays "pending" for gs_initialize_optimization)
    return GS_OK;
}

// e^T Omega e of every prior of the kind at the current estimates, insertion order, priors on fixed vertices included: the store's
// records go up with the call as planes (a query, not part of an iteration), a thread per prior
extern "C" int gs_get_prior_chi2(gs_graph *g, int32_t kind, int32_t capacity, double *out_chi2) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (kind != 0 && kind != 1) return fail(GS_ERR_INVALID, "prior kind must be 0 (pose) or 1 (landmark)");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (g->world > 1 || g->opt.force_shared_top > 0) return fail(GS_ERR_INVALID, "sharded graph: per-prior chi2 is not supported on sharded handles");
    rc = ensure_ready(g); if (rc != GS_OK) return rc;
    const PriorStore &S = g->prior.store;
    const int n = kind == 0 ? S.n_pose() : S.n_lm(), per = kind == 0 ? PRIOR_POSE_REC : PRIOR_LM_REC;
    if (out_chi2 && capacity < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    if (n == 0 || !out_chi2) return n;
    const std::vector<int32_t> &vert = kind == 0 ? S.pose_v : S.lm_v; const std::vector<double> &rec = kind == 0 ? S.pose_rec : S.lm_rec;
    std::vector<double> planes((size_t)per * n);
    for (int k = 0; k < n; ++k) for (int c = 0; c < per; ++c) planes[(size_t)c * n + k] = rec[(size_t)k * per + c];
    ArenaLayout lay; const size_t o_v = lay.add((size_t)n * sizeof(int32_t)), o_r = lay.add(planes.size() * sizeof(double)), o_out = lay.add((size_t)n * sizeof(double));
    DevScratch s; HIP_TRY(s.alloc(lay.total));
    std::vector<double> out((size_t)n);
    hipError_t e = hipMemcpyAsync(s.p + o_v, vert.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, g->stream);
    HIP_NEXT(e, hipMemcpyAsync(s.p + o_r, planes.data(), planes.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
    if (e == hipSuccess) { launch_prior_chi2_each(g->d, kind, n, (const int32_t *)(s.p + o_v), (const double *)(s.p + o_r), (double *)(s.p + o_out), g->stream); e = hipGetLastError(); }
    HIP_NEXT(e, hipMemcpyAsync(out.data(), s.p + o_out, out.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    e = sync_keep_first(e, g->stream);
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("prior chi2: ") + hipGetErrorString(e));
    std::memcpy(out_chi2, out.data(), (size_t)n * sizeof(double));
    return n;
}
