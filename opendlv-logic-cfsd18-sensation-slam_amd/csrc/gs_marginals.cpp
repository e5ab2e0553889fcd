// gs_marginals.cpp — marginal covariances (gs_compute_marginals and its getters).
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

// ------------------------------------------------------------------ marginal covariances (gs_compute_marginals)
// Sigma = H^-1 on the pattern of L by a selected inversion of the multifrontal factor (gs_kernels.hip, k_selinv_panel / k_selinv_big).  The tables
// (front -> Sigma image, level sizes, output entry -> arena offset) are built on the first call after a structure phase, not in it.
static int64_t marg_tri(int64_t r) { return r * (r + 1) / 2; }
// arena offset of Sigma(u, v), u / v scalars in elimination order; -1 when the pair is outside the pattern of L
static int64_t marg_offset(const gs_graph *g, int u, int v) {
    const Plan &P = g->plan; const auto &M = g->marg;
    const int lo = std::min(u, v), hi = std::max(u, v), s = M.front_of[lo];
    const Front &F = P.fronts[s];
    int rh;
    if (hi < F.piv0 + F.npiv) rh = hi - F.piv0;
    else { const int32_t *b = P.bnd_rows.data() + F.bnd_off, *e = b + F.nbnd, *it = std::lower_bound(b, e, hi);
        if (it == e || *it != hi) return -1;
        rh = F.npiv + (int)(it - b); }
    return M.sig_off[s] + marg_tri(rh) + (lo - F.piv0);
}
// offsets of the block Sigma(a, b), a / b = first scalar (-1: fixed vertex -> zeros, offset -1) and size; false: outside the pattern
static bool marg_block(const gs_graph *g, int ga, int na, int gb, int nb, int64_t *out) {
    for (int r = 0; r < na; ++r)
        for (int c = 0; c < nb; ++c) {
            int64_t o = -1;
            if (ga >= 0 && gb >= 0) { o = marg_offset(g, ga + r, gb + c); if (o < 0) return false; }
            out[r * nb + c] = o; }
    return true;
}
template <class T> static int marg_buffer(gs_graph *g, T **ptr, int64_t &cap, int64_t want) {
    if (*ptr && cap >= want) return GS_OK;
    const int64_t n = std::max<int64_t>(want + want / 4, 1);        // room for a few growth steps before the next allocation
    int rc = dev_alloc(g, ptr, (size_t)n); if (rc != GS_OK) return rc;
    cap = n; return GS_OK;
}
static int marg_tables(gs_graph *g) {
    auto &M = g->marg; const Plan &P = g->plan; const HostGraph &h = g->h;
    if (M.plan_version == g->plan_version && M.sig) return GS_OK;
    const int S = (int)P.fronts.size();
    M.sig_off.assign(S, 0); M.front_of.assign(P.n_scalar, 0);
    int64_t off = 0;
    for (int s = 0; s < S; ++s) { const Front &F = P.fronts[s];
        M.sig_off[s] = off; off += marg_tri(F.npiv + F.nbnd);
        for (int k = 0; k < F.npiv; ++k) M.front_of[F.piv0 + k] = s; }
    M.sig_doubles = off;
    // launch lists: every level from the root down, its fronts split by form (a wave: <= 63 scalars, a workgroup: 64 .. 159, HBM: larger)
    const int nlev = (int)g->sched.own.start.size() - 1;
    M.sel_list.clear(); M.sel_launch.clear();
    for (int l = nlev - 1; l >= 0; --l)
        for (int form = 0; form < 3; ++form) {
            const int first = (int)M.sel_list.size(); int max_f = 0;
            for (int q = g->sched.own.start[l]; q < g->sched.own.start[l + 1]; ++q) {
                const int s = P.level_fronts_owned[q], fs = P.fronts[s].npiv + P.fronts[s].nbnd;
                if ((fs <= 63 ? 0 : (fs <= 159 ? 1 : 2)) != form) continue;
                M.sel_list.push_back(s); max_f = std::max(max_f, fs); }
            if ((int)M.sel_list.size() > first) M.sel_launch.push_back({first, (int)M.sel_list.size() - first, max_f}); }
    const int N = h.n_poses(), Ml = h.n_lms(), Epp = h.n_pp(), Epl = h.n_pl();
    if ((int)P.pose_gidx.size() < N || (int)P.lm_gidx.size() < Ml) return fail(GS_ERR_INVALID, "marginals: the plan does not cover the graph");
    M.n_out = 9 * (int64_t)N + 4 * (int64_t)Ml + 9 * (int64_t)Epp + 6 * (int64_t)Epl;
    std::vector<int64_t> tab((size_t)M.n_out);
    int64_t *t = tab.data(); bool ok = true;
    for (int p = 0; p < N; ++p, t += 9) ok = marg_block(g, P.pose_gidx[p], 3, P.pose_gidx[p], 3, t) && ok;
    for (int l = 0; l < Ml; ++l, t += 4) ok = marg_block(g, P.lm_gidx[l], 2, P.lm_gidx[l], 2, t) && ok;
    for (int k = 0; k < Epp; ++k, t += 9) ok = marg_block(g, P.pose_gidx[h.pp_i[k]], 3, P.pose_gidx[h.pp_j[k]], 3, t) && ok;
    for (int k = 0; k < Epl; ++k, t += 6) ok = marg_block(g, P.pose_gidx[h.pl_p[k]], 3, P.lm_gidx[h.pl_l[k]], 2, t) && ok;
    if (!ok) return fail(GS_ERR_INVALID, "marginals: an edge's block lies outside the pattern of the factor (plan inconsistent)");
    int rc;
    if ((rc = marg_buffer(g, &M.sig, M.cap_sig, M.sig_doubles)) != GS_OK || (rc = marg_buffer(g, &M.dpiv, M.cap_piv, P.n_scalar)) != GS_OK ||
        (rc = marg_buffer(g, &M.d_sig_off, M.cap_fronts, S)) != GS_OK || (rc = marg_buffer(g, &M.d_tab, M.cap_out, M.n_out)) != GS_OK ||
        (rc = marg_buffer(g, &M.d_list, M.cap_list, (int64_t)M.sel_list.size())) != GS_OK) return rc;
    if ((rc = marg_buffer(g, &M.d_out, M.cap_dout, M.n_out)) != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(M.d_sig_off, M.sig_off.data(), (size_t)S * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
    if (!M.sel_list.empty()) HIP_TRY(hipMemcpyAsync(M.d_list, M.sel_list.data(), M.sel_list.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    if (M.n_out) HIP_TRY(hipMemcpyAsync(M.d_tab, tab.data(), (size_t)M.n_out * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // (tab is a host temporary)
    M.plan_version = g->plan_version;
    return GS_OK;
}
extern "C" int gs_compute_marginals(gs_graph *g, gs_marginals_info *info) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    g->marg.valid = false;
    if (info) { std::memset(info, 0, sizeof(*info)); info->struct_size = (int32_t)sizeof(*info); }
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (g->world > 1 || g->opt.force_shared_top > 0) return fail(GS_ERR_INVALID, "sharded graph: marginals need the whole factor on one device (not supported on sharded handles)");
    rc = ensure_ready(g); if (rc != GS_OK) return rc;
    if (g->plan.dist) return fail(GS_ERR_INVALID, "sharded graph: marginals need the whole factor on one device (not supported on sharded handles)");
    rc = marg_tables(g); if (rc != GS_OK) return rc;
    auto &M = g->marg;
    // the failure state of the iterations is put aside and restored: this call's codes are its own
    int32_t saved[4] = {0, 0, 0, 0}, ff[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(saved, g->d.fail, sizeof(saved), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    HIP_TRY(hipMemsetAsync(g->d.fail, 0, sizeof(saved), g->stream));
    const int ii = g->d.inject_iter, ic = g->d.inject_code; g->d.inject_iter = 0;      // (fault injection belongs to the iterations: kept armed for them)
    g->d.dpiv = M.dpiv;                                             // the LDL^T factor kernels write D (variant 4: L L^T, nothing to capture)
    hipEventRecord(g->ev[0], g->stream);
    enqueue_linearize(g);
    enqueue_factor_levels(g, g->sched.own, 0, 0);
    hipEventRecord(g->ev[1], g->stream);
    const int nlev = (int)g->sched.own.start.size() - 1;
    for (const auto &Lc : M.sel_launch) launch_selinv(g->d, M.d_sig_off, M.sig, M.d_list + Lc.first, Lc.count, Lc.max_f, g->stream);
    hipEventRecord(g->ev[2], g->stream);
    launch_sigma_gather(M.n_out, M.d_tab, M.sig, M.d_out, g->stream);
    hipEventRecord(g->ev[3], g->stream);
    g->d.dpiv = nullptr;
    M.out.resize((size_t)M.n_out);
    if (M.n_out) HIP_TRY(hipMemcpyAsync(M.out.data(), M.d_out, (size_t)M.n_out * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    hipEventRecord(g->ev[4], g->stream);
    HIP_TRY(hipMemcpyAsync(ff, g->d.fail, sizeof(ff), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    auto rearm = [&]() { g->d.inject_iter = ii; g->d.inject_code = ic; };     // (reset_failure disarms it)
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { reset_failure(g); rearm(); return fail(GS_ERR_HIP, std::string("marginals: ") + hipGetErrorString(e)); }
    if (ff[0] != 0) { rc = reset_failure(g); rearm(); if (rc != GS_OK) return rc; }
    rearm();
    HIP_TRY(hipMemcpyAsync(g->d.fail, saved, sizeof(saved), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // (saved is on this stack)
    if (info) {
        float a = 0, b = 0, c = 0, t = 0;
        hipEventElapsedTime(&a, g->ev[0], g->ev[1]); hipEventElapsedTime(&b, g->ev[1], g->ev[2]); hipEventElapsedTime(&c, g->ev[2], g->ev[3]); hipEventElapsedTime(&t, g->ev[0], g->ev[4]);
        info->numeric_failure = ff[0]; info->n_fronts = (int32_t)g->plan.fronts.size(); info->n_levels = nlev;
        info->sigma_bytes = M.sig_doubles * (int64_t)sizeof(double);
        info->ms_linearize_factor = a; info->ms_selinv = b; info->ms_extract = c; info->ms_total = t; }
    if (ff[0] == 2) { if (g->d.tree) fall_back_to_levels(g);
        return fail(GS_ERR_TIMEOUT, "marginals: a whole-tree launch gave up waiting for a front's flag; the handle now uses one launch per level (call again)"); }
    if (ff[0] != 0) return fail(GS_ERR_NUMERIC, "marginals: zero pivot, H is singular (no covariances)");
    M.valid = true; M.structure_version = g->h.structure_version; M.estimate_version = g->h.estimate_version; M.iter = g->d.iter;
    return GS_OK;
}
int marg_ready(gs_graph *g) {
    const auto &M = g->marg;
    if (!M.valid || !g->dev_valid || M.structure_version != g->h.structure_version || M.estimate_version != g->h.estimate_version || M.iter != g->d.iter)
        return fail(GS_ERR_NOT_INITIALIZED, "no marginals for the current graph and estimates: call gs_compute_marginals (results go stale after an "
                                            "iteration, gs_set_*_estimate, gs_add_*, a fixed flag or gs_clear)");
    return GS_OK;
}
static int marg_copy(gs_graph *g, int64_t first, int n, int per, int32_t cap, double *out) {
    int rc = marg_ready(g); if (rc != GS_OK) return rc;
    if (cap < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    if (n) std::memcpy(out, g->marg.out.data() + first, (size_t)n * per * sizeof(double));
    return n;
}
extern "C" int gs_get_pose_covariances(gs_graph *g, int32_t cap, int32_t *ids, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    const int n = g->h.n_poses();
    { int rc = marg_copy(g, 0, n, 9, cap, out); if (rc < 0) return rc; }
    if (ids && n) std::memcpy(ids, g->h.pose_id.data(), (size_t)n * sizeof(int32_t));
    return n;
}
extern "C" int gs_get_landmark_covariances(gs_graph *g, int32_t cap, int32_t *ids, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    const int n = g->h.n_lms();
    { int rc = marg_copy(g, 9 * (int64_t)g->h.n_poses(), n, 4, cap, out); if (rc < 0) return rc; }
    if (ids && n) std::memcpy(ids, g->h.lm_id.data(), (size_t)n * sizeof(int32_t));
    return n;
}
extern "C" int gs_get_odometry_edge_covariances(gs_graph *g, int32_t cap, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    return marg_copy(g, 9 * (int64_t)g->h.n_poses() + 4 * (int64_t)g->h.n_lms(), g->h.n_pp(), 9, cap, out);
}
extern "C" int gs_get_observation_edge_covariances(gs_graph *g, int32_t cap, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    return marg_copy(g, 9 * (int64_t)g->h.n_poses() + 4 * (int64_t)g->h.n_lms() + 9 * (int64_t)g->h.n_pp(), g->h.n_pl(), 6, cap, out);
}
extern "C" int gs_get_covariance_block(gs_graph *g, int32_t kind_a, int32_t id_a, int32_t kind_b, int32_t id_b, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    if ((kind_a != 0 && kind_a != 1) || (kind_b != 0 && kind_b != 1)) return fail(GS_ERR_INVALID, "kind must be 0 (pose) or 1 (landmark)");
    int rc = marg_ready(g); if (rc != GS_OK) return rc;
    auto vertex = [&](int kind, int32_t id, int &gidx, int &n) -> bool {
        const auto &ix = kind == 0 ? g->h.pose_index : g->h.lm_index;
        auto it = ix.find(id); if (it == ix.end()) return false;
        gidx = kind == 0 ? g->plan.pose_gidx[it->second] : g->plan.lm_gidx[it->second]; n = kind == 0 ? 3 : 2; return true; };
    int ga, na, gb, nb;
    if (!vertex(kind_a, id_a, ga, na) || !vertex(kind_b, id_b, gb, nb)) return fail(GS_ERR_UNKNOWN_ID, "unknown vertex id");
    int64_t off[9];
    if (!marg_block(g, ga, na, gb, nb, off))
        return fail(GS_ERR_OUT_OF_PATTERN, "the pair's block lies outside the pattern of the factor (no front holds both vertices): not computed by the selected inversion");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    for (int k = 0; k < na * nb; ++k) {
        out[k] = 0.0;
        if (off[k] >= 0) HIP_TRY(hipMemcpyAsync(out + k, g->marg.sig + off[k], sizeof(double), hipMemcpyDeviceToHost, g->stream)); }
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
