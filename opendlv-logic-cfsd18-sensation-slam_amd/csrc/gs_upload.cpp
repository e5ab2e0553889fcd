// gs_upload.cpp — a plan's way to HBM: the raw arrays that travel while the host builds the plan (upload_raw_begin), the plan itself
// (upload_graph, step by step), the append-only growth of that upload (upload_growth) and host-side estimate writes (push_estimates).
// Every table that goes up is built by gs_upload_host.hpp — once, for the full upload and for growth; this unit allocates, copies and
// launches.  The sequence of dev_alloc requests and the order of the stream's operations are part of the contract: the pool's
// footprint and its reuse across structure phases depend on the first, the results on the second.
#include "gs_private.hpp"
#include "gs_parallel.hpp"
#include "gs_upload_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

using namespace gs;

namespace {

// The device side of one upload: arrays out of the handle's pool (dev_alloc), asynchronous copies and fills on its stream.  The first
// error stays (rc, err) and every call behind it does nothing: a step asks ok() before it launches a kernel on what it allocated and
// ends with status()
struct DevWriter {
    gs_graph *g; const char *what; int rc = GS_OK; std::string err;
    DevWriter(gs_graph *g_, const char *what_) : g(g_), what(what_) {}
    bool ok() const { return rc == GS_OK; }
    int status() const { return ok() ? GS_OK : fail(rc, err); }
    void hip(hipError_t e) { if (e != hipSuccess) { rc = GS_ERR_HIP; err = std::string(what) + ": " + hipGetErrorString(e); } }
    template <class T> void alloc(T **p, size_t count) { *p = nullptr; if (ok() && (rc = dev_alloc(g, p, count)) != GS_OK) err = g_last_error; }
    void copy(void *dst, const void *src, size_t bytes) { if (ok() && bytes) hip(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g->stream)); }
    template <class T> void zero(T *p, size_t count) { if (ok()) hip(hipMemsetAsync(p, 0, std::max<size_t>(count, 1) * sizeof(T), g->stream)); }
    template <class T> void alloc_zero(T **p, size_t count) { alloc(p, count); zero(*p, count); }
    // a vector to an array of its own, with `room` more elements behind it
    template <class T, class A> void upload(T **p, const std::vector<T, A> &v, size_t room = 0) { alloc(p, v.size() + room); copy(*p, v.data(), v.size() * sizeof(T)); }
};

// upload_graph's steps share this
struct GraphUpload {
    gs_graph *g; RawUpload &raw; DevWriter w; StepTimer ut;
    ArenaCounts counts{}; ArenaOffsets arena{};
    std::vector<int32_t> lf;                                        // the level list: own fronts, then the shared top
    GraphUpload(gs_graph *g_, RawUpload &raw_) : g(g_), raw(raw_), w(g_, "upload"), ut(g_->opt.plan_timing > 0, "upload", 18), lf(level_list(g_->plan)) {}
};

}  // namespace

// Everything that does not depend on the plan goes to HBM on a helper thread WHILE the host builds the plan: estimates,
// fixed flags, odometry measurements (inverted, with their cos/sin: g2o keeps _inverseMeasurement) and information,
// and the observation edges as inserted (permuted into the ELL layout on the device afterwards).
int upload_raw_begin(gs_graph *g, RawUpload &R) {
    const HostGraph &h = g->h; DevGraph &d = g->d;
    const size_t N = h.n_poses(), M = h.n_lms(), Epp = h.n_pp(), Epl = h.n_pl();
    // room for the tail of a grown plan (gs::grow_plan) behind the per-pose and per-odometry-edge arrays
    const size_t TP = TAIL_POSES, TPP = TAIL_PP, TL = TAIL_LMS;
    DevWriter w(g, "raw upload");
    w.alloc(&d.pose_est, (N + TP) * 3); w.alloc(&d.lm_est, (M + TL) * 2); w.alloc(&d.pose_fixed, N + TP); w.alloc(&d.lm_fixed, M + TL);
    w.alloc(&d.pose_cs, (N + TP) * 2); w.alloc(&d.pp_zinv, (Epp + TPP) * 5); w.alloc(&d.pp_info, (Epp + TPP) * 6);
    if (!w.ok()) return w.status();
    HIP_TRY(hipMemsetAsync(d.pose_fixed + N, 0, TP, g->stream)); HIP_TRY(hipMemsetAsync(d.lm_fixed + M, 0, TL, g->stream));
    // the observation edges as inserted travel now only on a single GPU; a pose-window shard uploads the ones it evaluates, in
    // device layout, once the plan says which they are (upload_graph)
    const bool raw_pl = g->world <= 1;
    if (raw_pl) { w.alloc(&R.pl_l, Epl); w.alloc(&R.pl_z, Epl * 2); w.alloc(&R.pl_info, Epl * 3); if (!w.ok()) return w.status(); }
    R.th = std::thread([g, &R, N, M, Epp, Epl, raw_pl] {
        const HostGraph &h = g->h; DevGraph &d = g->d;
        if (hipSetDevice(g->device) != hipSuccess) { R.rc = GS_ERR_HIP; R.err = "hipSetDevice failed on the upload thread"; return; }
        DevWriter w(g, "raw upload");
        w.copy(d.pose_est, h.pose_est.data(), N * 3 * sizeof(double)); w.copy(d.lm_est, h.lm_est.data(), M * 2 * sizeof(double));
        w.copy(d.pose_fixed, h.pose_fixed.data(), N); w.copy(d.lm_fixed, h.lm_fixed.data(), M);
        if (raw_pl) { w.copy(R.pl_l, h.pl_l.data(), Epl * sizeof(int32_t)); w.copy(R.pl_z, h.pl_z.data(), Epl * 2 * sizeof(double));
            w.copy(R.pl_info, h.pl_info.data(), Epl * 3 * sizeof(double)); }
        // odometry edges keep their insertion order on the device.  A pose-window shard evaluates an odometry edge only if one of its poses lies in
        // the shard's window (gs_plan.cpp, rank_of_pp: the owner of an interior endpoint, else the window of the pose; an edge between two fixed
        // poses is rank 0's): the records of the first to the last such edge go up — an eighth of 0.8 M inverses, cosines, sines and of 70 MB at
        // world 8 (this thread took longer than the plan build).  upload_graph checks the plan's assignment against the range and sends what is missing.
        size_t k0 = 0, k1 = Epp;
        if (g->world > 1 && Epp > 0) {
            size_t nfree = 0; for (size_t p = 0; p < N; ++p) nfree += !h.pose_fixed[p];
            const size_t W = (size_t)g->world, r = (size_t)g->rank, f_lo = (r * nfree + W - 1) / W, f_hi = ((r + 1) * nfree + W - 1) / W;
            size_t p_lo = N, p_hi = N, f = 0;                        // insertion indices of the window's first free pose and of the next window's
            for (size_t p = 0; p < N; ++p) if (!h.pose_fixed[p]) { if (f == f_lo) p_lo = p; if (f == f_hi) { p_hi = p; break; } ++f; }
            auto in = [&](int32_t p) { return (size_t)p >= p_lo && (size_t)p < p_hi; };
            k0 = Epp; k1 = 0;
            for (size_t k = 0; k < Epp; ++k) { const int32_t i = h.pp_i[k], j = h.pp_j[k];
                if (in(i) || in(j) || (r == 0 && h.pose_fixed[i] && h.pose_fixed[j])) { k0 = std::min(k0, k); k1 = std::max(k1, k + 1); } }
            if (k1 <= k0) k0 = k1 = 0; }
        R.pp_lo = k0; R.pp_hi = k1;
        w.copy(d.pp_info + 6 * k0, h.pp_info.data() + 6 * k0, (k1 - k0) * 6 * sizeof(double));
        R.zinv.resize((k1 - k0) * 5);
        for (size_t k = k0; k < k1; ++k) zinv5(&h.pp_z[3 * k], &R.zinv[5 * (k - k0)]);
        w.copy(d.pp_zinv + 5 * k0, R.zinv.data(), (k1 - k0) * 5 * sizeof(double));
        R.rc = w.rc; R.err = w.err;
    });
    return GS_OK;
}

// the workgroup tables of the schedule (plans with a front of more than 63 scalars) go to the device with the plan; the copies read the
// handle's own vectors
int upload_tables(gs_graph *g) {
    DevWriter w(g, "upload");
    for (int t = 0; t < N_TABS; ++t) { g->d_wg[t] = nullptr;
        if (g->sched.big) w.upload((int32_t **)&g->d_wg[t], g->sched.tab[t].wg); }
    return w.status();
}

// ---- upload_graph, step by step.  Estimates, fixed flags, odometry edges and the insertion-order observation arrays are in HBM
// already (RawUpload).
static int up_estimates_and_edges(GraphUpload &U) {
    gs_graph *g = U.g; RawUpload &raw = U.raw; DevWriter &w = U.w; const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    const int N = d.N;
    launch_pose_trig(d, g->stream);
    // gs_debug_options.host_trig (an experiment, scripts/parity_spread.py): the cos / sin of the INITIAL pose angles from the host's libm
    // instead of the device's — what the CPU oracle linearises with — to tell how much of the first increment's distance
    // to the CPU paths is the last bit of two transcendental functions
    if (g->opt.host_trig > 0 && N > 0) {
        std::vector<double> cs(2 * (size_t)N);
        for (int p = 0; p < N; ++p) { cs[2 * (size_t)p] = std::cos(h.pose_est[3 * (size_t)p + 2]); cs[2 * (size_t)p + 1] = std::sin(h.pose_est[3 * (size_t)p + 2]); }
        HIP_TRY(hipMemcpyAsync(d.pose_cs, cs.data(), cs.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream)); }
    g->room = gs_graph::GrowRoom(); d.tN = d.tM = d.tEpp = d.tEpl = d.tLt = 0; d.tcapN = TAIL_POSES; d.tcapM = TAIL_LMS; d.tcapEpp = TAIL_PP; d.tcapEpl = TAIL_PL;
    w.upload(&d.pose_gidx, P.pose_gidx, TAIL_POSES);                // (room for a grown plan's tail poses)
    w.upload(&d.lm_gidx, P.lm_gidx, TAIL_LMS);
    d.ell_T = P.ell_T; d.ell_R = P.ell_R; d.ell_len = P.ell_len; d.ell_p0 = P.ell_p0; d.ell_np = P.ell_np;
    const size_t L = (size_t)P.ell_len;
    w.alloc(&d.ell_l, L); w.alloc(&d.ell_z, 2 * L); w.alloc(&d.ell_w, 3 * L);
    if (P.world <= 1) {                                              // ELL streams: permuted on the device out of the arrays that travelled during the plan build (k_build_ell)
        int32_t *ins = nullptr;
        w.upload(&ins, P.ell_ins);
        if (!w.ok()) return w.status();
        launch_build_ell((int64_t)L, ins, raw.pl_l, raw.pl_z, raw.pl_info, nullptr, P.rank, d.ell_l, d.ell_z, d.ell_w, g->stream);
        return GS_OK; }
    if (!w.ok()) return w.status();
    // pose-window shard: only the poses it sweeps are laid out; the streams are filled on the host
    // ... on a thread of its own, beside the rest of upload_graph (nothing there reads the streams; joined before the final wait): the fill
    // and three copies out of pageable memory were 2.5-5 of a rank's ~8 ms of upload at 8 x 100k poses
    raw.ell_l.resize(L); raw.ell_z.resize(2 * L); raw.ell_w.resize(3 * L);        // (threads) with the edges this rank evaluates, the others stay empty (l = -1)
    raw.th = std::thread([g, &raw, L] { const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
        if (hipSetDevice(g->device) != hipSuccess) { raw.rc = GS_ERR_HIP; raw.err = "hipSetDevice failed on the upload thread"; return; }
        parallel_chunks((int64_t)L, 16384, [&](int64_t b, int64_t e2, int) {
            for (int64_t e = b; e < e2; ++e) { int k = P.ell_ins[(size_t)e]; if (k >= 0 && P.pl_rank[k] != P.rank) k = -1;
                raw.ell_l[e] = k >= 0 ? h.pl_l[k] : -1;
                raw.ell_z[e] = k >= 0 ? h.pl_z[2 * (size_t)k] : 0.0; raw.ell_z[L + e] = k >= 0 ? h.pl_z[2 * (size_t)k + 1] : 0.0;
                raw.ell_w[e] = k >= 0 ? h.pl_info[3 * (size_t)k] : 0.0; raw.ell_w[L + e] = k >= 0 ? h.pl_info[3 * (size_t)k + 1] : 0.0;
                raw.ell_w[2 * L + e] = k >= 0 ? h.pl_info[3 * (size_t)k + 2] : 0.0; } });
        hipError_t e1 = hipMemcpyAsync(d.ell_l, raw.ell_l.data(), L * sizeof(int32_t), hipMemcpyHostToDevice, g->stream);
        hipError_t e2 = hipMemcpyAsync(d.ell_z, raw.ell_z.data(), 2 * L * sizeof(double), hipMemcpyHostToDevice, g->stream);
        hipError_t e3 = hipMemcpyAsync(d.ell_w, raw.ell_w.data(), 3 * L * sizeof(double), hipMemcpyHostToDevice, g->stream);
        if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { raw.rc = GS_ERR_HIP; raw.err = "edge streams: copy to the device failed"; } });
    return GS_OK;
}

static int up_linearisation_tiles(GraphUpload &U) {
    gs_graph *g = U.g; RawUpload &raw = U.raw; DevWriter &w = U.w; const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    w.upload(&d.lm_start, P.lm_start); w.upload(&d.lm_edges, P.lm_edges); w.upload(&d.ppadj_start, P.ppadj_start);
    { const std::vector<int32_t> inc = incidence_records(P);
      w.upload(&d.ppinc, inc);
      if (!w.ok()) return w.status();
      // a shard's helper thread sent the records of the odometry edges [pp_lo, pp_hi) — the ones that touch its window; an edge the plan gives
      // this rank outside that range (none, by the assignment rule: kept as a check that cannot go wrong silently) is sent now
      std::vector<int32_t> miss;
      for (size_t q = 0; q < inc.size() / 2; ++q) { const int32_t k = inc[2 * q]; if (k >= 0 && ((size_t)k < raw.pp_lo || (size_t)k >= raw.pp_hi)) miss.push_back(k); }
      std::sort(miss.begin(), miss.end()); miss.erase(std::unique(miss.begin(), miss.end()), miss.end());
      for (int32_t k : miss) { double o[5]; zinv5(&h.pp_z[3 * (size_t)k], o);
          HIP_TRY(hipMemcpy(d.pp_zinv + 5 * (size_t)k, o, sizeof(o), hipMemcpyHostToDevice));
          HIP_TRY(hipMemcpy(d.pp_info + 6 * (size_t)k, &h.pp_info[6 * (size_t)k], 6 * sizeof(double), hipMemcpyHostToDevice)); }
      g->pp_records_late = (int)miss.size();
      if (U.ut.on && !miss.empty()) std::fprintf(stderr, "upload: %d odometry edge records sent after the plan\n", (int)miss.size()); }
    d.n_wtiles = 0; d.n_groups = 0; d.wt_lo = 0; d.wt_hi = 0; d.rank = P.rank;
    // the fused kernel addresses the ELL planes with 32-bit byte offsets: 8 B * ell_len must stay below 4 GiB
    if (P.lin_ell_ok && !g->force_gather && P.ell_len < ((int64_t)1 << 29)) {
        d.n_wtiles = P.n_wtiles; d.n_groups = (int32_t)P.grp_lm.size();
        w.upload(&d.wt_desc, P.wt_desc); w.upload(&d.lm_grp_start, P.lm_grp_start);
        w.upload(&d.grp_tab, group_table(P));
        w.upload(&d.ell_dst, P.ell_dst);
        d.wt_lo = P.wt_lo; d.wt_hi = P.wt_hi;                             // the wave tiles this shard has any edge in (gs_plan.cpp)
    } else if (P.world > 1) return fail(GS_ERR_INVALID, "pose-window shards need the fused linearisation layout (<= 32 observations per pose)");
    return w.status();
}

// block-sparse H and b live in ONE arena (the variant-3 front assembly addresses every scalar by its offset in it); the tail's tables
static int up_arena_and_tail(GraphUpload &U) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d;
    U.counts = ArenaCounts{d.N, d.Epp, P.ell_len, d.n_groups, d.M, TAIL_POSES, TAIL_PP, TAIL_PL, TAIL_LMS};
    if (!arena_layout(U.counts, U.arena)) return fail(GS_ERR_INVALID, "graph too large for 32-bit arena offsets");
    w.alloc_zero(&d.H_arena, (size_t)U.arena.doubles() + 2);        // blocks of edges / tiles this rank never evaluates must read as zero
    auto part = [&](ArenaPart p) { return d.H_arena + U.arena.at[p]; };
    d.t_Hpp_diag = part(ARENA_t_Hpp_diag); d.t_b_pose = part(ARENA_t_b_pose); d.t_Hpp_off = part(ARENA_t_Hpp_off); d.t_Hpl = part(ARENA_t_Hpl);
    d.t_Hll_diag = part(ARENA_t_Hll_diag); d.t_b_lm = part(ARENA_t_b_lm);
    w.alloc(&d.t_pp_ij, (size_t)TAIL_PP * 2); w.alloc(&d.t_pl, (size_t)TAIL_PL * 2); w.alloc(&d.t_pl_z, (size_t)TAIL_PL * 2); w.alloc(&d.t_pl_w, (size_t)TAIL_PL * 3);
    w.alloc(&d.t_pose_start, (size_t)TAIL_POSES + 1); w.alloc(&d.t_pose_edges, (size_t)TAIL_PL); w.alloc(&d.t_lt_id, (size_t)TAIL_PL);
    w.alloc(&d.t_lt_start, (size_t)TAIL_PL + 1); w.alloc(&d.t_lt_edges, (size_t)TAIL_PL);
    d.Hpp_diag = part(ARENA_Hpp_diag); d.b_pose = part(ARENA_b_pose); d.Hpp_off = part(ARENA_Hpp_off);
    d.Hpl = part(ARENA_Hpl); d.lm_part = part(ARENA_lm_part); d.Hll_diag = part(ARENA_Hll_diag); d.b_lm = part(ARENA_b_lm);
    d.n_chi2_partial = std::max((d.N + 255) / 256, d.n_wtiles);
    w.alloc(&d.chi2_partial, d.n_chi2_partial + 1); w.alloc(&d.chi2, 80); w.zero(d.chi2_partial, d.n_chi2_partial + 1);     // (+1: the partial of a grown plan's tail)
    w.upload(&d.pose_known, P.pose_known); w.upload(&d.lm_known, P.lm_known);
    return w.status();
}

// fronts, boundary rows, child maps and assembly records — the last three with room behind them: a growth step re-writes the runs of
// the fronts it changes there
static int up_plan_arrays(GraphUpload &U) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d;
    { std::vector<DevFront> df(P.fronts.size());
      for (size_t s = 0; s < P.fronts.size(); ++s) df[s] = dev_front(P.fronts[s]);
      w.upload(&d.fronts, df); d.n_fronts = (int32_t)df.size(); }
    const size_t rows = room_rows(P), recs = room_recs(P);
    w.upload(&d.bnd_rows, P.bnd_rows, rows); w.upload(&d.child_map, P.child_map, rows);
    g->room.cap_bnd = (int64_t)(P.bnd_rows.size() + rows); g->room.cap_map = (int64_t)(P.child_map.size() + rows);
    w.upload(&d.children, P.children);
    w.upload(&d.child_desc, child_desc(P));
    w.upload(&d.level_fronts, U.lf);
    d.xfail_off = -1; d.iter = 0; d.inject_iter = 0; d.inject_code = 0;
    if (P.dist) { w.upload(&d.x_off, P.x_off);
        d.xfail_off = P.exchange_doubles - 2;                             // the ranks' failure flags ride at the tail of the exchange buffer
        if (!g->exchange_external) w.alloc_zero(&d.exchange, P.exchange_doubles);
        else d.exchange = g->exchange; }
    static_assert(sizeof(AsmRec) == 16, "AsmRec is uploaded as 4 int32");
    w.alloc(&d.asm_recs, (P.asm_recs.size() + recs) * 4);
    w.copy(d.asm_recs, P.asm_recs.data(), P.asm_recs.size() * sizeof(AsmRec));
    g->room.cap_asm = (int64_t)(P.asm_recs.size() + recs);
    return w.status();
}

// variant 3: the update matrices' slots, the completion flags and tickets of the whole-tree launches, and the block assembly records
// as the device expands them: the plan's, as they are (AsmRec = 4 ints); landmark-diagonal records of the fused linearisation get
// their partial-slot range patched in by a kernel
static int up_update_matrices_and_asm3(GraphUpload &U, bool fused) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d;
    std::vector<int32_t> u3_off(P.fronts.size()), u3_size(P.fronts.size());
    int64_t tot = 0;
    for (size_t s = 0; s < P.fronts.size(); ++s) { u3_off[s] = (int32_t)tot; u3_size[s] = u3_slot_size(P.fronts[s].nbnd); tot += u3_slot_advance(u3_size[s]);
        if (tot >= ((int64_t)1 << 31)) return fail(GS_ERR_INVALID, "update-matrix arena beyond 32-bit offsets"); }
    const int64_t room = room_U(P, tot);
    if (tot + room >= ((int64_t)1 << 31)) return fail(GS_ERR_INVALID, "update-matrix arena beyond 32-bit offsets");
    w.alloc_zero(&d.Uimg, (size_t)(tot + room) + 2);
    g->room.used_U = tot; g->room.cap_U = tot + room;
    w.upload(&d.u3_off, u3_off); w.upload(&d.u3_size, u3_size);
    g->u3_off_host = u3_off; g->u3_size_host = u3_size;
    w.alloc_zero(&d.done_f, P.fronts.size());
    d.tickets = nullptr; d.ticket_base = 0;
    if (g->opt.tickets != 0) w.alloc_zero(&d.tickets, 2);           // workgroups of the whole-tree launches take their number from this counter (gs_kernels.hip, "tickets")
    d.epoch = 0; d.tree = g->opt.tree != 0 ? 1 : 0; g->fell_back = false; g->fallback_calls = 0; g->fallback_retry_after = 4; g->fallback_retrying = false;   // whole-tree launches for this rank's own subtrees (gs_debug_options.tree = 0: one launch per level)
    // ---- everything below is expanded ON THE DEVICE from the compact plan arrays
    w.alloc(&d.asm3, (P.asm_recs.size() + room_recs(P)) * 4);
    w.copy(d.asm3, P.asm_recs.data(), P.asm_recs.size() * sizeof(AsmRec));
    if (!w.ok()) return w.status();
    if (fused) { for (int l = 0; l < d.M; ++l) if (P.lm_grp_start[l + 1] - P.lm_grp_start[l] >= (1 << 22)) return fail(GS_ERR_INVALID, "landmark seen from too many wave tiles");
        launch_patch_asm3((int64_t)P.asm_recs.size(), d.asm3, d.lm_grp_start, g->stream); }
    U.ut("asm3");
    return GS_OK;
}

// scalar assembly records {offset in H_arena, offset in the staging image}, padded per front to a multiple of 64 with (0 -> image
// offset 1, a don't-care upper-triangle slot); fused landmark diagonals go to lm3.  The host only counts them per front (bf).
static int up_scalar_records(GraphUpload &U, bool fused) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d;
    const size_t S = P.fronts.size();
    std::vector<RecCount> cnt(S);
    parallel_chunks((int64_t)S, 2048, [&](int64_t b, int64_t e, int) { for (int64_t s = b; s < e; ++s) cnt[s] = front_record_count(P, P.fronts[s], fused); });
    std::vector<int32_t> bf(BF_INTS * S, 0);
    int64_t so = 0, lo = 0;
    for (size_t s = 0; s < S; ++s) {
        if (so >= ((int64_t)1 << 31) - 64) return fail(GS_ERR_INVALID, "too many assembly scalars");
        bf_row(P.fronts[s], cnt[s], so, lo, &bf[BF_INTS * s]); so += cnt[s].padded(); lo += cnt[s].nl; }
    const int64_t room = room_sc(P, so);
    if (so + room >= ((int64_t)1 << 31) - 64) return fail(GS_ERR_INVALID, "too many assembly scalars");
    w.alloc(&d.sc3, 2 * (size_t)(so + room) + 2); w.alloc(&d.lm3, 4 * (size_t)lo + 4);
    g->room.used_sc = so; g->room.cap_sc = so + room;
    w.upload(&g->d_bf, bf);
    if (!w.ok()) return w.status();
    g->bf_host = bf;
    g->sc3_args = sc3_args(U.arena, U.counts, fused);
    launch_build_sc3(g->d_bf, d.asm3, d.sc3, d.lm3, (int)S, g->sc3_args, g->stream);
    U.ut("sc3 build");
    return GS_OK;
}

// descriptors + children tables: one wave per level position (k_build_f3); the staging of a growth step's patch
static int up_front_tables(GraphUpload &U, bool fused) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d; const std::vector<int32_t> &lf = U.lf;
    constexpr int F3W = 224;                                        // 32 descriptor ints + the row tables of the first two children + the front's own store table
    d.f3x_stride = f3x_stride(P);
    std::vector<int32_t> xrow;
    if (!children_row_offsets(P, lf, xrow)) return fail(GS_ERR_INVALID, "children table too large");
    w.upload(&g->d_xrow, xrow);
    g->pos_of_front = pos_of_front(P, lf);
    w.upload(&g->d_posof, g->pos_of_front);                         // front -> level position: into the children's headers (k_factor3_sub finds a leaf's descriptor through it)
    w.alloc(&g->d_patch, (size_t)1024 * PATCH_INTS); w.alloc(&g->d_list, (size_t)2048);
    w.alloc(&d.f3_desc, lf.size() * (size_t)F3W); w.alloc(&d.f3_x, (size_t)xrow[lf.size()] + 168);
    if (!w.ok()) return w.status();
    launch_build_f3((int)lf.size(), d.level_fronts, d.fronts, d.children, d.child_map, d.u3_off, d.u3_size, g->d_bf, g->d_xrow,
                    P.dist ? d.x_off : nullptr, d.f3_desc, d.f3_x, d.f3x_stride, g->stream, nullptr, g->d_posof);
    // a growth step needs all of the above: variant 3, one GPU, the fused linearisation layout
    g->room.ok = !P.dist && fused;
    U.ut("f3 tables");
    return GS_OK;
}

// factor and solve buffers; the solver launches of this plan, decided here once (gs_schedule.hpp); the global workspace for fronts
// beyond the LDS limit, one slice per block; the workgroup tables of a plan with fronts beyond a wave
static int up_solver_buffers(GraphUpload &U) {
    gs_graph *g = U.g; DevWriter &w = U.w; const Plan &P = g->plan; DevGraph &d = g->d;
    const size_t NP = (size_t)d.N + TAIL_POSES, ML = (size_t)d.M + TAIL_LMS;
    w.alloc_zero(&d.dbg_ts, 64);
    w.alloc_zero(&d.done_ts, 2 * P.fronts.size() + 2);
    const int64_t room = g->room.ok ? room_L(P) : 0;
    w.alloc(&d.Lbuf, P.l_doubles + room); g->room.cap_L = P.l_doubles + room;
    w.alloc(&d.Ubuf, d.factor_variant == 0 ? P.u_doubles : 1);     // variant 3 keeps its update matrices in Uimg
    w.alloc(&d.xe, P.n_scalar + 3 * TAIL_POSES + 2 * TAIL_LMS); g->room.cap_xe = P.n_scalar + 3 * TAIL_POSES + 2 * TAIL_LMS;
    w.alloc(&d.dpose, NP * 3); w.alloc(&d.dlm, ML * 2); w.alloc(&d.fail, 4);
    if (!w.ok()) return w.status();
    HIP_TRY(hipMemsetAsync(d.fail, 0, 4 * sizeof(int32_t), g->stream));
    HIP_TRY(hipMemsetAsync(d.chi2, 0, 80 * sizeof(double), g->stream));
    HIP_TRY(hipMemsetAsync(d.dpose, 0, NP * 3 * sizeof(double), g->stream));
    HIP_TRY(hipMemsetAsync(d.dlm, 0, ML * 2 * sizeof(double), g->stream));
    g->sched = build_schedule(P, g->pos_of_front, d.factor_variant, g->opt.tree != 0, g->opt);
    d.front_ws_stride = g->sched.front_ws_stride;
    if (g->sched.ws_blocks > 0) { w.alloc(&d.front_ws, d.front_ws_stride * g->sched.ws_blocks); if (!w.ok()) return w.status(); }
    return upload_tables(g);
}

int upload_graph(gs_graph *g, RawUpload &raw) {
    const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    GraphUpload U(g, raw);
    d.N = h.n_poses(); d.M = h.n_lms(); d.Epp = h.n_pp(); d.Epl = h.n_pl(); d.n_scalar = P.n_scalar;
    int rc;
    if ((rc = up_estimates_and_edges(U)) != GS_OK) return rc;
    U.ut("estimates+edges");
    if ((rc = up_linearisation_tiles(U)) != GS_OK || (rc = up_arena_and_tail(U)) != GS_OK) return rc;
    U.ut("tiles+arena");
    if ((rc = up_plan_arrays(U)) != GS_OK) return rc;
    U.ut("plan arrays");
    // factor kernel variant (gs_config.factor_variant; gs_debug_options.factor_variant overrides): 0 = default = 3 when every
    // front fits 159 scalars, else 4.  3 = LDL^T on the fp64 matrix cores, a wave or a workgroup per front; 4 = block-per-front
    // VALU Cholesky (any front size).
    const int v = d.factor_variant = plan_factor_variant(g, U.arena.doubles());
    d.dbg = g->opt.dbg; d.leaf_nt3 = g->opt.leaf_nt3 != 0 ? 1 : 0; d.f3_lds_kb = std::max(g->opt.f3_lds_kb, 0);
    if (v == 3) { const bool fused = P.lin_ell_ok && d.n_wtiles > 0;
        if ((rc = up_update_matrices_and_asm3(U, fused)) != GS_OK || (rc = up_scalar_records(U, fused)) != GS_OK || (rc = up_front_tables(U, fused)) != GS_OK) return rc; }
    U.ut("f3 x+desc upload");
    if ((rc = up_solver_buffers(U)) != GS_OK) return rc;
    U.ut("arenas+levels");
    if (raw.th.joinable()) { raw.th.join(); if (raw.rc != GS_OK) return fail(raw.rc, raw.err); }      // a shard's edge streams (up_estimates_and_edges)
    HIP_TRY(hipStreamSynchronize(g->stream));
    U.ut("final sync");
    g->dev_valid = true; g->linearised = false; g->dev_estimates_newer = false; g->tree_proven = false;
    ++g->value_uploads;                                              // every edge's own information is on the device again (edge_mask_sync)
    g->dev_estimate_version = h.estimate_version;
    return GS_OK;
}

namespace {
// what a growth step stages on the host: it lives until upload_growth has waited for the stream
struct GrowthStaging { std::vector<int32_t> patch, poslist, ppij, plpl; std::vector<double> zinv; TailGroups tail; };
}  // namespace

// update-matrix slots and scalar-record runs of the changed fronts, behind the used room: their patch records and level positions
static int growth_patch(gs_graph *g, const Growth &gr, GrowthStaging &S, int64_t &used_U, int64_t &used_sc) {
    const Plan &P = g->plan; const int nf = (int)gr.fronts.size(); const bool fused = g->sc3_args.fused != 0;
    S.patch.assign((size_t)nf * PATCH_INTS, 0); S.poslist.resize(nf);
    for (int i = 0; i < nf; ++i) { const int s = gr.fronts[i]; int32_t *r = &S.patch[(size_t)i * PATCH_INTS];
        patch_record(P, s, fused, used_U, used_sc, g->bf_host[BF_INTS * (size_t)s + 5], r);
        const int32_t usz = r[PATCH_U3_SIZE], sc_cnt = r[PATCH_BF + 4];
        if (used_U + usz + 4 > g->room.cap_U || used_sc + sc_cnt > g->room.cap_sc) return fail(GS_ERR_CAPACITY, "growth: room behind the update matrices / scalar records used up");
        used_U += u3_slot_advance(usz); used_sc += sc_cnt;
        S.poslist[i] = g->pos_of_front[s];
        if (S.poslist[i] < 0) return fail(GS_ERR_INVALID, "growth: front without a level position"); }
    return GS_OK;
}

// the new vertices' and edges' data into the tail arrays; the tail's edges grouped by pose and by touched landmark (the whole tail, not
// only this step's part)
static void growth_tail_data(gs_graph *g, const Growth &gr, GrowthStaging &S, DevWriter &w) {
    const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    const int N0 = gr.first_pose, N1 = P.planned_N, M0 = gr.first_lm, M1 = P.planned_M, E0 = gr.first_pp, E1 = P.planned_Epp, K0 = gr.first_pl, K1 = P.planned_Epl;
    w.copy(d.pose_est + 3 * (size_t)N0, &h.pose_est[3 * (size_t)N0], (size_t)(N1 - N0) * 3 * sizeof(double));
    w.copy(d.pose_gidx + N0, &P.pose_gidx[N0], (size_t)(N1 - N0) * sizeof(int32_t));
    if (M1 > M0) { w.copy(d.lm_est + 2 * (size_t)M0, &h.lm_est[2 * (size_t)M0], (size_t)(M1 - M0) * 2 * sizeof(double));     // landmarks first seen by the new poses
        w.copy(d.lm_gidx + M0, &P.lm_gidx[M0], (size_t)(M1 - M0) * sizeof(int32_t)); }
    if (g->dev_estimate_version != h.estimate_version) {          // a host-side setEstimate on an OLDER vertex since the last upload (g2o: setEstimate, then
        w.copy(d.pose_est, h.pose_est.data(), (size_t)N1 * 3 * sizeof(double));   // optimize() uses the new value): the whole estimate arrays go up again, not only the tail's
        w.copy(d.lm_est, h.lm_est.data(), (size_t)M1 * 2 * sizeof(double));
        if (w.ok()) launch_pose_trig_range(d, 0, N1, g->stream);
    } else if (w.ok()) launch_pose_trig_range(d, N0, N1 - N0, g->stream);
    S.zinv.resize((size_t)(E1 - E0) * 5); S.ppij.resize((size_t)(E1 - E0) * 2);
    for (int k = E0; k < E1; ++k) { zinv5(&h.pp_z[3 * (size_t)k], &S.zinv[5 * (size_t)(k - E0)]);
        S.ppij[2 * (size_t)(k - E0)] = h.pp_i[k]; S.ppij[2 * (size_t)(k - E0) + 1] = h.pp_j[k]; }
    w.copy(d.pp_zinv + 5 * (size_t)E0, S.zinv.data(), S.zinv.size() * sizeof(double));
    w.copy(d.pp_info + 6 * (size_t)E0, &h.pp_info[6 * (size_t)E0], (size_t)(E1 - E0) * 6 * sizeof(double));
    w.copy(d.t_pp_ij + 2 * (size_t)(E0 - P.base_Epp), S.ppij.data(), S.ppij.size() * sizeof(int32_t));
    S.plpl.resize((size_t)(K1 - K0) * 2);
    for (int k = K0; k < K1; ++k) { S.plpl[2 * (size_t)(k - K0)] = h.pl_p[k]; S.plpl[2 * (size_t)(k - K0) + 1] = h.pl_l[k]; }
    const size_t s0 = (size_t)(K0 - P.base_Epl);
    w.copy(d.t_pl + 2 * s0, S.plpl.data(), S.plpl.size() * sizeof(int32_t));
    w.copy(d.t_pl_z + 2 * s0, h.pl_z.data() + 2 * (size_t)K0, (size_t)(K1 - K0) * 2 * sizeof(double));
    w.copy(d.t_pl_w + 3 * s0, h.pl_info.data() + 3 * (size_t)K0, (size_t)(K1 - K0) * 3 * sizeof(double));
    tail_groups(h, P, S.tail);
    d.tLt = (int32_t)S.tail.lt_id.size();
    auto ints = [&](int32_t *dst, const std::vector<int32_t> &v) { w.copy(dst, v.data(), v.size() * sizeof(int32_t)); };
    ints(d.t_pose_start, S.tail.pose_start); ints(d.t_pose_edges, S.tail.pose_edges);
    ints(d.t_lt_id, S.tail.lt_id); ints(d.t_lt_start, S.tail.lt_start); ints(d.t_lt_edges, S.tail.lt_edges);
}

// the re-written runs behind the plan arrays, the changed fronts' rows of the compact tables, then the device-side expansion for
// those fronts: scalar records, then descriptors + children tables (a changed front's parent is a changed front too: its copy of the
// child's row table is rebuilt with it)
static void growth_front_tables(gs_graph *g, const Growth &gr, const GrowthStaging &S, DevWriter &w) {
    const Plan &P = g->plan; DevGraph &d = g->d; const int nf = (int)gr.fronts.size();
    w.copy(d.bnd_rows + gr.bnd_from, &P.bnd_rows[(size_t)gr.bnd_from], (P.bnd_rows.size() - (size_t)gr.bnd_from) * sizeof(int32_t));
    w.copy(d.child_map + gr.map_from, &P.child_map[(size_t)gr.map_from], (P.child_map.size() - (size_t)gr.map_from) * sizeof(int32_t));
    const size_t na = P.asm_recs.size() - (size_t)gr.asm_from;
    if (na) { w.copy(d.asm_recs + 4 * gr.asm_from, &P.asm_recs[(size_t)gr.asm_from], na * sizeof(AsmRec));
        w.copy(d.asm3 + 4 * gr.asm_from, &P.asm_recs[(size_t)gr.asm_from], na * sizeof(AsmRec));
        if (w.ok() && g->sc3_args.fused) launch_patch_asm3((int64_t)na, d.asm3 + 4 * gr.asm_from, d.lm_grp_start, g->stream); }
    w.copy(g->d_patch, S.patch.data(), S.patch.size() * sizeof(int32_t));
    if (w.ok()) launch_apply_front_patch(nf, g->d_patch, d.fronts, d.u3_off, d.u3_size, g->d_bf, g->stream);
    w.copy(g->d_list, gr.fronts.data(), (size_t)nf * sizeof(int32_t));
    w.copy(g->d_list + 1024, S.poslist.data(), (size_t)nf * sizeof(int32_t));
    if (!w.ok()) return;
    launch_build_sc3(g->d_bf, d.asm3, d.sc3, d.lm3, nf, g->sc3_args, g->stream, g->d_list);
    launch_build_f3(nf, d.level_fronts, d.fronts, d.children, d.child_map, d.u3_off, d.u3_size, g->d_bf, g->d_xrow, nullptr, d.f3_desc, d.f3_x, d.f3x_stride, g->stream, g->d_list + 1024, g->d_posof);
}

// ---- append-only growth on the device (after gs::grow_plan changed the host plan): the new poses' and edges' data into the tail
// arrays, the re-written runs of the changed fronts behind the plan arrays, those fronts' rows of the compact tables through one
// patch buffer, then the device-side expansion (k_build_sc3, k_build_f3) for those fronts only.  Everything older stays where it
// is.  Returns GS_ERR_CAPACITY when the room left by the full structure phase is used up (the caller rebuilds).
int upload_growth(gs_graph *g, const Growth &gr) {
    const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    if (!g->room.ok || d.factor_variant != 3) return fail(GS_ERR_CAPACITY, "growth: this plan was not uploaded with room to grow");
    const int nf = (int)gr.fronts.size();
    if (nf > 1024 || (int64_t)P.bnd_rows.size() > g->room.cap_bnd || (int64_t)P.child_map.size() > g->room.cap_map ||
        (int64_t)P.asm_recs.size() > g->room.cap_asm || P.l_doubles > g->room.cap_L || P.n_scalar > g->room.cap_xe)
        return fail(GS_ERR_CAPACITY, "growth: room behind the plan arrays used up");
    GrowthStaging S; int64_t used_U = g->room.used_U, used_sc = g->room.used_sc;
    int rc = growth_patch(g, gr, S, used_U, used_sc); if (rc != GS_OK) return rc;
    // ---- from here on the device changes
    DevWriter w(g, "growth upload");
    growth_tail_data(g, gr, S, w);
    growth_front_tables(g, gr, S, w);
    if (!w.ok()) return w.status();
    d.n_scalar = P.n_scalar; d.tN = P.planned_N - P.base_N; d.tM = P.planned_M - P.base_M; d.tEpp = P.planned_Epp - P.base_Epp; d.tEpl = P.planned_Epl - P.base_Epl;
    HIP_TRY(hipStreamSynchronize(g->stream));                       // the staging vectors go out of scope
    { hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("growth: ") + hipGetErrorString(e)); }
    // host mirrors and launch parameters
    for (int i = 0; i < nf; ++i) { const int s = gr.fronts[i]; const int32_t *r = &S.patch[(size_t)i * PATCH_INTS];
        g->u3_off_host[s] = r[PATCH_U3_OFF]; g->u3_size_host[s] = r[PATCH_U3_SIZE]; for (int c = 0; c < BF_INTS; ++c) g->bf_host[BF_INTS * (size_t)s + c] = r[PATCH_BF + c]; }
    g->room.used_U = used_U; g->room.used_sc = used_sc;
    // the launch geometry is chosen again from the grown fronts: level maxima, leaf instance and its LDS slot, the workgroup tables (a
    // grown front may change its size class).  The old tables stay in the pool until the next full structure phase.
    g->sched = build_schedule(P, g->pos_of_front, d.factor_variant, g->opt.tree != 0, g->opt);
    if ((rc = upload_tables(g)) != GS_OK) return rc;
    g->tree_proven = false; g->linearised = false;                  // (the tail arenas hold nothing of the new edges yet)
    g->dev_estimate_version = h.estimate_version;
    return GS_OK;
}

// host-side setEstimate since the upload: the estimates (and the poses' cos / sin) to the device of the current plan
int push_estimates(gs_graph *g) {
    if (g->dev_estimate_version == g->h.estimate_version) return GS_OK;
    const int N = g->d.N + g->d.tN, M = g->d.M + g->d.tM;
    if (N > 0) HIP_TRY(hipMemcpyAsync(g->d.pose_est, g->h.pose_est.data(), (size_t)N * 3 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    if (M > 0) HIP_TRY(hipMemcpyAsync(g->d.lm_est, g->h.lm_est.data(), (size_t)M * 2 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    launch_pose_trig(g->d, g->stream);
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->dev_estimate_version = g->h.estimate_version; g->dev_estimates_newer = false;
    return GS_OK;
}
