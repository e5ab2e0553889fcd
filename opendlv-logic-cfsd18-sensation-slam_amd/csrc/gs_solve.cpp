// gs_solve.cpp — the solver launches of one iteration and the entry points that run iterations (gs_iterate, gs_optimize*,
// gs_optimize_lm, gs_optimize_dogleg), with the timing and export hooks (gs_export_system, gs_multiply_hessian, ...).
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_hmul.hpp"
#include "gs_export_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

// ------------------------------------------------------------------ one Gauss-Newton iteration (A5-A9)
// The launches an iteration is made of are decided with the plan (gs_schedule.hpp: build_schedule, walk_*); nothing is decided here:
// this sink hands each launch of the walk to its launcher on the handle's stream
namespace {
struct Launcher {
    gs_graph *g;
    void epoch() { ++g->d.epoch; }
    void factor_tree(int n_leaf, int leaf_slot, int leaf_max_f, int count, int n_block, int sub_first, int n_sub) { launch_factor_tree(g->d, n_leaf, leaf_slot, leaf_max_f, count, n_block, sub_first, n_sub, g->stream); }
    void factor_level(int off, int count, int max_f, int mode) { launch_factor_level(g->d, off, count, max_f, mode, g->stream); }
    void factor_tree_top(int first, int count) { launch_factor_tree_top(g->d, first, count, g->stream); }
    void factor_tab(int t, int first, int n, int leaf_pre, size_t lds, int cls, int mode) { launch_factor_tab(g->d, g->d_wg[t] + first, n, leaf_pre, lds, cls, g->stream, mode); }
    void backsolve_tree(int first, int count, int max_npiv, int max_f) { launch_backsolve_tree(g->d, first, count, max_npiv, max_f, g->stream); }
    void backsolve_low(int first, int count, int n_up, int up_fronts, int up_slot, int slot, size_t lds) { launch_backsolve_low(g->d, first, count, n_up, up_fronts, up_slot, slot, lds, g->stream); }
    void backsolve_level(int off, int count, int max_npiv, int max_nbnd) { launch_backsolve_level(g->d, off, count, max_npiv, max_nbnd, g->stream); }
    void backsolve_tab(int t, int first, int n, int max_npiv_small, int max_f_small, size_t lds, int cls) { launch_backsolve_tab(g->d, g->d_wg[t] + first, n, max_npiv_small, max_f_small, lds, cls, g->stream); }
};
}  // namespace
void enqueue_factor_levels(gs_graph *g, const LevelSet &ls, int base, int mode) { Launcher L{g}; walk_factor_levels(g->sched, g->d.tree != 0, ls, base, mode, L); }
// linearise -> tail -> priors -> polar edges.  The prior total of chi2 goes where this pass's total is formed from: a partial k_update / k_linearize_finalize
// sum (fused kernel), or chi2[0] (gather kernels: k_reduce_chi2 has totalled it); the polar pass adds its total to the same slot.  A handle
// without priors and without polar edges launches what it always did
void enqueue_linearize(gs_graph *g, hipEvent_t start, hipEvent_t stop) {
    g->linearised = true;
    launch_linearize(g->d, g->stream, start, stop);
    launch_linearize_tail(g->d, g->stream);                          // a grown plan's tail (no launch without one)
    const bool fused = g->d.n_wtiles > 0;
    if (fused && g->d.wt_hi <= g->d.wt_lo && (prior_grid(g->prior.dev) > 0 || polar_grid(g->polar.dev) > 0))      // no wave tile swept, no launch above: nobody has written the slot the pass adds to
        hipMemsetAsync(g->d.chi2_partial, 0, sizeof(double), g->stream);
    launch_prior_pass(g->d, g->prior.dev, true, fused ? g->d.chi2_partial : g->d.chi2, g->stream);
    launch_polar_pass(g->d, g->polar.dev, true, fused ? g->d.chi2_partial : g->d.chi2, g->stream);      // (returns on an empty table)
}
void enqueue_chi2(gs_graph *g) {
    launch_chi2_only(g->d, g->stream);
    launch_prior_pass(g->d, g->prior.dev, false, g->d.chi2, g->stream);
    launch_polar_pass(g->d, g->polar.dev, false, g->d.chi2, g->stream);
}
// pose-window shards, first half: linearise this shard's edges, factorise its own subtrees, write its contribution
// to every shared front into the exchange buffer (the caller all-reduces that buffer: RCCL sum, fp64)
void enqueue_local(gs_graph *g, bool timed) {
    ++g->d.iter;                                                     // kernels see the iteration they belong to (fault injection, gs_debug_fail_at_iteration)
    if (timed) hipEventRecord(g->ev[0], g->stream);
    enqueue_linearize(g, g->ev_lin[0], g->ev_lin[1]);                // (null outside gs_time_iterations' second pass)
    if (timed) hipEventRecord(g->ev[1], g->stream);
    Launcher L{g}; walk_local(g->sched, g->d.tree != 0, L);
}
// second half: the shared top (redundantly on every rank), backward solve top-down, update
void enqueue_finish(gs_graph *g, bool timed) {
    Launcher L{g}; const bool tree = g->d.tree != 0;
    walk_finish_factor(g->sched, tree, L);
    if (timed) hipEventRecord(g->ev[2], g->stream);
    walk_finish_backsolve(g->sched, tree, L);
    if (timed) hipEventRecord(g->ev[3], g->stream);
    launch_update(g->d, g->stream);
    if (timed) hipEventRecord(g->ev[4], g->stream);
    g->dev_estimates_newer = true;
}
static void enqueue_iteration(gs_graph *g, bool timed) { enqueue_local(g, timed); enqueue_finish(g, timed); }

extern "C" int gs_iterate(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->dev_valid || g->plan_version != g->h.structure_version) return fail(GS_ERR_NOT_INITIALIZED, "call gs_initialize_optimization first");
    if (g->plan.dist) return fail(GS_ERR_INVALID, "sharded graph: use gs_dist_iterate (RCCL inside the library) or gs_dist_iterate_local / all-reduce / gs_dist_iterate_finish");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if ((rc = side_sync(g)) != GS_OK) return rc;
    enqueue_iteration(g, false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return 1;
}

// ------------------------------------------------------------------ the run scaffold of gs_optimize*, run_trials (and, in parts, gs_dist_optimize)
// a whole-tree launch gave up on a front's flag: one launch per level from now on; a retry of the whole-tree launches that ends this way
// waits four times longer before the next one (run_begin, gs_compute_marginals)
void fall_back_to_levels(gs_graph *g) {
    if (g->fallback_retrying) { g->fallback_retrying = false; g->fallback_retry_after = std::min(g->fallback_retry_after * 4, 1024); }
    g->fallback_calls = 0;
    g->d.tree = 0; g->fell_back = true;
}
// Before the first launch of a call.  retry: a handle that fell back to one launch per level (a whole-tree launch gave up on a front's flag)
// does not stay there until the next plan: what makes a flag late — the chip shared with another process, a debugger, a profiler replaying
// kernels — passes.  After 4 calls on the slow path the whole-tree launches are tried again (first iteration on its own, like a new
// plan's); another timeout quadruples the wait (16, 64, ... 1024 calls), a clean launch ends the episode.
// The failure state starts from zero; an armed fault injection (host-side fields) survives.
int run_begin(gs_graph *g, int32_t iterations, bool retry) {
    if (retry && g->fell_back && iterations > 0 && g->opt.tree != 0 && !g->d.tree && ++g->fallback_calls >= g->fallback_retry_after) {
        g->d.tree = 1; g->tree_proven = false; g->fallback_calls = 0; g->fallback_retrying = true; }
    HIP_TRY(hipMemsetAsync(g->d.fail, 0, 4 * sizeof(int32_t), g->stream));
    return GS_OK;
}
// After a chunk of iterations is enqueued (and whatever else the caller wants back with the same wait): the ONE host round trip of the
// chunk, then the bookkeeping every run shares.  A flag timeout of a whole-tree launch (code 2) is not a property of H: the handle falls
// back to one launch per level, once per call, and the caller runs the iterations that were not applied again (RUN_RERUN; the code is
// cleared, the update count fail[1] goes on).
enum { RUN_CONTINUE = 0, RUN_RERUN = 1, RUN_STOP = 2 };
struct RunState { int32_t ff[4] = {0, 0, 0, 0}; int first_failure = 0; bool fell_back = false; };
static int run_chunk_done(gs_graph *g, RunState &R) {
    HIP_TRY(hipMemcpyAsync(R.ff, g->d.fail, sizeof(R.ff), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (R.ff[0] == 0 && g->d.tree) { g->tree_proven = true;
        if (g->fallback_retrying) { g->fallback_retrying = false; g->fell_back = false; g->fallback_retry_after = 4; } }     // back on the whole-tree launches
    if (R.ff[0] != 0 && R.first_failure == 0) R.first_failure = R.ff[0];
    if (R.ff[0] == 2 && g->d.tree && !R.fell_back) {
        fall_back_to_levels(g);
        R.fell_back = true; g->d.inject_iter = 0;
        HIP_TRY(hipMemsetAsync(g->d.fail, 0, sizeof(int32_t), g->stream));      // the code only: the update count goes on
        R.ff[0] = 0; return RUN_RERUN; }
    return R.ff[0] != 0 ? RUN_STOP : RUN_CONTINUE;
}
// After the last wait of a call: a launch that never ran (the ticket counter and its running sum start again), the time between ev[5] and ev[6]
int run_check(gs_graph *g, const char *what, float *ms) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) { reset_failure(g); return fail(GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e)); }
    *ms = 0; hipEventElapsedTime(ms, g->ev[5], g->ev[6]);
    return GS_OK;
}
// The end of a call, behind the caller's own result copies: the estimates come back with the same wait (on failure: the last good
// iterate, what g2o's vertices hold)
static int run_end(gs_graph *g, const char *what, float *ms) {
    bool pull = false; int rc = pull_estimates_enqueue(g, pull); if (rc != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (pull) g->dev_estimates_newer = false;
    return run_check(g, what, ms);
}
void run_stats(gs_graph *g, gs_stats *stats, int32_t iterations, int32_t failure, int first_failure, double chi2_initial, double chi2_final, float ms) {
    if (!stats) return;
    std::memset(stats, 0, sizeof(*stats)); stats->struct_size = (int32_t)sizeof(*stats);
    fill_plan_stats(g, stats); stats->iterations = iterations; stats->numeric_failure = failure; stats->first_failure = first_failure;
    stats->chi2_initial = chi2_initial; stats->chi2_final = chi2_final; stats->ms_total = ms;
}

// gs_optimize (rel_tol < 0: the reference's fixed iteration count) and gs_optimize_until (rel_tol >= 0: the stop rule)
static int optimize_impl(gs_graph *g, int32_t iterations, double rel_tol, gs_stats *stats) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (iterations < 0) return fail(GS_ERR_INVALID, "negative iteration count");
    if (g->world > 1 || g->opt.force_shared_top > 0) return fail(GS_ERR_INVALID, "sharded graph: use gs_dist_optimize (RCCL inside the library), or drive gs_dist_iterate_local / all-reduce / gs_dist_iterate_finish");
    // g2o: optimize() is always preceded by initializeOptimization() (reference src/slam.cpp:480-481);
    // the plan is rebuilt only when the structure changed since the last call.
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    if ((rc = run_begin(g, iterations, true)) != GS_OK) return rc;
    const bool until = rel_tol >= 0.0;
    g->d.conv_tol = until ? rel_tol : -1.0;
    if (until) { const double none = -1.0; HIP_TRY(hipMemcpyAsync(g->d.chi2 + 70, &none, sizeof(double), hipMemcpyHostToDevice, g->stream)); }
    hipEventRecord(g->ev[5], g->stream);
    const int nh = std::min(iterations, 64);
    // All iterations are enqueued up front (no host round trip between them).  g2o leaves its loop at the first failed
    // solve and keeps the previous iterate: k_update applies nothing once the failure flag is up, and fail[1] says how
    // many updates went in.  After a flag timeout (run_chunk_done) the remaining iterations run again from the last good iterate.
    // Stop rule (gs_optimize_until): k_update compares the chi2 of consecutive linearisation points on the device and
    // raises fail[2]; later updates are skipped like after a failure.  The host enqueues chunks of 4 iterations and
    // looks at the flags in between, so at most 3 enqueued iterations run as no-ops after convergence.
    // Chunks: the FIRST iteration on its own, then groups of 8 — a remainder of up to 12 in one — (stop rule: 4).  A whole-tree launch whose flag hand-off fails
    // (its pollers are bounded and leave at once when any front has reported a failure, so such a launch drains in one poll
    // budget, ~30 ms) would otherwise have every remaining iteration queued up behind it, each paying the same again: with
    // chunks a timeout costs one chunk before the per-level fallback takes over.  One host round trip per chunk.
    int applied = 0, enq = 0; RunState R; const int32_t *ff = R.ff;
    while (enq < iterations) {
        // (a remainder of up to 12 goes out as one chunk: the reference's optimize(10) is 1 + 9, two host round trips instead of three)
        // (the FIRST iteration goes out alone only until a whole-tree launch of THIS plan has come back clean once: the flag hand-off
        // depends on the launch geometry, not on the numbers — a repeated optimize(10), the reference's quirk path, is one host round trip)
        const bool alone = enq == 0 && !(g->tree_proven && g->d.tree);
        const int upto = std::min(iterations, alone ? 1 : (until ? enq + 4 : (iterations - enq <= 12 ? iterations : enq + 8)));
        for (int it = enq; it < upto; ++it) {
            g->d.hist_slot = it < nh ? it : -1;                      // k_update files the chi2 of this iteration's linearisation point itself
            enqueue_iteration(g, false);
        }
        g->d.hist_slot = -1;
        enq = upto;
        const int next = run_chunk_done(g, R); if (next < 0) return next;
        applied = ff[1];
        if (next == RUN_RERUN) { enq = applied; continue; }
        if (next == RUN_STOP || ff[2] != 0) break;
    }
    g->d.conv_tol = -1.0;
    if (until) HIP_TRY(hipMemsetAsync(g->d.fail + 2, 0, sizeof(int32_t), g->stream));     // the stop flag must not gate later gs_iterate calls
    const int nshow = std::min(applied, nh);
    if (g->cfg.verbose || stats) { enqueue_chi2(g);
        hipMemcpyAsync(g->d.chi2 + 1 + nh, g->d.chi2, sizeof(double), hipMemcpyDeviceToDevice, g->stream); }
    hipEventRecord(g->ev[6], g->stream);
    double hist[80]; float ms;
    HIP_TRY(hipMemcpyAsync(hist, g->d.chi2, sizeof(hist), hipMemcpyDeviceToHost, g->stream));
    if ((rc = run_end(g, "iteration", &ms)) != GS_OK) return rc;
    if (g->cfg.verbose) for (int it = 0; it < nshow; ++it)  // g2o prints the chi2 AFTER the update of iteration it
        std::fprintf(stderr, "iteration= %d\t chi2= %.6f\t edges= %d\t schur= 0\n", it, it + 1 < applied ? hist[2 + it] : hist[1 + nh], g->h.n_pp() + g->h.n_pl());
    run_stats(g, stats, applied, ff[0], R.first_failure, iterations > 0 ? hist[1] : hist[1 + nh], hist[1 + nh], ms);
    if (ff[0]) { rc = reset_failure(g); if (rc != GS_OK) return rc; }
    if (ff[0] == 2) { g_last_error = "a front's completion flag did not arrive in time, with one launch per level as well"; return 0; }
    if (ff[0]) { g_last_error = "zero pivot: H is singular (g2o: optimize() returns 0, the vertices keep the last good iterate)"; return 0; }
    return applied;
}
extern "C" int gs_optimize(gs_graph *g, int32_t iterations, gs_stats *stats) { return optimize_impl(g, iterations, -1.0, stats); }
extern "C" int gs_optimize_until(gs_graph *g, int32_t max_iterations, double rel_chi2_tol, gs_stats *stats) {
    if (!(rel_chi2_tol >= 0.0)) return fail(GS_ERR_INVALID, "rel_chi2_tol must be >= 0");
    return optimize_impl(g, max_iterations, rel_chi2_tol, stats);
}

// ------------------------------------------------------------------ the step-control methods: one trial scaffold for both (gs_trial.hpp)
// a caller's parameter struct over the defaults: as many bytes as its struct_size says it holds
template <class P> static void copy_params(P &dst, const P *src) {
    if (!src) return;
    std::memcpy(&dst, src, std::min<size_t>(sizeof(P), (size_t)std::max(src->struct_size, 0))); dst.struct_size = (int32_t)sizeof(P);
}
// the entry points that run on one device only ask twice: the handle's configuration before ensure_ready, the plan it built after it
static int single_device_only(const gs_graph *g, bool plan_built, const char *what) {
    if (plan_built ? !!g->plan.dist : (g->world > 1 || g->opt.force_shared_top > 0))
        return fail(GS_ERR_INVALID, std::string("sharded graph: ") + what + " is not supported on sharded handles");
    return GS_OK;
}
// ... and what lies between: the device, the structure phase if the graph changed
static int ready_on_one_device(gs_graph *g, const char *what) {
    int rc = single_device_only(g, false, what); if (rc != GS_OK) return rc;
    if ((rc = ensure_device(g)) != GS_OK || (rc = ensure_ready(g)) != GS_OK) return rc;
    return single_device_only(g, true, what);
}
// a method's workspace, grow-only.  b: the allocation when this call made it (the method then sets its own pointers from L), else null
template <class Ws> static int trial_reserve(gs_graph *g, Ws &W, const TrialExtras &x, TrialLayout &L, char *&b) {
    const size_t NP = (size_t)(g->d.N + g->d.tN), ML = (size_t)(g->d.M + g->d.tM);
    b = nullptr;
    if (!W.mem || NP > W.cap_p || ML > W.cap_l) {
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (W.mem) { hipFree(W.mem); W.mem = nullptr; }
        L = trial_carve(NP, ML, x);
        HIP_TRY(hipMalloc(&W.mem, L.total));
        b = (char *)W.mem; TrialDev &T = W.dev.t; W.dev.state = (decltype(W.dev.state))(b + L.state);
        T.hist_chi2 = (double *)(b + L.hist_chi2); T.hist_trials = (int32_t *)(b + L.hist_trials);
        T.base_pose = (double *)(b + L.base_pose); T.base_cs = (double *)(b + L.base_cs); T.base_lm = (double *)(b + L.base_lm); T.part = (double *)(b + L.part);
        W.cap_p = L.cp; W.cap_l = L.cl; }
    W.dev.t.n_part = (int32_t)lm_grid(g->d);
    return GS_OK;
}
struct TrialHist { void *dev, *host; size_t bytes; };               // a method's own [64] history array, and where the host wants it
struct TrialCall { int32_t iterations; gs_stats *stats; bool want_chi2; const char *what, *numeric_msg; int n_hist; TrialHist hist[2]; };
struct TrialOut { double chi_last, chi2[64]; int32_t n_trials[64]; };
// The trials of one call from the record W.host[0].  enqueue(seq, first): one trial, asynchronous, reading state[seq & 1] (first: no
// trial of this call has run).  tail(it, O, buf, n): the method's end of iteration it's verbose line.  report(S, O): its info struct.
template <class Ws, class Enqueue, class Tail, class Report>
static int run_trials(gs_graph *g, Ws &W, const TrialCall &c, Enqueue enqueue, Tail tail, Report report) {
    auto *H = W.host; auto S = H[0]; const TrialDev &T = W.dev.t; const int32_t iterations = c.iterations;
    int rc = run_begin(g, iterations, true); if (rc != GS_OK) return rc;
    g->d.conv_tol = -1.0; g->d.hist_slot = -1;
    HIP_TRY(hipMemcpyAsync(W.dev.state, H, 2 * sizeof(S), hipMemcpyHostToDevice, g->stream));
    TrialOut O; const TrialHist hist[4] = {{T.hist_chi2, O.chi2, sizeof(O.chi2)}, {T.hist_trials, O.n_trials, sizeof(O.n_trials)}, c.hist[0], c.hist[1]};
    for (int k = 0; k < 2 + c.n_hist; ++k) HIP_TRY(hipMemsetAsync(hist[k].dev, 0, hist[k].bytes, g->stream));
    hipEventRecord(g->ev[5], g->stream);
    // Chunks of trials, the device record read in between (one host round trip per chunk).  Never more trials than iterations still
    // to accept — each needs one at least —, so the only trials that run as no-ops are the ones enqueued behind a "terminate"; the first
    // trial alone until a whole-tree launch of this plan has come back clean, as in gs_optimize.
    int seq = 0; RunState R; const int32_t *ff = R.ff;
    while (iterations > 0 && !S.t.done && S.t.iterations < iterations) {
        const bool alone = S.t.trials == 0 && !(g->tree_proven && g->d.tree);
        const int n = alone ? 1 : std::min(iterations - S.t.iterations, 8);
        for (int k = 0; k < n; ++k, ++seq) enqueue(seq, k == 0 && S.t.trials == 0);
        HIP_TRY(hipMemcpyAsync(&H[1], W.dev.state + (seq & 1), sizeof(S), hipMemcpyDeviceToHost, g->stream));
        const int next = run_chunk_done(g, R); if (next < 0) return next;
        S = H[1];
        if (next == RUN_STOP) break;                                // (RUN_RERUN: the trials behind the timeout were no-ops: the loop runs them again, one launch per level)
    }
    HIP_TRY(hipMemsetAsync(g->d.fail + 1, 0, 2 * sizeof(int32_t), g->stream));     // the update count and the stop flag must not gate later gs_iterate calls
    if (S.t.trials == 0 && c.want_chi2) enqueue_chi2(g);           // nothing ran: chi2 at the estimates as they are
    hipEventRecord(g->ev[6], g->stream);
    double chi_here = 0.0; float ms;
    HIP_TRY(hipMemcpyAsync(&chi_here, g->d.chi2, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    for (int k = 0; k < 2 + c.n_hist; ++k) HIP_TRY(hipMemcpyAsync(hist[k].host, hist[k].dev, hist[k].bytes, hipMemcpyDeviceToHost, g->stream));
    if ((rc = run_end(g, c.what, &ms)) != GS_OK) return rc;
    const double chi_first = S.t.trials > 0 ? O.chi2[0] : chi_here; O.chi_last = S.t.trials > 0 ? S.t.chi_base : chi_here;
    if (g->cfg.verbose) for (int it = 0; it < std::min(S.t.iterations, 64); ++it) { char buf[96]; tail(it, O, buf, sizeof(buf));
        std::fprintf(stderr, "iteration= %d\t chi2= %.6f\t edges= %d\t schur= 0\t %s\n", it,
                     it + 1 < S.t.iterations && it + 1 < 64 ? O.chi2[it + 1] : O.chi_last, g->h.n_pp() + g->h.n_pl(), buf); }
    run_stats(g, c.stats, S.t.iterations, ff[0], R.first_failure, chi_first, O.chi_last, ms);
    report(S, O);
    if (ff[0]) { rc = reset_failure(g); if (rc != GS_OK) return rc;
        if (ff[0] == 2) return fail(GS_ERR_TIMEOUT, "a front's completion flag did not arrive in time, with one launch per level as well (estimates = last accepted point)");
        return fail(GS_ERR_NUMERIC, c.numeric_msg); }
    return S.t.iterations;
}
template <class Info> static void info_counts(Info *info, const TrialState &t, const TrialOut &O) {
    std::memset(info, 0, sizeof(*info)); info->struct_size = (int32_t)sizeof(*info);
    info->iterations = t.iterations; info->trials = t.trials; info->rejected = t.rejected; info->terminated = t.terminated;
    std::memcpy(info->chi2, O.chi2, sizeof(O.chi2)); std::memcpy(info->n_trials, O.n_trials, sizeof(O.n_trials));
}

// ------------------------------------------------------------------ Levenberg-Marquardt (gs_lm.hpp: trial sequence, device record)
extern "C" int gs_lm_params_default(gs_lm_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(*p); p->max_trials_after_failure = 10; p->initial_lambda = 0.0; p->tau = 1e-5;
    return GS_OK;
}
static int lm_reserve(gs_graph *g) {
    TrialLayout L; char *b;
    const int rc = trial_reserve(g, g->lm, {2 * sizeof(LmState), 1, 0, 1, 0}, L, b);       // + hist_lambda; one partial array
    if (rc == GS_OK && b) g->lm.dev.hist_lambda = (double *)(b + L.hist_f64[0]);
    return rc;
}
// one trial, asynchronous: today's linearise / factor / back-solve / update launches in today's launch modes, with the LM kernels around them
static void enqueue_lm_trial(gs_graph *g, int par, bool init) {
    const LmDev &lm = g->lm.dev;
    ++g->d.iter;
    enqueue_linearize(g);
    if (init) launch_lm_maxdiag(g->d, lm, g->stream);
    launch_lm_damp(g->d, lm, par, init ? 1 : 0, g->stream);
    enqueue_factor_levels(g, g->sched.own, 0, 0);
    enqueue_finish(g, false);                                        // (no shared top on a single device), back-solve, update
    launch_lm_scale(g->d, lm, par, g->stream);
    enqueue_chi2(g);                                                 // chi2 at x_try -> chi2[0]
    launch_lm_step(g->d, lm, par, g->stream);
}
extern "C" int gs_optimize_lm(gs_graph *g, int32_t iterations, const gs_lm_params *params, gs_stats *stats, gs_lm_info *info) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (iterations < 0) return fail(GS_ERR_INVALID, "negative iteration count");
    gs_lm_params P; gs_lm_params_default(&P); copy_params(P, params);
    if (!std::isfinite(P.tau) || !(P.tau > 0.0)) return fail(GS_ERR_INVALID, "gs_lm_params.tau must be finite and > 0");
    if (!std::isfinite(P.initial_lambda)) return fail(GS_ERR_INVALID, "gs_lm_params.initial_lambda must be finite (<= 0: tau * max diag(H))");
    if (P.max_trials_after_failure < 1) return fail(GS_ERR_INVALID, "gs_lm_params.max_trials_after_failure must be >= 1");
    int rc = ready_on_one_device(g, "Levenberg-Marquardt"); if (rc != GS_OK) return rc;
    rc = lm_reserve(g); if (rc != GS_OK) return rc;
    LmState *H = g->lm.host, &S0 = H[0]; std::memset(H, 0, 2 * sizeof(LmState));
    double hl[64]; const bool need_lambda = !(P.initial_lambda > 0.0);
    S0.lambda = need_lambda ? 0.0 : P.initial_lambda; S0.lambda_initial = S0.lambda; S0.nu = 2.0; S0.tau = P.tau;
    S0.t.budget = iterations; S0.t.max_trials = P.max_trials_after_failure; S0.need_lambda = need_lambda ? 1 : 0;
    const TrialCall call{iterations, stats, stats || info || g->cfg.verbose, "LM iteration",
        "a solver failure the step control could not treat as a rejected trial (estimates = last accepted point)", 1, {{g->lm.dev.hist_lambda, hl, sizeof(hl)}}};
    return run_trials(g, g->lm, call,
        [&](int seq, bool first) { enqueue_lm_trial(g, seq & 1, first && need_lambda); },
        [&](int it, const TrialOut &O, char *buf, size_t n) { std::snprintf(buf, n, "lambda= %.6g\t levenbergIter= %d", hl[it], O.n_trials[it]); },
        [&](const LmState &S, const TrialOut &O) { if (!info) return;
            info_counts(info, S.t, O); info->lambda_initial = S.lambda_initial; info->lambda_final = S.lambda; std::memcpy(info->lambda, hl, sizeof(hl)); });
}

// ------------------------------------------------------------------ Powell's dogleg (gs_dogleg.hpp: trial sequence, device record)
extern "C" int gs_dogleg_params_default(gs_dogleg_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p));
    p->struct_size = (int32_t)sizeof(*p); p->max_trials_after_failure = 100; p->initial_delta = 1e4;
    return GS_OK;
}
// (also the vectors gs_multiply_hessian stages its operand and result in)
static int dl_reserve(gs_graph *g) {
    TrialLayout L; char *b; DlDev &D = g->dl.dev;
    const int rc = trial_reserve(g, g->dl, {2 * sizeof(DlState), 1, 1, DL_NPART, 4}, L, b);      // + hist_delta, hist_kind; b, H b, h_dl, H h_dl
    if (rc == GS_OK && b) { D.hist_delta = (double *)(b + L.hist_f64[0]); D.hist_kind = (int32_t *)(b + L.hist_i32[0]); D.part_stride = (int32_t)L.cpart;
        double **vp[4] = {&D.b_pose, &D.Hb_pose, &D.h_pose, &D.Hh_pose}, **vl[4] = {&D.b_lm, &D.Hb_lm, &D.h_lm, &D.Hh_lm};
        for (int k = 0; k < 4; ++k) { *vp[k] = (double *)(b + L.vec_pose[k]); *vl[k] = (double *)(b + L.vec_lm[k]); } }
    return rc;
}
// one trial, asynchronous: today's linearise / factor / back-solve / update launches in today's launch modes, with the dogleg kernels and
// the two Hessian products around them.  Both products run before the chi2 pass (which writes nothing of H or b, on a grown plan either: the order is free)
static void enqueue_dogleg_trial(gs_graph *g, int par) {
    const DlDev &dl = g->dl.dev; const bool tree = g->d.tree != 0;
    ++g->d.iter;
    enqueue_linearize(g);
    launch_dl_begin(g->d, dl, g->stream);
    launch_hmul(g->d, dl.b_pose, dl.b_lm, dl.Hb_pose, dl.Hb_lm, g->stream);
    launch_dl_dot(g->d, dl, g->stream);
    enqueue_factor_levels(g, g->sched.own, 0, 0);
    { Launcher L{g}; walk_finish_factor(g->sched, tree, L); walk_finish_backsolve(g->sched, tree, L); }     // (no shared top on a single device), back-solve: xe = h_gn
    launch_dl_norms(g->d, dl, g->stream);
    launch_dl_blend(g->d, dl, par, g->stream);                       // xe = h_dl
    launch_hmul(g->d, dl.h_pose, dl.h_lm, dl.Hh_pose, dl.Hh_lm, g->stream);
    launch_update(g->d, g->stream);
    g->dev_estimates_newer = true;
    launch_dl_gain(g->d, dl, par, g->stream);
    enqueue_chi2(g);                                                 // chi2 at x_try -> chi2[0]
    launch_dl_step(g->d, dl, par, g->stream);
}
extern "C" int gs_optimize_dogleg(gs_graph *g, int32_t iterations, const gs_dogleg_params *params, gs_stats *stats, gs_dogleg_info *info) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (iterations < 0) return fail(GS_ERR_INVALID, "negative iteration count");
    gs_dogleg_params P; gs_dogleg_params_default(&P); copy_params(P, params);
    if (!std::isfinite(P.initial_delta) || !(P.initial_delta > 0.0)) return fail(GS_ERR_INVALID, "gs_dogleg_params.initial_delta must be finite and > 0");
    if (P.max_trials_after_failure < 1) return fail(GS_ERR_INVALID, "gs_dogleg_params.max_trials_after_failure must be >= 1");
    int rc = ready_on_one_device(g, "the dogleg"); if (rc != GS_OK) return rc;
    rc = dl_reserve(g); if (rc != GS_OK) return rc;
    DlState *H = g->dl.host, &S0 = H[0]; std::memset(H, 0, 2 * sizeof(DlState));
    S0.delta = P.initial_delta; S0.delta_initial = P.initial_delta; S0.t.budget = iterations; S0.t.max_trials = P.max_trials_after_failure;
    double hd[64]; int32_t hk[64]; const DlDev &dl = g->dl.dev; static const char *const kind_name[3] = {"GN", "SD", "DL"};
    const TrialCall call{iterations, stats, stats || info || g->cfg.verbose, "dogleg iteration",
        "the Gauss-Newton solve of a dogleg trial failed (zero pivot: H is singular; estimates = last accepted point)", 2,
        {{dl.hist_delta, hd, sizeof(hd)}, {dl.hist_kind, hk, sizeof(hk)}}};
    return run_trials(g, g->dl, call,
        [&](int seq, bool) { enqueue_dogleg_trial(g, seq & 1); },
        [&](int it, const TrialOut &O, char *buf, size_t n) { std::snprintf(buf, n, "delta= %.6g\t kind= %s\t tries= %d", hd[it], kind_name[hk[it] % 3], O.n_trials[it]); },
        [&](const DlState &S, const TrialOut &O) { if (!info) return;
            info_counts(info, S.t, O); info->n_gn = S.n_kind[DL_GN]; info->n_sd = S.n_kind[DL_SD]; info->n_dl = S.n_kind[DL_DL];
            info->delta_initial = S.delta_initial; info->delta_final = S.delta;
            std::memcpy(info->delta, hd, sizeof(hd)); std::memcpy(info->step_kind, hk, sizeof(hk)); });
}

extern "C" int gs_chi2(gs_graph *g, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    enqueue_chi2(g);
    HIP_TRY(hipMemcpyAsync(out, g->d.chi2, sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}

// ------------------------------------------------------------------ measurement / parity hooks
extern "C" int gs_linearize(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    enqueue_linearize(g);
    launch_linearize_finalize(g->d, g->stream);              // stand-alone pass: materialise H_ll, b_l, chi2 for export
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("linearize: ") + hipGetErrorString(e));
    return GS_OK;
}
extern "C" int gs_time_linearize(gs_graph *g, int32_t reps, double *out_ms) {
    if (!g || !out_ms || reps <= 0) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    launch_linearize(g->d, g->stream);                       // warm
    hipEventRecord(g->ev[0], g->stream);
    for (int r = 0; r < reps; ++r) launch_linearize(g->d, g->stream);
    hipEventRecord(g->ev[1], g->stream);
    HIP_TRY(hipEventSynchronize(g->ev[1]));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
    *out_ms = (double)ms / reps;
    return GS_OK;
}
extern "C" int gs_debug_front_times(gs_graph *g, int64_t *out, int64_t capacity) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    if (!g->dev_valid) return fail(GS_ERR_NOT_INITIALIZED, "nothing on the device yet");
    const int64_t n = 2 * (int64_t)g->plan.fronts.size();
    if (capacity < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    HIP_TRY(hipMemcpyAsync(out, g->d.done_ts, (size_t)n * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return (int)(n / 2);
}
extern "C" int gs_debug_timestamps(gs_graph *g, int64_t *out64) {
    if (!g || !out64) return fail(GS_ERR_INVALID, "null argument");
    if (!g->dev_valid) return fail(GS_ERR_NOT_INITIALIZED, "nothing on the device yet");
    HIP_TRY(hipMemcpyAsync(out64, g->d.dbg_ts, 64 * sizeof(int64_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
extern "C" int64_t gs_linearize_bytes(gs_graph *g) {
    if (!g) return 0;
    return (int64_t)g->h.n_pp() * 152 + (int64_t)g->h.n_pl() * 96 + (int64_t)g->h.n_poses() * 120 + (int64_t)g->h.n_lms() * 64;
}
extern "C" int gs_export_system(gs_graph *g, double *Hpp_diag, double *Hll_diag, double *Hpp_off, double *Hpl,
                                double *b_pose, double *b_lm, int32_t *pp_order, int32_t *pl_order) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->dev_valid) return fail(GS_ERR_NOT_INITIALIZED, "nothing linearised yet");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    const DevGraph &d = g->d;
    // an iteration and gs_compute_marginals leave the landmark blocks as per-edge partials (the fronts sum them): sum them here, so
    // that H_ll and b_l are those of the last linearisation whichever call ran it (an old cone's first slot holds the tail's shares)
    launch_linearize_finalize(d, g->stream, false);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("export: ") + hipGetErrorString(e)); }
    // the device keeps these arrays structure-of-arrays (and the diagonal blocks packed symmetric), a grown plan's tail in arenas of
    // their own; the export format is array-of-blocks, full and row-major: gs_export_host.hpp
    const size_t N = (size_t)d.N, M = (size_t)d.M, Epp = (size_t)d.Epp, Epl = (size_t)d.Epl + (size_t)d.tEpl;
    const size_t L = (size_t)d.ell_len;
    if (g->plan.ell_of_ins.size() < Epl) return fail(GS_ERR_INVALID, "export: the plan does not cover the device's observation edges");
    const bool tail = d.tN > 0;                                      // (tail cones and edges come with tail poses only)
    const size_t cN = tail ? (size_t)d.tcapN : 0, cM = tail ? (size_t)d.tcapM : 0, cPP = tail ? (size_t)d.tcapEpp : 0, cPL = tail ? (size_t)d.tcapEpl : 0;
    std::vector<double> t0(N * 6), t1(M * 3), t2(Epp * 9), t3(L * 6), t4(N * 3), t5(M * 2);
    std::vector<double> u0(cN * 6), u1(cM * 3), u2(cPP * 9), u3(cPL * 6), u4(cN * 3), u5(cM * 2);
    auto dl = [&](std::vector<double> &dst, const double *src) -> hipError_t {
        return dst.empty() ? hipSuccess : hipMemcpyAsync(dst.data(), src, dst.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream); };
    HIP_TRY(dl(t0, d.Hpp_diag)); HIP_TRY(dl(t1, d.Hll_diag)); HIP_TRY(dl(t2, d.Hpp_off)); HIP_TRY(dl(t3, d.Hpl));
    HIP_TRY(dl(t4, d.b_pose)); HIP_TRY(dl(t5, d.b_lm));
    HIP_TRY(dl(u0, d.t_Hpp_diag)); HIP_TRY(dl(u1, d.t_Hll_diag)); HIP_TRY(dl(u2, d.t_Hpp_off)); HIP_TRY(dl(u3, d.t_Hpl));
    HIP_TRY(dl(u4, d.t_b_pose)); HIP_TRY(dl(u5, d.t_b_lm));
    HIP_TRY(hipStreamSynchronize(g->stream));
    const ExportCounts cnt{(int64_t)N, (int64_t)M, (int64_t)Epp, (int64_t)L, (int64_t)Epl, tail ? d.tN : 0, tail ? d.tM : 0, tail ? d.tEpp : 0, tail ? d.tEpl : 0,
                           (int64_t)cN, (int64_t)cM, (int64_t)cPP, (int64_t)cPL};
    const ExportSrc src{t0.data(), t1.data(), t2.data(), t3.data(), t4.data(), t5.data(), u0.data(), u1.data(), u2.data(), u3.data(), u4.data(), u5.data(),
                        g->plan.ell_of_ins.data()};
    export_layout(cnt, src, ExportDst{Hpp_diag, Hll_diag, Hpp_off, Hpl, b_pose, b_lm});
    if (pp_order) std::memcpy(pp_order, g->plan.pp_order.data(), g->plan.pp_order.size() * sizeof(int32_t));
    if (pl_order) for (size_t k = 0; k < Epl; ++k) pl_order[k] = (int32_t)k;                 // exported in insertion order
    return GS_OK;
}
// y = H v with the H of the last linearisation, as it lies in HBM (gs_hmul.hpp); changes no state of the handle
extern "C" int gs_multiply_hessian(gs_graph *g, const double *v_pose, const double *v_lm, double *out_pose, double *out_lm) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    const HostGraph &h = g->h; const size_t NP = (size_t)h.n_poses(), ML = (size_t)h.n_lms();
    if ((NP > 0 && !v_pose) || (ML > 0 && !v_lm)) return fail(GS_ERR_INVALID, "null vector");
    int rc = single_device_only(g, false, "the Hessian product"); if (rc != GS_OK) return rc;
    // fixed vertices: their entries of v are ignored (sent as zeros); every other entry must be finite
    std::vector<double> vp(3 * NP), vl(2 * ML);
    for (size_t p = 0; p < NP; ++p) for (int c = 0; c < 3; ++c) { const double x = h.pose_fixed[p] ? 0.0 : v_pose[3 * p + c];
        if (!std::isfinite(x)) return fail(GS_ERR_INVALID, "v_pose holds a value that is not finite"); vp[3 * p + c] = x; }
    for (size_t l = 0; l < ML; ++l) for (int c = 0; c < 2; ++c) { const double x = h.lm_fixed[l] ? 0.0 : v_lm[2 * l + c];
        if (!std::isfinite(x)) return fail(GS_ERR_INVALID, "v_lm holds a value that is not finite"); vl[2 * l + c] = x; }
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (!g->dev_valid || !g->linearised) return fail(GS_ERR_NOT_INITIALIZED, "nothing linearised yet (since the last structure phase or growth step)");
    if ((rc = single_device_only(g, true, "the Hessian product")) != GS_OK) return rc;
    if (g->plan_version != h.structure_version || (size_t)(g->d.N + g->d.tN) != NP || (size_t)(g->d.M + g->d.tM) != ML)
        return fail(GS_ERR_NOT_INITIALIZED, "the graph changed since the last linearisation");
    if ((rc = dl_reserve(g)) != GS_OK) return rc;
    const DlDev &dl = g->dl.dev;
    if (NP) HIP_TRY(hipMemcpyAsync(dl.b_pose, vp.data(), vp.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
    if (ML) HIP_TRY(hipMemcpyAsync(dl.b_lm, vl.data(), vl.size() * sizeof(double), hipMemcpyHostToDevice, g->stream));
    launch_hmul(g->d, dl.b_pose, dl.b_lm, dl.Hb_pose, dl.Hb_lm, g->stream);
    { const hipError_t e = hipGetLastError(); if (e != hipSuccess) { hipStreamSynchronize(g->stream); return fail(GS_ERR_HIP, std::string("Hessian product: ") + hipGetErrorString(e)); } }
    if (out_pose && NP) HIP_TRY(hipMemcpyAsync(out_pose, dl.Hb_pose, vp.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (out_lm && ML) HIP_TRY(hipMemcpyAsync(out_lm, dl.Hb_lm, vl.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                        // (vp / vl are host temporaries)
    return GS_OK;
}
// per-edge s = e^T W e and weight at the current estimates (k_edge_chi2).  The index table of the kind's edges goes up with the call
// (a query, not part of an iteration): endpoints from the host graph, an observation edge's place from the plan — its ELL index,
// or its tail slot when a growth step appended it
extern "C" int gs_get_edge_chi2(gs_graph *g, int32_t edge_kind, int32_t capacity, double *out_chi2, double *out_weight) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (edge_kind != GS_EDGE_ODOMETRY && edge_kind != GS_EDGE_OBSERVATION) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if ((rc = single_device_only(g, false, "per-edge chi2")) != GS_OK) return rc;
    rc = ensure_ready(g); if (rc != GS_OK) return rc;
    if ((rc = single_device_only(g, true, "per-edge chi2")) != GS_OK) return rc;
    const HostGraph &h = g->h;
    const bool pp = edge_kind == GS_EDGE_ODOMETRY;
    const int n = pp ? h.n_pp() : h.n_pl();
    if ((out_chi2 || out_weight) && capacity < n) return fail(GS_ERR_CAPACITY, "buffer too small");
    if (n == 0 || (!out_chi2 && !out_weight)) return n;
    const int per = pp ? 2 : 3;
    std::vector<int32_t> tab((size_t)n * per);
    if (pp) for (int k = 0; k < n; ++k) { tab[2 * (size_t)k] = h.pp_i[k]; tab[2 * (size_t)k + 1] = h.pp_j[k]; }
    else for (int k = 0; k < n; ++k) {
        int32_t src; rc = pl_location(g, k, src, ""); if (rc != GS_OK) return rc;
        tab[3 * (size_t)k] = h.pl_p[k]; tab[3 * (size_t)k + 1] = h.pl_l[k]; tab[3 * (size_t)k + 2] = src; }
    if (pp && n > g->d.Epp + g->d.tEpp) return fail(GS_ERR_INVALID, "odometry edge not on the device");
    if (g->emask.store.any_off()) return edge_mask_edge_chi2(g, edge_kind, n, tab, out_chi2, out_weight);     // the device arrays hold zeros for the inactive edges: s from the edges' own information
    ArenaLayout lay; const size_t o_out = lay.add((size_t)n * 2 * sizeof(double)), o_tab = lay.add(tab.size() * sizeof(int32_t));
    DevScratch s; HIP_TRY(s.alloc(lay.total));
    int32_t *dtab = (int32_t *)(s.p + o_tab); double *dout = (double *)(s.p + o_out);
    std::vector<double> out((size_t)n * 2);
    hipError_t e = hipMemcpyAsync(dtab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) { launch_edge_chi2(g->d, edge_kind, n, dtab, dout, g->stream); e = hipGetLastError(); }
    if (e == hipSuccess && !pp && polar_edge_chi2_overwrite(g, n, dout) != GS_OK) { hipStreamSynchronize(g->stream); return GS_ERR_HIP; }   // (nothing without polar edges)
    HIP_NEXT(e, hipMemcpyAsync(out.data(), dout, out.size() * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    e = sync_keep_first(e, g->stream);
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("edge chi2: ") + hipGetErrorString(e));
    if (out_chi2) std::memcpy(out_chi2, out.data(), (size_t)n * sizeof(double));
    if (out_weight) std::memcpy(out_weight, out.data() + n, (size_t)n * sizeof(double));
    return n;
}
extern "C" int gs_export_delta(gs_graph *g, double *dpose, double *dlm) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->dev_valid) return fail(GS_ERR_NOT_INITIALIZED, "no iteration run yet");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (dpose && g->d.N) HIP_TRY(hipMemcpyAsync(dpose, g->d.dpose, (size_t)(g->d.N + g->d.tN) * 3 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (dlm && g->d.M) HIP_TRY(hipMemcpyAsync(dlm, g->d.dlm, (size_t)(g->d.M + g->d.tM) * 2 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
extern "C" int gs_time_iterations(gs_graph *g, int32_t reps, gs_stats *s) {
    if (!g || !s || reps <= 0) return fail(GS_ERR_INVALID, "bad argument");
    if (g->world > 1 || g->opt.force_shared_top > 0) return fail(GS_ERR_INVALID, "sharded graph: time the two halves from the caller");
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    const int N = g->d.N + g->d.tN, M = g->d.M + g->d.tM;
    double *sp = nullptr, *sl = nullptr;                        // save estimates
    HIP_TRY(hipMalloc((void **)&sp, std::max<size_t>((size_t)N * 3, 1) * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&sl, std::max<size_t>((size_t)M * 2, 1) * sizeof(double)));
    hipMemcpyAsync(sp, g->d.pose_est, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToDevice, g->stream);
    hipMemcpyAsync(sl, g->d.lm_est, (size_t)M * 2 * sizeof(double), hipMemcpyDeviceToDevice, g->stream);
    const bool newer = g->dev_estimates_newer;
    std::memset(s, 0, sizeof(*s)); s->struct_size = (int32_t)sizeof(*s); fill_plan_stats(g, s);
    enqueue_iteration(g, false);                                 // warm
    // all repetitions are enqueued back to back like the iterations of gs_optimize (no host round trip in between);
    // every repetition has its own five phase events plus a sixth right behind the fifth: that empty interval is what
    // one event boundary costs on this stream (ms_event_overhead), i.e. how much of each phase time is the measurement
    // ... then `reps` more iterations with a start / stop pair attached to the linearisation kernel's own dispatch (hipExtLaunchKernelGGL):
    // its begin -> end as a kernel trace reports it, without the hand-over from k_update that the event-to-event interval also holds
    std::vector<hipEvent_t> evs((size_t)reps * 8);
    for (auto &e : evs) HIP_TRY(hipEventCreate(&e));
    hipEvent_t saved[5]; for (int k = 0; k < 5; ++k) saved[k] = g->ev[k];
    for (int r = 0; r < reps; ++r) {
        for (int k = 0; k < 5; ++k) g->ev[k] = evs[(size_t)r * 8 + k];
        enqueue_iteration(g, true);
        hipEventRecord(evs[(size_t)r * 8 + 5], g->stream);
    }
    for (int k = 0; k < 5; ++k) g->ev[k] = saved[k];
    // second pass, nothing recorded between the phases (a dispatch with events attached lengthens the event-to-event interval
    // around it by ~10 us: the two measurements do not share iterations)
    for (int r = 0; r < reps; ++r) {
        g->ev_lin[0] = evs[(size_t)r * 8 + 6]; g->ev_lin[1] = evs[(size_t)r * 8 + 7];
        enqueue_iteration(g, false);
    }
    g->ev_lin[0] = g->ev_lin[1] = nullptr;
    HIP_TRY(hipStreamSynchronize(g->stream));
    double ovh = 0.0, link = 0.0; int nlink = 0;
    for (int r = 0; r < reps; ++r) { const hipEvent_t *e = &evs[(size_t)r * 8];
        float a = 0, b = 0, c = 0, dd = 0, o = 0, lk = 0;
        hipEventElapsedTime(&a, e[0], e[1]); hipEventElapsedTime(&b, e[1], e[2]);
        hipEventElapsedTime(&c, e[2], e[3]); hipEventElapsedTime(&dd, e[3], e[4]); hipEventElapsedTime(&o, e[4], e[5]);
        if (hipEventElapsedTime(&lk, e[6], e[7]) == hipSuccess && lk > 0) { link += lk; ++nlink; }     // (the gather path launches several kernels: no pair)
        s->ms_linearize += a; s->ms_factor += b; s->ms_backsolve += c; s->ms_update += dd; ovh += o; }
    (void)hipGetLastError();
    for (auto &e : evs) hipEventDestroy(e);
    s->ms_linearize /= reps; s->ms_factor /= reps; s->ms_backsolve /= reps; s->ms_update /= reps; s->ms_event_overhead = ovh / reps;
    s->ms_linearize_kernel = nlink > 0 ? link / nlink : 0.0;
    s->ms_total = s->ms_linearize + s->ms_factor + s->ms_backsolve + s->ms_update; s->iterations = reps;
    hipMemcpyAsync(g->d.pose_est, sp, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToDevice, g->stream);
    launch_pose_trig(g->d, g->stream);
    hipMemcpyAsync(g->d.lm_est, sl, (size_t)M * 2 * sizeof(double), hipMemcpyDeviceToDevice, g->stream);
    int32_t failflag = 0;
    hipMemcpyAsync(&failflag, g->d.fail, sizeof(int32_t), hipMemcpyDeviceToHost, g->stream);
    hipMemsetAsync(g->d.fail, 0, sizeof(int32_t), g->stream);
    HIP_TRY(hipStreamSynchronize(g->stream));
    hipFree(sp); hipFree(sl);
    g->dev_estimates_newer = newer; s->numeric_failure = failflag;
    return GS_OK;
}
