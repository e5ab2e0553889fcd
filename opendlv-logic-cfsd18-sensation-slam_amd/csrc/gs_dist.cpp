// gs_dist.cpp — pose-window shards: the sharding entry points of the C-ABI and the RCCL loader.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>          // types and prototypes only: the library is resolved at run time (rccl_api), never linked

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

// ------------------------------------------------------------------ multi-GPU
extern "C" int gs_dist_configure(gs_graph *g, int32_t rank, int32_t world) {
    if (!g || world < 1 || rank < 0 || rank >= world) return fail(GS_ERR_INVALID, "bad rank/world");
    if (world > 1 && (g->cfg.odometry_robust_kernel != GS_ROBUST_NONE || g->cfg.observation_robust_kernel != GS_ROBUST_NONE))
        return fail(GS_ERR_INVALID, "robust kernels are not supported on sharded handles: set GS_ROBUST_NONE on both edge kinds first");
    if (world > 1 && !g->prior.store.empty())
        return fail(GS_ERR_INVALID, "prior edges are not supported on sharded handles: gs_clear_priors first");
    if (world > 1 && !g->polar.store.empty())
        return fail(GS_ERR_INVALID, "polar observation edges are not supported on sharded handles: gs_clear first");
    if (world > 1 && g->emask.store.any_off())
        return fail(GS_ERR_INVALID, "inactive edges are not supported on sharded handles: gs_activate_all_edges first");
    g->rank = rank; g->world = world; ++g->h.structure_version; ++g->h.reshape_version;
    return GS_OK;
}
// ---- rank-local ingestion (round 4): a rank need not hold the observation edges of the other windows' interiors
static void window_starts_of(const gs_graph *g, std::vector<int32_t> &first_pose, std::vector<int32_t> *fp_of_pose = nullptr) {
    const HostGraph &h = g->h; const int N = h.n_poses(), W = std::max(1, g->world);
    int nfree = 0; for (int p = 0; p < N; ++p) nfree += !h.pose_fixed[p];
    first_pose.assign((size_t)W + 1, N);
    if (fp_of_pose) fp_of_pose->assign((size_t)N, -1);
    int f = 0, w = 0;
    for (int p = 0; p < N; ++p) if (!h.pose_fixed[p]) {
        while (w <= W && (int)(((int64_t)w * nfree + W - 1) / W) == f) first_pose[(size_t)w++] = p;     // (empty windows share a start)
        if (fp_of_pose) (*fp_of_pose)[(size_t)p] = f;
        ++f; }
}
extern "C" int gs_dist_window_starts(gs_graph *g, int32_t *out_first_pose, int32_t capacity) {
    if (!g || !out_first_pose) return fail(GS_ERR_INVALID, "null argument");
    if (capacity < g->world + 1) return fail(GS_ERR_CAPACITY, "gs_dist_window_starts: world + 1 entries are written");
    std::vector<int32_t> fp; window_starts_of(g, fp);
    std::memcpy(out_first_pose, fp.data(), fp.size() * sizeof(int32_t));
    return GS_OK;
}
extern "C" int gs_dist_local_landmark_windows(gs_graph *g, uint64_t *seen_interior, uint64_t *seen_first, int32_t n_landmarks) {
    if (!g || !seen_interior || !seen_first) return fail(GS_ERR_INVALID, "null argument");
    const HostGraph &h = g->h;
    if (n_landmarks != h.n_lms()) return fail(GS_ERR_INVALID, "gs_dist_local_landmark_windows: one entry per landmark of the graph");
    if (g->world > 64) return fail(GS_ERR_INVALID, "landmark windows are 64-bit masks: at most 64 ranks");
    std::vector<int32_t> first; window_starts_of(g, first);
    const int r = g->rank; const uint64_t bit = 1ull << r;
    std::fill(seen_interior, seen_interior + n_landmarks, 0ull); std::fill(seen_first, seen_first + n_landmarks, 0ull);
    for (size_t k = 0; k < h.pl_p.size(); ++k) { const int p = h.pl_p[k], l = h.pl_l[k];
        if (h.pose_fixed[p] || h.lm_fixed[l] || p < first[(size_t)r] || p >= first[(size_t)r + 1]) continue;      // this rank's own window only: the ranks' bits are disjoint, their sum is the union
        if (r >= 1 && p == first[(size_t)r]) seen_first[l] |= bit; else seen_interior[l] |= bit; }
    return GS_OK;
}
extern "C" int gs_dist_set_landmark_windows(gs_graph *g, const uint64_t *seen_interior, const uint64_t *seen_first, int32_t n_landmarks) {
    if (!g || n_landmarks < 0 || (n_landmarks > 0 && (!seen_interior || !seen_first))) return fail(GS_ERR_INVALID, "bad argument");
    g->lm_seen_interior.assign(seen_interior, seen_interior + n_landmarks); g->lm_seen_first.assign(seen_first, seen_first + n_landmarks);
    ++g->h.structure_version; ++g->h.reshape_version;
    return GS_OK;
}
extern "C" int64_t gs_dist_exchange_doubles(gs_graph *g) { return (g && g->plan.valid) ? g->plan.exchange_doubles : 0; }
extern "C" int gs_dist_set_exchange_buffer(gs_graph *g, void *p) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    g->exchange = (double *)p; g->exchange_external = p != nullptr;
    if (g->dev_valid && p) g->d.exchange = (double *)p;        // the previous (own) buffer stays allocated until the next upload
    return GS_OK;
}
static int dist_ready(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->dev_valid || g->plan_version != g->h.structure_version) return fail(GS_ERR_NOT_INITIALIZED, "call gs_initialize_optimization first");
    if (g->plan.dist && !g->d.exchange) return fail(GS_ERR_NOT_INITIALIZED, "no exchange buffer");
    if (!g->prior.store.empty()) return fail(GS_ERR_INVALID, "prior edges are not supported by the two-half (sharded) iteration");
    return ensure_device(g);
}
extern "C" int gs_dist_iterate_local(gs_graph *g) {
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    enqueue_local(g, false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return GS_OK;
}
extern "C" int gs_dist_iterate_finish(gs_graph *g) {
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    enqueue_finish(g, false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return 1;
}
// host copies of the exchange buffer (tests; all-reduce over a CPU backend when ranks share one GPU)
extern "C" int gs_dist_read_exchange(gs_graph *g, double *host) {
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    if (!host) return fail(GS_ERR_INVALID, "null buffer");
    if (g->plan.exchange_doubles > 0) HIP_TRY(hipMemcpyAsync(host, g->d.exchange, (size_t)g->plan.exchange_doubles * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
extern "C" int gs_dist_write_exchange(gs_graph *g, const double *host) {
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    if (!host) return fail(GS_ERR_INVALID, "null buffer");
    if (g->plan.exchange_doubles > 0) HIP_TRY(hipMemcpyAsync(g->d.exchange, host, (size_t)g->plan.exchange_doubles * sizeof(double), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}

// ---- RCCL inside the library: the host side of the sharded iteration stays C++ (north_star: "Host stays C++ ... RCCL all-reduce over
// xGMI on the shared-landmark rows").  The RCCL library is resolved at run time — first the copy the process has loaded already (under
// bench.py: torch's), then the system's — so libgraphslam_hip.so has no link-time dependency on it and a single-GPU consumer never loads it.
namespace {
struct RcclApi {
    void *lib = nullptr;
    decltype(&ncclGetUniqueId) GetUniqueId = nullptr; decltype(&ncclCommInitRank) CommInitRank = nullptr;
    decltype(&ncclAllReduce) AllReduce = nullptr; decltype(&ncclCommDestroy) CommDestroy = nullptr;
    decltype(&ncclGetErrorString) GetErrorString = nullptr; decltype(&ncclCommCount) CommCount = nullptr;
};
RcclApi *rccl_api(std::string &err) {
    static RcclApi api; static bool tried = false; static std::string why;
    if (!tried) { tried = true;
        const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1", "/opt/rocm/lib/librccl.so"};
        for (const char *n : names) if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_NOLOAD);     // a copy the process has loaded already
        for (const char *n : names) if (!api.lib) api.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL);
        if (!api.lib) why = std::string("librccl.so not found: ") + (dlerror() ? dlerror() : "");
        else {
            api.GetUniqueId = (decltype(api.GetUniqueId))dlsym(api.lib, "ncclGetUniqueId"); api.CommInitRank = (decltype(api.CommInitRank))dlsym(api.lib, "ncclCommInitRank");
            api.AllReduce = (decltype(api.AllReduce))dlsym(api.lib, "ncclAllReduce"); api.CommDestroy = (decltype(api.CommDestroy))dlsym(api.lib, "ncclCommDestroy");
            api.GetErrorString = (decltype(api.GetErrorString))dlsym(api.lib, "ncclGetErrorString"); api.CommCount = (decltype(api.CommCount))dlsym(api.lib, "ncclCommCount");
            if (!api.GetUniqueId || !api.CommInitRank || !api.AllReduce || !api.CommDestroy) { why = "librccl.so lacks ncclGetUniqueId / ncclCommInitRank / ncclAllReduce / ncclCommDestroy"; api.lib = nullptr; } } }
    if (!api.lib) { err = why; return nullptr; }
    return &api;
}
int rccl_fail(RcclApi *R, ncclResult_t rc, const char *what) {
    return fail(GS_ERR_HIP, std::string(what) + ": " + (R && R->GetErrorString ? R->GetErrorString(rc) : "RCCL error") + " (" + std::to_string((int)rc) + ")");
}
}  // namespace
extern "C" int gs_dist_unique_id(void *out128) {
    if (!out128) return fail(GS_ERR_INVALID, "null buffer");
    std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
    static_assert(sizeof(ncclUniqueId) == 128, "gs_dist_unique_id hands out NCCL_UNIQUE_ID_BYTES = 128 bytes");
    ncclUniqueId id; ncclResult_t rc = R->GetUniqueId(&id); if (rc != ncclSuccess) return rccl_fail(R, rc, "ncclGetUniqueId");
    std::memcpy(out128, &id, sizeof(id)); return GS_OK;
}
extern "C" int gs_dist_comm_init(gs_graph *g, const void *unique_id_128, int32_t rank, int32_t world) {
    if (!g || !unique_id_128 || world < 1 || rank < 0 || rank >= world) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
    if (g->comm && g->own_comm) { R->CommDestroy((ncclComm_t)g->comm); g->comm = nullptr; }
    ncclUniqueId id; std::memcpy(&id, unique_id_128, sizeof(id));
    ncclComm_t c = nullptr; ncclResult_t nr = R->CommInitRank(&c, world, id, rank);      // (collective: every rank of the group calls it; the current device is the handle's)
    if (nr != ncclSuccess) return rccl_fail(R, nr, "ncclCommInitRank");
    g->comm = c; g->own_comm = true; g->comm_world = world;
    return GS_OK;
}
extern "C" int gs_dist_set_communicator(gs_graph *g, void *nccl_comm) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
    if (g->comm && g->own_comm) R->CommDestroy((ncclComm_t)g->comm);
    g->comm = nccl_comm; g->own_comm = false; g->comm_world = 0;
    if (nccl_comm && R->CommCount) { int n = 0; if (R->CommCount((ncclComm_t)nccl_comm, &n) == ncclSuccess) g->comm_world = n; }
    return GS_OK;
}
void gs_dist_comm_release(gs_graph *g) {      // gs_destroy
    if (!g->comm || !g->own_comm) { g->comm = nullptr; return; }
    std::string err; if (RcclApi *R = rccl_api(err)) R->CommDestroy((ncclComm_t)g->comm);
    g->comm = nullptr;
}
// the all-reduce of the shared fronts' slots (and of the ranks' failure flags at the buffer's tail), enqueued on the handle's stream
static int enqueue_allreduce(gs_graph *g) {
    if (!g->comm) return fail(GS_ERR_NOT_INITIALIZED, "no RCCL communicator: gs_dist_comm_init or gs_dist_set_communicator first");
    if (g->comm_world > 0 && g->comm_world != g->world) return fail(GS_ERR_INVALID, "the communicator's size differs from gs_dist_configure's world");
    std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
    const int64_t n = g->plan.exchange_doubles;
    if (n <= 0) return GS_OK;
    ncclResult_t nr = R->AllReduce(g->d.exchange, g->d.exchange, (size_t)n, ncclDouble, ncclSum, (ncclComm_t)g->comm, g->stream);
    return nr == ncclSuccess ? GS_OK : rccl_fail(R, nr, "ncclAllReduce");
}
// rank-local ingestion without any other channel between the replicas than the library's own communicator: this rank's bits of the landmark windows
// (from the edges it holds), ncclAllReduce(uint64, sum) — the ranks' bits are disjoint, the sum is the union —, the result handed to the handle
extern "C" int gs_dist_share_landmark_windows(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->comm) return fail(GS_ERR_NOT_INITIALIZED, "no RCCL communicator: gs_dist_comm_init or gs_dist_set_communicator first");
    if (g->comm_world > 0 && g->comm_world != g->world) return fail(GS_ERR_INVALID, "the communicator's size differs from gs_dist_configure's world");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
    const int M = g->h.n_lms();
    std::vector<uint64_t> m(2 * (size_t)M);
    if ((rc = gs_dist_local_landmark_windows(g, m.data(), m.data() + M, M)) != GS_OK) return rc;
    if (M == 0) return gs_dist_set_landmark_windows(g, nullptr, nullptr, 0);
    uint64_t *dev = nullptr;
    HIP_TRY(hipMalloc(&dev, m.size() * sizeof(uint64_t)));
    hipError_t e = hipMemcpyAsync(dev, m.data(), m.size() * sizeof(uint64_t), hipMemcpyHostToDevice, g->stream);
    ncclResult_t nr = e == hipSuccess ? R->AllReduce(dev, dev, m.size(), ncclUint64, ncclSum, (ncclComm_t)g->comm, g->stream) : ncclSuccess;
    if (e == hipSuccess && nr == ncclSuccess) e = hipMemcpyAsync(m.data(), dev, m.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    hipFree(dev);
    if (nr != ncclSuccess) return rccl_fail(R, nr, "ncclAllReduce (landmark windows)");
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("landmark windows: ") + hipGetErrorString(e));
    return gs_dist_set_landmark_windows(g, m.data(), m.data() + M, M);
}
extern "C" int gs_dist_iterate(gs_graph *g) {
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    if (!g->plan.dist) return fail(GS_ERR_INVALID, "not a sharded graph: gs_iterate");
    enqueue_local(g, false);
    if ((rc = enqueue_allreduce(g)) != GS_OK) return rc;
    enqueue_finish(g, false);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("kernel launch: ") + hipGetErrorString(e));
    return 1;
}
// measurement hook (graphslam_debug.h): `reps` all-reduces of the exchange buffer back to back on the handle's stream, HIP events around
// them; mean milliseconds per all-reduce.  Collective: every rank of the communicator calls it.
extern "C" int gs_debug_time_exchange(gs_graph *g, int32_t reps, double *out_ms) {
    if (!out_ms || reps <= 0) return fail(GS_ERR_INVALID, "bad argument");
    int rc = dist_ready(g); if (rc != GS_OK) return rc;
    if ((rc = enqueue_allreduce(g)) != GS_OK) return rc;           // warm
    hipEventRecord(g->ev[0], g->stream);
    for (int r = 0; r < reps && rc == GS_OK; ++r) rc = enqueue_allreduce(g);
    hipEventRecord(g->ev[1], g->stream);
    HIP_TRY(hipEventSynchronize(g->ev[1]));
    float ms = 0; HIP_TRY(hipEventElapsedTime(&ms, g->ev[0], g->ev[1]));
    *out_ms = (double)ms / reps;
    return rc;
}
// Slam's optimize(10) (reference src/slam.cpp:481) on a sharded graph: every rank makes the same call; g2o's failure rule holds across
// ranks (a rank's failure flag rides through the all-reduce: no rank applies the update of that iteration or any later one).  Returns the
// iterations whose update was applied, 0 when any rank's factorisation failed.  The estimates this rank tracks (gs_dist_known) come back.
extern "C" int gs_dist_optimize(gs_graph *g, int32_t iterations, gs_stats *stats) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (iterations < 0) return fail(GS_ERR_INVALID, "negative iteration count");
    int rc = ensure_ready(g); if (rc != GS_OK) return rc;
    if (!g->plan.dist) return fail(GS_ERR_INVALID, "not a sharded graph: gs_optimize");
    if ((rc = dist_ready(g)) != GS_OK) return rc;
    if ((rc = run_begin(g, iterations, false)) != GS_OK) return rc;      // (no retry of the whole-tree launches here: a rank that fell back stays there until the next plan)
    g->d.conv_tol = -1.0;
    hipEventRecord(g->ev[5], g->stream);
    const int nh = std::min(iterations, 64);
    // A flag timeout on ANY rank (code 2 where it happened, 4 on the others: the same all-reduce tells everybody) is not a property of H: the rank it
    // happened on switches to one launch per level, every rank runs the iterations that were not applied again — the repair gs_optimize makes on one GPU,
    // decided identically on every rank (the count of applied updates is the same everywhere).  At most twice per call.
    int32_t ff[4] = {0, 0, 0, 0}; double hist[80]; int from = 0, first_failure = 0;
    for (int repair = 0; ; ++repair) {
        for (int it = from; it < iterations; ++it) {
            g->d.hist_slot = it < nh ? it : -1;
            enqueue_local(g, false);
            if ((rc = enqueue_allreduce(g)) != GS_OK) { g->d.hist_slot = -1; return rc; }
            enqueue_finish(g, false);
        }
        g->d.hist_slot = -1;
        hipEventRecord(g->ev[6], g->stream);
        HIP_TRY(hipMemcpyAsync(ff, g->d.fail, sizeof(ff), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipMemcpyAsync(hist, g->d.chi2, sizeof(hist), hipMemcpyDeviceToHost, g->stream));
        HIP_TRY(hipStreamSynchronize(g->stream));
        if (ff[0] != 0 && first_failure == 0) first_failure = ff[0];
        if ((ff[0] != 2 && ff[0] != 4) || repair >= 2) break;
        if (ff[0] == 2) fall_back_to_levels(g);
        // Every rank is here (the code came with the same all-reduce).  A launch that gave up BEHIND the exchange — the shared top, a backward solve — is only
        // heard of with the NEXT contribution: by then the other ranks have applied an update the rank it happened on has not.  The ranks compare their counts
        // (one more all-reduce, only in this branch); if they differ the estimates have parted and no re-run can mend that: every rank says so, nobody goes on.
        { std::string err; RcclApi *R = rccl_api(err); if (!R) return fail(GS_ERR_NO_DEVICE, err);
          double v[2] = {(double)ff[1], -(double)ff[1]}, *dv = nullptr;
          HIP_TRY(hipMalloc(&dv, sizeof(v)));
          hipError_t e2 = hipMemcpyAsync(dv, v, sizeof(v), hipMemcpyHostToDevice, g->stream);
          ncclResult_t nr = e2 == hipSuccess ? R->AllReduce(dv, dv, 2, ncclDouble, ncclMax, (ncclComm_t)g->comm, g->stream) : ncclSuccess;
          if (e2 == hipSuccess && nr == ncclSuccess) e2 = hipMemcpyAsync(v, dv, sizeof(v), hipMemcpyDeviceToHost, g->stream);
          if (e2 == hipSuccess) e2 = hipStreamSynchronize(g->stream);
          hipFree(dv);
          if (nr != ncclSuccess) return rccl_fail(R, nr, "ncclAllReduce (applied updates)");
          if (e2 != hipSuccess) return fail(GS_ERR_HIP, std::string("applied updates: ") + hipGetErrorString(e2));
          if (v[0] != -v[1]) { reset_failure(g);
              return fail(GS_ERR_TIMEOUT, "a launch behind the exchange gave up on one rank after the others had applied that iteration's update: the ranks' estimates have parted "
                                          "(updates applied: " + std::to_string((long long)-v[1]) + " .. " + std::to_string((long long)v[0]) + "); set the estimates again on every rank"); } }
        g->d.inject_iter = 0;
        HIP_TRY(hipMemsetAsync(g->d.fail, 0, sizeof(int32_t), g->stream));      // the code only: the update count goes on
        if (g->d.tickets) { HIP_TRY(hipMemsetAsync(g->d.tickets, 0, 2 * sizeof(uint32_t), g->stream)); g->d.ticket_base = 0; }
        from = ff[1]; ff[0] = 0;
    }
    rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    float ms;
    if ((rc = run_check(g, "iteration", &ms)) != GS_OK) return rc;
    run_stats(g, stats, ff[1], ff[0], first_failure, iterations > 0 ? hist[1] : 0.0, iterations > 0 ? hist[std::min(iterations, nh)] : 0.0, ms);     // chi2: THIS rank's edges only (the ranks' sums add up to the graph's)
    if (ff[0]) { rc = reset_failure(g); if (rc != GS_OK) return rc;
        if (ff[0] == 2) { fall_back_to_levels(g); g_last_error = "a front's completion flag did not arrive in time: the handle now uses one launch per level"; }
        else if (ff[0] == 4) g_last_error = "another rank's whole-tree launch gave up on a front's flag, twice in this call";
        else g_last_error = ff[0] == 3 ? "another rank met a zero pivot (g2o: optimize() returns 0, the vertices keep the last good iterate)" : "zero pivot: H is singular (g2o: optimize() returns 0, the vertices keep the last good iterate)";
        return 0; }
    return ff[1];
}
// which vertex estimates this rank tracks (its own subtrees + the shared top), insertion order; a vertex is
// `primary` on exactly one rank (shared vertices: rank 0), so summing primary-masked estimates over ranks merges them
extern "C" int gs_dist_known(gs_graph *g, uint8_t *pose_known, uint8_t *lm_known, uint8_t *pose_primary, uint8_t *lm_primary) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->plan.valid) return fail(GS_ERR_NOT_INITIALIZED, "no plan built");
    const Plan &P = g->plan;
    auto primary = [&](int gidx, uint8_t known, uint8_t fixed) -> uint8_t {
        if (fixed || gidx < 0) return P.rank == 0;                      // fixed vertices never move: take them from rank 0
        if (!known) return 0;
        // shared <=> known on every rank
        return 1; };
    // a shared vertex is known everywhere; make rank 0 its primary holder
    std::vector<int32_t> front_of_scalar;                              // scalar -> front owner lookup via pivots
    front_of_scalar.assign(P.n_scalar, 0);
    for (size_t s = 0; s < P.fronts.size(); ++s) for (int k = 0; k < P.fronts[s].npiv; ++k) front_of_scalar[P.fronts[s].piv0 + k] = P.fronts[s].owner;
    for (int p = 0; p < g->h.n_poses(); ++p) { const int gi = P.pose_gidx[p]; uint8_t kn = P.pose_known[p], pr = primary(gi, kn, g->h.pose_fixed[p]);
        if (gi >= 0 && kn && front_of_scalar[gi] < 0) pr = P.rank == 0;
        if (pose_known) pose_known[p] = kn; if (pose_primary) pose_primary[p] = pr; }
    for (int l = 0; l < g->h.n_lms(); ++l) { const int gi = P.lm_gidx[l]; uint8_t kn = P.lm_known[l], pr = primary(gi, kn, g->h.lm_fixed[l]);
        if (gi >= 0 && kn && front_of_scalar[gi] < 0) pr = P.rank == 0;
        if (lm_known) lm_known[l] = kn; if (lm_primary) lm_primary[l] = pr; }
    return GS_OK;
}
