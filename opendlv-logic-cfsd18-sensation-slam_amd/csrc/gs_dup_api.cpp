// gs_dup_api.cpp — map twins behind the C-ABI (include/graphslam.h, "map twins"; kernels: gs_dup.hip): the batch and resident queries, the
// batch and in-place consolidations, which all end in the same launches, gs_map_get_xy, and gs_merge_landmarks on the handle's graph.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_dup.hpp"
#include "gs_dup_host.hpp"

#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

using namespace gs;

static_assert(DUP_MAP_MAX == GS_DUP_MAP_MAX && sizeof(gs_dup_info) == 16, "gs_dup_host.hpp restates the sizes");

extern "C" int gs_dup_params_default(gs_dup_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->require_same_type = 1; p->exclusive = 0; p->gate_chi2 = 5.991464547107979; p->max_distance = 1.0; p->sigma_floor = 0.05;
    return GS_OK;
}
// everything a caller can get wrong about the parameters, decided before the device is touched
static int dup_params_check(const gs_dup_params *p, DupDev &d) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_dup_params)) return fail(GS_ERR_INVALID, "gs_dup_params: wrong struct_size");
    if (!std::isfinite(p->gate_chi2) || !std::isfinite(p->max_distance) || !std::isfinite(p->sigma_floor)) return fail(GS_ERR_INVALID, "gs_dup_params: a parameter is not finite");
    if (p->gate_chi2 <= 0.0 || p->max_distance <= 0.0) return fail(GS_ERR_INVALID, "gs_dup_params: gate_chi2 and max_distance must be positive");
    if (p->sigma_floor < 0.0) return fail(GS_ERR_INVALID, "gs_dup_params: sigma_floor is negative");
    if ((p->require_same_type | p->exclusive) & ~1) return fail(GS_ERR_INVALID, "gs_dup_params: require_same_type and exclusive are 0 or 1");
    // sqrt(r2) < max_distance implies r2 < max_distance^2 <= fl(max_distance max_distance) (1 + 2^-52) while the product is a normal number:
    // the bound leaves room above that.  A max_distance so small that its square is not normal gets +inf: the first look lets every pair through
    const double md2 = p->max_distance * p->max_distance;
    const double md2_hi = md2 >= std::numeric_limits<double>::min() ? md2 * (1.0 + 0x1p-50) : std::numeric_limits<double>::infinity();
    d = DupDev{p->require_same_type, p->exclusive, p->gate_chi2, p->max_distance, md2_hi, p->sigma_floor * p->sigma_floor};
    return GS_OK;
}
static int dup_size_check(int64_t n) {
    return n > GS_DUP_MAP_MAX ? fail(GS_ERR_INVALID, "map twins: a map of more than GS_DUP_MAP_MAX cones") : GS_OK;
}
void gs_dup_release(gs_graph *g) { arena_release(g->fe.dp_mem); }
static int dup_launch_error(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GS_OK : fail(GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// room for a map of n cones (grow-only), and the pieces the consolidation's kernels pass on
static int dup_reserve(gs_graph *g, int n, DupLayout &L) {
    if (!dup_layout(n, L)) return fail(GS_ERR_INVALID, "map twins: bad size");
    return arena_reserve(g, g->fe.dp_mem, L.bytes);
}
static DupWork dup_work(const DevArena &a, const DupLayout &L, bool cov) {
    DupWork W{};
    W.twin = (const int32_t *)a.at(L.twin); W.nadm = (const int32_t *)a.at(L.nadm);
    W.slot = (int32_t *)a.at(L.slot); W.f_xy = (double *)a.at(L.f_xy); W.f_cov = (double *)a.at(L.f_cov);
    W.blk = (int32_t *)a.at(L.blk); W.blk_off = (int32_t *)a.at(L.blk_off); W.info = (gs_dup_info *)a.at(L.info);
    W.out_xy = (double *)a.at(L.out_xy); W.out_type = (int32_t *)a.at(L.out_type); W.out_cov = cov ? (double *)a.at(L.out_cov) : nullptr;
    W.remap = (int32_t *)a.at(L.remap);
    return W;
}
// a batch call's map into the arena
static hipError_t dup_upload(gs_graph *g, const DupLayout &L, int n, const double *xy, const int32_t *type, const double *cov, DupMap &m) {
    const DevArena &a = g->fe.dp_mem; hipError_t e = hipSuccess;
    HIP_NEXT(e, arena_upload(g, a, L.in_xy, xy, (size_t)n * 16));
    HIP_NEXT(e, arena_upload(g, a, L.in_type, type, (size_t)n * 4));
    if (cov) HIP_NEXT(e, arena_upload(g, a, L.in_cov, cov, (size_t)n * 32));
    m = DupMap{n, (const double *)a.at(L.in_xy), (const int32_t *)a.at(L.in_type), cov ? (const double *)a.at(L.in_cov) : nullptr};
    return e;
}
// the search into the arena's own outputs
static void dup_search(gs_graph *g, const DupMap &m, const DupDev &d, const DupLayout &L, hipEvent_t start, hipEvent_t stop) {
    const DevArena &a = g->fe.dp_mem;
    launch_dup_nearest(m, d, (int32_t *)a.at(L.twin), (double *)a.at(L.d2), (double *)a.at(L.second), (int32_t *)a.at(L.nadm), g->stream, start, stop);
}
// a consolidation enqueued: the search, the fusion, the scan, the scatter into the second buffer
static void dup_merge_enqueue(gs_graph *g, const DupMap &m, const DupDev &d, const DupLayout &L, const DupWork &W, hipEvent_t start, hipEvent_t stop) {
    dup_search(g, m, d, L, start, nullptr);
    launch_dup_fuse(m, d, W, g->stream);
    launch_dup_scan(m.n, W, g->stream);
    launch_dup_scatter(m, W, g->stream, stop);
}

extern "C" int gs_map_twins_batch(gs_graph *g, int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov, const gs_dup_params *params,
                                  int32_t *out_twin, double *out_d2, double *out_second, int32_t *out_na) {
    if (!g || n_map < 0 || (n_map > 0 && (!map_xy || !map_type || !out_twin))) return fail(GS_ERR_INVALID, "bad argument");
    DupDev d; int rc = dup_params_check(params, d); if (rc != GS_OK) return rc;
    if ((rc = dup_size_check(n_map)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_map == 0) return GS_OK;
    DupLayout L; if ((rc = dup_reserve(g, n_map, L)) != GS_OK) return rc;
    DupMap m; hipError_t e = dup_upload(g, L, n_map, map_xy, map_type, map_cov, m);
    if (e != hipSuccess) { (void)hipStreamSynchronize(g->stream); return fail(GS_ERR_HIP, std::string("map twins: upload: ") + hipGetErrorString(e)); }
    dup_search(g, m, d, L, nullptr, nullptr);
    const DevArena &a = g->fe.dp_mem; const size_t n = (size_t)n_map;
    auto fetch = [&](void *dst, size_t off, size_t bytes) { if (dst) HIP_NEXT(e, hipMemcpyAsync(dst, a.at(off), bytes, hipMemcpyDeviceToHost, g->stream)); };
    fetch(out_twin, L.twin, n * 4); fetch(out_d2, L.d2, n * 8); fetch(out_second, L.second, n * 8); fetch(out_na, L.nadm, n * 4);
    e = sync_keep_first(e, g->stream);                              // the one wait of the call
    g->fe.pin_map_busy = false;
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("map twins: ") + hipGetErrorString(e));
    return dup_launch_error("map twins");
}
extern "C" int gs_map_twins_resident(gs_graph *g, const gs_dup_params *params, int32_t *dev_out_twin, double *dev_out_d2, double *dev_out_second,
                                     int32_t *dev_out_na) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    DupDev d; int rc = dup_params_check(params, d); if (rc != GS_OK) return rc;
    const auto &fe = g->fe;
    if (fe.map_n > 0 && !dev_out_twin) return fail(GS_ERR_INVALID, "bad argument");
    if ((rc = dup_size_check(fe.map_n)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (fe.map_n == 0) return GS_OK;
    launch_dup_nearest(DupMap{fe.map_n, fe.map_xy, fe.map_type, fe.map_cov}, d, dev_out_twin, dev_out_d2, dev_out_second, dev_out_na, g->stream,
                       g->ev_lin[0], g->ev_lin[1]);
    return dup_launch_error("map twins");
}
extern "C" int gs_map_merge_twins_batch(gs_graph *g, int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov,
                                        const gs_dup_params *params, double *out_xy, int32_t *out_type, double *out_cov, int32_t *out_remap,
                                        gs_dup_info *out_info) {
    if (!g || n_map < 0 || (n_map > 0 && (!map_xy || !map_type || !out_xy || !out_type))) return fail(GS_ERR_INVALID, "bad argument");
    DupDev d; int rc = dup_params_check(params, d); if (rc != GS_OK) return rc;
    if ((rc = dup_size_check(n_map)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (out_info) *out_info = gs_dup_info{0, 0, 0, 0};
    if (n_map == 0) return GS_OK;
    DupLayout L; if ((rc = dup_reserve(g, n_map, L)) != GS_OK) return rc;
    DupMap m; hipError_t e = dup_upload(g, L, n_map, map_xy, map_type, map_cov, m);
    if (e != hipSuccess) { (void)hipStreamSynchronize(g->stream); return fail(GS_ERR_HIP, std::string("map twins: upload: ") + hipGetErrorString(e)); }
    const DevArena &a = g->fe.dp_mem; const size_t n = (size_t)n_map;
    const DupWork W = dup_work(a, L, map_cov != nullptr);
    dup_merge_enqueue(g, m, d, L, W, nullptr, nullptr);
    auto fetch = [&](void *dst, const void *src, size_t bytes) { if (dst && src) HIP_NEXT(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g->stream)); };
    fetch(out_xy, W.out_xy, n * 16); fetch(out_type, W.out_type, n * 4); fetch(out_cov, W.out_cov, n * 32); fetch(out_remap, W.remap, n * 4);
    fetch(out_info, W.info, sizeof(gs_dup_info));
    e = sync_keep_first(e, g->stream);                              // the one wait of the call
    g->fe.pin_map_busy = false;
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("map twins: ") + hipGetErrorString(e));
    return dup_launch_error("map twins");
}
extern "C" int gs_map_merge_twins(gs_graph *g, const gs_dup_params *params, int32_t capacity, int32_t *out_remap, gs_dup_info *out_info) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    DupDev d; int rc = dup_params_check(params, d); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    const int n_map = fe.map_n;
    if ((rc = dup_size_check(n_map)) != GS_OK) return rc;
    if (out_remap && capacity < n_map) return fail(GS_ERR_CAPACITY, "gs_map_merge_twins: out_remap holds fewer entries than the map has cones");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (out_info) *out_info = gs_dup_info{0, 0, 0, 0};
    if (n_map == 0) return GS_OK;
    DupLayout L; if ((rc = dup_reserve(g, n_map, L)) != GS_OK) return rc;
    const DevArena &a = fe.dp_mem; const size_t n = (size_t)n_map;
    const DupMap m{n_map, fe.map_xy, fe.map_type, fe.map_cov};
    const DupWork W = dup_work(a, L, fe.map_cov != nullptr);
    dup_merge_enqueue(g, m, d, L, W, nullptr, nullptr);
    // the second buffer back over the map, whole: behind n_out the scatter left free cones (NaN, type 0, zero covariance)
    hipError_t e = hipSuccess; gs_dup_info info{0, 0, 0, 0};
    HIP_NEXT(e, hipMemcpyAsync(fe.map_xy, W.out_xy, n * 16, hipMemcpyDeviceToDevice, g->stream));
    HIP_NEXT(e, hipMemcpyAsync(fe.map_type, W.out_type, n * 4, hipMemcpyDeviceToDevice, g->stream));
    if (fe.map_cov) HIP_NEXT(e, hipMemcpyAsync(fe.map_cov, W.out_cov, n * 32, hipMemcpyDeviceToDevice, g->stream));
    if (out_remap) HIP_NEXT(e, hipMemcpyAsync(out_remap, W.remap, n * 4, hipMemcpyDeviceToHost, g->stream));
    HIP_NEXT(e, hipMemcpyAsync(&info, W.info, sizeof(info), hipMemcpyDeviceToHost, g->stream));
    e = sync_keep_first(e, g->stream);                              // the one wait of the call: the host needs the new size
    fe.pin_map_busy = false;
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("map twins: ") + hipGetErrorString(e));
    if ((rc = dup_launch_error("map twins")) != GS_OK) return rc;
    if (info.n_in != n_map || info.n_out < 0 || info.n_out > n_map) return fail(GS_ERR_HIP, "map twins: the device's counters do not describe the map");
    fe.map_n = info.n_out; map_changed(g);
    if (out_info) *out_info = info;
    return GS_OK;
}
extern "C" int gs_map_get_xy(gs_graph *g, int32_t first, int32_t n, double *out_xy, int32_t *out_type) {
    if (!g || first < 0 || n < 0) return fail(GS_ERR_INVALID, "bad argument");
    if ((int64_t)first + n > g->fe.map_n) return fail(GS_ERR_INVALID, "beyond the end of the map");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    if (out_xy) HIP_TRY(hipMemcpyAsync(out_xy, g->fe.map_xy + 2 * (size_t)first, (size_t)n * 16, hipMemcpyDeviceToHost, g->stream));
    if (out_type) HIP_TRY(hipMemcpyAsync(out_type, g->fe.map_type + first, (size_t)n * 4, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->fe.pin_map_busy = false;
    return GS_OK;
}

// ---- timing hooks (graphslam_debug.h): a warming run, then `reps` runs each between an event pair on its first and last dispatch
template <class Once>
static int dup_time(gs_graph *g, int32_t reps, double *out_ms, Once once) {
    if (!g || !out_ms || reps <= 0) return fail(GS_ERR_INVALID, "bad argument");
    int rc = once(nullptr, nullptr); if (rc != GS_OK) return rc;
    std::vector<hipEvent_t> ev(2 * (size_t)reps, nullptr);
    hipError_t e = hipSuccess;
    for (auto &v : ev) HIP_NEXT(e, hipEventCreate(&v));
    for (int r = 0; r < reps && rc == GS_OK && e == hipSuccess; ++r) rc = once(ev[2 * (size_t)r], ev[2 * (size_t)r + 1]);
    e = sync_keep_first(e, g->stream);
    double tot = 0; int cnt = 0;
    for (int r = 0; r < reps && e == hipSuccess && rc == GS_OK; ++r) { float ms = 0;
        if (hipEventElapsedTime(&ms, ev[2 * (size_t)r], ev[2 * (size_t)r + 1]) == hipSuccess && ms > 0) { tot += ms; ++cnt; } }
    (void)hipGetLastError();
    for (auto &v : ev) if (v) hipEventDestroy(v);                    // on every path: nothing returns between the create and here
    *out_ms = cnt ? tot / cnt : 0.0;
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("map twins: timing: ") + hipGetErrorString(e));
    return rc;
}
extern "C" int gs_debug_time_map_twins_resident(gs_graph *g, const gs_dup_params *params, int32_t *dev_out_twin, double *dev_out_d2, double *dev_out_second,
                                                int32_t *dev_out_na, int32_t reps, double *out_ms) {
    if (!g || g->fe.map_n <= 0) return fail(GS_ERR_INVALID, "bad argument");
    return dup_time(g, reps, out_ms, [&](hipEvent_t a, hipEvent_t b) { g->ev_lin[0] = a; g->ev_lin[1] = b;
        const int rc = gs_map_twins_resident(g, params, dev_out_twin, dev_out_d2, dev_out_second, dev_out_na);
        g->ev_lin[0] = g->ev_lin[1] = nullptr; return rc; });
}
// the consolidation's four dispatches over the resident map into the second buffer; the map itself is left as it is
extern "C" int gs_debug_time_map_merge_twins(gs_graph *g, const gs_dup_params *params, int32_t reps, double *out_ms) {
    if (!g || g->fe.map_n <= 0) return fail(GS_ERR_INVALID, "bad argument");
    DupDev d; int rc = dup_params_check(params, d); if (rc != GS_OK) return rc;
    if ((rc = dup_size_check(g->fe.map_n)) != GS_OK) return rc;
    if ((rc = ensure_device(g)) != GS_OK) return rc;
    auto &fe = g->fe;
    DupLayout L; if ((rc = dup_reserve(g, fe.map_n, L)) != GS_OK) return rc;
    const DupMap m{fe.map_n, fe.map_xy, fe.map_type, fe.map_cov};
    const DupWork W = dup_work(fe.dp_mem, L, fe.map_cov != nullptr);
    return dup_time(g, reps, out_ms, [&](hipEvent_t a, hipEvent_t b) { dup_merge_enqueue(g, m, d, L, W, a, b); return dup_launch_error("map twins"); });
}

// ---- the graph side: g2o's mergeVertices(keep, drop, erase = true)
extern "C" int gs_merge_landmarks(gs_graph *g, int32_t keep_id, int32_t drop_id) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    auto k = g->h.lm_index.find(keep_id), dr = g->h.lm_index.find(drop_id);
    if (k == g->h.lm_index.end() || dr == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "gs_merge_landmarks: unknown landmark id");
    if (keep_id == drop_id) return fail(GS_ERR_INVALID, "gs_merge_landmarks: keep and drop are the same landmark");
    if (g->world > 1) return fail(GS_ERR_INVALID, "gs_merge_landmarks is not supported on sharded handles (gs_dist_configure with world > 1)");
    const int ki = k->second, di = dr->second;
    if (g->h.lm_fixed[(size_t)di] && !g->h.lm_fixed[(size_t)ki]) return fail(GS_ERR_INVALID, "gs_merge_landmarks: drop is fixed while keep is free");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;     // the host copy is about to be reshaped: it must be the newest
    if (!merge_landmarks(g->h, g->prior.store.lm_v, g->polar.store.lm_v, ki, di)) return fail(GS_ERR_INVALID, "gs_merge_landmarks: bad indices");
    if (!g->prior.store.lm_v.empty()) ++g->prior.store.version;     // both stores keep landmark INDICES: their device copies are stale
    if (!g->polar.store.empty()) ++g->polar.store.version;
    g->marg.valid = false;
    return GS_OK;
}
