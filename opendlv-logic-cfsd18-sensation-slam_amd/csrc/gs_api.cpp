// gs_api.cpp — C-ABI of the GraphSLAM back-end (include/graphslam.h) over the HIP kernels.
// Host side of the drop-in boundary: everything Slam calls on g2o::SparseOptimizer
// (reference src/slam.cpp:53-65, 433-484, 525-550, 713-732) lands here.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_parallel.hpp"
#include "gs_upload_host.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

namespace gs {
thread_local std::string g_last_error;
int fail(int code, const std::string &msg) { g_last_error = msg; return code; }
}  // namespace gs

// ------------------------------------------------------------------ helpers
static int usable_devices() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

// the handle's robust kernels (cfg.*_robust_*) travel to the kernels by value in DevGraph
static void apply_robust(gs_graph *g) {
    g->d.rk_pp = g->cfg.odometry_robust_kernel; g->d.rd_pp = g->cfg.odometry_robust_delta;
    g->d.rk_pl = g->cfg.observation_robust_kernel; g->d.rd_pl = g->cfg.observation_robust_delta;
}
static int robust_check(int32_t kernel, double delta) {
    if (kernel != GS_ROBUST_NONE && kernel != GS_ROBUST_HUBER && kernel != GS_ROBUST_CAUCHY) return fail(GS_ERR_INVALID, "unknown robust kernel (GS_ROBUST_NONE / HUBER / CAUCHY)");
    if (kernel != GS_ROBUST_NONE && !(std::isfinite(delta) && delta > 0.0)) return fail(GS_ERR_INVALID, "robust kernel: delta must be finite and > 0");
    return GS_OK;
}
// the device side of a plan goes away; keep = the memory stays with the handle for the next plan
static void dev_release(gs_graph *g, bool keep) {
    if (!keep) { for (auto &c : g->allocs) hipFree(c.p); g->allocs.clear(); }
    else for (auto &c : g->allocs) { c.in_use = false; if (pool_poison(g) && g->stream) hipMemsetAsync(c.p, 0xFF, c.size, g->stream); }
    g->pool_base = nullptr; g->pool_size = g->pool_off = 0; g->pool_next = 0; g->pool_total = 0;
    g->d = DevGraph(); apply_robust(g);
    g->dev_valid = false; g->linearised = false;
    g->room = gs_graph::GrowRoom(); g->d_bf = g->d_xrow = g->d_patch = g->d_list = nullptr;
    g->marg = gs_graph::Marginals();                                // its buffers were pool memory of the plan
    g->sched = Schedule(); for (auto &t : g->d_wg) t = nullptr;     // ... and so were the schedule's tables
}
static void dev_free_all(gs_graph *g) { dev_release(g, false); }
// after a structure phase: what the new plan did not take again goes back to the device
static void dev_trim(gs_graph *g) {
    size_t idle = 0;
    for (const auto &c : g->allocs) if (!c.in_use) idle += c.size;
    if (idle <= std::max<size_t>((size_t)64 << 20, g->pool_total / 2)) return;      // a modest reserve stays (hipFree is not free either: 0.3-0.5 ms for a 32 MB chunk)
    size_t w = 0;
    for (size_t i = 0; i < g->allocs.size(); ++i) { if (g->allocs[i].in_use) g->allocs[w++] = g->allocs[i]; else hipFree(g->allocs[i].p); }
    g->allocs.resize(w);
}

int ensure_device(gs_graph *g) {
    if (g->host_only) return fail(GS_ERR_NO_DEVICE, "host-only handle (device = -2): no compute without a gfx950 device");
    HIP_TRY(hipSetDevice(g->device));
    return GS_OK;
}

// ------------------------------------------------------------------ misc
extern "C" int gs_version(void) { return GS_VERSION_MAJOR * 100 + GS_VERSION_MINOR; }
extern "C" const char *gs_last_error(void) { return g_last_error.c_str(); }
extern "C" int gs_device_count(void) { return usable_devices(); }

extern "C" int gs_config_default(gs_config *c) {
    if (!c) return fail(GS_ERR_INVALID, "null config");
    std::memset(c, 0, sizeof(*c));
    c->struct_size = (int32_t)sizeof(gs_config);
    c->device = -1; c->verbose = 0; c->leaf_poses = 0; c->factor_variant = 0; c->linearize_gather = 0;
    c->odometry_information = 5.0;       // reference src/slam.cpp:456
    c->cone_information = 0.01;          // reference src/slam.cpp:546
    c->same_cone_threshold = 1.0;        // m_newConeThreshold default, reference src/slam.hpp:114
    c->cone_mapping_threshold = 67.0;    // reference src/slam.hpp:117
    c->lidar_to_cog = 1.5;               // reference src/slam.cpp:514
    c->loop_closing_radius = 1.0;        // reference src/slam.cpp:702
    c->loop_closing_min_index = 20;      // reference src/slam.cpp:702
    c->optimize_iterations = 10;         // reference src/slam.cpp:481
    c->reference_quirks = 0;
    c->odometry_robust_kernel = GS_ROBUST_NONE; c->odometry_robust_delta = 1.0;       // the reference sets no robust kernel
    c->observation_robust_kernel = GS_ROBUST_NONE; c->observation_robust_delta = 1.0;
    return GS_OK;
}


// ------------------------------------------------------------------ tuning switches (include/graphslam_debug.h)
extern "C" int gs_debug_options_default(gs_debug_options *o) {
    if (!o) return fail(GS_ERR_INVALID, "null options");
    std::memset(o, 0, sizeof(*o));
    o->struct_size = (int32_t)sizeof(*o);
    o->subtree = 0; o->tickets = 0; o->shard_by_window = 1;
    o->tree = 1; o->block_fronts = 512; o->leaf_kernel = -1; o->leaf_min = 2048; o->bs_wide = 1024; o->bs_low = 1; o->leaf_nt3 = 1; o->f3_lds_kb = 0;
    o->leaf_poses = 0; o->cluster_ways = 0; o->ell_lanes = 0; o->big_cluster = -1; o->grow_headroom = -1; o->factor_variant = 0;
    o->grow = 1; o->grow_min_poses = 128;
    o->assoc_grid = -1;
    o->force_shared_top = 0;
    o->host_trig = 0; o->pool_poison = 0; o->plan_timing = 0; o->dbg = 0;
    return GS_OK;
}
// The ONE place the environment is read: once per gs_create (graphslam_debug.h names the variable of every field).
static void options_from_environment(gs_debug_options &o) {
    gs_debug_options_default(&o);
    auto env = [](const char *name, int32_t &field) { if (const char *e = std::getenv(name)) field = (int32_t)std::atoi(e); };
    env("GS_TREE", o.tree); env("GS_BLOCK_FRONTS", o.block_fronts); env("GS_LEAF_KERNEL", o.leaf_kernel); env("GS_LEAF_MIN", o.leaf_min);
    env("GS_SUBTREE", o.subtree); env("GS_TICKETS", o.tickets); env("GS_SHARD_BY_WINDOW", o.shard_by_window); env("GS_BS_WIDE", o.bs_wide); env("GS_BS_LOW", o.bs_low); env("GS_LEAF_NT3", o.leaf_nt3); env("GS_F3_LDS_KB", o.f3_lds_kb);
    env("GS_LEAF_POSES", o.leaf_poses); env("GS_CLUSTER_WAYS", o.cluster_ways); env("GS_ELL_LANES", o.ell_lanes); env("GS_BIG_CLUSTER", o.big_cluster);
    env("GS_GROW_HEADROOM", o.grow_headroom); env("GS_FACTOR_VARIANT", o.factor_variant);
    env("GS_GROW", o.grow); env("GS_GROW_MIN_POSES", o.grow_min_poses); env("GS_ASSOC_GRID", o.assoc_grid); env("GS_FORCE_SHARED_TOP", o.force_shared_top);
    env("GS_HOST_TRIG", o.host_trig); env("GS_POOL_POISON", o.pool_poison); env("GS_DBG", o.dbg);
    if (std::getenv("GS_PLAN_TIMING")) o.plan_timing = 1;
}
extern "C" int gs_debug_get_options(gs_graph *g, gs_debug_options *o) {
    if (!g || !o) return fail(GS_ERR_INVALID, "null argument");
    *o = g->opt; return GS_OK;
}
extern "C" int gs_debug_set_options(gs_graph *g, const gs_debug_options *o) {
    if (!g || !o) return fail(GS_ERR_INVALID, "null argument");
    gs_debug_options n; gs_debug_options_default(&n);
    std::memcpy(&n, o, std::min<size_t>(sizeof(n), (size_t)std::max(o->struct_size, 0))); n.struct_size = (int32_t)sizeof(n);
    const gs_debug_options &c = g->opt;
    // a "plan" field changed: the next structure phase is a full one (a grown plan keeps the launch shapes it was built with)
    const bool plan_changed = n.tree != c.tree || n.block_fronts != c.block_fronts || n.leaf_kernel != c.leaf_kernel || n.leaf_min != c.leaf_min ||
        n.bs_wide != c.bs_wide || n.bs_low != c.bs_low || n.subtree != c.subtree || n.tickets != c.tickets || n.shard_by_window != c.shard_by_window || n.leaf_nt3 != c.leaf_nt3 || n.f3_lds_kb != c.f3_lds_kb || n.leaf_poses != c.leaf_poses ||
        n.cluster_ways != c.cluster_ways || n.ell_lanes != c.ell_lanes || n.big_cluster != c.big_cluster || n.grow_headroom != c.grow_headroom ||
        n.factor_variant != c.factor_variant || n.force_shared_top != c.force_shared_top || n.host_trig != c.host_trig || n.pool_poison != c.pool_poison ||
        n.dbg != c.dbg;
    g->opt = n;
    if (plan_changed) { ++g->h.structure_version; ++g->h.reshape_version; }
    return GS_OK;
}

extern "C" int gs_create(const gs_config *cfg, gs_graph **out) {
    if (!out) return fail(GS_ERR_INVALID, "null out");
    *out = nullptr;
    gs_config c;
    gs_config_default(&c);
    if (cfg) { size_t n = std::min<size_t>(sizeof(c), (size_t)std::max(cfg->struct_size, 0)); std::memcpy(&c, cfg, n); c.struct_size = (int32_t)sizeof(c); }
    { int rc = robust_check(c.odometry_robust_kernel, c.odometry_robust_delta); if (rc != GS_OK) return rc;
      rc = robust_check(c.observation_robust_kernel, c.observation_robust_delta); if (rc != GS_OK) return rc;
      if (c.odometry_robust_kernel == GS_ROBUST_NONE) c.odometry_robust_delta = 1.0;           // (unused; kept valid)
      if (c.observation_robust_kernel == GS_ROBUST_NONE) c.observation_robust_delta = 1.0; }
    if (c.device == -2) {   // host-only handle: graph container + plan inspection, never any arithmetic
        gs_graph *g = new gs_graph(); g->cfg = c; g->device = -2; g->host_only = true; options_from_environment(g->opt); *out = g; return GS_OK; }
    int ndev = usable_devices();
    if (ndev <= 0) return fail(GS_ERR_NO_DEVICE, "no HIP device: this back-end has no CPU fallback");
    int dev = c.device;
    if (dev < 0) { if (hipGetDevice(&dev) != hipSuccess) dev = 0; }
    if (dev >= ndev) return fail(GS_ERR_NO_DEVICE, "device ordinal out of range");
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GS_ERR_NO_DEVICE, std::string("device is ") + prop.gcnArchName + ", kernels are built for gfx950 only");
    gs_graph *g = new gs_graph();
    g->cfg = c; g->device = dev; g->force_gather = c.linearize_gather != 0;
    apply_robust(g);
    options_from_environment(g->opt);
    HIP_TRY(hipSetDevice(dev));
    if (hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking) != hipSuccess) { delete g; return fail(GS_ERR_HIP, "hipStreamCreate failed"); }
    g->own_stream = true;
    for (auto &e : g->ev) hipEventCreate(&e);
    *out = g;
    return GS_OK;
}

extern "C" int gs_destroy(gs_graph *g) {
    if (!g) return GS_OK;
    if (g->host_only) { delete g; return GS_OK; }
    hipSetDevice(g->device);
    hipStreamSynchronize(g->stream);
    dev_free_all(g);
    if (g->lm.mem) hipFree(g->lm.mem);
    if (g->dl.mem) hipFree(g->dl.mem);
    side_release(g);
    gs_dist_comm_release(g);
    gs_frontend_release(g);
    for (auto &e : g->ev) hipEventDestroy(e);
    if (g->own_stream) hipStreamDestroy(g->stream);
    delete g;
    return GS_OK;
}

extern "C" int gs_clear(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (!g->host_only) { hipSetDevice(g->device); hipStreamSynchronize(g->stream); dev_free_all(g); }
    g->h.clear(); g->plan = Plan(); g->plan_version = ~0ull;
    side_clear(g);
    return GS_OK;
}

// ------------------------------------------------------------------ robust kernels
extern "C" int gs_set_robust_kernel(gs_graph *g, int32_t edge_kind, int32_t kernel, double delta) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (edge_kind != GS_EDGE_ODOMETRY && edge_kind != GS_EDGE_OBSERVATION) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    int rc = robust_check(kernel, delta); if (rc != GS_OK) return rc;
    if (kernel != GS_ROBUST_NONE && g->world > 1) return fail(GS_ERR_INVALID, "robust kernels are not supported on sharded handles (gs_dist_configure with world > 1)");
    if (kernel == GS_ROBUST_NONE) delta = 1.0;
    if (edge_kind == GS_EDGE_ODOMETRY) { g->cfg.odometry_robust_kernel = kernel; g->cfg.odometry_robust_delta = delta; }
    else { g->cfg.observation_robust_kernel = kernel; g->cfg.observation_robust_delta = delta; }
    apply_robust(g);                        // the kernels take the setting by value at their next launch: no structure phase, no wait
    g->marg.valid = false;                  // H changes with the weights
    return GS_OK;
}
extern "C" int gs_get_robust_kernel(gs_graph *g, int32_t edge_kind, int32_t *out_kernel, double *out_delta) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    if (edge_kind != GS_EDGE_ODOMETRY && edge_kind != GS_EDGE_OBSERVATION) return fail(GS_ERR_INVALID, "edge kind must be GS_EDGE_ODOMETRY or GS_EDGE_OBSERVATION");
    const bool pp = edge_kind == GS_EDGE_ODOMETRY;
    if (out_kernel) *out_kernel = pp ? g->cfg.odometry_robust_kernel : g->cfg.observation_robust_kernel;
    if (out_delta) *out_delta = pp ? g->cfg.odometry_robust_delta : g->cfg.observation_robust_delta;
    return GS_OK;
}

extern "C" int gs_reserve_device(gs_graph *g, int64_t bytes) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    int64_t have = 0;
    for (const auto &c : g->allocs) if (!c.big && !c.in_use) have += (int64_t)c.size;
    for (size_t want = (size_t)8 << 20; have < bytes; want = std::min<size_t>(want << 1, (size_t)128 << 20)) {     // the sizes dev_alloc asks for, in its order
        bool held = false;
        for (const auto &c : g->allocs) held = held || (!c.big && !c.in_use && c.size == want);
        if (held && want < ((size_t)128 << 20)) continue;
        void *p = nullptr;
        HIP_TRY(hipMalloc(&p, want));
        HIP_TRY(hipMemsetAsync(p, 0, want, g->stream));              // touch it now: the mapping work of a fresh allocation otherwise lands on the first launch that follows
        gs_graph::DevChunk c; c.p = p; c.size = want; g->allocs.push_back(c); have += (int64_t)want; }
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
extern "C" int gs_set_stream(gs_graph *g, void *s) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    { int rc = ensure_device(g); if (rc != GS_OK) return rc; }
    hipStreamSynchronize(g->stream);
    if (g->own_stream) { hipStreamDestroy(g->stream); g->own_stream = false; }
    if (s) g->stream = (hipStream_t)s;
    else { HIP_TRY(hipStreamCreateWithFlags(&g->stream, hipStreamNonBlocking)); g->own_stream = true; }
    return GS_OK;
}


extern "C" int gs_add_pose(gs_graph *g, int32_t id, const double est[3]) {
    if (!g || !est) return fail(GS_ERR_INVALID, "null argument");
    if (g->h.pose_index.count(id)) return fail(GS_ERR_DUPLICATE_ID, "pose id already present");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    g->h.pose_index[id] = g->h.n_poses();
    g->h.pose_id.push_back(id); g->h.pose_est.insert(g->h.pose_est.end(), est, est + 3); g->h.pose_fixed.push_back(0);
    ++g->h.structure_version;
    return GS_OK;
}
extern "C" int gs_add_landmark(gs_graph *g, int32_t id, const double est[2]) {
    if (!g || !est) return fail(GS_ERR_INVALID, "null argument");
    if (g->h.lm_index.count(id)) return fail(GS_ERR_DUPLICATE_ID, "landmark id already present");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    g->h.lm_index[id] = g->h.n_lms();
    g->h.lm_id.push_back(id); g->h.lm_est.insert(g->h.lm_est.end(), est, est + 2); g->h.lm_fixed.push_back(0);
    ++g->h.structure_version;
    return GS_OK;
}
bool sym_ok(const double *m, int n) {
    for (int r = 0; r < n; ++r) for (int c = 0; c < r; ++c) {
        double a = m[r * n + c], b = m[c * n + r];
        if (!(std::fabs(a - b) <= 1e-12 * (std::fabs(a) + std::fabs(b)) + 1e-300)) return false;
    }
    return true;
}
extern "C" int gs_add_odometry_edge(gs_graph *g, int32_t idi, int32_t idj, const double z[3], const double info[9]) {
    if (!g || !z || !info) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.pose_index.find(idi), b = g->h.pose_index.find(idj);
    if (a == g->h.pose_index.end() || b == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "odometry edge references an unknown pose");
    if (a->second == b->second) return fail(GS_ERR_INVALID, "odometry edge joins a pose to itself");
    if (!sym_ok(info, 3)) return fail(GS_ERR_INVALID, "information matrix not symmetric");
    g->h.pp_i.push_back(a->second); g->h.pp_j.push_back(b->second);
    g->h.pp_z.insert(g->h.pp_z.end(), z, z + 3);
    const double s[6] = {info[0], info[1], info[2], info[4], info[5], info[8]};
    g->h.pp_info.insert(g->h.pp_info.end(), s, s + 6);
    ++g->h.structure_version;
    return GS_OK;
}
extern "C" int gs_add_observation_edge(gs_graph *g, int32_t idp, int32_t idl, const double z[2], const double info[4]) {
    if (!g || !z || !info) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.pose_index.find(idp); auto b = g->h.lm_index.find(idl);
    if (a == g->h.pose_index.end() || b == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "observation edge references an unknown vertex");
    if (!sym_ok(info, 2)) return fail(GS_ERR_INVALID, "information matrix not symmetric");
    g->h.pl_p.push_back(a->second); g->h.pl_l.push_back(b->second);
    g->h.pl_z.insert(g->h.pl_z.end(), z, z + 2);
    const double s[3] = {info[0], info[1], info[3]};
    g->h.pl_info.insert(g->h.pl_info.end(), s, s + 3);
    ++g->h.structure_version;
    return GS_OK;
}
extern "C" int gs_add_poses(gs_graph *g, int32_t n, const int32_t *ids, const double *est) {
    if (!g || (n > 0 && (!ids || !est))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_pose(g, ids[k], est + 3 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_landmarks(gs_graph *g, int32_t n, const int32_t *ids, const double *est) {
    if (!g || (n > 0 && (!ids || !est))) return fail(GS_ERR_INVALID, "null argument");
    for (int k = 0; k < n; ++k) { int rc = gs_add_landmark(g, ids[k], est + 2 * (size_t)k); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_odometry_edges(gs_graph *g, int32_t n, const int32_t *idi, const int32_t *idj, const double *z, const double *info) {
    if (!g || (n > 0 && (!idi || !idj || !z))) return fail(GS_ERR_INVALID, "null argument");
    const double w = g->cfg.odometry_information;
    const double def[9] = {w, 0, 0, 0, w, 0, 0, 0, w};
    for (int k = 0; k < n; ++k) { int rc = gs_add_odometry_edge(g, idi[k], idj[k], z + 3 * (size_t)k, info ? info + 9 * (size_t)k : def); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_add_observation_edges(gs_graph *g, int32_t n, const int32_t *idp, const int32_t *idl, const double *z, const double *info) {
    if (!g || (n > 0 && (!idp || !idl || !z))) return fail(GS_ERR_INVALID, "null argument");
    const double w = g->cfg.cone_information;
    const double def[4] = {w, 0, 0, w};
    for (int k = 0; k < n; ++k) { int rc = gs_add_observation_edge(g, idp[k], idl[k], z + 2 * (size_t)k, info ? info + 4 * (size_t)k : def); if (rc != GS_OK) return rc; }
    return GS_OK;
}
extern "C" int gs_set_fixed_pose(gs_graph *g, int32_t id, int32_t fixed) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    auto a = g->h.pose_index.find(id);
    if (a == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown pose id");
    uint8_t f = fixed != 0;
    if (g->h.pose_fixed[a->second] != f) { g->h.pose_fixed[a->second] = f; ++g->h.structure_version; ++g->h.reshape_version; }
    return GS_OK;
}
extern "C" int gs_set_fixed_landmark(gs_graph *g, int32_t id, int32_t fixed) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    auto a = g->h.lm_index.find(id);
    if (a == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown landmark id");
    uint8_t f = fixed != 0;
    if (g->h.lm_fixed[a->second] != f) { g->h.lm_fixed[a->second] = f; ++g->h.structure_version; ++g->h.reshape_version; }
    return GS_OK;
}
extern "C" int gs_set_pose_estimate(gs_graph *g, int32_t id, const double est[3]) {
    if (!g || !est) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.pose_index.find(id);
    if (a == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown pose id");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    std::memcpy(&g->h.pose_est[3 * (size_t)a->second], est, 3 * sizeof(double));
    ++g->h.estimate_version;
    return GS_OK;
}
extern "C" int gs_set_landmark_estimate(gs_graph *g, int32_t id, const double est[2]) {
    if (!g || !est) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.lm_index.find(id);
    if (a == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown landmark id");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    std::memcpy(&g->h.lm_est[2 * (size_t)a->second], est, 2 * sizeof(double));
    ++g->h.estimate_version;
    return GS_OK;
}

// ------------------------------------------------------------------ read-back (A11)
int pull_estimates_enqueue(gs_graph *g, bool &pull) {
    pull = g->dev_valid && g->dev_estimates_newer;
    if (!pull) return GS_OK;
    const int N = g->d.N + g->d.tN, M = g->d.M + g->d.tM;          // (tail vertices of a grown plan follow the base ones in the same arrays)
    if (N > 0) HIP_TRY(hipMemcpyAsync(g->h.pose_est.data(), g->d.pose_est, (size_t)N * 3 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    if (M > 0) HIP_TRY(hipMemcpyAsync(g->h.lm_est.data(), g->d.lm_est, (size_t)M * 2 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    return GS_OK;
}
int pull_estimates_if_needed(gs_graph *g) {
    if (!g->dev_valid || !g->dev_estimates_newer) return GS_OK;
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    bool pull; if ((rc = pull_estimates_enqueue(g, pull)) != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->dev_estimates_newer = false;
    return GS_OK;
}
// The device-side failure state: fail[0] = code (1 zero pivot, 2 a whole-tree launch gave up on a front's flag, 3 a
// zero pivot another rank reported, 4 a flag timeout another rank reported), fail[1] = updates applied since the last reset.  k_update applies nothing once the
// code is non-zero, so the estimates in HBM are those of the last good iterate, as in g2o after a failed solve.
static int read_failure(gs_graph *g, int32_t out[2]) {
    out[0] = out[1] = 0;
    if (!g->dev_valid || !g->d.fail) return GS_OK;
    HIP_TRY(hipMemcpyAsync(out, g->d.fail, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    return GS_OK;
}
int reset_failure(gs_graph *g) {
    g->d.inject_iter = 0; g->d.inject_code = 0;
    HIP_TRY(hipMemsetAsync(g->d.fail, 0, 4 * sizeof(int32_t), g->stream));
    // the ticket counter and its host-side running sum start again together (a launch that failed to ENQUEUE was counted on the host only)
    if (g->d.tickets) { HIP_TRY(hipMemsetAsync(g->d.tickets, 0, 2 * sizeof(uint32_t), g->stream)); g->d.ticket_base = 0; }
    return GS_OK;
}
// After gs_iterate / gs_dist_iterate_*: report a failure of the iterations run since the last report (once), apply the
// one-launch-per-level fallback after a flag timeout.  The estimates stay at the last good iterate either way.
static int surface_failure(gs_graph *g) {
    int32_t st[2]; int rc = read_failure(g, st); if (rc != GS_OK) return rc;
    if (st[0] == 0) return GS_OK;
    rc = reset_failure(g); if (rc != GS_OK) return rc;
    if (st[0] == 2) { g->d.tree = 0; g->fell_back = true;
        return fail(GS_ERR_TIMEOUT, "whole-tree launch: a front's completion flag did not arrive in time; no update was applied from that "
                                    "iteration on (estimates = last good iterate); the handle now uses one launch per level"); }
    if (st[0] == 4) return fail(GS_ERR_TIMEOUT, "a whole-tree launch of ANOTHER rank gave up on a front's flag (that rank now uses one launch per level); no update was applied from that "
                                                "iteration on (estimates = last good iterate): the iteration can be run again");
    return fail(GS_ERR_NUMERIC, st[0] == 3 ? "another rank met a zero pivot: no update applied from that iteration on (estimates = last good iterate)"
                                           : "zero pivot: H is singular; no update applied from that iteration on (estimates = last good iterate)");
}
extern "C" int gs_sync_estimates(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    if (g->host_only || !g->dev_valid) return GS_OK;
    return surface_failure(g);
}
extern "C" int gs_stream_synchronize(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    return surface_failure(g);
}
extern "C" int gs_debug_fail_at_iteration(gs_graph *g, int32_t k, int32_t code) {
    if (!g || k < 0 || (code != 1 && code != 2)) return fail(GS_ERR_INVALID, "bad argument");
    if (!g->dev_valid) return fail(GS_ERR_NOT_INITIALIZED, "call gs_initialize_optimization first");
    g->d.inject_iter = k > 0 ? g->d.iter + k : 0; g->d.inject_code = code;
    return GS_OK;
}
extern "C" int gs_get_pose(gs_graph *g, int32_t id, double out[3]) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.pose_index.find(id);
    if (a == g->h.pose_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown pose id");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    std::memcpy(out, &g->h.pose_est[3 * (size_t)a->second], 3 * sizeof(double));
    return GS_OK;
}
extern "C" int gs_get_landmark(gs_graph *g, int32_t id, double out[2]) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    auto a = g->h.lm_index.find(id);
    if (a == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown landmark id");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    std::memcpy(out, &g->h.lm_est[2 * (size_t)a->second], 2 * sizeof(double));
    return GS_OK;
}
extern "C" int gs_num_poses(gs_graph *g) { return g ? g->h.n_poses() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_num_landmarks(gs_graph *g) { return g ? g->h.n_lms() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_num_odometry_edges(gs_graph *g) { return g ? g->h.n_pp() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_num_observation_edges(gs_graph *g) { return g ? g->h.n_pl() : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_get_poses(gs_graph *g, int32_t cap, int32_t *ids, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    if (cap < g->h.n_poses()) return fail(GS_ERR_CAPACITY, "buffer too small");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    if (ids) std::memcpy(ids, g->h.pose_id.data(), g->h.pose_id.size() * sizeof(int32_t));
    std::memcpy(out, g->h.pose_est.data(), g->h.pose_est.size() * sizeof(double));
    return g->h.n_poses();
}
extern "C" int gs_get_landmarks(gs_graph *g, int32_t cap, int32_t *ids, double *out) {
    if (!g || !out) return fail(GS_ERR_INVALID, "null argument");
    if (cap < g->h.n_lms()) return fail(GS_ERR_CAPACITY, "buffer too small");
    int rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    if (ids) std::memcpy(ids, g->h.lm_id.data(), g->h.lm_id.size() * sizeof(int32_t));
    std::memcpy(out, g->h.lm_est.data(), g->h.lm_est.size() * sizeof(double));
    return g->h.n_lms();
}

// ------------------------------------------------------------------ structure phase (A3/A4); the upload: gs_upload.cpp
// The factor kernel a plan gets (gs_config.factor_variant; gs_debug_options.factor_variant overrides): 0 = default = 3.
//   3 = LDL^T on the fp64 matrix cores, latency-shaped: a front of up to 63 scalars a wave, one of 64 .. 159 a workgroup, chosen per
//   front; 4 = block-per-front VALU Cholesky (any front size, 64-bit addressing throughout).  (Rounds 1-3 also kept a wave-per-front
//   VALU kernel and a first matrix-core Cholesky as variants 1 and 2; nothing but tests ran them: removed in round 4, requests for
//   them get variant 3.)
// Variant 3 names every scalar of the linearised system by a 32-bit BYTE offset into H_arena ((uint32_t)record * 8 in the front
// kernels): beyond 2^29 doubles (4 GiB) those would wrap and assemble the wrong entries silently, so such a graph gets variant 4.
extern "C" int gs_debug_select_factor_variant(int32_t requested, int32_t max_front, int64_t arena_doubles) {
    int v = requested;
    if (v != 4) v = 3;
    if (v == 3 && max_front > 159) v = 4;                           // variant 3: a wave up to 63 scalars, a workgroup up to 159 (ten tile rows)
    if (v == 3 && arena_doubles >= ((int64_t)1 << 29)) v = 4;
    return v;
}

// ... as the device-side code a plan's upload and its schedule use (0 = the block-per-front kernel)
int plan_factor_variant(const gs_graph *g, int64_t arena_doubles) {
    const int v = gs_debug_select_factor_variant(g->opt.factor_variant > 0 ? g->opt.factor_variant : g->cfg.factor_variant, g->plan.max_front, arena_doubles);
    return v == 4 ? 0 : v;
}

static int build_plan_host(gs_graph *g) {
    PlanOptions o; o.leaf_poses = g->cfg.leaf_poses; o.world = g->world; o.rank = g->rank;
    const gs_debug_options &t = g->opt;                             // tuning overrides (graphslam_debug.h)
    if (t.leaf_poses > 0) o.leaf_poses = t.leaf_poses;
    if (t.cluster_ways > 0) o.cluster_ways = t.cluster_ways;             // 2 = binary dissection down to the leaves
    if (t.ell_lanes > 0) o.ell_lanes = t.ell_lanes;                      // lanes per pose of the ELL layout
    if (t.big_cluster >= 0) o.big_cluster_front = t.big_cluster;         // 0 = clusters only where they fit a wave
    if (t.grow_headroom >= 0) { o.grow_headroom = t.grow_headroom; o.grow_spine_headroom = std::min(o.grow_spine_headroom, 3 * o.grow_headroom); }   // 0 = cluster fronts up to the full 63 scalars
    o.timing = t.plan_timing > 0;
    o.by_window = t.shard_by_window != 0;
    o.force_shared_top = g->world <= 1 ? std::max(t.force_shared_top, 0) : 0;
    if (g->world > 1 && !g->lm_seen_interior.empty()) {
        if ((int)g->lm_seen_interior.size() != g->h.n_lms()) return fail(GS_ERR_INVALID, "gs_dist_set_landmark_windows: the masks cover another number of landmarks than the graph holds");
        o.lm_seen_interior = g->lm_seen_interior.data(); o.lm_seen_first = g->lm_seen_first.data(); }
    std::string err;
    if (!build_plan(g->h, o, g->plan, err, &g->plan_ws)) { g->plan_version = ~0ull; return fail(GS_ERR_EMPTY, "plan: " + err); }
    g->plan_version = g->h.structure_version;
    return GS_OK;
}

extern "C" int gs_plan_build_host(gs_graph *g, gs_plan_info *info) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = GS_OK;
    // a host-only handle absorbs appended poses / edges the way a device handle does (gs::grow_plan), so that the grown plan can be
    // inspected and replayed without a GPU; GS_GROW=0 or any other change: full build
    bool grown = false;
    if (g->host_only && g->plan.valid && g->plan_version != ~0ull && g->plan_version != g->h.structure_version) {
        const bool on = g->opt.grow != 0;
        Growth gr; std::string why;
        if (on && grow_plan(g->h, g->plan, gr, why)) { grown = true; g->plan_version = g->h.structure_version; g->no_growth_reason.clear(); }
        else g->no_growth_reason = on ? why : "growth switched off (gs_debug_options.grow = 0 / GS_GROW=0)";
    }
    if (!grown) { rc = build_plan_host(g); if (rc != GS_OK) return rc; }
    if (info) { const Plan &P = g->plan; info->n_scalar = P.n_scalar; info->n_fronts = (int32_t)P.fronts.size();
        info->n_levels = (int32_t)P.level_start.size() - 1; info->max_front = P.max_front; info->l_doubles = P.l_doubles;
        info->u_doubles = P.u_doubles; info->n_asm_blocks = (int64_t)P.asm_recs.size(); info->n_child_map = (int64_t)P.child_map.size(); }
    // a host-only plan must not be mistaken for an uploaded one
    if (g->dev_valid && !g->host_only) { hipSetDevice(g->device); hipStreamSynchronize(g->stream); pull_estimates_if_needed(g); dev_free_all(g); }
    return GS_OK;
}
extern "C" int gs_plan_growths(gs_graph *g) { return g ? g->plan.n_growths : fail(GS_ERR_INVALID, "null graph"); }
extern "C" const char *gs_growth_refusal(gs_graph *g) { return g ? g->no_growth_reason.c_str() : ""; }
extern "C" int gs_plan_export(gs_graph *g, int32_t *out, int64_t *out_len) {
    if (!g || !out_len) return fail(GS_ERR_INVALID, "null argument");
    if (!g->plan.valid) return fail(GS_ERR_NOT_INITIALIZED, "no plan built");
    std::vector<int32_t> v; export_plan(g->plan, v);
    if (!out) { *out_len = (int64_t)v.size(); return GS_OK; }
    if (*out_len < (int64_t)v.size()) return fail(GS_ERR_CAPACITY, "buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(int32_t)); *out_len = (int64_t)v.size();
    return GS_OK;
}

// the schedule of the current plan: the one the device runs from when the plan is uploaded, else (host-only handle, after gs_plan_build_host)
// built the way upload_graph builds it — without the arena-size rule of the variant choice, which needs the device layout
extern "C" int gs_debug_schedule_export(gs_graph *g, int32_t *out, int64_t *out_len) {
    if (!g || !out_len) return fail(GS_ERR_INVALID, "null argument");
    if (!g->plan.valid) return fail(GS_ERR_NOT_INITIALIZED, "no plan built");
    std::vector<int32_t> v;
    if (g->dev_valid && g->plan_version == g->h.structure_version) export_schedule(g->plan, g->sched, v);
    else { const Plan &P = g->plan;
        const std::vector<int32_t> pos = pos_of_front(P, level_list(P));
        export_schedule(P, build_schedule(P, pos, plan_factor_variant(g, 0), g->opt.tree != 0, g->opt), v); }
    if (!out) { *out_len = (int64_t)v.size(); return GS_OK; }
    if (*out_len < (int64_t)v.size()) return fail(GS_ERR_CAPACITY, "buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(int32_t)); *out_len = (int64_t)v.size();
    return GS_OK;
}

extern "C" int gs_initialize_optimization(gs_graph *g) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto t0 = std::chrono::steady_clock::now();
    rc = pull_estimates_if_needed(g); if (rc != GS_OK) return rc;
    HIP_TRY(hipStreamSynchronize(g->stream));
    // priors added or cleared since the last call, nothing else: not a structural change — the plan on the device stays (grown or not),
    // the prior tables go up.  (A call with NO change at all still rebuilds, as g2o's initializeOptimization does.)
    if (g->dev_valid && g->plan.valid && g->plan_version == g->h.structure_version && g->prior.store.version != g->prior.settled) {
        g->no_growth_reason.clear();
        rc = push_estimates(g); if (rc != GS_OK) return rc;          // (what the rebuild this call replaces would have uploaded: gs_iterate does not look)
        return prior_sync(g); }
    // append-only growth: poses / edges added since the plan was built enter the existing plan and device tables (gs::grow_plan,
    // upload_growth); anything else — or GS_GROW=0 — rebuilds
    g->no_growth_reason.clear();
    if (g->dev_valid && g->plan.valid && g->plan_version != ~0ull && g->plan_version != g->h.structure_version) {
        const bool on = g->opt.grow != 0;
        Growth gr; std::string why;
        // below ~a hundred poses the full phase costs 0.25 ms, the tail kernel of ten iterations 0.08: nothing to gain (a lap, 200 poses
        // mapped: 1.03 ms per optimize(10) grown against 1.16 rebuilt, scripts/keyframe_stream.py)
        const int min_poses = g->opt.grow_min_poses;
        if (!on) g->no_growth_reason = "growth switched off (gs_debug_options.grow = 0 / GS_GROW=0)";
        else if (g->plan.base_N < min_poses) g->no_growth_reason = "graph below the size at which growing pays (GS_GROW_MIN_POSES)";
        else if (!g->room.ok) g->no_growth_reason = "plan uploaded without room to grow";
        else if (grow_plan(g->h, g->plan, gr, why)) {
            rc = upload_growth(g, gr);
            if (rc == GS_OK) { g->plan_version = g->h.structure_version;
                g->ms_structure = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
                return GS_OK; }
            g->no_growth_reason = g_last_error;                     // (the plan object is rebuilt from scratch below)
        } else g->no_growth_reason = why;
    }
    StepTimer ST(g->opt.plan_timing != 0, "structure", 24);
    dev_release(g, true);                                            // the handle keeps its device memory for the new plan
    RawUpload raw;
    rc = upload_raw_begin(g, raw); if (rc != GS_OK) { if (raw.th.joinable()) raw.th.join(); dev_free_all(g); return rc; }
    ST("release + raw begin");
    rc = build_plan_host(g);                                        // the host threads build the plan while the raw arrays travel
    ST("plan (host)");
    raw.th.join();
    ST("wait for the raw upload");
    if (rc == GS_OK && raw.rc != GS_OK) rc = fail(raw.rc, raw.err);
    if (rc != GS_OK) { dev_free_all(g); return rc; }
    rc = upload_graph(g, raw); if (rc != GS_OK) { dev_free_all(g); return rc; }
    ST("upload_graph");
    dev_trim(g);
    ST("trim");
    g->ms_structure = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    return GS_OK;
}

int ensure_ready(gs_graph *g) {
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (!g->dev_valid || g->plan_version != g->h.structure_version) { if ((rc = gs_initialize_optimization(g)) != GS_OK) return rc; }
    else if ((rc = push_estimates(g)) != GS_OK) return rc;
    return side_sync(g);
}

// ------------------------------------------------------------------ what the three side passes share on the host (gs_private.hpp)
int arena_reserve(gs_graph *g, DevArena &a, size_t total) {
    if (a.mem && total <= a.cap) return GS_OK;
    HIP_TRY(hipStreamSynchronize(g->stream));
    arena_release(a);
    const size_t cap = total + total / 2 + 4096;
    if (hipMalloc(&a.mem, cap) != hipSuccess) { a.mem = nullptr; return fail(GS_ERR_HIP, "hipMalloc failed"); }
    a.cap = cap;
    return GS_OK;
}
hipError_t arena_upload(gs_graph *g, const DevArena &a, size_t off, const void *src, size_t bytes) {
    return bytes ? hipMemcpyAsync(a.at(off), src, bytes, hipMemcpyHostToDevice, g->stream) : hipSuccess;
}
void arena_release(DevArena &a) { if (a.mem) hipFree(a.mem); a.mem = nullptr; a.cap = 0; }

int side_sync(gs_graph *g) {
    int rc = prior_sync(g); if (rc != GS_OK) return rc;              // (nothing without priors)
    if ((rc = edge_mask_sync(g)) != GS_OK) return rc;                // (nothing on a handle that never had an inactive edge)
    return polar_sync(g);                                            // (nothing without polar edges)
}
void side_clear(gs_graph *g) {
    g->prior.store.clear(); g->prior.dev.n_pv = g->prior.dev.n_lv = 0; g->prior.sync.invalidate();      // the priors go with their vertices
    g->emask.store.clear(); g->emask.sync.invalidate();              // ... and the flags with their edges
    g->polar.store.clear(); g->polar.dev = PolarDev(); g->polar.sync.invalidate();                      // ... and the polar measurements with their carriers
}
void side_release(gs_graph *g) { arena_release(g->prior.arena); arena_release(g->emask.arena); arena_release(g->polar.arena); }
int pl_location(const gs_graph *g, int32_t k, int32_t &src, const char *prefix) {
    const Plan &P = g->plan;
    if (k < P.base_Epl) { src = (size_t)k < P.ell_of_ins.size() ? P.ell_of_ins[(size_t)k] : -1;
        if (src < 0) return fail(GS_ERR_INVALID, std::string(prefix) + "observation edge outside the linearisation layout"); }
    else { if (k - P.base_Epl >= g->d.tEpl) return fail(GS_ERR_INVALID, std::string(prefix) + "observation edge not on the device"); src = -(k - P.base_Epl) - 1; }
    return GS_OK;
}
bool lm_lacks_fused_slot(const gs_graph *g, int32_t l) {
    return g->d.n_wtiles > 0 && l < g->d.M && !g->h.lm_fixed[(size_t)l] && !(g->plan.lm_grp_start[(size_t)l] < g->plan.lm_grp_start[(size_t)l + 1]);
}

void fill_plan_stats(gs_graph *g, gs_stats *s) {
    const Plan &P = g->plan;
    s->n_free_poses = 0; s->n_free_landmarks = 0;
    for (auto v : P.pose_gidx) s->n_free_poses += v >= 0;
    for (auto v : P.lm_gidx) s->n_free_landmarks += v >= 0;
    s->n_odometry_edges = g->h.n_pp(); s->n_observation_edges = g->h.n_pl();
    s->n_fronts = (int32_t)P.fronts.size(); s->n_levels = (int32_t)P.level_start.size() - 1; s->max_front = P.max_front;
    s->factor_flops = P.factor_flops; s->factor_bytes = (P.l_doubles + P.u_doubles) * 8; s->ms_structure = g->ms_structure;
    s->fell_back = g->fell_back ? 1 : 0;
    s->factor_variant = g->dev_valid ? (g->d.factor_variant == 0 ? 4 : g->d.factor_variant) : 0;
    s->n_big_fronts = 0;
    for (const Front &F : P.fronts) s->n_big_fronts += (!F.opaque && F.npiv + F.nbnd > 63);
    s->device_bytes = (int64_t)g->pool_total; s->ms_plan_host = P.ms_build; s->n_growths = P.n_growths;
    s->n_own_fronts = (int32_t)P.level_fronts_owned.size(); s->n_shared_fronts = (int32_t)P.level_fronts_shared.size();
    s->n_subtrees = g->sched.sub_n;
    s->n_pose_priors = g->prior.store.n_pose(); s->n_landmark_priors = g->prior.store.n_lm();
}

extern "C" int gs_get_stats(gs_graph *g, gs_stats *s) {
    if (!g || !s) return fail(GS_ERR_INVALID, "null argument");
    if (!g->plan.valid) return fail(GS_ERR_NOT_INITIALIZED, "no plan built");
    std::memset(s, 0, sizeof(*s)); s->struct_size = (int32_t)sizeof(*s);
    fill_plan_stats(g, s);
    return GS_OK;
}
