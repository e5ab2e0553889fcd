// gs_api.cpp — C-ABI of the GraphSLAM back-end (include/graphslam.h) over the HIP kernels.
// Host side of the drop-in boundary: everything Slam calls on g2o::SparseOptimizer
// (reference src/slam.cpp:53-65, 433-484, 525-550, 713-732) lands here.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_parallel.hpp"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
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

template <class T, class A> static int dev_upload(gs_graph *g, T **ptr, const std::vector<T, A> &v) {
    int rc = dev_alloc(g, ptr, v.size());
    if (rc != GS_OK) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(*ptr, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, g->stream));
    return GS_OK;
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
    g->dev_valid = false;
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
    o->tree = 1; o->block_fronts = 512; o->leaf_kernel = -1; o->leaf_min = 2048; o->bs_wide = 2048; o->leaf_nt3 = 1; o->f3_lds_kb = 0;
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
    env("GS_SUBTREE", o.subtree); env("GS_TICKETS", o.tickets); env("GS_SHARD_BY_WINDOW", o.shard_by_window); env("GS_BS_WIDE", o.bs_wide); env("GS_LEAF_NT3", o.leaf_nt3); env("GS_F3_LDS_KB", o.f3_lds_kb);
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
        n.bs_wide != c.bs_wide || n.subtree != c.subtree || n.tickets != c.tickets || n.shard_by_window != c.shard_by_window || n.leaf_nt3 != c.leaf_nt3 || n.f3_lds_kb != c.f3_lds_kb || n.leaf_poses != c.leaf_poses ||
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
    g->cfg = c; g->device = dev; g->force_gather = c.linearize_gather != 0; g->default_factor_variant = c.factor_variant;
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

// ------------------------------------------------------------------ structure phase (A3/A4) + upload
static void se2_inverse_host(const double *a, double *out) {
    auto norm = [](double th) { if (th >= -M_PI && th < M_PI) return th; double m = std::floor(th / (2 * M_PI)); th -= m * 2 * M_PI;
                                if (th >= M_PI) th -= 2 * M_PI; if (th < -M_PI) th += 2 * M_PI; return th; };
    double th = norm(-a[2]); double c = std::cos(th), s = std::sin(th);
    out[0] = c * (-a[0]) - s * (-a[1]); out[1] = s * (-a[0]) + c * (-a[1]); out[2] = th;
}

// Everything that does not depend on the plan goes to HBM on a helper thread WHILE the host builds the plan: estimates,
// fixed flags, odometry measurements (inverted, with their cos/sin: g2o keeps _inverseMeasurement) and information,
// and the observation edges as inserted (permuted into the ELL layout on the device afterwards).
struct RawUpload {
    std::thread th; int rc = GS_OK; std::string err;
    ~RawUpload() { if (th.joinable()) th.join(); }                  // an exception (bad_alloc in the plan build) must not meet a joinable thread: std::terminate
    int32_t *pl_l = nullptr; double *pl_z = nullptr, *pl_info = nullptr;
    std::vector<double> zinv; size_t pp_lo = 0, pp_hi = 0;         // the odometry edges whose records went up: [pp_lo, pp_hi) (all of them on a single GPU)
    uvec<int32_t> ell_l; uvec<double> ell_z, ell_w;               // pose-window shards: the ELL streams, filled on the host (they must outlive the copies: upload_graph ends with a sync)
};
static int upload_raw_begin(gs_graph *g, RawUpload &R) {
    const HostGraph &h = g->h; DevGraph &d = g->d;
    const size_t N = h.n_poses(), M = h.n_lms(), Epp = h.n_pp(), Epl = h.n_pl();
    int rc;
    // room for the tail of a grown plan (gs::grow_plan) behind the per-pose and per-odometry-edge arrays
    const size_t TP = TAIL_POSES, TPP = TAIL_PP;
    const size_t TL = TAIL_LMS;
    if ((rc = dev_alloc(g, &d.pose_est, (N + TP) * 3)) != GS_OK || (rc = dev_alloc(g, &d.lm_est, (M + TL) * 2)) != GS_OK ||
        (rc = dev_alloc(g, &d.pose_fixed, N + TP)) != GS_OK || (rc = dev_alloc(g, &d.lm_fixed, M + TL)) != GS_OK ||
        (rc = dev_alloc(g, &d.pose_cs, (N + TP) * 2)) != GS_OK || (rc = dev_alloc(g, &d.pp_zinv, (Epp + TPP) * 5)) != GS_OK ||
        (rc = dev_alloc(g, &d.pp_info, (Epp + TPP) * 6)) != GS_OK) return rc;
    HIP_TRY(hipMemsetAsync(d.pose_fixed + N, 0, TP, g->stream)); HIP_TRY(hipMemsetAsync(d.lm_fixed + M, 0, TL, g->stream));
    // the observation edges as inserted travel now only on a single GPU; a pose-window shard uploads the ones it evaluates, in
    // device layout, once the plan says which they are (upload_graph)
    const bool raw_pl = g->world <= 1;
    if (raw_pl && ((rc = dev_alloc(g, &R.pl_l, Epl)) != GS_OK || (rc = dev_alloc(g, &R.pl_z, Epl * 2)) != GS_OK || (rc = dev_alloc(g, &R.pl_info, Epl * 3)) != GS_OK)) return rc;
    R.th = std::thread([g, &R, N, M, Epp, Epl, raw_pl] {
        const HostGraph &h = g->h; DevGraph &d = g->d;
        auto cp = [&](void *dst, const void *src, size_t bytes) {
            if (R.rc != GS_OK || bytes == 0) return;
            hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g->stream);
            if (e != hipSuccess) { R.rc = GS_ERR_HIP; R.err = std::string("raw upload: ") + hipGetErrorString(e); } };
        if (hipSetDevice(g->device) != hipSuccess) { R.rc = GS_ERR_HIP; R.err = "hipSetDevice failed on the upload thread"; return; }
        cp(d.pose_est, h.pose_est.data(), N * 3 * sizeof(double)); cp(d.lm_est, h.lm_est.data(), M * 2 * sizeof(double));
        cp(d.pose_fixed, h.pose_fixed.data(), N); cp(d.lm_fixed, h.lm_fixed.data(), M);
        if (raw_pl) { cp(R.pl_l, h.pl_l.data(), Epl * sizeof(int32_t)); cp(R.pl_z, h.pl_z.data(), Epl * 2 * sizeof(double));
            cp(R.pl_info, h.pl_info.data(), Epl * 3 * sizeof(double)); }
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
        cp(d.pp_info + 6 * k0, h.pp_info.data() + 6 * k0, (k1 - k0) * 6 * sizeof(double));
        R.zinv.resize((k1 - k0) * 5);
        for (size_t k = k0; k < k1; ++k) { double inv[3]; se2_inverse_host(&h.pp_z[3 * k], inv);
            double *o = &R.zinv[5 * (k - k0)]; o[0] = inv[0]; o[1] = inv[1]; o[2] = inv[2]; o[3] = std::cos(inv[2]); o[4] = std::sin(inv[2]); }
        cp(d.pp_zinv + 5 * k0, R.zinv.data(), (k1 - k0) * 5 * sizeof(double));
    });
    return GS_OK;
}

// the workgroup tables of the schedule (plans with a front of more than 63 scalars) go to the device with the plan; the copies read the
// handle's own vectors
static int upload_tables(gs_graph *g) {
    for (int t = 0; t < N_TABS; ++t) { g->d_wg[t] = nullptr;
        if (g->sched.big) { int rc = dev_upload(g, (int32_t **)&g->d_wg[t], g->sched.tab[t].wg); if (rc != GS_OK) return rc; } }
    return GS_OK;
}

static int upload_graph(gs_graph *g, RawUpload &raw) {
    const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    const bool ut_on = g->opt.plan_timing > 0; auto ut_prev = std::chrono::steady_clock::now();
#define GS_UT(name) do { if (ut_on) { auto n_ = std::chrono::steady_clock::now(); std::fprintf(stderr, "upload %-18s %.2f ms\n", (name), std::chrono::duration<double, std::milli>(n_ - ut_prev).count()); ut_prev = n_; } } while (0)
    const int N = h.n_poses(), M = h.n_lms(), Epp = h.n_pp(), Epl = h.n_pl();
    d.N = N; d.M = M; d.Epp = Epp; d.Epl = Epl; d.n_scalar = P.n_scalar;
    int rc;
#define UP(dst, vec) if ((rc = dev_upload(g, &d.dst, vec)) != GS_OK) return rc
    // estimates, fixed flags, odometry edges and the insertion-order observation arrays are in HBM already (RawUpload)
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
    if ((rc = dev_alloc(g, &d.pose_gidx, (size_t)N + TAIL_POSES)) != GS_OK) return rc;              // (room for a grown plan's tail poses)
    if (N > 0) HIP_TRY(hipMemcpyAsync(d.pose_gidx, P.pose_gidx.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    if ((rc = dev_alloc(g, &d.lm_gidx, (size_t)M + TAIL_LMS)) != GS_OK) return rc;
    if (M > 0) HIP_TRY(hipMemcpyAsync(d.lm_gidx, P.lm_gidx.data(), (size_t)M * sizeof(int32_t), hipMemcpyHostToDevice, g->stream));
    d.ell_T = P.ell_T; d.ell_R = P.ell_R; d.ell_len = P.ell_len; d.ell_p0 = P.ell_p0; d.ell_np = P.ell_np;
    { const size_t L = (size_t)P.ell_len;
      if ((rc = dev_alloc(g, &d.ell_l, L)) != GS_OK || (rc = dev_alloc(g, &d.ell_z, 2 * L)) != GS_OK || (rc = dev_alloc(g, &d.ell_w, 3 * L)) != GS_OK) return rc;
      if (P.world <= 1) {                                            // ELL streams: permuted on the device out of the arrays that travelled during the plan build (k_build_ell)
          int32_t *ins = nullptr;
          if ((rc = dev_upload(g, &ins, P.ell_ins)) != GS_OK) return rc;
          launch_build_ell((int64_t)L, ins, raw.pl_l, raw.pl_z, raw.pl_info, nullptr, P.rank, d.ell_l, d.ell_z, d.ell_w, g->stream);
      } else {                                                       // pose-window shard: only the poses it sweeps are laid out; the streams are filled on the host
          // ... on a thread of its own, beside the rest of this function (nothing here reads the streams; joined before the final wait): the fill
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
              if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess) { raw.rc = GS_ERR_HIP; raw.err = "edge streams: copy to the device failed"; } }); } }
    GS_UT("estimates+edges");
    UP(lm_start, P.lm_start); UP(lm_edges, P.lm_edges); UP(ppadj_start, P.ppadj_start);
    { const size_t Q = P.ppinc.size() / 4;                                // device records are 8 bytes: {edge, other endpoint | role << 31}; the pose that
      std::vector<int32_t> inc(2 * Q);                                    // holds the record is known to the kernel; an edge another rank evaluates: edge = -1
      for (size_t q = 0; q < Q; ++q) { const int32_t k = P.ppinc[4 * q], role = P.ppinc[4 * q + 1], other = role ? P.ppinc[4 * q + 2] : P.ppinc[4 * q + 3];
          inc[2 * q] = (P.world > 1 && P.pp_rank[k] != P.rank) ? -1 : k; inc[2 * q + 1] = (int32_t)((uint32_t)other | ((uint32_t)role << 31)); }
      UP(ppinc, inc);
      // a shard's helper thread sent the records of the odometry edges [pp_lo, pp_hi) — the ones that touch its window; an edge the plan gives
      // this rank outside that range (none, by the assignment rule: kept as a check that cannot go wrong silently) is sent now
      std::vector<int32_t> miss;
      for (size_t q = 0; q < Q; ++q) { const int32_t k = inc[2 * q]; if (k >= 0 && ((size_t)k < raw.pp_lo || (size_t)k >= raw.pp_hi)) miss.push_back(k); }
      std::sort(miss.begin(), miss.end()); miss.erase(std::unique(miss.begin(), miss.end()), miss.end());
      for (int32_t k : miss) { double inv[3], o[5]; se2_inverse_host(&h.pp_z[3 * (size_t)k], inv);
          o[0] = inv[0]; o[1] = inv[1]; o[2] = inv[2]; o[3] = std::cos(inv[2]); o[4] = std::sin(inv[2]);
          HIP_TRY(hipMemcpy(d.pp_zinv + 5 * (size_t)k, o, sizeof(o), hipMemcpyHostToDevice));
          HIP_TRY(hipMemcpy(d.pp_info + 6 * (size_t)k, &h.pp_info[6 * (size_t)k], 6 * sizeof(double), hipMemcpyHostToDevice)); }
      g->pp_records_late = (int)miss.size();
      if (ut_on && !miss.empty()) std::fprintf(stderr, "upload: %d odometry edge records sent after the plan\n", (int)miss.size()); }
#define AL(dst, cnt) if ((rc = dev_alloc(g, &d.dst, (size_t)(cnt))) != GS_OK) return rc
#define ZERO(dst, cnt) HIP_TRY(hipMemsetAsync(d.dst, 0, std::max<size_t>((size_t)(cnt), 1) * sizeof(*d.dst), g->stream))
    d.n_wtiles = 0; d.n_groups = 0; d.wt_lo = 0; d.wt_hi = 0; d.rank = P.rank;
    // the fused kernel addresses the ELL planes with 32-bit byte offsets: 8 B * ell_len must stay below 4 GiB
    if (P.lin_ell_ok && !g->force_gather && P.ell_len < ((int64_t)1 << 29)) {
        d.n_wtiles = P.n_wtiles; d.n_groups = (int32_t)P.grp_lm.size();
        UP(wt_desc, P.wt_desc); UP(lm_grp_start, P.lm_grp_start);
        { const size_t Gn = P.grp_slot.size(); std::vector<int32_t> gt(2 * Gn + 2, 0);   // per group {first | end << 16 of its tile-local positions, partial-sum slot}
          for (int w = P.wt_lo; w < P.wt_hi; ++w) { const int ga = P.wt_desc[4 * (size_t)w], gn = P.wt_desc[4 * (size_t)w + 1], pos_off = P.wt_desc[4 * (size_t)w + 2];
              for (int q = ga; q < ga + gn; ++q) { gt[2 * (size_t)q] = (P.grp_pos_start[q] - pos_off) | ((P.grp_pos_start[q + 1] - pos_off) << 16); gt[2 * (size_t)q + 1] = P.grp_slot[q]; } }
          UP(grp_tab, gt); }
        UP(ell_dst, P.ell_dst);
        d.wt_lo = P.wt_lo; d.wt_hi = P.wt_hi;                             // the wave tiles this shard has any edge in (gs_plan.cpp)
    } else if (P.world > 1) return fail(GS_ERR_INVALID, "pose-window shards need the fused linearisation layout (<= 32 observations per pose)");
    // block-sparse H and b live in ONE arena (the variant-3 front assembly addresses every scalar by its offset in it)
    int64_t arena_off[14], arena_doubles = 0;
    { // (the last six parts: the blocks of a grown plan's tail — diagonal blocks and rhs of tail poses / landmarks, off-diagonal blocks of tail edges)
      const int64_t sizes[13] = {(int64_t)N * 6, (int64_t)N * 3, (int64_t)Epp * 9, (int64_t)P.ell_len * 6, (int64_t)d.n_groups * 8, (int64_t)M * 3, (int64_t)M * 2,
                                 (int64_t)TAIL_POSES * 6, (int64_t)TAIL_POSES * 3, (int64_t)TAIL_PP * 9, (int64_t)TAIL_PL * 6, (int64_t)TAIL_LMS * 3, (int64_t)TAIL_LMS * 2};
      arena_off[0] = 0;
      for (int k = 0; k < 13; ++k) { arena_off[k + 1] = arena_off[k] + ((sizes[k] + 1) & ~(int64_t)1);       // 16-byte aligned parts
          if (k + 1 == 4) arena_off[4] = (arena_off[4] + 7) & ~(int64_t)7; }                                   // (the partial-sum records: one 64-byte line each)
      if (arena_off[13] >= ((int64_t)1 << 31)) return fail(GS_ERR_INVALID, "graph too large for 32-bit arena offsets");
      arena_doubles = arena_off[13];
      AL(H_arena, (size_t)arena_off[13] + 2);
      // blocks of edges / tiles this rank never evaluates must read as zero
      ZERO(H_arena, (size_t)arena_off[13] + 2);
      d.t_Hpp_diag = d.H_arena + arena_off[7]; d.t_b_pose = d.H_arena + arena_off[8]; d.t_Hpp_off = d.H_arena + arena_off[9]; d.t_Hpl = d.H_arena + arena_off[10];
      d.t_Hll_diag = d.H_arena + arena_off[11]; d.t_b_lm = d.H_arena + arena_off[12];
      AL(t_pp_ij, (size_t)TAIL_PP * 2); AL(t_pl, (size_t)TAIL_PL * 2); AL(t_pl_z, (size_t)TAIL_PL * 2); AL(t_pl_w, (size_t)TAIL_PL * 3);
      AL(t_pose_start, (size_t)TAIL_POSES + 1); AL(t_pose_edges, (size_t)TAIL_PL); AL(t_lt_id, (size_t)TAIL_PL); AL(t_lt_start, (size_t)TAIL_PL + 1); AL(t_lt_edges, (size_t)TAIL_PL);
      // (the fused linearisation kernel stores Hpp_diag's 6 planes and b_pose's 3 as 9 contiguous planes: 6N is even, no padding between)
      d.Hpp_diag = d.H_arena + arena_off[0]; d.b_pose = d.H_arena + arena_off[1]; d.Hpp_off = d.H_arena + arena_off[2];
      d.Hpl = d.H_arena + arena_off[3]; d.lm_part = d.H_arena + arena_off[4]; d.Hll_diag = d.H_arena + arena_off[5]; d.b_lm = d.H_arena + arena_off[6]; }
    d.n_chi2_partial = std::max((N + 255) / 256, d.n_wtiles);
    AL(chi2_partial, d.n_chi2_partial + 1); AL(chi2, 80); ZERO(chi2_partial, d.n_chi2_partial + 1);     // (+1: the partial of a grown plan's tail)
    UP(pose_known, P.pose_known); UP(lm_known, P.lm_known);
    GS_UT("tiles+arena");
    // plan
    { std::vector<DevFront> df(P.fronts.size());
      for (size_t s = 0; s < P.fronts.size(); ++s) { const Front &F = P.fronts[s]; DevFront &o = df[s];
          o.npiv = F.npiv; o.nbnd = F.nbnd; o.piv0 = F.piv0; o.parent = F.parent; o.asm_off = F.asm_off; o.asm_cnt = F.asm_cnt;
          o.asm_dup = F.asm_dup; o.child_off = F.child_off; o.child_cnt = F.child_cnt; o.owner = F.owner; o.level = F.level; o.pad0 = 0;
          o.bnd_off = F.bnd_off; o.map_off = F.map_off; o.L_off = F.L_off; o.U_off = F.U_off; }
      UP(fronts, df); d.n_fronts = (int32_t)df.size(); }
    // boundary rows, child maps and assembly records with room behind them: a growth step re-writes the runs of the fronts it changes there
    // (sized with the plan, within bounds: a lap-sized graph must not pay for a 100k-pose graph's room with extra device chunks)
    auto room_of = [](size_t n, size_t lo, size_t hi) { return std::min(hi, std::max(lo, n / 2)); };
    const size_t ROOM_ROWS = room_of(P.bnd_rows.size(), 8 * 1024, 64 * 1024), ROOM_RECS = room_of(P.asm_recs.size(), 12 * 1024, 96 * 1024);
    { auto up_room = [&](int32_t **dst, const int32_t *src, size_t n, size_t room) -> int {
          int r2 = dev_alloc(g, dst, n + room); if (r2 != GS_OK) return r2;
          if (n) { hipError_t e = hipMemcpyAsync(*dst, src, n * sizeof(int32_t), hipMemcpyHostToDevice, g->stream); if (e != hipSuccess) return fail(GS_ERR_HIP, hipGetErrorString(e)); }
          return GS_OK; };
      if ((rc = up_room(&d.bnd_rows, P.bnd_rows.data(), P.bnd_rows.size(), ROOM_ROWS)) != GS_OK) return rc;
      if ((rc = up_room(&d.child_map, P.child_map.data(), P.child_map.size(), ROOM_ROWS)) != GS_OK) return rc;
      g->room.cap_bnd = (int64_t)(P.bnd_rows.size() + ROOM_ROWS); g->room.cap_map = (int64_t)(P.child_map.size() + ROOM_ROWS); }
    UP(children, P.children);
    { std::vector<int32_t> cd(P.children.size() * 4);
      for (size_t q = 0; q < P.children.size(); ++q) { const Front &C = P.fronts[P.children[q]];
          cd[4 * q] = P.children[q]; cd[4 * q + 1] = C.npiv | (C.nbnd << 16); cd[4 * q + 2] = C.owner; cd[4 * q + 3] = (int32_t)C.map_off; }
      UP(child_desc, cd); }
    // level lists on the device: this rank's own fronts, then the shared top (empty when world == 1)
    { std::vector<int32_t> lf = P.level_fronts_owned;
      lf.insert(lf.end(), P.level_fronts_shared.begin(), P.level_fronts_shared.end());
      UP(level_fronts, lf); }
    d.xfail_off = -1; d.iter = 0; d.inject_iter = 0; d.inject_code = 0;
    if (P.dist) { UP(x_off, P.x_off);
        d.xfail_off = P.exchange_doubles - 2;                             // the ranks' failure flags ride at the tail of the exchange buffer
        if (!g->exchange_external) { AL(exchange, P.exchange_doubles); ZERO(exchange, P.exchange_doubles); }
        else d.exchange = g->exchange; }
    { static_assert(sizeof(AsmRec) == 16, "AsmRec is uploaded as 4 int32");
      if ((rc = dev_alloc(g, &d.asm_recs, (P.asm_recs.size() + ROOM_RECS) * 4)) != GS_OK) return rc;
      if (!P.asm_recs.empty()) HIP_TRY(hipMemcpyAsync(d.asm_recs, P.asm_recs.data(), P.asm_recs.size() * sizeof(AsmRec), hipMemcpyHostToDevice, g->stream));
      g->room.cap_asm = (int64_t)(P.asm_recs.size() + ROOM_RECS); }
    GS_UT("plan arrays");
    // factor kernel variant (gs_config.factor_variant; gs_debug_options.factor_variant overrides): 0 = default = 3 when every
    // front fits 159 scalars, else 4.  3 = LDL^T on the fp64 matrix cores, a wave or a workgroup per front; 4 = block-per-front
    // VALU Cholesky (any front size).
    { int v = g->default_factor_variant;
      if (g->opt.factor_variant > 0) v = g->opt.factor_variant;
      v = gs_debug_select_factor_variant(v, P.max_front, arena_doubles);
      if (v == 4) v = 0;                                              // device-side code for the block-per-front kernel
      d.factor_variant = v;
      d.dbg = g->opt.dbg; d.leaf_nt3 = g->opt.leaf_nt3 != 0 ? 1 : 0; d.f3_lds_kb = std::max(g->opt.f3_lds_kb, 0);
      if (v == 3) {
          std::vector<int32_t> lf = P.level_fronts_owned;
          lf.insert(lf.end(), P.level_fronts_shared.begin(), P.level_fronts_shared.end());
          constexpr int F3W = 224;                           // 32 descriptor ints + the row tables of the first two children + the front's own store table
          // update matrices, packed: row r' (0 .. nbnd, the last = rhs) of the boundary block holds columns 0 .. min(r', nbnd - 1)
          // at r'(r'+1)/2; then one double that stays zero (clamped gathers land on it) and one that collects clamped stores
          std::vector<int32_t> u3_off(P.fronts.size()), u3_size(P.fronts.size());
          { int64_t tot = 0;
            for (size_t f0 = 0; f0 < P.fronts.size(); ++f0) { const int nb = P.fronts[f0].nbnd;
                u3_off[f0] = (int32_t)tot; u3_size[f0] = (nb * (nb + 1)) / 2 + nb; tot += ((u3_size[f0] + 2 + 1) & ~1);
                if (tot >= ((int64_t)1 << 31)) return fail(GS_ERR_INVALID, "update-matrix arena beyond 32-bit offsets"); }
            const int64_t ROOM_U = (int64_t)room_of((size_t)tot, (size_t)128 << 10, (size_t)(P.max_front > 63 ? 4 : 1) << 20);      // doubles: the update matrices of fronts a growth step enlarges move here
            if (tot + ROOM_U >= ((int64_t)1 << 31)) return fail(GS_ERR_INVALID, "update-matrix arena beyond 32-bit offsets");
            AL(Uimg, (size_t)(tot + ROOM_U) + 2); ZERO(Uimg, (size_t)(tot + ROOM_U) + 2);
            g->room.used_U = tot; g->room.cap_U = tot + ROOM_U; }
          UP(u3_off, u3_off); UP(u3_size, u3_size);
          g->u3_off_host = u3_off; g->u3_size_host = u3_size;
          AL(done_f, P.fronts.size()); ZERO(done_f, P.fronts.size());
          d.tickets = nullptr; d.ticket_base = 0;
          if (g->opt.tickets != 0) { AL(tickets, 2); ZERO(tickets, 2); }    // workgroups of the whole-tree launches take their number from this counter (gs_kernels.hip, "tickets")
          d.epoch = 0; d.tree = g->opt.tree != 0 ? 1 : 0; g->fell_back = false; g->fallback_calls = 0; g->fallback_retry_after = 4; g->fallback_retrying = false;   // whole-tree launches for this rank's own subtrees (gs_debug_options.tree = 0: one launch per level)
          // ---- everything below is expanded ON THE DEVICE from the compact plan arrays
          const bool fused = P.lin_ell_ok && d.n_wtiles > 0;
          // block assembly records: the plan's, as they are (AsmRec = 4 ints); landmark-diagonal records of the fused
          // linearisation get their partial-slot range patched in by a kernel
          if ((rc = dev_alloc(g, &d.asm3, (P.asm_recs.size() + ROOM_RECS) * 4)) != GS_OK) return rc;
          if (!P.asm_recs.empty()) HIP_TRY(hipMemcpyAsync(d.asm3, P.asm_recs.data(), P.asm_recs.size() * sizeof(AsmRec), hipMemcpyHostToDevice, g->stream));
          if (fused) { for (int l = 0; l < M; ++l) if (P.lm_grp_start[l + 1] - P.lm_grp_start[l] >= (1 << 22)) return fail(GS_ERR_INVALID, "landmark seen from too many wave tiles");
              launch_patch_asm3((int64_t)P.asm_recs.size(), d.asm3, d.lm_grp_start, g->stream); }
          GS_UT("asm3");
          // scalar assembly records {offset in H_arena, offset in the staging image}, padded per front to a multiple of
          // 64 with (0 -> image offset 1, a don't-care upper-triangle slot); fused landmark diagonals go to lm3.
          // The host only counts them per front.
          { const size_t S = P.fronts.size();
            std::vector<int32_t> bf(8 * S, 0);
            parallel_chunks((int64_t)S, 2048, [&](int64_t b, int64_t e, int) {
                for (int64_t sidx = b; sidx < e; ++sidx) { const Front &F = P.fronts[sidx]; int ns = 0, nl = 0;
                    for (int t = F.asm_off; t < F.asm_off + F.asm_cnt - F.asm_dup; ++t) { const int k = P.asm_recs[t].kind;
                        if (k == 0) ns += 9; else if (k == 1) { if (fused) ++nl; else ns += 5; } else if (k <= 3) ns += 9; else if (k == 6) ns += 5; else ns += 6; }
                    bf[8 * sidx + 4] = (ns + 63) & ~63; bf[8 * sidx + 6] = nl; } });
            int64_t so = 0, lo = 0;
            for (size_t sidx = 0; sidx < S; ++sidx) { const Front &F = P.fronts[sidx]; int32_t *r = &bf[8 * sidx];
                if (so >= ((int64_t)1 << 31) - 64) return fail(GS_ERR_INVALID, "too many assembly scalars");
                r[0] = F.asm_off; r[1] = F.asm_cnt - F.asm_dup; r[2] = F.npiv + F.nbnd; r[3] = (int32_t)so; r[5] = (int32_t)lo; so += r[4]; lo += r[6]; }
            const int64_t ROOM_SC = (int64_t)room_of((size_t)so, (size_t)64 << 10, (size_t)(P.max_front > 63 ? 4 : 1) << 19);         // scalar records of the fronts a growth step rebuilds
            if (so + ROOM_SC >= ((int64_t)1 << 31) - 64) return fail(GS_ERR_INVALID, "too many assembly scalars");
            AL(sc3, 2 * (size_t)(so + ROOM_SC) + 2); AL(lm3, 4 * (size_t)lo + 4);
            g->room.used_sc = so; g->room.cap_sc = so + ROOM_SC;
            int32_t *bf_dev = nullptr; if ((rc = dev_upload(g, &bf_dev, bf)) != GS_OK) return rc;
            g->d_bf = bf_dev; g->bf_host = bf;
            Sc3Args A; for (int k = 0; k < 8; ++k) A.off[k] = arena_off[k];
            A.L = P.ell_len; A.N = N; A.M = M; A.Epp = Epp; A.fused = fused ? 1 : 0;
            for (int k = 0; k < 6; ++k) A.toff[k] = arena_off[7 + k];
            A.tcapN = TAIL_POSES; A.tcapEpp = TAIL_PP; A.tcapEpl = TAIL_PL; A.tcapM = TAIL_LMS;
            g->sc3_args = A;
            launch_build_sc3(bf_dev, d.asm3, d.sc3, d.lm3, (int)S, A, g->stream);
            GS_UT("sc3 build");
            // descriptors + children tables: one wave per level position (k_build_f3)
            d.f3x_stride = P.max_front > 63 ? 168 : 72;                 // a child's row table: 64 entries, or 160 when the plan holds a big front
            std::vector<int32_t> xrow(lf.size() + 1, 0);
            for (size_t q = 0; q < lf.size(); ++q) { xrow[q + 1] = xrow[q] + d.f3x_stride * P.fronts[lf[q]].child_cnt;
                if (xrow[q + 1] >= (1 << 30)) return fail(GS_ERR_INVALID, "children table too large"); }
            int32_t *xrow_dev = nullptr; if ((rc = dev_upload(g, &xrow_dev, xrow)) != GS_OK) return rc;
            g->d_xrow = xrow_dev;
            g->pos_of_front.assign(P.fronts.size(), -1);
            for (size_t q = 0; q < lf.size(); ++q) g->pos_of_front[lf[q]] = (int32_t)q;
            if ((rc = dev_upload(g, &g->d_posof, g->pos_of_front)) != GS_OK) return rc;      // front -> level position: into the children's headers (k_factor3_sub finds a leaf's descriptor through it)
            if ((rc = dev_alloc(g, &g->d_patch, (size_t)1024 * 32)) != GS_OK || (rc = dev_alloc(g, &g->d_list, (size_t)2048)) != GS_OK) return rc;
            AL(f3_desc, lf.size() * (size_t)F3W); AL(f3_x, (size_t)xrow[lf.size()] + 168);
            launch_build_f3((int)lf.size(), d.level_fronts, d.fronts, d.children, d.child_map, d.u3_off, d.u3_size, bf_dev, xrow_dev,
                            P.dist ? d.x_off : nullptr, d.f3_desc, d.f3_x, d.f3x_stride, g->stream, nullptr, g->d_posof);
            // a growth step needs all of the above: variant 3, one GPU, the fused linearisation layout
            g->room.ok = !P.dist && fused;
            GS_UT("f3 tables"); }
      } }
    GS_UT("f3 x+desc upload");
    AL(dbg_ts, 64); ZERO(dbg_ts, 64);
    AL(done_ts, 2 * P.fronts.size() + 2); ZERO(done_ts, 2 * P.fronts.size() + 2);
    { const int64_t room_L = g->room.ok ? (int64_t)room_of((size_t)P.l_doubles, (size_t)256 << 10, (size_t)(P.max_front > 63 ? 8 : 2) << 20) : 0;          // doubles: the L panels of fronts a growth step enlarges move here
      AL(Lbuf, P.l_doubles + room_L); g->room.cap_L = P.l_doubles + room_L; }
    AL(Ubuf, d.factor_variant == 0 ? P.u_doubles : 1);              // variant 3 keeps its update matrices in Uimg
    AL(xe, P.n_scalar + 3 * TAIL_POSES + 2 * TAIL_LMS); g->room.cap_xe = P.n_scalar + 3 * TAIL_POSES + 2 * TAIL_LMS;
    AL(dpose, ((size_t)N + TAIL_POSES) * 3); AL(dlm, ((size_t)M + TAIL_LMS) * 2); AL(fail, 4);
    HIP_TRY(hipMemsetAsync(d.fail, 0, 4 * sizeof(int32_t), g->stream));
    HIP_TRY(hipMemsetAsync(d.chi2, 0, 80 * sizeof(double), g->stream));
    HIP_TRY(hipMemsetAsync(d.dpose, 0, ((size_t)N + TAIL_POSES) * 3 * sizeof(double), g->stream));
    HIP_TRY(hipMemsetAsync(d.dlm, 0, ((size_t)M + TAIL_LMS) * 2 * sizeof(double), g->stream));
    // the solver launches of this plan, decided here once (gs_schedule.hpp); the global workspace for fronts beyond the LDS limit,
    // one slice per block; the workgroup tables of a plan with fronts beyond a wave
    g->sched = build_schedule(P, g->pos_of_front, d.factor_variant, g->opt.tree != 0, g->opt);
    d.front_ws_stride = g->sched.front_ws_stride;
    if (g->sched.ws_blocks > 0) AL(front_ws, d.front_ws_stride * g->sched.ws_blocks);
    if ((rc = upload_tables(g)) != GS_OK) return rc;
#undef UP
#undef AL
#undef ZERO
    GS_UT("arenas+levels");
    if (raw.th.joinable()) { raw.th.join(); if (raw.rc != GS_OK) return fail(raw.rc, raw.err); }      // a shard's edge streams (above)
    HIP_TRY(hipStreamSynchronize(g->stream));
    GS_UT("final sync");
    g->dev_valid = true; g->dev_estimates_newer = false; g->tree_proven = false;
    ++g->value_uploads;                                              // every edge's own information is on the device again (edge_mask_sync)
    g->dev_estimate_version = h.estimate_version;
    return GS_OK;
}

// ---- append-only growth on the device (after gs::grow_plan changed the host plan): the new poses' and edges' data into the tail
// arrays, the re-written runs of the changed fronts behind the plan arrays, those fronts' rows of the compact tables through one
// patch buffer, then the device-side expansion (k_build_sc3, k_build_f3) for those fronts only.  Everything older stays where it
// is.  Returns GS_ERR_CAPACITY when the room left by the full structure phase is used up (the caller rebuilds).
static int upload_growth(gs_graph *g, const Growth &gr) {
    const HostGraph &h = g->h; const Plan &P = g->plan; DevGraph &d = g->d;
    if (!g->room.ok || d.factor_variant != 3) return fail(GS_ERR_CAPACITY, "growth: this plan was not uploaded with room to grow");
    const int nf = (int)gr.fronts.size();
    if (nf > 1024 || (int64_t)P.bnd_rows.size() > g->room.cap_bnd || (int64_t)P.child_map.size() > g->room.cap_map ||
        (int64_t)P.asm_recs.size() > g->room.cap_asm || P.l_doubles > g->room.cap_L || P.n_scalar > g->room.cap_xe)
        return fail(GS_ERR_CAPACITY, "growth: room behind the plan arrays used up");
    const bool fused = g->sc3_args.fused != 0;
    // update-matrix slots and scalar-record runs of the changed fronts
    std::vector<int32_t> patch((size_t)nf * 32, 0), poslist(nf);
    int64_t used_U = g->room.used_U, used_sc = g->room.used_sc;
    for (int i = 0; i < nf; ++i) { const int s = gr.fronts[i]; const Front &F = P.fronts[s]; int32_t *r = &patch[(size_t)i * 32];
        const int nb = F.nbnd; const int32_t usz = (nb * (nb + 1)) / 2 + nb;
        int ns = 0;
        for (int t = F.asm_off; t < F.asm_off + F.asm_cnt - F.asm_dup; ++t) { const int k = P.asm_recs[t].kind;
            if (k == 0) ns += 9; else if (k == 1) { if (!fused) ns += 5; } else if (k <= 3) ns += 9; else if (k == 6) ns += 5; else ns += 6; }
        const int32_t sc_cnt = (ns + 63) & ~63;
        if (used_U + usz + 4 > g->room.cap_U || used_sc + sc_cnt > g->room.cap_sc) return fail(GS_ERR_CAPACITY, "growth: room behind the update matrices / scalar records used up");
        DevFront o; o.npiv = F.npiv; o.nbnd = F.nbnd; o.piv0 = F.piv0; o.parent = F.parent; o.asm_off = F.asm_off; o.asm_cnt = F.asm_cnt;
        o.asm_dup = F.asm_dup; o.child_off = F.child_off; o.child_cnt = F.child_cnt; o.owner = F.owner; o.level = F.level; o.pad0 = 0;
        o.bnd_off = F.bnd_off; o.map_off = F.map_off; o.L_off = F.L_off; o.U_off = F.U_off;
        r[0] = s; std::memcpy(r + 1, &o, sizeof(o));
        r[21] = (int32_t)used_U; r[22] = usz; used_U += (usz + 2 + 1) & ~1;
        const int32_t *b0 = &g->bf_host[8 * (size_t)s];
        r[23] = F.asm_off; r[24] = F.asm_cnt - F.asm_dup; r[25] = F.npiv + F.nbnd; r[26] = (int32_t)used_sc; r[27] = sc_cnt; r[28] = b0[5]; r[29] = b0[6]; r[30] = 0;
        used_sc += sc_cnt;
        poslist[i] = g->pos_of_front[s];
        if (poslist[i] < 0) return fail(GS_ERR_INVALID, "growth: front without a level position"); }
    // ---- from here on the device changes
    const int N0 = gr.first_pose, N1 = P.planned_N, E0 = gr.first_pp, E1 = P.planned_Epp, K0 = gr.first_pl, K1 = P.planned_Epl;
    std::vector<double> zinv((size_t)(E1 - E0) * 5), plz((size_t)(K1 - K0) * 2), plw((size_t)(K1 - K0) * 3);
    std::vector<int32_t> ppij((size_t)(E1 - E0) * 2), plpl((size_t)(K1 - K0) * 2);
    auto H2D = [&](void *dst, const void *src, size_t bytes) -> int {
        if (!bytes) return GS_OK;
        hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g->stream);
        return e == hipSuccess ? GS_OK : fail(GS_ERR_HIP, std::string("growth upload: ") + hipGetErrorString(e)); };
    int rc;
    if ((rc = H2D(d.pose_est + 3 * (size_t)N0, &h.pose_est[3 * (size_t)N0], (size_t)(N1 - N0) * 3 * sizeof(double))) != GS_OK) return rc;
    if ((rc = H2D(d.pose_gidx + N0, &P.pose_gidx[N0], (size_t)(N1 - N0) * sizeof(int32_t))) != GS_OK) return rc;
    { const int M0 = gr.first_lm, M1 = P.planned_M;                  // landmarks first seen by the new poses
      if (M1 > M0) { if ((rc = H2D(d.lm_est + 2 * (size_t)M0, &h.lm_est[2 * (size_t)M0], (size_t)(M1 - M0) * 2 * sizeof(double))) != GS_OK) return rc;
          if ((rc = H2D(d.lm_gidx + M0, &P.lm_gidx[M0], (size_t)(M1 - M0) * sizeof(int32_t))) != GS_OK) return rc; } }
    if (g->dev_estimate_version != h.estimate_version) {          // a host-side setEstimate on an OLDER vertex since the last upload (g2o: setEstimate, then
        const int M1 = P.planned_M;                                 // optimize() uses the new value): the whole estimate arrays go up again, not only the tail's
        if ((rc = H2D(d.pose_est, h.pose_est.data(), (size_t)N1 * 3 * sizeof(double))) != GS_OK) return rc;
        if ((rc = H2D(d.lm_est, h.lm_est.data(), (size_t)M1 * 2 * sizeof(double))) != GS_OK) return rc;
        launch_pose_trig_range(d, 0, N1, g->stream);
    } else launch_pose_trig_range(d, N0, N1 - N0, g->stream);
    for (int k = E0; k < E1; ++k) { double inv[3]; se2_inverse_host(&h.pp_z[3 * (size_t)k], inv);
        double *o = &zinv[5 * (size_t)(k - E0)]; o[0] = inv[0]; o[1] = inv[1]; o[2] = inv[2]; o[3] = std::cos(inv[2]); o[4] = std::sin(inv[2]);
        ppij[2 * (size_t)(k - E0)] = h.pp_i[k]; ppij[2 * (size_t)(k - E0) + 1] = h.pp_j[k]; }
    if ((rc = H2D(d.pp_zinv + 5 * (size_t)E0, zinv.data(), zinv.size() * sizeof(double))) != GS_OK) return rc;
    if ((rc = H2D(d.pp_info + 6 * (size_t)E0, &h.pp_info[6 * (size_t)E0], (size_t)(E1 - E0) * 6 * sizeof(double))) != GS_OK) return rc;
    if ((rc = H2D(d.t_pp_ij + 2 * (size_t)(E0 - P.base_Epp), ppij.data(), ppij.size() * sizeof(int32_t))) != GS_OK) return rc;
    for (int k = K0; k < K1; ++k) { const size_t q = (size_t)(k - K0);
        plpl[2 * q] = h.pl_p[k]; plpl[2 * q + 1] = h.pl_l[k]; plz[2 * q] = h.pl_z[2 * (size_t)k]; plz[2 * q + 1] = h.pl_z[2 * (size_t)k + 1];
        for (int c = 0; c < 3; ++c) plw[3 * q + c] = h.pl_info[3 * (size_t)k + c]; }
    { const size_t s0 = (size_t)(K0 - P.base_Epl);
      if ((rc = H2D(d.t_pl + 2 * s0, plpl.data(), plpl.size() * sizeof(int32_t))) != GS_OK) return rc;
      if ((rc = H2D(d.t_pl_z + 2 * s0, plz.data(), plz.size() * sizeof(double))) != GS_OK) return rc;
      if ((rc = H2D(d.t_pl_w + 3 * s0, plw.data(), plw.size() * sizeof(double))) != GS_OK) return rc; }
    // the tail's edges grouped by pose and by touched landmark (edge order inside a group: the order of the sums in k_linearize_tail);
    // the whole tail, not only this step's part
    std::vector<int32_t> tps, tpe, ltid, lts, lte;
    { const int tN = N1 - P.base_N, tE = K1 - P.base_Epl;
      tps.assign((size_t)tN + 1, 0); tpe.resize((size_t)tE);
      for (int e = 0; e < tE; ++e) tps[(size_t)(h.pl_p[P.base_Epl + e] - P.base_N) + 1]++;
      for (int t = 0; t < tN; ++t) tps[(size_t)t + 1] += tps[(size_t)t];
      { std::vector<int32_t> fill(tps.begin(), tps.end() - 1); for (int e = 0; e < tE; ++e) tpe[(size_t)fill[(size_t)(h.pl_p[P.base_Epl + e] - P.base_N)]++] = e; }
      std::vector<std::pair<int32_t, int32_t>> le; le.reserve((size_t)tE);        // (landmark, edge), fixed cones left out: nothing is summed for them
      for (int e = 0; e < tE; ++e) { const int l = h.pl_l[P.base_Epl + e]; if (!h.lm_fixed[l]) le.emplace_back(l, e); }
      std::sort(le.begin(), le.end());
      lts.push_back(0);
      for (size_t q = 0; q < le.size(); ++q) { if (q == 0 || le[q].first != le[q - 1].first) { if (q) lts.push_back((int32_t)q); ltid.push_back(le[q].first); } lte.push_back(le[q].second); }
      if (!le.empty()) lts.push_back((int32_t)le.size());
      d.tLt = (int32_t)ltid.size();
      if ((rc = H2D(d.t_pose_start, tps.data(), tps.size() * sizeof(int32_t))) != GS_OK || (rc = H2D(d.t_pose_edges, tpe.data(), tpe.size() * sizeof(int32_t))) != GS_OK ||
          (rc = H2D(d.t_lt_id, ltid.data(), ltid.size() * sizeof(int32_t))) != GS_OK || (rc = H2D(d.t_lt_start, lts.data(), lts.size() * sizeof(int32_t))) != GS_OK ||
          (rc = H2D(d.t_lt_edges, lte.data(), lte.size() * sizeof(int32_t))) != GS_OK) return rc; }
    // the re-written runs
    if ((rc = H2D(d.bnd_rows + gr.bnd_from, &P.bnd_rows[(size_t)gr.bnd_from], (P.bnd_rows.size() - (size_t)gr.bnd_from) * sizeof(int32_t))) != GS_OK) return rc;
    if ((rc = H2D(d.child_map + gr.map_from, &P.child_map[(size_t)gr.map_from], (P.child_map.size() - (size_t)gr.map_from) * sizeof(int32_t))) != GS_OK) return rc;
    { const size_t na = P.asm_recs.size() - (size_t)gr.asm_from;
      if (na) { if ((rc = H2D(d.asm_recs + 4 * gr.asm_from, &P.asm_recs[(size_t)gr.asm_from], na * sizeof(AsmRec))) != GS_OK) return rc;
          if ((rc = H2D(d.asm3 + 4 * gr.asm_from, &P.asm_recs[(size_t)gr.asm_from], na * sizeof(AsmRec))) != GS_OK) return rc;
          if (fused) launch_patch_asm3((int64_t)na, d.asm3 + 4 * gr.asm_from, d.lm_grp_start, g->stream); } }
    // compact tables: the changed fronts' rows
    if ((rc = H2D(g->d_patch, patch.data(), patch.size() * sizeof(int32_t))) != GS_OK) return rc;
    launch_apply_front_patch(nf, g->d_patch, d.fronts, d.u3_off, d.u3_size, g->d_bf, g->stream);
    if ((rc = H2D(g->d_list, gr.fronts.data(), (size_t)nf * sizeof(int32_t))) != GS_OK) return rc;
    if ((rc = H2D(g->d_list + 1024, poslist.data(), (size_t)nf * sizeof(int32_t))) != GS_OK) return rc;
    // device-side expansion for those fronts: scalar records, then descriptors + children tables (a changed front's parent is a
    // changed front too: its copy of the child's row table is rebuilt with it)
    launch_build_sc3(g->d_bf, d.asm3, d.sc3, d.lm3, nf, g->sc3_args, g->stream, g->d_list);
    launch_build_f3(nf, d.level_fronts, d.fronts, d.children, d.child_map, d.u3_off, d.u3_size, g->d_bf, g->d_xrow, nullptr, d.f3_desc, d.f3_x, d.f3x_stride, g->stream, g->d_list + 1024, g->d_posof);
    d.n_scalar = P.n_scalar; d.tN = N1 - P.base_N; d.tM = P.planned_M - P.base_M; d.tEpp = E1 - P.base_Epp; d.tEpl = K1 - P.base_Epl;
    HIP_TRY(hipStreamSynchronize(g->stream));                       // the staging vectors above go out of scope
    { hipError_t e = hipGetLastError(); if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("growth: ") + hipGetErrorString(e)); }
    // host mirrors and launch parameters
    for (int i = 0; i < nf; ++i) { const int s = gr.fronts[i]; const int32_t *r = &patch[(size_t)i * 32];
        g->u3_off_host[s] = r[21]; g->u3_size_host[s] = r[22]; for (int c = 0; c < 8; ++c) g->bf_host[8 * (size_t)s + c] = r[23 + c]; }
    g->room.used_U = used_U; g->room.used_sc = used_sc;
    // the launch geometry is chosen again from the grown fronts: level maxima, leaf instance and its LDS slot, the workgroup tables (a
    // grown front may change its size class).  The old tables stay in the pool until the next full structure phase.
    g->sched = build_schedule(P, g->pos_of_front, d.factor_variant, g->opt.tree != 0, g->opt);
    if ((rc = upload_tables(g)) != GS_OK) return rc;
    g->tree_proven = false;
    g->dev_estimate_version = h.estimate_version;
    return GS_OK;
}

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
        int fv = gs_debug_select_factor_variant(g->opt.factor_variant > 0 ? g->opt.factor_variant : g->cfg.factor_variant, P.max_front, 0);
        if (fv == 4) fv = 0;
        std::vector<int32_t> pos(P.fronts.size(), -1); int32_t q = 0;
        for (int32_t s : P.level_fronts_owned) pos[s] = q++;
        for (int32_t s : P.level_fronts_shared) pos[s] = q++;
        export_schedule(P, build_schedule(P, pos, fv, g->opt.tree != 0, g->opt), v); }
    if (!out) { *out_len = (int64_t)v.size(); return GS_OK; }
    if (*out_len < (int64_t)v.size()) return fail(GS_ERR_CAPACITY, "buffer too small");
    std::memcpy(out, v.data(), v.size() * sizeof(int32_t)); *out_len = (int64_t)v.size();
    return GS_OK;
}

// host-side setEstimate since the upload: the estimates (and the poses' cos / sin) to the device of the current plan
static int push_estimates(gs_graph *g) {
    if (g->dev_estimate_version == g->h.estimate_version) return GS_OK;
    const int N = g->d.N + g->d.tN, M = g->d.M + g->d.tM;
    if (N > 0) HIP_TRY(hipMemcpyAsync(g->d.pose_est, g->h.pose_est.data(), (size_t)N * 3 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    if (M > 0) HIP_TRY(hipMemcpyAsync(g->d.lm_est, g->h.lm_est.data(), (size_t)M * 2 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    launch_pose_trig(g->d, g->stream);
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->dev_estimate_version = g->h.estimate_version; g->dev_estimates_newer = false;
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
    const bool st_on = g->opt.plan_timing != 0; auto st_prev = std::chrono::steady_clock::now();      // gs_debug_options.plan_timing: the steps of this call on stderr
    auto ST = [&](const char *what) { if (st_on) { auto n_ = std::chrono::steady_clock::now();
        std::fprintf(stderr, "structure %-24s %.2f ms\n", what, std::chrono::duration<double, std::milli>(n_ - st_prev).count()); st_prev = n_; } };
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
