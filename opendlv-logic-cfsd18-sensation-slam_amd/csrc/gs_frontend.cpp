// gs_frontend.cpp — the front end (A0, A1) of the C-ABI: batch conversions, association, the resident map.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_assoc_nn.hpp"
#include "gs_follow.hpp"
#include "gs_follow_host.hpp"
#include "gs_frame_host.hpp"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

// ------------------------------------------------------------------ front end (A0, A1)
// Device memory of the front end lives on the handle and only ever grows: the batch calls carve a scratch arena, the
// per-frame path has pinned staging buffers and a device-resident copy of the map.  Nothing is allocated, freed or
// synchronised beyond the one wait for the results per call.
static size_t padded(size_t n, size_t elem) { return (std::max<size_t>(n, 1) * elem + 255) & ~(size_t)255; }
// what the launches left behind: a resident call's whole tail, and the end of a batch and a live call behind their one wait
static int resident_done(gs_graph *, const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GS_OK : fail(GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
namespace {
// a batch call's device memory: the pieces it names, in the order it names them, carved from the handle's arena — whose size is the sum over
// the same list, so the two cannot drift — and uploaded where a host array is given.  Valid until the next front-end call
struct Staging {
    struct Piece { void **dev; const void *host; size_t bytes; };
    gs_graph *g; std::vector<Piece> pieces{};
    // `count` elements at dev once commit() has run; host null: not uploaded (an output or scratch)
    template <class T> void add(T *&dev, size_t count, const T *host = nullptr) { pieces.push_back(Piece{(void **)&dev, host, count * sizeof(T)}); }
    // an input array of a view: as add, but an array the caller did not give is no piece, and dev null
    template <class T> void input(const T *&dev, size_t count, const T *host) { dev = nullptr; if (host) pieces.push_back(Piece{(void **)&dev, host, count * sizeof(T)}); }
    int commit() {
        size_t total = 0; for (const Piece &p : pieces) total += padded(p.bytes, 1);
        const int rc = arena_reserve(g, g->fe.arena, total); if (rc != GS_OK) return rc;
        size_t off = 0;
        for (const Piece &p : pieces) { *p.dev = g->fe.arena.at(off); off += padded(p.bytes, 1);
            if (p.host && p.bytes) HIP_TRY(hipMemcpyAsync(*p.dev, p.host, p.bytes, hipMemcpyHostToDevice, g->stream)); }
        return GS_OK;
    }
    // a result back to the host, when the caller asked for it; after a copy that failed nothing more is enqueued, and finish() says so
    int err = GS_OK;
    void fetch(void *dst, const void *src, size_t bytes) {
        if (err != GS_OK || !dst || !bytes) return;
        const hipError_t e = hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g->stream);
        if (e != hipSuccess) err = fail(GS_ERR_HIP, std::string("result copy: ") + hipGetErrorString(e));
    }
    // the one wait of the call (the result copies), and what the launches left behind
    int finish(const char *what) {
        if (err != GS_OK) return err;
        HIP_TRY(hipStreamSynchronize(g->stream));
        return resident_done(g, what);
    }
};
}
// bench / profiling hooks (graphslam_debug.h): one warming call of the resident entry point (which also builds its grid), then `reps` calls,
// each with a start / stop event pair that the entry point attaches to its first / last dispatch (g->ev_lin: the kernels' own begin -> end);
// mean milliseconds per call
template <class Once>
static int time_resident(gs_graph *g, int32_t reps, double *out_ms, Once once) {
    if (!g || !out_ms || reps <= 0) return fail(GS_ERR_INVALID, "bad argument");
    int rc = once(); if (rc != GS_OK) return rc;
    std::vector<hipEvent_t> ev(2 * (size_t)reps); for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
    for (int r = 0; r < reps && rc == GS_OK; ++r) { g->ev_lin[0] = ev[2 * (size_t)r]; g->ev_lin[1] = ev[2 * (size_t)r + 1]; rc = once(); }
    g->ev_lin[0] = g->ev_lin[1] = nullptr;
    HIP_TRY(hipStreamSynchronize(g->stream));
    double tot = 0; int cnt = 0;
    for (int r = 0; r < reps; ++r) { float ms = 0; if (hipEventElapsedTime(&ms, ev[2 * (size_t)r], ev[2 * (size_t)r + 1]) == hipSuccess && ms > 0) { tot += ms; ++cnt; } }
    (void)hipGetLastError();
    for (auto &e : ev) hipEventDestroy(e);
    *out_ms = cnt ? tot / cnt : 0.0;
    return rc;
}
static int dev_obs_aligned(const double *dev_obs) {
    if (((uintptr_t)dev_obs & 31) != 0) return fail(GS_ERR_INVALID, "dev_obs must be 32-byte aligned (an observation is read in one load)");
    return GS_OK;
}
// which search a call takes: the hashed grid beyond a few LDS tiles of map, the tile kernel below; gs_debug_options.assoc_grid = 0 / 1 forces
// either (A/B, tests).  usable: false where the call's threshold rules the grid out.  A batch call decides by the map it was given, a live
// frame call the same way by the resident map; a resident call takes the grid unless told otherwise (it is built once per map change)
static bool grid_batch(const gs_graph *g, int n_map, bool usable = true) {
    bool grid = n_map >= 2048 && usable;
    if (g->opt.assoc_grid >= 0) grid = g->opt.assoc_grid != 0 && n_map > 0 && usable;
    return grid;
}
static bool grid_resident(const gs_graph *g, bool usable = true) { return usable && g->fe.map_n > 0 && g->opt.assoc_grid != 0; }
static bool grid_live(const gs_graph *g) { return grid_batch(g, g->fe.map_n); }
// the hashed grid of a map that is in device memory: built on the device (launch_grid_build), nothing crosses PCIe, nothing waits
struct GridBufs { int32_t *count, *start, *cursor, *items; long long buckets; };
static size_t grid_bytes(int n_map, long long &buckets) {
    buckets = 4096; while (buckets < 4 * (long long)n_map) buckets <<= 1;      // a power of two >= 4 n_map: mostly empty buckets, L2-resident
    return 3 * padded((size_t)buckets + 1, 4) + padded((size_t)n_map, 4) + 5 * 256;
}
static GridBufs grid_carve(char *base, int n_map, long long buckets) {
    GridBufs b; size_t off = 0; auto take = [&](size_t bytes) { char *p = base + off; off += (std::max<size_t>(bytes, 1) + 255) & ~(size_t)255; return p; };
    b.count = (int32_t *)take(((size_t)buckets + 1) * 4); b.start = (int32_t *)take(((size_t)buckets + 1) * 4);
    b.cursor = (int32_t *)take(((size_t)buckets + 1) * 4); b.items = (int32_t *)take((size_t)n_map * 4); b.buckets = buckets;
    return b;
}
// the resident map as the launchers take it: walked whole (what a launcher that searches nothing is given, too) ...
static MapRef resident_map_whole(const gs_graph *g) { return MapRef{g->fe.map_n, g->fe.map_xy, g->fe.map_type, g->fe.map_cov, 0, nullptr, nullptr}; }
// ... or, where `grid`, through rg — which is built here, on the device and ahead of the caller's query on the stream, when the map, its
// size or thr (the distance its cell edge comes from) differ from what rg was last built for
static int resident_map(gs_graph *g, gs_graph::FrontEnd::ResidentGrid &rg, bool grid, double thr, MapRef &out) {
    const auto &fe = g->fe;
    out = resident_map_whole(g);
    if (!grid) return GS_OK;
    const bool fresh = rg.valid && rg.map_n == fe.map_n && rg.thr == thr;
    if (!fresh) { const int rc = arena_reserve(g, rg.mem, grid_bytes(fe.map_n, rg.cells)); rg.valid = false; if (rc != GS_OK) return rc; }
    const GridBufs gb = grid_carve(rg.mem.at(0), fe.map_n, rg.cells);
    if (!fresh) { launch_grid_build(fe.map_n, fe.map_xy, thr, rg.cells, gb.count, gb.start, gb.cursor, gb.items, g->stream);
        rg.valid = true; rg.map_n = fe.map_n; rg.thr = thr; }
    out.buckets = rg.cells; out.cell_start = gb.start; out.cell_items = gb.items;
    return GS_OK;
}
// the resident map's cones moved or their number changed: every grid of it is stale
void map_changed(gs_graph *g) { g->fe.grid.valid = g->fe.rl_grid.valid = false; }
namespace {
// a batch call's observations and map, staged beside its own pieces: add() before commit() names the host arrays the call was given (views
// of host pointers; an array that is null there stays null on the device) and, where `grid`, the grid's memory; after commit() o and m are
// the device views, and build_grid() enqueues the grid's build (cell edge from thr) ahead of the query
struct BatchIo {
    ObsRef o{}; MapRef m{}; char *grid_mem = nullptr;
    void add(Staging &sg, const ObsRef &ho, const MapRef &hm, bool grid) {
        o = ho; m = hm; m.buckets = 0; m.cell_start = m.cell_items = nullptr;
        sg.input(o.poses, 3 * (size_t)o.n_poses, ho.poses); sg.input(o.pose_cov, 9 * (size_t)o.n_poses, ho.pose_cov);
        sg.input(o.pose_of_obs, (size_t)o.n, ho.pose_of_obs); sg.input(o.obs, 4 * (size_t)o.n, ho.obs); sg.input(o.frame_start, (size_t)o.n_frames + 1, ho.frame_start);
        sg.input(m.xy, 2 * (size_t)m.n, hm.xy); sg.input(m.type, (size_t)m.n, hm.type); sg.input(m.cov, 4 * (size_t)m.n, hm.cov);
        if (grid) sg.add(grid_mem, grid_bytes(m.n, m.buckets));
    }
    void build_grid(gs_graph *g, double thr) {
        if (!grid_mem) return;
        const GridBufs gb = grid_carve(grid_mem, m.n, m.buckets);
        launch_grid_build(m.n, m.xy, thr, m.buckets, gb.count, gb.start, gb.cursor, gb.items, g->stream);
        m.cell_start = gb.start; m.cell_items = gb.items;
    }
};
}

// ---- the live frame calls' staging (gs::FrameStage, layouts: gs_frame_host.hpp) ----
static_assert(FRAME_MAX == GS_NN_FRAME_MAX, "gs_frame_host.hpp restates the frame size");
int gs::FrameStage::reserve(gs_graph *g, size_t want) {
    if (want <= bytes) return GS_OK;
    HIP_TRY(hipStreamSynchronize(g->stream));                       // a copy out of or into the smaller pair may still be in flight
    release();
    HIP_TRY(hipHostMalloc((void **)&pin, want, hipHostMallocDefault)); HIP_TRY(hipMalloc((void **)&dev, want));
    bytes = want;
    return GS_OK;
}
void gs::FrameStage::release() {
    if (pin) hipHostFree(pin);
    if (dev) hipFree(dev);
    pin = dev = nullptr; bytes = 0;
}
// room for a frame of k observations in a pair that holds bytes_of(m) for m of them: grow-only, to max(64, k + k / 2) observations, `limit` at the most
template <class BytesOf> static int stage_for(gs_graph *g, FrameStage &s, int k, int limit, BytesOf bytes_of) {
    return bytes_of((size_t)k) <= s.bytes ? GS_OK : s.reserve(g, bytes_of((size_t)std::min(limit, std::max(64, k + k / 2))));
}
static int stage_send(gs_graph *g, const FrameStage &s, size_t bytes) {
    HIP_TRY(hipMemcpyAsync(s.dev, s.pin, bytes, hipMemcpyHostToDevice, g->stream));
    return GS_OK;
}
static int stage_fetch(gs_graph *g, const FrameStage &s, size_t bytes, size_t off = 0) {
    HIP_TRY(hipMemcpyAsync(s.pin + off, s.dev + off, bytes, hipMemcpyDeviceToHost, g->stream));
    return GS_OK;
}
// what every live call ends in once its copies back are enqueued: the one wait of the call, and what the launches left behind
static int frame_finish(gs_graph *g, const char *what) {
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->fe.pin_map_busy = false;
    return resident_done(g, what);
}
void gs_frontend_release(gs_graph *g) {      // gs_destroy
    for (FrameStage *s : {&g->fe.fr_in, &g->fe.fr_out, &g->fe.ch_rec, &g->fe.rl_out, &g->fe.fo_in, &g->fe.fo_out}) s->release();
    for (DevArena *a : {&g->fe.arena, &g->fe.grid.mem, &g->fe.rl_grid.mem, &g->fe.pcs, &g->fe.rl_rec, &g->fe.fo_mem}) arena_release(*a);
    if (g->fe.map_xy) hipFree(g->fe.map_xy);
    if (g->fe.map_type) hipFree(g->fe.map_type);
    if (g->fe.pin_map) hipHostFree(g->fe.pin_map);
    if (g->fe.map_cov) hipFree(g->fe.map_cov);
    if (g->fe.cov_src) hipFree(g->fe.cov_src);
    if (g->fe.fo_state) hipFree(g->fe.fo_state);
    if (g->fe.fo_best) hipFree(g->fe.fo_best);
    gs_cand_release(g);
    gs_dup_release(g);
    g->fe = gs_graph::FrontEnd();
}

extern "C" int gs_polar_to_xy_batch(gs_graph *g, int32_t n, const double *az, const double *zen, const double *dist, double *out) {
    if (!g || n < 0 || (n > 0 && (!az || !zen || !dist || !out))) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    Staging sg{g}; double *a, *z, *d, *o;
    sg.add(a, n, az); sg.add(z, n, zen); sg.add(d, n, dist); sg.add(o, 2 * (size_t)n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    launch_polar_to_xy(n, a, z, d, g->cfg.lidar_to_cog, o, g->stream);
    sg.fetch(out, o, 2 * (size_t)n * sizeof(double));
    return sg.finish("polar to XY");
}
extern "C" int gs_cone_to_global_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs,
                                       const double *obs, double *out) {
    if (!g || n < 0 || npose < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !out))) return fail(GS_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) if (pose_of_obs[i] < 0 || pose_of_obs[i] >= npose) return fail(GS_ERR_INVALID, "pose_of_obs out of range");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    Staging sg{g}; double *p, *ob, *o; int32_t *po;
    sg.add(p, 3 * (size_t)npose, poses); sg.add(po, n, pose_of_obs); sg.add(ob, 4 * (size_t)n, obs); sg.add(o, 2 * (size_t)n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    launch_cone_to_global(n, p, po, ob, g->cfg.lidar_to_cog, o, g->stream);
    sg.fetch(out, o, 2 * (size_t)n * sizeof(double));
    return sg.finish("cone to global");
}
extern "C" int gs_associate_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                  int32_t n_map, const double *map_xy, const int32_t *map_type, double thr, double type_tol, int32_t *out) {
    if (!g || n < 0 || npose < 0 || n_map < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !out)) || (n_map > 0 && (!map_xy || !map_type)))
        return fail(GS_ERR_INVALID, "bad argument");
    for (int i = 0; i < n; ++i) if (pose_of_obs[i] < 0 || pose_of_obs[i] >= npose) return fail(GS_ERR_INVALID, "pose_of_obs out of range");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    // maps beyond a few LDS tiles go through a hashed uniform grid (cell edge a hair above the threshold, so that every cone
    // within the threshold sits in the 3 x 3 cells around the query) that is BUILT ON THE DEVICE from the uploaded map; the brute-force
    // kernel stays for small maps and non-positive thresholds (grid_batch).
    Staging sg{g}; BatchIo io; double *pcs; int32_t *o;
    io.add(sg, ObsRef{n, poses, npose, pose_of_obs, obs, 0, nullptr, nullptr}, MapRef{n_map, map_xy, map_type, nullptr, 0, nullptr, nullptr}, grid_batch(g, n_map, thr > 0.0));
    sg.add(pcs, 2 * (size_t)npose); sg.add(o, n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    io.build_grid(g, thr);
    const ObsRef &ob = io.o; const MapRef &m = io.m;
    if (m.cell_start) launch_associate_grid_dev(n, ob.poses, ob.pose_of_obs, ob.obs, g->cfg.lidar_to_cog, m.xy, m.type, thr, type_tol, m.buckets, m.cell_start, m.cell_items, o,
                                                npose, pcs, g->stream);
    else launch_associate(n, ob.poses, ob.pose_of_obs, ob.obs, g->cfg.lidar_to_cog, n_map, m.xy, m.type, thr, type_tol, o, g->stream);
    sg.fetch(out, o, (size_t)n * sizeof(int32_t));
    return sg.finish("association");                 // the one wait of the call: the result copy
}
// A1 batched with EVERYTHING resident: the map of gs_map_append (its grid is built on the device, once per map change or threshold),
// poses / observations / result in device memory, asynchronous on the handle's stream (the caller waits: gs_stream_synchronize).
extern "C" int gs_associate_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                     double thr, double type_tol, int32_t *dev_out) {
    if (!g || n < 0 || npose < 0 || (n > 0 && (!dev_poses || !dev_pose_of_obs || !dev_obs || !dev_out))) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    auto &fe = g->fe; MapRef m;
    if ((rc = resident_map(g, fe.grid, grid_resident(g, thr > 0.0), thr, m)) != GS_OK) return rc;
    if (m.cell_start) { if ((rc = arena_reserve(g, fe.pcs, (size_t)npose * 2 * sizeof(double))) != GS_OK) return rc;      // scratch for the poses' cos / sin
        launch_associate_grid_dev(n, dev_poses, dev_pose_of_obs, dev_obs, g->cfg.lidar_to_cog, m.xy, m.type, thr, type_tol, m.buckets, m.cell_start, m.cell_items, dev_out,
                                  npose, (double *)fe.pcs.mem, g->stream, g->ev_lin[0], g->ev_lin[1]);
    } else launch_associate(n, dev_poses, dev_pose_of_obs, dev_obs, g->cfg.lidar_to_cog, m.n, m.xy, m.type, thr, type_tol, dev_out, g->stream);
    return resident_done(g, "association");
}
extern "C" int gs_debug_time_associate_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                                const double *dev_obs, double thr, double type_tol, int32_t *dev_out, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] { return gs_associate_resident(g, n, dev_poses, npose, dev_pose_of_obs, dev_obs, thr, type_tol, dev_out); });
}

// ---- the per-keyframe path: resident map + one fused launch -------------------------------------------------------
static int map_reserve(gs_graph *g, int want) {
    if (want <= g->fe.map_cap) return GS_OK;
    const int cap = std::max(want + want / 2, 1024);
    double *xy = nullptr, *cv = nullptr; int32_t *ty = nullptr;
    HIP_TRY(hipMalloc((void **)&xy, (size_t)cap * 2 * sizeof(double)));
    HIP_TRY(hipMalloc((void **)&ty, (size_t)cap * sizeof(int32_t)));
    if (g->fe.map_cov) {                                            // a handle that set covariances: they grow with the map (the rest is zero)
        HIP_TRY(hipMalloc((void **)&cv, (size_t)cap * 4 * sizeof(double)));
        HIP_TRY(hipMemsetAsync(cv, 0, (size_t)cap * 4 * sizeof(double), g->stream));
        if (g->fe.map_n > 0) HIP_TRY(hipMemcpyAsync(cv, g->fe.map_cov, (size_t)g->fe.map_n * 4 * sizeof(double), hipMemcpyDeviceToDevice, g->stream)); }
    if (g->fe.map_n > 0) { HIP_TRY(hipMemcpyAsync(xy, g->fe.map_xy, (size_t)g->fe.map_n * 2 * sizeof(double), hipMemcpyDeviceToDevice, g->stream));
                           HIP_TRY(hipMemcpyAsync(ty, g->fe.map_type, (size_t)g->fe.map_n * sizeof(int32_t), hipMemcpyDeviceToDevice, g->stream)); }
    HIP_TRY(hipStreamSynchronize(g->stream));
    if (g->fe.map_xy) hipFree(g->fe.map_xy);
    if (g->fe.map_type) hipFree(g->fe.map_type);
    if (cv) { hipFree(g->fe.map_cov); g->fe.map_cov = cv; }
    g->fe.map_xy = xy; g->fe.map_type = ty; g->fe.map_cap = cap;
    return GS_OK;
}
static int pin_map_reserve(gs_graph *g, size_t bytes) {
    if (bytes <= g->fe.pin_map_bytes) return GS_OK;
    HIP_TRY(hipStreamSynchronize(g->stream));                       // a previous staged copy may still be in flight
    if (g->fe.pin_map) hipHostFree(g->fe.pin_map);
    g->fe.pin_map = nullptr; g->fe.pin_map_bytes = 0;
    const size_t want = std::max<size_t>(bytes + bytes / 2, 1 << 16);
    HIP_TRY(hipHostMalloc((void **)&g->fe.pin_map, want, hipHostMallocDefault));
    g->fe.pin_map_bytes = want;
    return GS_OK;
}
extern "C" int gs_map_size(gs_graph *g) { return g ? g->fe.map_n : fail(GS_ERR_INVALID, "null graph"); }
extern "C" int gs_map_clear(gs_graph *g) { if (!g) return fail(GS_ERR_INVALID, "null graph"); g->fe.map_n = 0; map_changed(g); return GS_OK; }
extern "C" int gs_map_append(gs_graph *g, int32_t n, const double *xy, const int32_t *type) {
    if (!g || n < 0 || (n > 0 && (!xy || !type))) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    if ((rc = map_reserve(g, g->fe.map_n + n)) != GS_OK) return rc;
    // staged through pinned memory so that the copy is asynchronous; the staging buffer is reused once the stream has passed
    // it — every gs_frame_frontend call waits for the stream, and two appends without one in between wait here
    const size_t bx = (size_t)n * 2 * sizeof(double), bt = (size_t)n * sizeof(int32_t);
    if (g->fe.pin_map_busy) { HIP_TRY(hipStreamSynchronize(g->stream)); g->fe.pin_map_busy = false; }
    if ((rc = pin_map_reserve(g, bx + bt)) != GS_OK) return rc;
    std::memcpy(g->fe.pin_map, xy, bx); std::memcpy(g->fe.pin_map + bx, type, bt);
    HIP_TRY(hipMemcpyAsync(g->fe.map_xy + 2 * (size_t)g->fe.map_n, g->fe.pin_map, bx, hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(g->fe.map_type + g->fe.map_n, g->fe.pin_map + bx, bt, hipMemcpyHostToDevice, g->stream));
    g->fe.pin_map_busy = true;                                      // no wait here: the next frame's launch is ordered behind the copies
    if (g->fe.map_cov) HIP_TRY(hipMemsetAsync(g->fe.map_cov + 4 * (size_t)g->fe.map_n, 0, (size_t)n * 4 * sizeof(double), g->stream));   // (also what gs_map_clear's "drops covariances" rests on)
    g->fe.map_n += n; map_changed(g);
    return GS_OK;
}
extern "C" int gs_map_set_xy(gs_graph *g, int32_t first, int32_t n, const double *xy) {
    if (!g || first < 0 || n < 0 || (n > 0 && !xy)) return fail(GS_ERR_INVALID, "bad argument");
    if (first + n > g->fe.map_n) return fail(GS_ERR_INVALID, "beyond the end of the map");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    HIP_TRY(hipMemcpyAsync(g->fe.map_xy + 2 * (size_t)first, xy, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // pageable source: the caller's buffer is free on return
    g->fe.pin_map_busy = false; map_changed(g);
    return GS_OK;
}
extern "C" int gs_frame_frontend(gs_graph *g, const double pose[3], const double *obs, int32_t k, double thr, double type_tol,
                                 int32_t signed_type, double *out_zxy, double *out_gxy, int32_t *out_idx) {
    if (!g || !pose || k < 0 || (k > 0 && (!obs || !out_zxy || !out_gxy || !out_idx))) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (k == 0) return GS_OK;
    auto &fe = g->fe; const FrameLayout L = frame_layout_plain(k);
    if ((rc = stage_for(g, fe.fr_in, k, INT_MAX, [](size_t m) { return frame_layout_plain(m).in_bytes; })) != GS_OK) return rc;
    if ((rc = stage_for(g, fe.fr_out, k, INT_MAX, [](size_t m) { return frame_layout_plain(m).out_bytes; })) != GS_OK) return rc;
    std::memcpy(fe.fr_in.pin + L.pose, pose, 3 * sizeof(double)); std::memcpy(fe.fr_in.pin + L.obs, obs, 4 * (size_t)k * sizeof(double));
    char *d = fe.fr_out.dev;
    if ((rc = stage_send(g, fe.fr_in, L.in_bytes)) != GS_OK) return rc;
    launch_frame_frontend(k, (const double *)fe.fr_in.dev, g->cfg.lidar_to_cog, fe.map_n, fe.map_xy, fe.map_type, thr, type_tol, signed_type, (double *)(d + L.z),
                          (double *)(d + L.g), (int32_t *)(d + L.idx), g->stream);
    if ((rc = stage_fetch(g, fe.fr_out, L.out_bytes)) != GS_OK) return rc;
    if ((rc = frame_finish(g, "association")) != GS_OK) return rc;
    const char *po = fe.fr_out.pin;
    std::memcpy(out_zxy, po + L.z, 2 * (size_t)k * sizeof(double)); std::memcpy(out_gxy, po + L.g, 2 * (size_t)k * sizeof(double));
    std::memcpy(out_idx, po + L.idx, (size_t)k * sizeof(int32_t));
    return GS_OK;
}

// ---- covariance-gated association (gs_assoc_nn.hip): the map's 2x2 blocks, the batch / resident / frame calls ----------------------
extern "C" int gs_nn_params_default(gs_nn_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->gate_chi2 = 5.991464547107979; p->max_distance = 3.0; p->type_tol = 1e-4; p->sigma_range = 0.3; p->sigma_bearing = 0.02; p->sigma_xy = 0.05;
    return GS_OK;
}
// everything a caller can get wrong about the parameters, decided before the device is touched
int nn_params_check(const gs_nn_params *p, NnDev &d) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_nn_params)) return fail(GS_ERR_INVALID, "gs_nn_params: wrong struct_size");
    const double v[6] = {p->gate_chi2, p->max_distance, p->type_tol, p->sigma_range, p->sigma_bearing, p->sigma_xy};
    for (double x : v) if (!std::isfinite(x)) return fail(GS_ERR_INVALID, "gs_nn_params: a parameter is not finite");
    if (p->gate_chi2 <= 0.0 || p->max_distance <= 0.0) return fail(GS_ERR_INVALID, "gs_nn_params: gate_chi2 and max_distance must be positive");
    if (p->sigma_range < 0.0 || p->sigma_bearing < 0.0 || p->sigma_xy < 0.0) return fail(GS_ERR_INVALID, "gs_nn_params: a sigma is negative");
    d = NnDev{p->gate_chi2, p->max_distance, p->type_tol, p->sigma_range, p->sigma_bearing, p->sigma_xy};
    return GS_OK;
}
// the covariance array, allocated (zeros) at the first call that needs it
static int map_cov_ensure(gs_graph *g) {
    auto &fe = g->fe;
    if (fe.map_cov || fe.map_cap == 0) return GS_OK;
    HIP_TRY(hipMalloc((void **)&fe.map_cov, (size_t)fe.map_cap * 4 * sizeof(double)));
    HIP_TRY(hipMemsetAsync(fe.map_cov, 0, (size_t)fe.map_cap * 4 * sizeof(double), g->stream));
    return GS_OK;
}
extern "C" int gs_map_set_cov(gs_graph *g, int32_t first, int32_t n, const double *cov) {
    if (!g || first < 0 || n < 0 || (n > 0 && !cov)) return fail(GS_ERR_INVALID, "bad argument");
    if ((int64_t)first + n > g->fe.map_n) return fail(GS_ERR_INVALID, "beyond the end of the map");
    for (int k = 0; k < n; ++k) { const double *c = cov + 4 * (size_t)k;              // all or nothing: nothing is uploaded before every block passed
        if (!(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(c[3]))) return fail(GS_ERR_INVALID, "map covariance: a block is not finite");
        if (std::memcmp(c + 1, c + 2, sizeof(double)) != 0) return fail(GS_ERR_INVALID, "map covariance: a block is not symmetric");
        if (c[0] < 0.0 || c[3] < 0.0) return fail(GS_ERR_INVALID, "map covariance: a negative diagonal"); }
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    if ((rc = map_cov_ensure(g)) != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(g->fe.map_cov + 4 * (size_t)first, cov, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // pageable source: the caller's buffer is free on return
    g->fe.pin_map_busy = false;
    return GS_OK;
}
extern "C" int gs_map_get_cov(gs_graph *g, int32_t first, int32_t n, double *out) {
    if (!g || first < 0 || n < 0 || (n > 0 && !out)) return fail(GS_ERR_INVALID, "bad argument");
    if ((int64_t)first + n > g->fe.map_n) return fail(GS_ERR_INVALID, "beyond the end of the map");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    if (!g->fe.map_cov) { std::memset(out, 0, (size_t)n * 4 * sizeof(double)); return GS_OK; }     // never set: zeros, and nothing allocated for asking
    HIP_TRY(hipMemcpyAsync(out, g->fe.map_cov + 4 * (size_t)first, (size_t)n * 4 * sizeof(double), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->fe.pin_map_busy = false;
    return GS_OK;
}
extern "C" int gs_map_set_cov_from_marginals(gs_graph *g, int32_t first, int32_t n, const int32_t *lm_ids) {
    if (!g || first < 0 || n < 0 || (n > 0 && !lm_ids)) return fail(GS_ERR_INVALID, "bad argument");
    if ((int64_t)first + n > g->fe.map_n) return fail(GS_ERR_INVALID, "beyond the end of the map");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    if ((rc = marg_ready(g)) != GS_OK) return rc;
    // landmark l's block sits at 9 n_poses + 4 l of the gathered result gs_compute_marginals keeps in device memory (gs_marginals.cpp, d_out)
    std::vector<int64_t> src((size_t)n);
    const int64_t base = 9 * (int64_t)g->h.n_poses();
    for (int k = 0; k < n; ++k) {
        if (lm_ids[k] == -1) { src[k] = -1; continue; }
        auto it = g->h.lm_index.find(lm_ids[k]);
        if (it == g->h.lm_index.end()) return fail(GS_ERR_UNKNOWN_ID, "unknown landmark id");
        src[k] = base + 4 * (int64_t)it->second; }
    if (n == 0) return GS_OK;
    auto &fe = g->fe;
    if ((rc = map_cov_ensure(g)) != GS_OK) return rc;
    if ((size_t)n > fe.cov_src_n) { HIP_TRY(hipStreamSynchronize(g->stream));
        if (fe.cov_src) hipFree(fe.cov_src);
        fe.cov_src = nullptr; fe.cov_src_n = 0;
        const size_t want = (size_t)n + (size_t)n / 2 + 64;
        HIP_TRY(hipMalloc((void **)&fe.cov_src, want * sizeof(int64_t))); fe.cov_src_n = want; }
    HIP_TRY(hipMemcpyAsync(fe.cov_src, src.data(), (size_t)n * sizeof(int64_t), hipMemcpyHostToDevice, g->stream));
    launch_map_cov_gather(n, fe.cov_src, g->marg.d_out, fe.map_cov + 4 * (size_t)first, g->stream);      // device to device: the values never visit the host
    HIP_TRY(hipStreamSynchronize(g->stream));                       // (src is a host temporary)
    g->fe.pin_map_busy = false;
    return resident_done(g, "map covariances from marginals");
}
extern "C" int gs_associate_nn_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                     int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov,
                                     const gs_nn_params *params, int32_t *out, double *out_d2, double *out_second) {
    if (!g || n < 0 || npose < 0 || n_map < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !out)) || (n_map > 0 && (!map_xy || !map_type)))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = nn_params_check(params, nd); if (rc != GS_OK) return rc;
    for (int i = 0; i < n; ++i) if (pose_of_obs[i] < 0 || pose_of_obs[i] >= npose) return fail(GS_ERR_INVALID, "pose_of_obs out of range");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    Staging sg{g}; BatchIo io; double *od, *os; int32_t *o;
    io.add(sg, ObsRef{n, poses, npose, pose_of_obs, obs, 0, nullptr, pose_cov}, MapRef{n_map, map_xy, map_type, map_cov, 0, nullptr, nullptr}, grid_batch(g, n_map));
    sg.add(o, n); sg.add(od, n); sg.add(os, n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    io.build_grid(g, nd.max_distance);
    launch_assoc_nn(io.o, io.m, g->cfg.lidar_to_cog, nd, o, od, os, Launch{g->stream});
    sg.fetch(out, o, (size_t)n * sizeof(int32_t)); sg.fetch(out_d2, od, (size_t)n * sizeof(double)); sg.fetch(out_second, os, (size_t)n * sizeof(double));
    return sg.finish("association (nn)");
}
extern "C" int gs_associate_nn_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                        const double *dev_pose_cov, const gs_nn_params *params, int32_t *dev_out, double *dev_out_d2, double *dev_out_second) {
    if (!g || n < 0 || npose < 0 || (n > 0 && (!dev_poses || !dev_pose_of_obs || !dev_obs || !dev_out))) return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = nn_params_check(params, nd); if (rc != GS_OK) return rc;
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    MapRef m; if ((rc = resident_map(g, g->fe.grid, grid_resident(g), nd.max_distance, m)) != GS_OK) return rc;
    launch_assoc_nn(ObsRef{n, dev_poses, npose, dev_pose_of_obs, dev_obs, 0, nullptr, dev_pose_cov}, m, g->cfg.lidar_to_cog, nd, dev_out, dev_out_d2, dev_out_second,
                    Launch{g->stream, g->ev_lin[0], g->ev_lin[1]});
    return resident_done(g, "association (nn)");
}
extern "C" int gs_debug_time_associate_nn_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                                   const double *dev_obs, const double *dev_pose_cov, const gs_nn_params *params, int32_t *dev_out,
                                                   double *dev_out_d2, double *dev_out_second, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_associate_nn_resident(g, n, dev_poses, npose, dev_pose_of_obs, dev_obs, dev_pose_cov, params, dev_out, dev_out_d2, dev_out_second); });
}
extern "C" int gs_frame_frontend_nn(gs_graph *g, const double pose[3], const double *pose_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                    double *out_zxy, double *out_gxy, int32_t *out_idx, double *out_d2, double *out_second) {
    if (!g || !pose || k < 0 || (k > 0 && (!obs || !out_zxy || !out_gxy || !out_idx || !out_d2 || !out_second))) return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = nn_params_check(params, nd); if (rc != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (k == 0) return GS_OK;
    auto &fe = g->fe; const FrameLayout L = frame_layout_nn(k);
    if ((rc = stage_for(g, fe.fr_in, k, INT_MAX, [](size_t m) { return frame_layout_nn(m).in_bytes; })) != GS_OK) return rc;
    if ((rc = stage_for(g, fe.fr_out, k, INT_MAX, [](size_t m) { return frame_layout_nn(m).out_bytes; })) != GS_OK) return rc;
    char *pi = fe.fr_in.pin, *d = fe.fr_out.dev;
    std::memcpy(pi + L.pose, pose, 3 * sizeof(double));
    if (pose_cov) std::memcpy(pi + L.cov, pose_cov, 9 * sizeof(double)); else std::memset(pi + L.cov, 0, 9 * sizeof(double));
    std::memcpy(pi + L.obs, obs, 4 * (size_t)k * sizeof(double));
    if ((rc = stage_send(g, fe.fr_in, L.in_bytes)) != GS_OK) return rc;
    launch_frame_nn(k, (const double *)fe.fr_in.dev, pose_cov ? 1 : 0, resident_map_whole(g), g->cfg.lidar_to_cog, nd,
                    (double *)(d + L.z), (double *)(d + L.g), (int32_t *)(d + L.idx), (double *)(d + L.d2), (double *)(d + L.second), g->stream);
    if ((rc = stage_fetch(g, fe.fr_out, L.out_bytes)) != GS_OK) return rc;
    if ((rc = frame_finish(g, "association (nn)")) != GS_OK) return rc;
    const char *po = fe.fr_out.pin; const size_t bz = 2 * (size_t)k * sizeof(double), bd = (size_t)k * sizeof(double);
    std::memcpy(out_zxy, po + L.z, bz); std::memcpy(out_gxy, po + L.g, bz); std::memcpy(out_d2, po + L.d2, bd); std::memcpy(out_second, po + L.second, bd);
    std::memcpy(out_idx, po + L.idx, (size_t)k * sizeof(int32_t));
    return GS_OK;
}

// ---- one-to-one association inside a frame (gs_assoc_nn.hip, k_assign_nn): the batch / resident / frame calls -----------------------
int frame_start_check(int32_t n, int32_t n_frames, const int32_t *fs) {
    if (n_frames < 0 || !fs) return fail(GS_ERR_INVALID, "bad argument");
    if (fs[0] != 0 || fs[n_frames] != n) return fail(GS_ERR_INVALID, "frame_start must begin at 0 and end at n");
    for (int f = 0; f < n_frames; ++f) {
        if (fs[f + 1] < fs[f]) return fail(GS_ERR_INVALID, "frame_start must ascend");
        if (fs[f + 1] - fs[f] > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "a frame holds more than GS_NN_FRAME_MAX observations"); }
    return GS_OK;
}
// what a batch call over frames checks of its host arrays: frame_start, pose_of_obs in range, in_index (null: the call takes none) in
// [-1, n_map), and with one_pose_per_frame that a frame's observations share one pose
static int frame_inputs_check(int32_t n, int32_t npose, const int32_t *pose_of_obs, int32_t n_frames, const int32_t *frame_start, const int32_t *in_index,
                              int32_t n_map, bool one_pose_per_frame) {
    const int rc = frame_start_check(n, n_frames, frame_start); if (rc != GS_OK) return rc;
    for (int i = 0; i < n; ++i) {
        if (pose_of_obs[i] < 0 || pose_of_obs[i] >= npose) return fail(GS_ERR_INVALID, "pose_of_obs out of range");
        if (in_index && (in_index[i] < -1 || in_index[i] >= n_map)) return fail(GS_ERR_INVALID, "in_index outside [-1, n_map)"); }
    if (one_pose_per_frame)
        for (int f = 0; f < n_frames; ++f)
            for (int i = frame_start[f] + 1; i < frame_start[f + 1]; ++i)
                if (pose_of_obs[i] != pose_of_obs[frame_start[f]]) return fail(GS_ERR_INVALID, "the observations of a frame must share one pose");
    return GS_OK;
}
// the greedy matching (opt false: k_assign_nn) or the minimum-cost one (opt true: k_assign_opt, which also counts the admissible cones)
static int assign_batch(gs_graph *g, bool opt, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                        int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const int32_t *map_type,
                        const double *map_cov, const double *pose_cov, const gs_nn_params *params, int32_t *out, double *out_d2, int32_t *out_na) {
    if (!g || n < 0 || npose < 0 || n_map < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !out)) || (n_map > 0 && (!map_xy || !map_type)))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = nn_params_check(params, nd); if (rc != GS_OK) return rc;
    if ((rc = frame_inputs_check(n, npose, pose_of_obs, n_frames, frame_start, nullptr, n_map, false)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0) return GS_OK;
    Staging sg{g}; BatchIo io; double *od; int32_t *o, *ona = nullptr;
    io.add(sg, ObsRef{n, poses, npose, pose_of_obs, obs, n_frames, frame_start, pose_cov}, MapRef{n_map, map_xy, map_type, map_cov, 0, nullptr, nullptr}, grid_batch(g, n_map));
    sg.add(o, n); sg.add(od, n); if (opt) sg.add(ona, n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    io.build_grid(g, nd.max_distance);
    if (opt) launch_assign_opt(io.o, io.m, g->cfg.lidar_to_cog, nd, o, od, ona, nullptr, nullptr, Launch{g->stream});
    else launch_assign_nn(io.o, io.m, g->cfg.lidar_to_cog, nd, o, od, nullptr, nullptr, Launch{g->stream});
    sg.fetch(out, o, (size_t)n * sizeof(int32_t)); sg.fetch(out_d2, od, (size_t)n * sizeof(double)); sg.fetch(out_na, ona, (size_t)n * sizeof(int32_t));
    return sg.finish("assignment (nn)");
}
extern "C" int gs_assign_nn_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                  int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const int32_t *map_type,
                                  const double *map_cov, const double *pose_cov, const gs_nn_params *params, int32_t *out, double *out_d2) {
    return assign_batch(g, false, n, poses, npose, pose_of_obs, obs, n_frames, frame_start, n_map, map_xy, map_type, map_cov, pose_cov, params, out, out_d2, nullptr);
}
extern "C" int gs_assign_opt_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                   int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const int32_t *map_type,
                                   const double *map_cov, const double *pose_cov, const gs_nn_params *params, int32_t *out, double *out_d2, int32_t *out_na) {
    return assign_batch(g, true, n, poses, npose, pose_of_obs, obs, n_frames, frame_start, n_map, map_xy, map_type, map_cov, pose_cov, params, out, out_d2, out_na);
}
// the resident map through either search (its grid built first where it is stale): the launch both the resident and the frame call end in
static int assign_resident_launch(gs_graph *g, bool opt, bool grid, const ObsRef &o, const NnDev &nd, int32_t *dev_out, double *dev_out_d2, int32_t *dev_out_na,
                                  double *dev_z, double *dev_g) {
    MapRef m; const int rc = resident_map(g, g->fe.grid, grid, nd.max_distance, m); if (rc != GS_OK) return rc;
    const Launch L{g->stream, g->ev_lin[0], g->ev_lin[1]};
    if (opt) launch_assign_opt(o, m, g->cfg.lidar_to_cog, nd, dev_out, dev_out_d2, dev_out_na, dev_z, dev_g, L);
    else launch_assign_nn(o, m, g->cfg.lidar_to_cog, nd, dev_out, dev_out_d2, dev_z, dev_g, L);
    return GS_OK;
}
static int assign_resident(gs_graph *g, bool opt, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                           int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov, const gs_nn_params *params,
                           int32_t *dev_out, double *dev_out_d2, int32_t *dev_out_na) {
    if (!g || n < 0 || npose < 0 || n_frames < 0 || !dev_frame_start || (n > 0 && (!dev_poses || !dev_pose_of_obs || !dev_obs || !dev_out)))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = nn_params_check(params, nd); if (rc != GS_OK) return rc;
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n == 0 || n_frames == 0) return GS_OK;
    if ((rc = assign_resident_launch(g, opt, grid_resident(g), ObsRef{n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov}, nd,
                                     dev_out, dev_out_d2, dev_out_na, nullptr, nullptr)) != GS_OK) return rc;
    return resident_done(g, "assignment (nn)");
}
extern "C" int gs_assign_nn_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                     int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov, const gs_nn_params *params,
                                     int32_t *dev_out, double *dev_out_d2) {
    return assign_resident(g, false, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, dev_out, dev_out_d2, nullptr);
}
extern "C" int gs_assign_opt_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                      int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov, const gs_nn_params *params,
                                      int32_t *dev_out, double *dev_out_d2, int32_t *dev_out_na) {
    return assign_resident(g, true, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, dev_out, dev_out_d2, dev_out_na);
}
extern "C" int gs_debug_time_assign_nn_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                                const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov,
                                                const gs_nn_params *params, int32_t *dev_out, double *dev_out_d2, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return assign_resident(g, false, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, dev_out, dev_out_d2, nullptr); });
}
extern "C" int gs_debug_time_assign_opt_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                                 const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov,
                                                 const gs_nn_params *params, int32_t *dev_out, double *dev_out_d2, int32_t *dev_out_na, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return assign_resident(g, true, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, dev_out, dev_out_d2, dev_out_na); });
}

// ---- joint compatibility of a frame's hypothesis (gs_assoc_nn.hip, k_joint_compat): the gate table, the batch / resident / frame calls ----
// Q(m, h) = e^-h sum_{k < m} h^k / k!: the upper tail of chi-square with 2 m degrees of freedom at x = 2 h, terms by t_k = t_{k-1} h / k
static double jc_tail(int m, double h) {
    double t = std::exp(-h), s = t;
    for (int k = 1; k < m; ++k) { t = t * h / k; s += t; }
    return s;
}
extern "C" int gs_jc_params_set_confidence(gs_jc_params *p, double confidence) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (!(confidence > 0.0 && confidence < 1.0)) return fail(GS_ERR_INVALID, "gs_jc_params: confidence must lie inside (0, 1)");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p); p->confidence = confidence;
    const double tail = 1.0 - confidence;
    p->gate[0] = 0.0;
    for (int m = 1; m <= GS_NN_FRAME_MAX; ++m) {                    // bisection on the decreasing tail until the bracket is two neighbouring doubles
        double lo = 0.0, hi = 2.0 * m + 16.0;
        while (jc_tail(m, hi) > tail && hi < 1e6) hi *= 2.0;
        for (int it = 0; it < 200; ++it) { const double mid = 0.5 * (lo + hi); if (!(mid > lo && mid < hi)) break;
            if (jc_tail(m, mid) > tail) lo = mid; else hi = mid; }
        p->gate[m] = 2.0 * hi;
        if (p->gate[m] < p->gate[m - 1]) p->gate[m] = p->gate[m - 1];   // (more degrees of freedom never lower a quantile; rounding must not either)
    }
    return GS_OK;
}
extern "C" int gs_jc_params_default(gs_jc_params *p) { return gs_jc_params_set_confidence(p, 0.95); }
static int jc_params_check(const gs_jc_params *p, JcGate &gt) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_jc_params)) return fail(GS_ERR_INVALID, "gs_jc_params: wrong struct_size");
    for (int m = 0; m <= GS_NN_FRAME_MAX; ++m) {
        if (!std::isfinite(p->gate[m]) || p->gate[m] < 0.0) return fail(GS_ERR_INVALID, "gs_jc_params: a gate is not finite or negative");
        if (m > 0 && p->gate[m] < p->gate[m - 1]) return fail(GS_ERR_INVALID, "gs_jc_params: the gates must not decrease");
        gt.g[m] = p->gate[m]; }
    return GS_OK;
}
// of gs_nn_params only struct_size and the three sigmas are read: the hypothesis is the caller's, no gate or distance test is repeated
static int jc_sigmas_check(const gs_nn_params *p, NnDev &d) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_nn_params)) return fail(GS_ERR_INVALID, "gs_nn_params: wrong struct_size");
    const double v[3] = {p->sigma_range, p->sigma_bearing, p->sigma_xy};
    for (double x : v) if (!std::isfinite(x) || x < 0.0) return fail(GS_ERR_INVALID, "gs_nn_params: a sigma is not finite or negative");
    d = NnDev{0.0, 0.0, 0.0, p->sigma_range, p->sigma_bearing, p->sigma_xy};
    return GS_OK;
}
extern "C" int gs_joint_compat_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                     int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const double *map_cov,
                                     const double *pose_cov, const gs_nn_params *params, const gs_jc_params *jc, const int32_t *in_index,
                                     int32_t *out, double *out_j, int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable, double *out_delta) {
    if (!g || n < 0 || npose < 0 || n_map < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !in_index || !out)) || (n_map > 0 && !map_xy))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = jc_sigmas_check(params, nd); if (rc != GS_OK) return rc;
    JcGate gt; if ((rc = jc_params_check(jc, gt)) != GS_OK) return rc;
    if ((rc = frame_inputs_check(n, npose, pose_of_obs, n_frames, frame_start, in_index, n_map, true)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    const size_t nf = (size_t)n_frames;
    Staging sg{g}; BatchIo io; double *oj, *odl; int32_t *ii, *o, *ok, *od, *ou;
    io.add(sg, ObsRef{n, poses, npose, pose_of_obs, obs, n_frames, frame_start, pose_cov}, MapRef{n_map, map_xy, nullptr, map_cov, 0, nullptr, nullptr}, false);
    sg.add(ii, n, in_index); sg.add(o, n); sg.add(oj, nf); sg.add(odl, 3 * nf); sg.add(ok, nf); sg.add(od, nf); sg.add(ou, nf);
    if ((rc = sg.commit()) != GS_OK) return rc;
    launch_joint_compat(io.o, io.m, g->cfg.lidar_to_cog, nd, gt, ii, o, oj, ok, od, ou, odl, Launch{g->stream});
    sg.fetch(out, o, (size_t)n * sizeof(int32_t)); sg.fetch(out_j, oj, nf * sizeof(double)); sg.fetch(out_kept, ok, nf * sizeof(int32_t));
    sg.fetch(out_dropped, od, nf * sizeof(int32_t)); sg.fetch(out_untestable, ou, nf * sizeof(int32_t)); sg.fetch(out_delta, odl, 3 * nf * sizeof(double));
    return sg.finish("joint compatibility");
}
extern "C" int gs_joint_compat_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                        int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov, const gs_nn_params *params,
                                        const gs_jc_params *jc, const int32_t *dev_in_index, int32_t *dev_out, double *dev_out_j, int32_t *dev_out_kept,
                                        int32_t *dev_out_dropped, int32_t *dev_out_untestable, double *dev_out_delta) {
    if (!g || n < 0 || npose < 0 || n_frames < 0 || !dev_frame_start || (n > 0 && (!dev_poses || !dev_pose_of_obs || !dev_obs || !dev_in_index || !dev_out)))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = jc_sigmas_check(params, nd); if (rc != GS_OK) return rc;
    JcGate gt; if ((rc = jc_params_check(jc, gt)) != GS_OK) return rc;
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    launch_joint_compat(ObsRef{n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov}, resident_map_whole(g), g->cfg.lidar_to_cog, nd, gt, dev_in_index,
                        dev_out, dev_out_j, dev_out_kept, dev_out_dropped, dev_out_untestable, dev_out_delta, Launch{g->stream, g->ev_lin[0], g->ev_lin[1]});
    return resident_done(g, "joint compatibility");
}
extern "C" int gs_debug_time_joint_compat_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                                   const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov,
                                                   const gs_nn_params *params, const gs_jc_params *jc, const int32_t *dev_in_index, int32_t *dev_out,
                                                   double *dev_out_j, int32_t *dev_out_kept, int32_t *dev_out_dropped, int32_t *dev_out_untestable,
                                                   double *dev_out_delta, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_joint_compat_resident(g, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, jc, dev_in_index,
        dev_out, dev_out_j, dev_out_kept, dev_out_dropped, dev_out_untestable, dev_out_delta); });
}

// ---- frame localisation (gs_assoc_nn.hip, k_localize): the iterated pose refinement of a frame against the map — batch / resident / frame calls ----
extern "C" int gs_loc_params_default(gs_loc_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->max_iterations = 5; p->tol_xy = 1e-6; p->tol_theta = 1e-8;
    return GS_OK;
}
static int loc_params_check(const gs_loc_params *p, LoParams &lp) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_loc_params)) return fail(GS_ERR_INVALID, "gs_loc_params: wrong struct_size");
    if (p->max_iterations < 1 || p->max_iterations > GS_LOC_ITER_MAX) return fail(GS_ERR_INVALID, "gs_loc_params: max_iterations outside 1 .. GS_LOC_ITER_MAX");
    if (!std::isfinite(p->tol_xy) || p->tol_xy < 0.0 || !std::isfinite(p->tol_theta) || p->tol_theta < 0.0)
        return fail(GS_ERR_INVALID, "gs_loc_params: a tolerance is not finite or negative");
    lp = LoParams{p->max_iterations, p->tol_xy, p->tol_theta};
    return GS_OK;
}
extern "C" int gs_debug_localize(gs_graph *g, int32_t kernel, double *dev_out_step_3) {
    if (!g || kernel < -1 || kernel > 1) return fail(GS_ERR_INVALID, "bad argument");
    g->fe.lo_kernel = kernel; g->fe.lo_step = dev_out_step_3;
    return GS_OK;
}
extern "C" int gs_localize_batch(gs_graph *g, int32_t n, const double *poses, int32_t npose, const int32_t *pose_of_obs, const double *obs,
                                 int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const double *map_cov,
                                 const double *pose_cov, const gs_nn_params *params, const gs_loc_params *loc, const int32_t *in_index,
                                 double *out_pose, double *out_cov, double *out_chi2, int32_t *out_pairs, int32_t *out_iters, int32_t *out_status) {
    if (!g || n < 0 || npose < 0 || n_map < 0 || (n > 0 && (!poses || !pose_of_obs || !obs || !in_index)) || (n_map > 0 && !map_xy))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = jc_sigmas_check(params, nd); if (rc != GS_OK) return rc;
    LoParams lp; if ((rc = loc_params_check(loc, lp)) != GS_OK) return rc;
    if ((rc = frame_inputs_check(n, npose, pose_of_obs, n_frames, frame_start, in_index, n_map, true)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    const size_t nf = (size_t)n_frames;
    Staging sg{g}; BatchIo io; double *op, *oc, *ox; int32_t *ii, *on, *oi, *os;
    io.add(sg, ObsRef{n, poses, npose, pose_of_obs, obs, n_frames, frame_start, pose_cov}, MapRef{n_map, map_xy, nullptr, map_cov, 0, nullptr, nullptr}, false);
    sg.add(ii, n, in_index); sg.add(op, 3 * nf); sg.add(oc, 9 * nf); sg.add(ox, nf); sg.add(on, nf); sg.add(oi, nf); sg.add(os, nf);
    if ((rc = sg.commit()) != GS_OK) return rc;
    launch_localize(io.o, io.m, g->cfg.lidar_to_cog, nd, lp, ii, LoOut{op, oc, ox, on, oi, os, nullptr}, g->fe.lo_kernel, Launch{g->stream});
    sg.fetch(out_pose, op, 3 * nf * sizeof(double)); sg.fetch(out_cov, oc, 9 * nf * sizeof(double)); sg.fetch(out_chi2, ox, nf * sizeof(double));
    sg.fetch(out_pairs, on, nf * sizeof(int32_t)); sg.fetch(out_iters, oi, nf * sizeof(int32_t)); sg.fetch(out_status, os, nf * sizeof(int32_t));
    return sg.finish("frame localisation");
}
extern "C" int gs_localize_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs, const double *dev_obs,
                                    int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov, const gs_nn_params *params,
                                    const gs_loc_params *loc, const int32_t *dev_in_index, double *dev_out_pose, double *dev_out_cov, double *dev_out_chi2,
                                    int32_t *dev_out_pairs, int32_t *dev_out_iters, int32_t *dev_out_status) {
    if (!g || n < 0 || npose < 0 || n_frames < 0 || !dev_frame_start || (n > 0 && (!dev_poses || !dev_pose_of_obs || !dev_obs || !dev_in_index)))
        return fail(GS_ERR_INVALID, "bad argument");
    NnDev nd; int rc = jc_sigmas_check(params, nd); if (rc != GS_OK) return rc;
    LoParams lp; if ((rc = loc_params_check(loc, lp)) != GS_OK) return rc;
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    auto &fe = g->fe;
    launch_localize(ObsRef{n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov}, resident_map_whole(g), g->cfg.lidar_to_cog, nd, lp, dev_in_index,
                    LoOut{dev_out_pose, dev_out_cov, dev_out_chi2, dev_out_pairs, dev_out_iters, dev_out_status, fe.lo_step}, fe.lo_kernel,
                    Launch{g->stream, g->ev_lin[0], g->ev_lin[1]});
    return resident_done(g, "frame localisation");
}
extern "C" int gs_debug_time_localize_resident(gs_graph *g, int32_t n, const double *dev_poses, int32_t npose, const int32_t *dev_pose_of_obs,
                                               const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov,
                                               const gs_nn_params *params, const gs_loc_params *loc, const int32_t *dev_in_index, double *dev_out_pose,
                                               double *dev_out_cov, double *dev_out_chi2, int32_t *dev_out_pairs, int32_t *dev_out_iters, int32_t *dev_out_status,
                                               int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_localize_resident(g, n, dev_poses, npose, dev_pose_of_obs, dev_obs, n_frames, dev_frame_start, dev_pose_cov, params, loc, dev_in_index,
        dev_out_pose, dev_out_cov, dev_out_chi2, dev_out_pairs, dev_out_iters, dev_out_status); });
}

// ---- relocalisation (gs_reloc.hip, k_reloc_seed / k_reloc_pick): a frame's pose found on the map without a prior — batch / resident / frame calls ----
extern "C" int gs_reloc_params_default(gs_reloc_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->seed_obs = 12; p->min_inliers = 4; p->min_baseline = 2.0; p->length_tol = 0.3; p->inlier_radius = 0.5; p->type_tol = 1e-4;
    p->distinct_xy = 2.0; p->distinct_cos = 0.98006657784124163;
    return GS_OK;
}
static int reloc_params_check(const gs_reloc_params *p, RlDev &d) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_reloc_params)) return fail(GS_ERR_INVALID, "gs_reloc_params: wrong struct_size");
    if (p->seed_obs < 2 || p->seed_obs > GS_RELOC_SEED_MAX) return fail(GS_ERR_INVALID, "gs_reloc_params: seed_obs outside 2 .. GS_RELOC_SEED_MAX");
    if (p->min_inliers < 2) return fail(GS_ERR_INVALID, "gs_reloc_params: min_inliers below 2");
    const double len[4] = {p->min_baseline, p->length_tol, p->inlier_radius, p->distinct_xy};
    for (double x : len) if (!std::isfinite(x) || !(x > 0.0)) return fail(GS_ERR_INVALID, "gs_reloc_params: a length is not finite or not positive");
    if (!std::isfinite(p->type_tol)) return fail(GS_ERR_INVALID, "gs_reloc_params: type_tol is not finite");
    if (!(p->distinct_cos >= -1.0 && p->distinct_cos <= 1.0)) return fail(GS_ERR_INVALID, "gs_reloc_params: distinct_cos outside [-1, 1]");
    d = RlDev{p->seed_obs, p->min_inliers, p->min_baseline, p->length_tol, p->inlier_radius, p->inlier_radius * p->inlier_radius, p->type_tol,
              p->distinct_xy * p->distinct_xy, p->distinct_cos};
    return GS_OK;
}
extern "C" int gs_debug_relocalize(gs_graph *g, int32_t slice_cones) {
    if (!g || slice_cones < 0) return fail(GS_ERR_INVALID, "bad argument");
    g->fe.rl_slice = slice_cones;
    return GS_OK;
}
extern "C" int gs_relocalize_batch(gs_graph *g, int32_t n, const double *obs, int32_t n_frames, const int32_t *frame_start, int32_t n_map,
                                   const double *map_xy, const int32_t *map_type, const gs_reloc_params *params, double *out_pose, int32_t *out_count,
                                   double *out_cost, int32_t *out_seed, int32_t *out_second_count, double *out_second_pose, int64_t *out_n_seeds,
                                   int32_t *out_status, int32_t *out_index, double *out_e2) {
    if (!g || n < 0 || n_map < 0 || (n > 0 && !obs) || (n_map > 0 && (!map_xy || !map_type))) return fail(GS_ERR_INVALID, "bad argument");
    RlDev rd; int rc = reloc_params_check(params, rd); if (rc != GS_OK) return rc;
    if ((rc = frame_start_check(n, n_frames, frame_start)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    const size_t nf = (size_t)n_frames;
    int slice = 0; const int n_slices = reloc_slices(n_frames, n_map, g->fe.rl_slice, slice);
    Staging sg{g}; BatchIo io; double *op, *osp, *oc, *oe; int32_t *osd, *ocn, *osc, *ost, *oi; long long *ons; char *rec;
    io.add(sg, ObsRef{n, nullptr, 0, nullptr, obs, n_frames, frame_start, nullptr}, MapRef{n_map, map_xy, map_type, nullptr, 0, nullptr, nullptr}, grid_batch(g, n_map));
    sg.add(rec, reloc_rec_bytes(n_frames, n_slices)); sg.add(op, 3 * nf); sg.add(osp, 3 * nf); sg.add(oc, nf); sg.add(ons, nf);
    sg.add(osd, 4 * nf); sg.add(ocn, nf); sg.add(osc, nf); sg.add(ost, nf); sg.add(oi, n); sg.add(oe, n);
    if ((rc = sg.commit()) != GS_OK) return rc;
    io.build_grid(g, rd.inlier_radius);
    const bool second = out_second_count || out_second_pose;
    launch_relocalize(io.o, io.m, g->cfg.lidar_to_cog, rd, slice, n_slices, (RlRec *)rec, RlOut{op, oc, ocn, osd, second ? osc : nullptr, second ? osp : nullptr, ons, ost, oi, oe},
                      nullptr, nullptr, Launch{g->stream});
    sg.fetch(out_pose, op, 3 * nf * sizeof(double)); sg.fetch(out_count, ocn, nf * sizeof(int32_t)); sg.fetch(out_cost, oc, nf * sizeof(double));
    sg.fetch(out_seed, osd, 4 * nf * sizeof(int32_t)); sg.fetch(out_second_count, osc, nf * sizeof(int32_t)); sg.fetch(out_second_pose, osp, 3 * nf * sizeof(double));
    sg.fetch(out_n_seeds, ons, nf * sizeof(int64_t)); sg.fetch(out_status, ost, nf * sizeof(int32_t)); sg.fetch(out_index, oi, (size_t)n * sizeof(int32_t));
    sg.fetch(out_e2, oe, (size_t)n * sizeof(double));
    return sg.finish("relocalisation");
}
// the search against the resident map through either scoring search (relocalisation's own grid, built first where it is stale): what the
// resident and the frame call end in.  o's pose fields are not read
static int reloc_resident_launch(gs_graph *g, bool grid, const ObsRef &o, const RlDev &rd, const RlOut &out, double *chain_pose, int32_t *chain_frame_end) {
    auto &fe = g->fe;
    int slice = 0; const int n_slices = reloc_slices(o.n_frames, fe.map_n, fe.rl_slice, slice);
    int rc = arena_reserve(g, fe.rl_rec, reloc_rec_bytes(o.n_frames, n_slices)); if (rc != GS_OK) return rc;
    MapRef m; if ((rc = resident_map(g, fe.rl_grid, grid, rd.inlier_radius, m)) != GS_OK) return rc;
    launch_relocalize(o, m, g->cfg.lidar_to_cog, rd, slice, n_slices, (RlRec *)fe.rl_rec.mem, out, chain_pose, chain_frame_end, Launch{g->stream, g->ev_lin[0], g->ev_lin[1]});
    return GS_OK;
}
extern "C" int gs_relocalize_resident(gs_graph *g, int32_t n, const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start,
                                      const gs_reloc_params *params, double *dev_out_pose, int32_t *dev_out_count, double *dev_out_cost, int32_t *dev_out_seed,
                                      int32_t *dev_out_second_count, double *dev_out_second_pose, int64_t *dev_out_n_seeds, int32_t *dev_out_status,
                                      int32_t *dev_out_index, double *dev_out_e2) {
    if (!g || n < 0 || n_frames < 0 || !dev_frame_start || (n > 0 && !dev_obs)) return fail(GS_ERR_INVALID, "bad argument");
    RlDev rd; int rc = reloc_params_check(params, rd); if (rc != GS_OK) return rc;
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    if (n_frames == 0) return GS_OK;
    if ((rc = reloc_resident_launch(g, grid_resident(g), ObsRef{n, nullptr, 0, nullptr, dev_obs, n_frames, dev_frame_start, nullptr}, rd,
                                    RlOut{dev_out_pose, dev_out_cost, dev_out_count, dev_out_seed, dev_out_second_count, dev_out_second_pose, (long long *)dev_out_n_seeds,
                                          dev_out_status, dev_out_index, dev_out_e2}, nullptr, nullptr)) != GS_OK) return rc;
    return resident_done(g, "relocalisation");
}
extern "C" int gs_debug_time_relocalize_resident(gs_graph *g, int32_t n, const double *dev_obs, int32_t n_frames, const int32_t *dev_frame_start,
                                                 const gs_reloc_params *params, double *dev_out_pose, int32_t *dev_out_count, double *dev_out_cost,
                                                 int32_t *dev_out_seed, int32_t *dev_out_second_count, double *dev_out_second_pose, int64_t *dev_out_n_seeds,
                                                 int32_t *dev_out_status, int32_t *dev_out_index, double *dev_out_e2, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_relocalize_resident(g, n, dev_obs, n_frames, dev_frame_start, params, dev_out_pose, dev_out_count, dev_out_cost, dev_out_seed,
        dev_out_second_count, dev_out_second_pose, dev_out_n_seeds, dev_out_status, dev_out_index, dev_out_e2); });
}

// ---- the live chain: one frame through the assignment and what a call asks behind it, back to back on the stream, one wait —
// gs_frame_frontend_assign / _assign_opt / _jc / _localize / _relocalize (staging and records: gs_frame_host.hpp) ----
namespace {
// the frame and the out-pointers of a call, bundled where the extern "C" function receives them (a null member: the caller did not ask)
struct FrameIn { const double *pose, *pose_cov, *obs; int32_t k; };
struct AssignOut { double *zxy, *gxy; int32_t *idx; double *d2; int32_t *na; };
struct JcOut { double *j; int32_t *kept, *dropped, *untestable; double *delta; };
struct LocOut { double *pose, *cov, *chi2; int32_t *pairs, *iters, *status; };
struct RelocOut { double *pose; int32_t *count; double *cost; int32_t *seed, *second_count; double *second_pose; int64_t *n_seeds; int32_t *status, *index; double *e2; };
// what a call asks of the chain: the greedy (opt false) or the minimum-cost assignment, then the joint test of its result, then the localisation
// under the pruned index; search: relocalisation's search in front, whose last kernel writes the pose the assignment reads
struct Chain { bool opt, jc, loc; const RlDev *search; bool second; NnDev nd; JcGate gt; LoParams lp; };
}
// a record to the caller's pointers: the pinned copy after the wait, or what the empty frame gets without a launch
static void jc_store(const JcOut &o, const JcRec &r) {
    if (o.j) *o.j = r.j;
    if (o.delta) std::memcpy(o.delta, r.delta, sizeof(r.delta));
    if (o.kept) *o.kept = r.kept;
    if (o.dropped) *o.dropped = r.dropped;
    if (o.untestable) *o.untestable = r.untestable;
}
static void lo_store(const LocOut &o, const LoRec &r) {
    if (o.pose) std::memcpy(o.pose, r.pose, sizeof(r.pose));
    if (o.cov) std::memcpy(o.cov, r.cov, sizeof(r.cov));
    if (o.chi2) *o.chi2 = r.chi2;
    if (o.pairs) *o.pairs = r.pairs;
    if (o.iters) *o.iters = r.iterations;
    if (o.status) *o.status = r.status;
}
static void reloc_store(const RelocOut &o, const RelocRec &r, int32_t k) {
    if (o.pose) std::memcpy(o.pose, r.pose, sizeof(r.pose));
    if (o.second_pose) std::memcpy(o.second_pose, r.second_pose, sizeof(r.second_pose));
    if (o.cost) *o.cost = r.cost;
    if (o.n_seeds) *o.n_seeds = r.n_seeds;
    if (o.seed) std::memcpy(o.seed, r.seed, sizeof(r.seed));
    if (o.count) *o.count = r.count;
    if (o.second_count) *o.second_count = r.second_count;
    if (o.status) *o.status = r.status;
    if (o.index) std::memcpy(o.index, r.index, (size_t)k * sizeof(int32_t));
    if (o.e2) std::memcpy(o.e2, r.e2, (size_t)k * sizeof(double));
}
// the empty frame's records: no pair and nothing tested (JcRec{}); the prior's bits, status 2; no seed
static LoRec lo_empty(const double pose[3], const double *pose_cov) {
    LoRec r{}; const int up[9] = {0, 1, 2, 1, 4, 5, 2, 5, 8};
    std::memcpy(r.pose, pose, sizeof(r.pose));
    for (int t = 0; t < 9; ++t) r.cov[t] = pose_cov ? pose_cov[up[t]] : 0.0;
    r.status = 2;
    return r;
}
static RelocRec reloc_none() {
    RelocRec r{}; r.cost = INFINITY; r.seed[0] = r.seed[1] = r.seed[2] = r.seed[3] = -1; r.status = 2;
    return r;
}
// everything a caller can get wrong about a chain call, decided before the device is touched; then the device
static int chain_checks(gs_graph *g, const FrameIn &f, const AssignOut &a, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, Chain &c) {
    if (!g || !f.pose || f.k < 0 || (f.k > 0 && (!f.obs || !a.zxy || !a.gxy || !a.idx || !a.d2))) return fail(GS_ERR_INVALID, "bad argument");
    int rc = nn_params_check(params, c.nd); if (rc != GS_OK) return rc;
    if (c.jc && (rc = jc_params_check(jc, c.gt)) != GS_OK) return rc;
    if (c.loc && (rc = loc_params_check(loc, c.lp)) != GS_OK) return rc;
    if (f.k > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "a frame holds more than GS_NN_FRAME_MAX observations");
    return ensure_device(g);
}
// a checked frame of 0 .. GS_NN_FRAME_MAX observations: staged and sent, the search if asked, the assignment through the resident launch, the
// joint test and the localisation if asked, the copies back, the one wait, and the results to the caller
static int frame_chain_run(gs_graph *g, const FrameIn &f, const Chain &c, const AssignOut &a, const JcOut &jo, const LocOut &lo, const RelocOut &ro) {
    auto &fe = g->fe; int rc; const int32_t k = f.k;
    if (k == 0) {                                                   // nothing is launched
        if (c.search) reloc_store(ro, reloc_none(), 0);
        if (c.jc) jc_store(jo, JcRec{});
        if (c.loc) lo_store(lo, lo_empty(f.pose, f.pose_cov));
        return GS_OK; }
    const FrameLayout L = frame_layout_chain(k);
    if ((rc = stage_for(g, fe.fr_in, k, GS_NN_FRAME_MAX, [](size_t m) { return frame_layout_chain(m).in_bytes; })) != GS_OK) return rc;
    if ((rc = stage_for(g, fe.fr_out, k, GS_NN_FRAME_MAX, [](size_t m) { return frame_layout_chain(m).out_bytes; })) != GS_OK) return rc;
    if (c.jc && (rc = fe.ch_rec.reserve(g, sizeof(ChainRec))) != GS_OK) return rc;       // once per handle: the sizes do not depend on k
    if (c.search && (rc = fe.rl_out.reserve(g, sizeof(RelocRec))) != GS_OK) return rc;
    char *pi = fe.fr_in.pin;
    std::memset(pi, 0, L.in_bytes);                                 // (no covariance: zeros; frame_start[0], pose_of_obs)
    std::memcpy(pi + L.pose, f.pose, 3 * sizeof(double));
    if (f.pose_cov) std::memcpy(pi + L.cov, f.pose_cov, 9 * sizeof(double));
    std::memcpy(pi + L.obs, f.obs, 4 * (size_t)k * sizeof(double));
    ((int32_t *)(pi + L.frame_start))[1] = k;
    if ((rc = stage_send(g, fe.fr_in, L.in_bytes)) != GS_OK) return rc;
    char *di = fe.fr_in.dev, *dv = fe.fr_out.dev;
    double *d_pose = (double *)(di + L.pose); const double *d_cov = f.pose_cov ? (const double *)(di + L.cov) : nullptr, *d_obs = (const double *)(di + L.obs);
    int32_t *d_fs = (int32_t *)(di + L.frame_start), *d_idx = (int32_t *)(dv + L.idx); const int32_t *d_po = (const int32_t *)(di + L.pose_of_obs);
    const bool grid = grid_live(g); const double lidar = g->cfg.lidar_to_cog;
    const ObsRef o{k, d_pose, 1, d_po, d_obs, 1, d_fs, d_cov};       // the frame as every launcher of the chain takes it
    if (c.search) { RelocRec *r = (RelocRec *)fe.rl_out.dev;
        if ((rc = reloc_resident_launch(g, grid, o, *c.search,
                                        RlOut{r->pose, &r->cost, &r->count, r->seed, c.second ? &r->second_count : nullptr, c.second ? r->second_pose : nullptr,
                                              &r->n_seeds, &r->status, r->index, r->e2}, d_pose, d_fs + 1)) != GS_OK) return rc;
        if ((rc = stage_fetch(g, fe.rl_out, sizeof(RelocRec))) != GS_OK) return rc; }
    if ((rc = assign_resident_launch(g, c.opt, grid, o, c.nd, d_idx, (double *)(dv + L.d2), c.opt ? (int32_t *)(dv + L.na) : nullptr, (double *)(dv + L.z),
                                     (double *)(dv + L.g))) != GS_OK) return rc;
    if (c.jc) { ChainRec *cr = (ChainRec *)fe.ch_rec.dev;           // (the localisation is asked for only behind the joint test)
        const MapRef m = resident_map_whole(g);                     // (neither searches the map)
        launch_joint_compat(o, m, lidar, c.nd, c.gt, d_idx, cr->jc.index, &cr->jc.j, &cr->jc.kept, &cr->jc.dropped, &cr->jc.untestable, cr->jc.delta, Launch{g->stream});
        if (c.loc) launch_localize(o, m, lidar, c.nd, c.lp, cr->jc.index, LoOut{cr->lo.pose, cr->lo.cov, &cr->lo.chi2, &cr->lo.pairs, &cr->lo.iterations, &cr->lo.status, nullptr},
                                   fe.lo_kernel, Launch{g->stream}); }
    const size_t bz = 2 * (size_t)k * sizeof(double), bd = (size_t)k * sizeof(double), bi = (size_t)k * sizeof(int32_t);
    if ((rc = stage_fetch(g, fe.fr_out, c.opt ? L.out_bytes : L.na)) != GS_OK) return rc;                       // (the greedy assignment counts no admissible cones)
    if (c.jc && (rc = stage_fetch(g, fe.ch_rec, c.loc ? sizeof(ChainRec) : offsetof(JcRec, index) + bi)) != GS_OK) return rc;
    if ((rc = frame_finish(g, c.loc ? "frame localisation" : c.jc ? "joint compatibility" : "assignment (nn)")) != GS_OK) return rc;
    const char *po = fe.fr_out.pin;
    std::memcpy(a.zxy, po + L.z, bz); std::memcpy(a.gxy, po + L.g, bz); std::memcpy(a.d2, po + L.d2, bd);
    if (a.na) std::memcpy(a.na, po + L.na, bi);
    if (!c.jc) std::memcpy(a.idx, po + L.idx, bi);
    else { const ChainRec *pr = (const ChainRec *)fe.ch_rec.pin;    // the joint test's pruned index in the assignment's place
        std::memcpy(a.idx, pr->jc.index, bi); jc_store(jo, pr->jc);
        if (c.loc) lo_store(lo, pr->lo); }
    if (c.search) { const RelocRec *rr = (const RelocRec *)fe.rl_out.pin;
        reloc_store(ro, *rr, k);
        if (rr->status >= 2)                                        // the chain found an empty frame: it wrote nothing per observation
            for (int i = 0; i < k; ++i) { a.zxy[2 * i] = a.zxy[2 * i + 1] = a.gxy[2 * i] = a.gxy[2 * i + 1] = 0.0; a.idx[i] = -1; a.d2[i] = INFINITY;
                if (a.na) a.na[i] = 0; } }
    return GS_OK;
}
extern "C" int gs_frame_frontend_assign(gs_graph *g, const double pose[3], const double *pose_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                        double *out_zxy, double *out_gxy, int32_t *out_idx, double *out_d2) {
    Chain c{}; const FrameIn f{pose, pose_cov, obs, k}; const AssignOut a{out_zxy, out_gxy, out_idx, out_d2, nullptr};
    const int rc = chain_checks(g, f, a, params, nullptr, nullptr, c);
    return rc != GS_OK ? rc : frame_chain_run(g, f, c, a, JcOut{}, LocOut{}, RelocOut{});
}
extern "C" int gs_frame_frontend_assign_opt(gs_graph *g, const double pose[3], const double *pose_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                            double *out_zxy, double *out_gxy, int32_t *out_idx, double *out_d2, int32_t *out_na) {
    Chain c{}; c.opt = true; const FrameIn f{pose, pose_cov, obs, k}; const AssignOut a{out_zxy, out_gxy, out_idx, out_d2, out_na};
    const int rc = chain_checks(g, f, a, params, nullptr, nullptr, c);
    return rc != GS_OK ? rc : frame_chain_run(g, f, c, a, JcOut{}, LocOut{}, RelocOut{});
}
extern "C" int gs_frame_frontend_jc(gs_graph *g, const double pose[3], const double *pose_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                    const gs_jc_params *jc, double *out_zxy, double *out_gxy, int32_t *out_idx, double *out_d2, int32_t *out_na,
                                    double *out_j, int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable, double *out_delta) {
    Chain c{}; c.opt = c.jc = true; const FrameIn f{pose, pose_cov, obs, k}; const AssignOut a{out_zxy, out_gxy, out_idx, out_d2, out_na};
    const int rc = chain_checks(g, f, a, params, jc, nullptr, c);
    return rc != GS_OK ? rc : frame_chain_run(g, f, c, a, JcOut{out_j, out_kept, out_dropped, out_untestable, out_delta}, LocOut{}, RelocOut{});
}
extern "C" int gs_frame_frontend_localize(gs_graph *g, const double pose[3], const double *pose_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                          const gs_jc_params *jc, const gs_loc_params *loc, double *out_zxy, double *out_gxy, int32_t *out_idx, double *out_d2,
                                          int32_t *out_na, double *out_j, int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable, double *out_delta,
                                          double *out_pose, double *out_cov, double *out_chi2, int32_t *out_pairs, int32_t *out_iters, int32_t *out_status) {
    Chain c{}; c.opt = c.jc = c.loc = true; const FrameIn f{pose, pose_cov, obs, k}; const AssignOut a{out_zxy, out_gxy, out_idx, out_d2, out_na};
    const int rc = chain_checks(g, f, a, params, jc, loc, c);
    return rc != GS_OK ? rc : frame_chain_run(g, f, c, a, JcOut{out_j, out_kept, out_dropped, out_untestable, out_delta},
                                              LocOut{out_pose, out_cov, out_chi2, out_pairs, out_iters, out_status}, RelocOut{});
}
// the search, then the chain of gs_frame_frontend_localize from the found pose under the diagonal prior (the empty frame: at the pose zero)
extern "C" int gs_frame_frontend_relocalize(gs_graph *g, const double *obs, int32_t k, const gs_reloc_params *reloc, double prior_sigma_xy, double prior_sigma_theta,
                                            const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, double *out_rl_pose, int32_t *out_rl_count,
                                            double *out_rl_cost, int32_t *out_rl_seed, int32_t *out_second_count, double *out_second_pose, int64_t *out_n_seeds,
                                            int32_t *out_rl_status, int32_t *out_rl_index, double *out_rl_e2, double *out_zxy, double *out_gxy, int32_t *out_idx,
                                            double *out_d2, int32_t *out_na, double *out_j, int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable,
                                            double *out_delta, double *out_pose, double *out_cov, double *out_chi2, int32_t *out_pairs, int32_t *out_iters,
                                            int32_t *out_status) {
    if (!g || k < 0 || (k > 0 && (!obs || !out_zxy || !out_gxy || !out_idx || !out_d2))) return fail(GS_ERR_INVALID, "bad argument");
    RlDev rd; int rc = reloc_params_check(reloc, rd); if (rc != GS_OK) return rc;
    if (!std::isfinite(prior_sigma_xy) || prior_sigma_xy < 0.0 || !std::isfinite(prior_sigma_theta) || prior_sigma_theta < 0.0)
        return fail(GS_ERR_INVALID, "a prior sigma is not finite or negative");
    const double zero3[3] = {0.0, 0.0, 0.0};
    const double prior[9] = {prior_sigma_xy * prior_sigma_xy, 0.0, 0.0, 0.0, prior_sigma_xy * prior_sigma_xy, 0.0, 0.0, 0.0, prior_sigma_theta * prior_sigma_theta};
    Chain c{}; c.opt = c.jc = c.loc = true; c.search = &rd; c.second = out_second_count || out_second_pose;
    const FrameIn f{zero3, prior, obs, k}; const AssignOut a{out_zxy, out_gxy, out_idx, out_d2, out_na};
    if ((rc = chain_checks(g, f, a, params, jc, loc, c)) != GS_OK) return rc;
    return frame_chain_run(g, f, c, a, JcOut{out_j, out_kept, out_dropped, out_untestable, out_delta}, LocOut{out_pose, out_cov, out_chi2, out_pairs, out_iters, out_status},
                           RelocOut{out_rl_pose, out_rl_count, out_rl_cost, out_rl_seed, out_second_count, out_second_pose, out_n_seeds, out_rl_status, out_rl_index, out_rl_e2});
}

// ---- frame following (gs_follow.hip): pose hypotheses carried from frame to frame on the device — batch / resident / live frame calls ----
extern "C" int gs_follow_params_default(gs_follow_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->min_pairs = 3; p->max_misses = 3; p->merge_xy = 0.5; p->merge_theta = 0.1;
    return GS_OK;
}
namespace {
static_assert(sizeof(gs_follow_step) == FOLLOW_STEP_BYTES && sizeof(gs_follow_state) == FOLLOW_STATE_BYTES, "gs_follow_host.hpp restates the record sizes");
struct FoParams { int min_pairs, max_misses; double merge2, merge_theta; };
// what a run is made of, in device memory: the frames, the motion records, the hypotheses, the map and its search, where the records go
struct FollowRun {
    int n_hyp, n, cap; const double *obs; const int32_t *fs; const double *motion, *motion_cov;
    gs_follow_state *state; int32_t *best2; gs_follow_step *rec; int32_t *index;
    MapRef map;
    NnDev nd; JcGate gt; LoParams lp; FoParams fp;
};
}
static int follow_params_check(const gs_follow_params *p, FoParams &f) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_follow_params)) return fail(GS_ERR_INVALID, "gs_follow_params: wrong struct_size");
    if (p->min_pairs < 1 || p->max_misses < 1) return fail(GS_ERR_INVALID, "gs_follow_params: min_pairs and max_misses must be at least 1");
    if (!std::isfinite(p->merge_xy) || p->merge_xy < 0.0 || !std::isfinite(p->merge_theta) || p->merge_theta < 0.0)
        return fail(GS_ERR_INVALID, "gs_follow_params: a merge value is not finite or negative");
    f = FoParams{p->min_pairs, p->max_misses, p->merge_xy * p->merge_xy, p->merge_theta};
    return GS_OK;
}
// the four parameter blocks of a following call, decided before the device is touched
static int follow_checks(const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, const gs_follow_params *follow, FollowRun &R) {
    int rc = nn_params_check(params, R.nd); if (rc != GS_OK) return rc;
    if ((rc = jc_params_check(jc, R.gt)) != GS_OK) return rc;
    if ((rc = loc_params_check(loc, R.lp)) != GS_OK) return rc;
    return follow_params_check(follow, R.fp);
}
static int follow_hyp_check(int32_t n_hyp) {
    return n_hyp < 1 || n_hyp > GS_FOLLOW_HYP_MAX ? fail(GS_ERR_INVALID, "n_hyp outside 1 .. GS_FOLLOW_HYP_MAX") : GS_OK;
}
// the hypotheses' state (two sets of 64: the live run's, a batch or resident run's) and the stage / chain buffers for n_hyp x cap observations
static int follow_reserve(gs_graph *g, int n_hyp, int cap, FollowLayout &L) {
    auto &fe = g->fe;
    if (!follow_layout(n_hyp, cap, L)) return fail(GS_ERR_INVALID, "frame following: bad sizes");
    if (!fe.fo_state) { HIP_TRY(hipMalloc((void **)&fe.fo_state, 2 * (size_t)GS_FOLLOW_HYP_MAX * sizeof(gs_follow_state)));
        HIP_TRY(hipMalloc((void **)&fe.fo_best, 4 * sizeof(int32_t))); }
    return arena_reserve(g, fe.fo_mem, L.bytes);
}
static gs_follow_state *follow_state(gs_graph *g, bool live) { return (gs_follow_state *)g->fe.fo_state + (live ? 0 : GS_FOLLOW_HYP_MAX); }
static int32_t *follow_best(gs_graph *g, bool live) { return g->fe.fo_best + (live ? 0 : 2); }
// the state a run starts from, as k_follow_init writes it
static void follow_init_host(int n_hyp, const double *poses, const double *covs, gs_follow_state *s) {
    const int up[9] = {0, 1, 2, 1, 4, 5, 2, 5, 8};
    std::memset(s, 0, (size_t)n_hyp * sizeof(gs_follow_state));
    for (int h = 0; h < n_hyp; ++h) {
        std::memcpy(s[h].pose, poses + 3 * (size_t)h, 3 * sizeof(double));
        if (covs) for (int e = 0; e < 9; ++e) s[h].cov[e] = covs[9 * (size_t)h + up[e]];
        s[h].state_step = -1; s[h].duplicate_of = -1; }
}
// one step enqueued: the stage, the chain over n_hyp frames (not for a frame the host knows to be empty), the update.
// step: its place in the run's frame bounds and records; t: its number (state_step); k: the frame's size, or -1 where only the device knows
// it; mrec: its motion record's place, -1 for none (no prediction)
static void follow_step_enqueue(gs_graph *g, const FollowRun &R, const FollowLayout &L, int step, int t, int k, int mrec, hipEvent_t start, hipEvent_t stop) {
    auto &fe = g->fe; char *m = fe.fo_mem.at(0);
    FoArgs A{};
    A.n_hyp = R.n_hyp; A.t = t; A.n = R.n; A.cap = R.cap; A.fs = R.fs + step; A.obs = R.obs;
    A.motion = mrec >= 0 ? R.motion + 3 * (size_t)mrec : nullptr;
    A.motion_cov = mrec >= 0 && R.motion_cov ? R.motion_cov + 9 * (size_t)mrec : nullptr;
    A.state = R.state;
    A.st_obs = (double *)(m + L.obs); A.st_pose_of_obs = (int32_t *)(m + L.pose_of_obs); A.st_frame_start = (int32_t *)(m + L.frame_start);
    A.st_pose = (double *)(m + L.pose); A.st_cov = (double *)(m + L.cov);
    int32_t *as_idx = (int32_t *)(m + L.as_idx), *jc_idx = (int32_t *)(m + L.jc_idx), *jc_kept = (int32_t *)(m + L.jc_kept);
    double *as_d2 = (double *)(m + L.as_d2), *lo_pose = (double *)(m + L.lo_pose), *lo_cov = (double *)(m + L.lo_cov), *lo_chi2 = (double *)(m + L.lo_chi2);
    int32_t *lo_pairs = (int32_t *)(m + L.lo_pairs), *lo_iters = (int32_t *)(m + L.lo_iters), *lo_status = (int32_t *)(m + L.lo_status);
    A.jc_idx = jc_idx; A.jc_kept = jc_kept; A.lo_pose = lo_pose; A.lo_cov = lo_cov; A.lo_chi2 = lo_chi2; A.lo_pairs = lo_pairs; A.lo_iters = lo_iters; A.lo_status = lo_status;
    A.min_pairs = R.fp.min_pairs; A.max_misses = R.fp.max_misses; A.merge2 = R.fp.merge2; A.merge_theta = R.fp.merge_theta;
    A.rec = R.rec ? R.rec + (size_t)step * R.n_hyp : nullptr; A.out_index = R.index; A.best2 = R.best2;
    const int kk = k >= 0 ? k : R.cap;
    launch_follow_stage(A, kk, g->stream, start, nullptr);
    if (kk > 0) {
        const double lidar = g->cfg.lidar_to_cog; const Launch S{g->stream};
        const ObsRef o{R.n_hyp * kk, A.st_pose, R.n_hyp, A.st_pose_of_obs, A.st_obs, R.n_hyp, A.st_frame_start, A.st_cov};    // the stage: every hypothesis a frame
        launch_assign_opt(o, R.map, lidar, R.nd, as_idx, as_d2, nullptr, nullptr, nullptr, S);
        launch_joint_compat(o, R.map, lidar, R.nd, R.gt, as_idx, jc_idx, nullptr, jc_kept, nullptr, nullptr, nullptr, S);
        launch_localize(o, R.map, lidar, R.nd, R.lp, jc_idx, LoOut{lo_pose, lo_cov, lo_chi2, lo_pairs, lo_iters, lo_status, nullptr}, fe.lo_kernel, S);
    }
    launch_follow_update(A, R.gt, g->stream, nullptr, stop);
}
extern "C" int gs_follow_batch(gs_graph *g, int32_t n_hyp, const double *poses, const double *covs, int32_t n_steps, int32_t n, const double *obs,
                               const int32_t *frame_start, const double *motion, const double *motion_cov, int32_t n_map, const double *map_xy,
                               const int32_t *map_type, const double *map_cov, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                               const gs_follow_params *follow, gs_follow_step *out_steps, int32_t *out_index, gs_follow_state *out_state, int32_t *out_best,
                               int32_t *out_n_tracking) {
    if (!g || !poses || n_steps < 0 || n < 0 || n_map < 0 || (n > 0 && !obs) || (n_steps > 1 && !motion) || (n_map > 0 && (!map_xy || !map_type)))
        return fail(GS_ERR_INVALID, "bad argument");
    FollowRun R{}; int rc = follow_checks(params, jc, loc, follow, R); if (rc != GS_OK) return rc;
    if ((rc = follow_hyp_check(n_hyp)) != GS_OK) return rc;
    if ((rc = frame_start_check(n, n_steps, frame_start)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    int cap = 0; for (int t = 0; t < n_steps; ++t) cap = std::max(cap, frame_start[t + 1] - frame_start[t]);
    FollowLayout L; if ((rc = follow_reserve(g, n_hyp, cap, L)) != GS_OK) return rc;
    std::vector<gs_follow_state> init((size_t)n_hyp); follow_init_host(n_hyp, poses, covs, init.data());
    const int32_t best0[2] = {0, n_hyp};
    const size_t nm = n_steps > 1 ? (size_t)n_steps - 1 : 0, nrec = (size_t)n_steps * n_hyp;
    Staging sg{g}; BatchIo io; double *mo, *mq; int32_t *b2, *oi; gs_follow_state *stt; gs_follow_step *rec;
    sg.add(stt, (size_t)n_hyp, (const gs_follow_state *)init.data()); sg.add(b2, 2, best0);
    io.add(sg, ObsRef{n, nullptr, 0, nullptr, obs, n_steps, frame_start, nullptr}, MapRef{n_map, map_xy, map_type, map_cov, 0, nullptr, nullptr}, grid_batch(g, n_map));
    sg.add(mo, 3 * nm, motion); sg.add(mq, 9 * nm, motion_cov); sg.add(rec, nrec); sg.add(oi, out_index ? (size_t)n_hyp * n : 0);
    if ((rc = sg.commit()) != GS_OK) return rc;
    io.build_grid(g, R.nd.max_distance);
    R.n_hyp = n_hyp; R.n = n; R.cap = cap; R.obs = io.o.obs; R.fs = io.o.frame_start; R.motion = mo; R.motion_cov = motion_cov ? mq : nullptr;
    R.state = stt; R.best2 = b2; R.rec = rec; R.index = out_index ? oi : nullptr; R.map = io.m;
    for (int t = 0; t < n_steps; ++t)                               // back to back: no host decision between the frames
        follow_step_enqueue(g, R, L, t, t, frame_start[t + 1] - frame_start[t], t - 1, nullptr, nullptr);
    sg.fetch(out_steps, rec, nrec * sizeof(gs_follow_step)); sg.fetch(out_index, oi, (size_t)n_hyp * n * sizeof(int32_t));
    sg.fetch(out_state, stt, (size_t)n_hyp * sizeof(gs_follow_state)); sg.fetch(out_best, b2, sizeof(int32_t)); sg.fetch(out_n_tracking, b2 + 1, sizeof(int32_t));
    return sg.finish("frame following");                            // the one wait of the call
}
extern "C" int gs_follow_resident(gs_graph *g, int32_t n_hyp, const double *dev_poses, const double *dev_covs, int32_t n_steps, int32_t n, const double *dev_obs,
                                  const int32_t *dev_frame_start, int32_t frame_cap, const double *dev_motion, const double *dev_motion_cov,
                                  const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, const gs_follow_params *follow,
                                  gs_follow_step *dev_out_steps, int32_t *dev_out_index, gs_follow_state *dev_out_state, int32_t *dev_out_best_2) {
    if (!g || !dev_poses || n_steps < 0 || n < 0 || !dev_frame_start || (n > 0 && !dev_obs) || (n_steps > 1 && !dev_motion)) return fail(GS_ERR_INVALID, "bad argument");
    FollowRun R{}; int rc = follow_checks(params, jc, loc, follow, R); if (rc != GS_OK) return rc;
    if ((rc = follow_hyp_check(n_hyp)) != GS_OK) return rc;
    if (frame_cap < 0 || frame_cap > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "frame_cap outside 0 .. GS_NN_FRAME_MAX");
    if ((rc = dev_obs_aligned(dev_obs)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    FollowLayout L; if ((rc = follow_reserve(g, n_hyp, frame_cap, L)) != GS_OK) return rc;
    if ((rc = resident_map(g, g->fe.grid, grid_resident(g), R.nd.max_distance, R.map)) != GS_OK) return rc;
    R.n_hyp = n_hyp; R.n = n; R.cap = frame_cap; R.obs = dev_obs; R.fs = dev_frame_start; R.motion = dev_motion; R.motion_cov = dev_motion_cov;
    R.state = follow_state(g, false); R.best2 = follow_best(g, false); R.rec = dev_out_steps; R.index = dev_out_index;
    launch_follow_init(n_hyp, dev_poses, dev_covs, R.state, R.best2, g->stream, g->ev_lin[0], n_steps == 0 ? g->ev_lin[1] : nullptr);
    for (int t = 0; t < n_steps; ++t) follow_step_enqueue(g, R, L, t, t, -1, t - 1, nullptr, t == n_steps - 1 ? g->ev_lin[1] : nullptr);
    if (dev_out_state) HIP_TRY(hipMemcpyAsync(dev_out_state, R.state, (size_t)n_hyp * sizeof(gs_follow_state), hipMemcpyDeviceToDevice, g->stream));
    if (dev_out_best_2) HIP_TRY(hipMemcpyAsync(dev_out_best_2, R.best2, 2 * sizeof(int32_t), hipMemcpyDeviceToDevice, g->stream));
    return resident_done(g, "frame following");
}
extern "C" int gs_debug_time_follow_resident(gs_graph *g, int32_t n_hyp, const double *dev_poses, const double *dev_covs, int32_t n_steps, int32_t n,
                                             const double *dev_obs, const int32_t *dev_frame_start, int32_t frame_cap, const double *dev_motion,
                                             const double *dev_motion_cov, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                                             const gs_follow_params *follow, gs_follow_step *dev_out_steps, int32_t *dev_out_index, gs_follow_state *dev_out_state,
                                             int32_t *dev_out_best_2, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_follow_resident(g, n_hyp, dev_poses, dev_covs, n_steps, n, dev_obs, dev_frame_start, frame_cap, dev_motion, dev_motion_cov, params, jc, loc, follow,
                                  dev_out_steps, dev_out_index, dev_out_state, dev_out_best_2); });
}
extern "C" int gs_debug_time_cand_resident(gs_graph *g, int32_t n_steps, int32_t n, const double *dev_obs, const int32_t *dev_frame_start, int32_t frame_cap,
                                           const double *dev_poses, const double *dev_pose_covs, const int32_t *dev_in_idx, int32_t n_in, const gs_cand *dev_in_table,
                                           const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *dev_out_steps, int32_t *dev_out_cand_id,
                                           int32_t *dev_out_cand_slot, gs_cand *dev_out_table, int32_t *dev_out_meta_4, int32_t reps, double *out_ms) {
    return time_resident(g, reps, out_ms, [&] {
        return gs_cand_resident(g, n_steps, n, dev_obs, dev_frame_start, frame_cap, dev_poses, dev_pose_covs, dev_in_idx, n_in, dev_in_table, params, cand,
                                dev_out_steps, dev_out_cand_id, dev_out_cand_slot, dev_out_table, dev_out_meta_4); });
}
// the live run: the hypotheses stay on the handle between frames
extern "C" int gs_follow_set(gs_graph *g, int32_t n_hyp, const double *poses, const double *covs) {
    if (!g || !poses) return fail(GS_ERR_INVALID, "bad argument");
    int rc = follow_hyp_check(n_hyp); if (rc != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    FollowLayout L; if ((rc = follow_reserve(g, n_hyp, 0, L)) != GS_OK) return rc;
    std::vector<gs_follow_state> init((size_t)n_hyp); follow_init_host(n_hyp, poses, covs, init.data());
    const int32_t best0[2] = {0, n_hyp};
    HIP_TRY(hipMemcpyAsync(follow_state(g, true), init.data(), (size_t)n_hyp * sizeof(gs_follow_state), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipMemcpyAsync(follow_best(g, true), best0, sizeof(best0), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // pageable sources
    g->fe.pin_map_busy = false; g->fe.fo_n_hyp = n_hyp; g->fe.fo_t = 0;
    return GS_OK;
}
extern "C" int gs_follow_get(gs_graph *g, gs_follow_state *out_state, int32_t *out_n_hyp, int32_t *out_best, int32_t *out_n_tracking) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    if (fe.fo_n_hyp == 0) return fail(GS_ERR_INVALID, "gs_follow_get before gs_follow_set");
    int32_t b2[2] = {0, 0};
    if (out_state) HIP_TRY(hipMemcpyAsync(out_state, follow_state(g, true), (size_t)fe.fo_n_hyp * sizeof(gs_follow_state), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(b2, follow_best(g, true), sizeof(b2), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    fe.pin_map_busy = false;
    if (out_n_hyp) *out_n_hyp = fe.fo_n_hyp;
    if (out_best) *out_best = b2[0];
    if (out_n_tracking) *out_n_tracking = b2[1];
    return GS_OK;
}
extern "C" int gs_frame_frontend_follow(gs_graph *g, const double *motion, const double *motion_cov, const double *obs, int32_t k, const gs_nn_params *params,
                                        const gs_jc_params *jc, const gs_loc_params *loc, const gs_follow_params *follow, gs_follow_step *out_steps,
                                        int32_t *out_index, int32_t *out_best, int32_t *out_n_tracking) {
    if (!g || k < 0 || (k > 0 && !obs) || (motion_cov && !motion)) return fail(GS_ERR_INVALID, "bad argument");
    FollowRun R{}; int rc = follow_checks(params, jc, loc, follow, R); if (rc != GS_OK) return rc;
    if (k > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "a frame holds more than GS_NN_FRAME_MAX observations");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    if (fe.fo_n_hyp == 0) return fail(GS_ERR_INVALID, "gs_frame_frontend_follow before gs_follow_set");
    if ((fe.fo_t == 0) != (motion == nullptr)) return fail(GS_ERR_INVALID, "motion must be NULL on the first frame after gs_follow_set and given on every later one");
    const int n_hyp = fe.fo_n_hyp;
    FollowLayout L; if ((rc = follow_reserve(g, n_hyp, k, L)) != GS_OK) return rc;
    using Io = FollowFrameIo;
    if ((rc = fe.fo_in.reserve(g, Io::IN_BYTES)) != GS_OK || (rc = fe.fo_out.reserve(g, Io::OUT_BYTES)) != GS_OK) return rc;    // once per handle: fixed sizes
    char *pi = fe.fo_in.pin, *di = fe.fo_in.dev, *po = fe.fo_out.pin, *dv = fe.fo_out.dev;
    std::memset(pi, 0, Io::IN_OBS);
    if (motion) std::memcpy(pi + Io::IN_MOTION, motion, 3 * sizeof(double));
    if (motion_cov) std::memcpy(pi + Io::IN_COV, motion_cov, 9 * sizeof(double));
    ((int32_t *)(pi + Io::IN_FS))[1] = k;
    if (k > 0) std::memcpy(pi + Io::IN_OBS, obs, 4 * (size_t)k * sizeof(double));
    if ((rc = stage_send(g, fe.fo_in, Io::in_bytes(k))) != GS_OK) return rc;
    if ((rc = resident_map(g, fe.grid, grid_live(g), R.nd.max_distance, R.map)) != GS_OK) return rc;
    R.n_hyp = n_hyp; R.n = k; R.cap = k; R.obs = (const double *)(di + Io::IN_OBS); R.fs = (const int32_t *)(di + Io::IN_FS);
    R.motion = (const double *)(di + Io::IN_MOTION); R.motion_cov = motion_cov ? (const double *)(di + Io::IN_COV) : nullptr;
    R.state = follow_state(g, true); R.best2 = follow_best(g, true);
    R.rec = (gs_follow_step *)(dv + Io::OUT_REC); R.index = out_index ? (int32_t *)(dv + Io::OUT_IDX) : nullptr;
    follow_step_enqueue(g, R, L, 0, fe.fo_t, k, motion ? 0 : -1, nullptr, nullptr);
    const size_t brec = (size_t)n_hyp * sizeof(gs_follow_step), bidx = (size_t)n_hyp * k * sizeof(int32_t);
    if ((rc = stage_fetch(g, fe.fo_out, brec, Io::OUT_REC)) != GS_OK) return rc;
    HIP_TRY(hipMemcpyAsync(po + Io::OUT_BEST, R.best2, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, g->stream));     // (the pair lives with the state, not in the staging)
    if (out_index && bidx && (rc = stage_fetch(g, fe.fo_out, bidx, Io::OUT_IDX)) != GS_OK) return rc;
    if ((rc = frame_finish(g, "frame following")) != GS_OK) return rc;
    fe.fo_t += 1;
    if (out_steps) std::memcpy(out_steps, po + Io::OUT_REC, brec);
    if (out_index && bidx) std::memcpy(out_index, po + Io::OUT_IDX, bidx);
    if (out_best) std::memcpy(out_best, po + Io::OUT_BEST, sizeof(int32_t));
    if (out_n_tracking) std::memcpy(out_n_tracking, po + Io::OUT_N_TRACKING, sizeof(int32_t));
    return GS_OK;
}
