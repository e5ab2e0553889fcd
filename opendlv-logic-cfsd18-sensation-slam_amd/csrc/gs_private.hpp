// gs_private.hpp — what the translation units behind the C-ABI (gs_api.cpp, gs_upload.cpp, gs_solve.cpp, gs_frontend.cpp, gs_dist.cpp,
// gs_marginals.cpp) share beyond the handle itself.
#pragma once
#include "gs_internal.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <string>
#include <thread>
#include <vector>

#define HIP_TRY(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) \
    return gs::fail(GS_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); } while (0)

// Device memory of a plan comes out of a few large chunks (8 MB, then doubling): the ~70 arrays of one structure phase
// cost a dozen hipMalloc calls instead of 70 (each is 50-100 us of the structure phase), and dev_free_all returns them together.
// Arrays of 32 MB and more get an allocation of their own.
// gs_debug_options.pool_poison (tests): every chunk is filled with 0xFF bytes (NaN doubles, negative indices) when it is allocated and whenever a plan
// releases it — an array that is read before this code writes it cannot pass for zero-initialised
static inline bool pool_poison(const gs_graph *g) { return g->opt.pool_poison > 0; }
template <class T> int dev_alloc(gs_graph *g, T **ptr, size_t count) {
    *ptr = nullptr;
    const size_t bytes = (std::max<size_t>(count, 1) * sizeof(T) + 255) & ~(size_t)255;
    if (bytes >= ((size_t)32 << 20)) {                                // a big array: its own allocation, exactly its size (a chunk rounded up to a
        int best = -1;                                                // power of two for it, or the abandoned rest of the current chunk, were 270 MB of
        for (size_t i = 0; i < g->allocs.size(); ++i) { const auto &c = g->allocs[i];      // an 800 MB footprint at 100k poses); one kept from the last plan
            if (c.big && !c.in_use && c.size >= bytes && c.size <= bytes + bytes / 4 && (best < 0 || c.size < g->allocs[best].size)) best = (int)i; }   // serves if it fits within 25 %
        if (best < 0) { void *p = nullptr;
            HIP_TRY(hipMalloc(&p, bytes));
            if (pool_poison(g)) HIP_TRY(hipMemsetAsync(p, 0xFF, bytes, g->stream));
            gs_graph::DevChunk c; c.p = p; c.size = bytes; c.big = true; g->allocs.push_back(c); best = (int)g->allocs.size() - 1; }
        g->allocs[best].in_use = true; g->pool_total += g->allocs[best].size; *ptr = (T *)g->allocs[best].p;
        return GS_OK; }
    if (g->pool_off + bytes > g->pool_size) {
        size_t want = std::max<size_t>(g->pool_next, (size_t)8 << 20);
        while (want < bytes) want <<= 1;
        int pick = -1;
        for (size_t i = 0; i < g->allocs.size() && pick < 0; ++i) { const auto &c = g->allocs[i]; if (!c.big && !c.in_use && c.size >= want) pick = (int)i; }   // a chunk of the last plan
        if (pick < 0) { void *p = nullptr;
            HIP_TRY(hipMalloc(&p, want));
            if (pool_poison(g)) HIP_TRY(hipMemsetAsync(p, 0xFF, want, g->stream));
            gs_graph::DevChunk c; c.p = p; c.size = want; g->allocs.push_back(c); pick = (int)g->allocs.size() - 1; }
        auto &c = g->allocs[pick]; c.in_use = true; g->pool_total += c.size;
        g->pool_base = (char *)c.p; g->pool_size = c.size; g->pool_off = 0;
        g->pool_next = std::min<size_t>(std::max(want, c.size) << 1, (size_t)128 << 20);      // chunks of at most 128 MB: little slack in the footprint
    }
    *ptr = (T *)(g->pool_base + g->pool_off);
    g->pool_off += bytes;
    return GS_OK;
}

// Query calls (per-edge / per-prior values): "first error wins" over a chain of HIP calls — a call behind a failed one is not made —
// and one device scratch per call, laid out by an ArenaLayout and freed on every exit
#define HIP_NEXT(e, expr) do { if ((e) == hipSuccess) (e) = (expr); } while (0)
static inline hipError_t sync_keep_first(hipError_t e, hipStream_t st) { const hipError_t s = hipStreamSynchronize(st); return e != hipSuccess ? e : s; }   // (waits either way: the scratch is freed behind it)
struct DevScratch {
    char *p = nullptr;
    DevScratch() = default;
    DevScratch(const DevScratch &) = delete;
    DevScratch &operator=(const DevScratch &) = delete;
    ~DevScratch() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { const hipError_t e = hipMalloc((void **)&p, bytes); if (e != hipSuccess) p = nullptr; return e; }
};

// gs_api.cpp
// the handle's grow-only arenas (gs::DevArena): room for `total` bytes — a larger allocation (total + total / 2 + 4096) behind a wait for
// the stream when the present one is too small, which then holds nothing; on failure the arena is empty —, a block to offset `off` on
// the handle's stream, and the release
int arena_reserve(gs_graph *g, gs::DevArena &a, size_t total);
hipError_t arena_upload(gs_graph *g, const gs::DevArena &a, size_t off, const void *src, size_t bytes);
void arena_release(gs::DevArena &a);
// the three side passes (priors, edge flags, polar edges) together: their device copies brought up to date, in this order, with the plan
// of the CURRENT graph on the device (ensure_ready, gs_iterate); the handle's stores emptied (gs_clear); the arenas freed (gs_destroy)
int side_sync(gs_graph *g);
void side_clear(gs_graph *g);
void side_release(gs_graph *g);
// where observation edge k lives on the device: its ELL index, or -(tail slot) - 1 (the table format of launch_edge_chi2); the refusals
// start with `prefix`
int pl_location(const gs_graph *g, int32_t k, int32_t &src, const char *prefix);
// fused linearisation: the block of a free landmark of the layout lives in its first partial-sum slot — true when landmark l has none
// (no observation edge in the linearisation layout), i.e. there is no address a side pass could add its block to
bool lm_lacks_fused_slot(const gs_graph *g, int32_t l);
bool sym_ok(const double *m, int n);           // the information-matrix check of every gs_add_*_edge / gs_add_*_prior
int ensure_device(gs_graph *g);
int ensure_ready(gs_graph *g);                 // the structure phase if the graph changed, host-side estimates to the device
int pull_estimates_if_needed(gs_graph *g);
int pull_estimates_enqueue(gs_graph *g, bool &pull);        // the copies only: they come back with the caller's next wait, which then clears dev_estimates_newer if `pull`
int reset_failure(gs_graph *g);
void fill_plan_stats(gs_graph *g, gs_stats *s);
int plan_factor_variant(const gs_graph *g, int64_t arena_doubles);   // the factor kernel of the current plan as DevGraph::factor_variant names it: 3, or 0 for the C-ABI's variant 4
// (gs::StepTimer, the plan_timing lines of the structure driver, the upload and the plan build: gs_parallel.hpp)
// gs_upload.cpp
// What does not depend on the plan travels on a helper thread while the host builds the plan (upload_raw_begin starts it; the caller joins
// it before upload_graph); a pose-window shard's edge streams travel on a second one beside upload_graph, which joins it
struct RawUpload {
    std::thread th; int rc = GS_OK; std::string err;
    ~RawUpload() { if (th.joinable()) th.join(); }                  // an exception (bad_alloc in the plan build) must not meet a joinable thread: std::terminate
    int32_t *pl_l = nullptr; double *pl_z = nullptr, *pl_info = nullptr;
    std::vector<double> zinv; size_t pp_lo = 0, pp_hi = 0;         // the odometry edges whose records went up: [pp_lo, pp_hi) (all of them on a single GPU)
    gs::uvec<int32_t> ell_l; gs::uvec<double> ell_z, ell_w;       // pose-window shards: the ELL streams, filled on the host (they must outlive the copies: upload_graph ends with a sync)
};
int upload_raw_begin(gs_graph *g, RawUpload &R);
int upload_tables(gs_graph *g);                // the schedule's workgroup tables (g->sched) to the device
int upload_graph(gs_graph *g, RawUpload &raw); // the plan of the current graph to the device, schedule included
int upload_growth(gs_graph *g, const gs::Growth &gr);          // what gs::grow_plan changed; GS_ERR_CAPACITY: the room behind the plan's arrays is used up (the caller rebuilds)
int push_estimates(gs_graph *g);               // host-side setEstimate since the upload: estimates and the poses' cos / sin to the device
// gs_prior_api.cpp
int prior_sync(gs_graph *g);                   // the prior tables to the device when the priors or the plan changed (side_sync); nothing without priors
// gs_edge_mask_api.cpp
int edge_mask_sync(gs_graph *g);               // the information of the edges whose flag changed (or that an upload rewrote) on the device (side_sync); nothing on a handle that never had an inactive edge
int edge_mask_edge_chi2(gs_graph *g, int32_t kind, int32_t n, const std::vector<int32_t> &tab, double *out_chi2, double *out_weight);   // gs_get_edge_chi2 on a handle with inactive edges: s with the edges' own information
// gs_polar_api.cpp
int polar_sync(gs_graph *g);                   // the polar edges' tables to the device when they, the plan, the edge flags or the edge values changed (side_sync); nothing without polar edges
int polar_edge_chi2_overwrite(gs_graph *g, int32_t n, double *dev_out);   // gs_get_edge_chi2 (observation kind): s and weight of the polar edges over the per-edge kernel's device output [2][n]; nothing without polar edges
// gs_solve.cpp
// every linearisation of H and every chi2 pass goes through these two, so that no site can leave the priors out
void enqueue_linearize(gs_graph *g, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);   // linearise + a grown plan's tail + the priors (start / stop: on the linearisation dispatch)
void enqueue_chi2(gs_graph *g);                // chi2 at the current estimates -> chi2[0], priors included
void enqueue_factor_levels(gs_graph *g, const gs::LevelSet &ls, int base, int mode);
void enqueue_local(gs_graph *g, bool timed);
void enqueue_finish(gs_graph *g, bool timed);
void fall_back_to_levels(gs_graph *g);
// the run scaffold gs_optimize* / gs_optimize_lm share; gs_dist_optimize uses these pieces of it
int run_begin(gs_graph *g, int32_t iterations, bool retry);
int run_check(gs_graph *g, const char *what, float *ms);
void run_stats(gs_graph *g, gs_stats *stats, int32_t iterations, int32_t failure, int first_failure, double chi2_initial, double chi2_final, float ms);
int marg_ready(gs_graph *g);                  // gs_marginals.cpp: GS_OK when the last gs_compute_marginals still describes the graph and its estimates (the getters' test)
void gs_frontend_release(gs_graph *g);       // gs_frontend.cpp: front-end buffers of the handle
void map_changed(gs_graph *g);               // gs_frontend.cpp: what every call that moves, adds or removes cones of the resident map ends in (its grids are stale)
namespace gs { struct NnDev; }
int nn_params_check(const gs_nn_params *p, gs::NnDev &d);                      // gs_frontend.cpp: what every call refuses of gs_nn_params, before the device is touched
int frame_start_check(int32_t n, int32_t n_frames, const int32_t *fs);         // gs_frontend.cpp: a batch call's frame bounds
void gs_cand_release(gs_graph *g);           // gs_cand_api.cpp: the cone candidates' buffers (gs_frontend_release)
void gs_dup_release(gs_graph *g);            // gs_dup_api.cpp: the map twins' buffers (gs_frontend_release)
void gs_dist_comm_release(gs_graph *g);      // gs_dist.cpp: the handle's own RCCL communicator
