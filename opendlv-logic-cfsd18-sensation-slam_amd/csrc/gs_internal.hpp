// gs_internal.hpp — the opaque handle behind gs_graph (shared by the C-ABI units, see gs_private.hpp, and gs_slam.cpp).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <string>
#include <vector>

#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
struct gs_graph;
#include "gs_device.hpp"
#include "gs_dogleg.hpp"
#include "gs_edge_mask.hpp"
#include "gs_host.hpp"
#include "gs_lm.hpp"
#include "gs_polar.hpp"
#include "gs_prior.hpp"
#include "gs_schedule.hpp"

namespace gs {
// One grow-only device allocation of the handle's own, holding the blocks of an ArenaLayout (gs_side_host.hpp); reserve / upload /
// release: gs_private.hpp
struct DevArena { void *mem = nullptr; size_t cap = 0; char *at(size_t off) const { return (char *)mem + off; } };
// A live frame call's staging: pinned host memory and device memory of one size, grow-only — reserve waits for the stream before it frees the
// smaller pair, which then holds nothing (gs_frontend.cpp; the layouts: gs_frame_host.hpp)
struct FrameStage { char *pin = nullptr, *dev = nullptr; size_t bytes = 0; int reserve(gs_graph *g, size_t want); void release(); };
}

struct gs_graph {
    gs_config cfg{};
    gs_debug_options opt{};                 // every tuning switch (graphslam_debug.h): filled once at gs_create, replaced by gs_debug_set_options
    int device = 0;
    bool host_only = false;                 // cfg.device == -2: no HIP calls, no arithmetic
    gs::HostGraph h;
    gs::Plan plan;
    std::vector<uint64_t> lm_seen_interior, lm_seen_first;        // rank-local ingestion: which windows see a landmark (gs_dist_set_landmark_windows); empty: the plan build walks all edges
    int pp_records_late = 0;                                       // odometry edges whose records a shard had to send after the plan (expected: 0)
    std::shared_ptr<void> plan_ws;          // scratch of gs::build_plan, kept between the plan builds of this handle
    uint64_t plan_version = ~0ull;          // h.structure_version the plan was built for
    gs::DevGraph d;
    // device memory of this handle: chunks the plan's small arrays are carved from, and one allocation per big array.  They SURVIVE a
    // structure phase (dev_release keeps them: on some boxes hipFree + hipMalloc of a plan's memory costs more than building the plan);
    // what the next plan does not take again is returned afterwards (dev_trim).
    struct DevChunk { void *p = nullptr; size_t size = 0; bool big = false, in_use = false; };
    std::vector<DevChunk> allocs;
    char *pool_base = nullptr; size_t pool_size = 0, pool_off = 0, pool_next = 0, pool_total = 0;     // pool_total: bytes of the chunks in use
    bool dev_valid = false;                 // device mirrors the host graph + plan
    bool linearised = false;                // the H arena holds a linearisation of the CURRENT plan (enqueue_linearize ran since the last upload / growth step): gs_multiply_hessian
    bool dev_estimates_newer = false;       // estimates in HBM are ahead of the host copy
    uint64_t dev_estimate_version = 0;
    hipStream_t stream = nullptr; bool own_stream = false;
    hipEvent_t ev[8]{};
    hipEvent_t ev_lin[2]{};                 // timed iterations: start / stop attached to the linearisation dispatch (null: none)
    gs::Schedule sched;                     // the solver launches of the CURRENT plan (gs_schedule.hpp): built with the plan by upload_graph / upload_growth, read by the enqueue path
    int2 *d_wg[gs::N_TABS]{};               // device copies of sched.tab (plans with a front of more than 63 scalars; else null)
    int32_t *d_posof = nullptr;                 // device: front -> level position
    double ms_structure = 0;
    int rank = 0, world = 1;
    double *exchange = nullptr; bool exchange_external = false;   // caller-provided exchange buffer (e.g. a torch tensor)
    void *comm = nullptr; bool own_comm = false; int comm_world = 0;   // RCCL communicator of gs_dist_iterate / gs_dist_optimize (ncclComm_t; own: created by gs_dist_comm_init)
    bool force_gather = false;              // cfg.linearize_gather
    // front end (A0 / A1): nothing is allocated or freed per call
    struct FrontEnd {
        gs::DevArena arena;                                     // grow-only device scratch of the batch calls (Staging)
        // the live frame calls' staging (each null until a call needs it): a frame in and its per-observation results out — one pair for
        // gs_frame_frontend, gs_frame_frontend_nn and the assignment chain, whose calls each end in a wait —, the chain's records (ChainRec),
        // the search's record of gs_frame_frontend_relocalize (RelocRec), and gs_frame_frontend_follow's in and out (FollowFrameIo)
        gs::FrameStage fr_in, fr_out, ch_rec, rl_out, fo_in, fo_out;
        double *map_xy = nullptr; int32_t *map_type = nullptr;  // the resident association map (mirror of Slam::m_map), grow-only
        int map_n = 0, map_cap = 0;
        char *pin_map = nullptr; size_t pin_map_bytes = 0; bool pin_map_busy = false;   // pinned staging of map appends (busy: a copy out of it may be in flight)
        // a hashed grid of the resident map, built on the device (resident_map): counts, cell starts, cursors and items in mem (grow-only), and
        // what it was built for — a map of map_n cones, a cell edge from thr, `cells` buckets; valid: the map has not changed since (map_changed).
        // Two of them: the association's (cell edge from max_distance / the threshold) and relocalisation's (from inlier_radius) — two edges in
        // one grid would evict each other on every frame that runs both
        struct ResidentGrid { gs::DevArena mem; bool valid = false; int map_n = 0; double thr = 0.0; long long cells = 0; };
        ResidentGrid grid, rl_grid;
        gs::DevArena pcs;                                       // cos / sin of the poses of a batched association (scratch, grow-only)
        // covariance-gated association: the resident map's 2x2 blocks (map_cap x 4; null until a call needs them: every cone's block is
        // zero then) and the index table of gs_map_set_cov_from_marginals
        double *map_cov = nullptr;
        int64_t *cov_src = nullptr; size_t cov_src_n = 0;
        // frame localisation: gs_debug_localize's kernel choice (-1: by the mean frame size) and step output (a device pointer of the caller's, or null)
        int lo_kernel = -1; double *lo_step = nullptr;
        // relocalisation: the seed kernel's records of the resident and the frame call (empty until one of them is made, grow-only; its grid:
        // rl_grid above), gs_debug_relocalize's slice (0: the launcher's choice)
        gs::DevArena rl_rec;
        int rl_slice = 0;
        // frame following (empty / null until one of its calls is made): the per-step stage and chain buffers (gs_follow_host.hpp's FollowLayout,
        // grow-only), the hypotheses' state — 64 records that live between gs_frame_frontend_follow calls, 64 more that a batch or resident
        // run works in — with {best, n_tracking} of either, and the live run's size and step count
        gs::DevArena fo_mem;
        char *fo_state = nullptr; int32_t *fo_best = nullptr;
        int fo_n_hyp = 0, fo_t = 0;
        // cone candidates (empty until one of their calls is made): the two tables and the per-step stage in one allocation of a fixed size
        // (gs_cand_host.hpp's CandLayout; live: the live table has been initialised), a batch call's uploads and outputs (CandBatch,
        // grow-only), the frame call's staging (CandFrameIo)
        gs::DevArena cd_mem, cd_batch; bool cd_live = false;
        gs::FrameStage cd_io;
        // map twins (empty until one of their calls is made): a call's uploads, search outputs, second buffer and counters (gs_dup_host.hpp's
        // DupLayout, grow-only)
        gs::DevArena dp_mem;
    } fe;
    bool tree_proven = false;               // a whole-tree launch sequence of the CURRENT plan has completed without a flag timeout (gs_optimize then sends all iterations of a call at once)
    bool fell_back = false;                 // a whole-tree launch gave up on a flag: this handle uses one launch per level — until the next plan, or until a retry (below) comes back clean
    int fallback_calls = 0, fallback_retry_after = 4; bool fallback_retrying = false;   // gs_optimize calls on the slow path since the fallback; the call that tries the whole-tree launches again
    // append-only growth (gs::grow_plan): the full structure phase leaves room behind the plan's arrays; a growth step re-writes the
    // changed fronts' runs there and rebuilds those fronts' device tables.  used_* = entries taken so far, cap_* = allocated.
    struct GrowRoom { int64_t cap_bnd = 0, cap_map = 0, cap_asm = 0, cap_sc = 0, used_sc = 0, cap_L = 0, cap_U = 0, used_U = 0, cap_xe = 0; bool ok = false; } room;
    int32_t *d_bf = nullptr, *d_xrow = nullptr, *d_patch = nullptr, *d_list = nullptr;      // per-front counts / children-table offsets (kept for growth), patch + list staging
    std::vector<int32_t> bf_host, u3_off_host, u3_size_host, pos_of_front;                  // host mirrors the patch is computed from
    gs::Sc3Args sc3_args{};
    std::string no_growth_reason;           // why the last structure change was not absorbed by growing (empty: it was, or nothing tried)
    // gs_compute_marginals: tables built on the first call after a structure phase (plan_version), device buffers from the pool (reused while they fit)
    struct Marginals {
        uint64_t plan_version = ~0ull;      // the plan the tables below were built for
        std::vector<int64_t> sig_off;       // front -> its Sigma image in the arena (packed lower triangle of f x f)
        std::vector<int32_t> front_of;      // scalar -> the front that has it as a pivot
        std::vector<int32_t> sel_list;      // the selinv launches' fronts: per level (root first) and form (<= 63, 64 .. 159, larger), consecutive
        struct Launch { int first, count, max_f; };
        std::vector<Launch> sel_launch;     // in launch order
        int64_t sig_doubles = 0, n_out = 0; // arena size; entries of the dense output (poses 9 N | landmarks 4 M | odometry 9 E | observation 6 E)
        int64_t cap_sig = 0, cap_out = 0, cap_dout = 0, cap_fronts = 0, cap_piv = 0, cap_list = 0;
        double *sig = nullptr, *dpiv = nullptr, *d_out = nullptr; int64_t *d_sig_off = nullptr, *d_tab = nullptr; int32_t *d_list = nullptr;
        // results: valid for the graph / estimates / iteration count below
        bool valid = false; uint64_t structure_version = 0, estimate_version = 0; int32_t iter = 0;
        std::vector<double> out;
    } marg;
    // gs_optimize_lm, and gs_optimize_dogleg with gs_multiply_hessian (the allocation is made by the first call of either): the device
    // state record, history, base copy of the estimates, reduction partials and the dogleg's vertex-order vectors (gs_trial.hpp)
    gs::TrialWs<gs::LmDev, gs::LmState> lm;
    gs::TrialWs<gs::DlDev, gs::DlState> dl;
    // prior edges (gs_prior.hpp): the priors as added, the grouped tables, and their device copy — one allocation of the handle's own,
    // grow-only; uploaded whole by prior_sync when the priors or the plan changed.  dev stays empty while there is no prior on a free vertex
    struct Prior { gs::PriorStore store; gs::PriorTables tab; gs::PriorSync sync; gs::PriorDev dev{}; gs::DevArena arena;
                   uint64_t settled = 0; /* store.version prior_sync last looked at */ } prior;
    // edge deactivation (gs_edge_mask.hpp): the flags, what the device holds against them, and the staging of one k_edge_mask_apply
    // launch per kind — one allocation of the handle's own, grow-only, made at the first sync of a handle that has had an inactive edge
    struct EdgeMask { gs::EdgeMaskStore store; gs::EdgeMaskSync sync; gs::DevArena arena;
                      std::vector<int32_t> loc; std::vector<double> orig; std::vector<uint8_t> act; /* host side of the staging */ } emask;
    // polar observation edges (gs_polar.hpp): the measurements as added (under their carriers' observation indices), the tables, and
    // their device copy — one allocation of the handle's own, grow-only, made at the first sync of a handle that holds a polar edge
    struct Polar { gs::PolarStore store; gs::PolarTables tab; gs::PolarSync sync; gs::PolarDev dev{}; gs::DevArena arena; } polar;
    uint64_t value_uploads = 0;             // full uploads of the edge values (upload_graph): each puts every edge's own information on the device
};

namespace gs {
extern thread_local std::string g_last_error;
int fail(int code, const std::string &msg);
}
