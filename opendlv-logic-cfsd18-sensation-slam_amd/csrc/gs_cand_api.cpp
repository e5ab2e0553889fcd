// gs_cand_api.cpp — cone candidates behind the C-ABI (include/graphslam.h, "cone candidates"; kernels: gs_cand.hip): the batch, resident
// and live frame calls, which all end in cand_step_enqueue, and the live table's set / get / clear / take.
#include "../../include/graphslam.h"
#include "../../include/graphslam_debug.h"
#include "gs_private.hpp"
#include "gs_cand.hpp"
#include "gs_cand_host.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

using namespace gs;

static_assert(sizeof(gs_cand) == CAND_REC_BYTES && sizeof(gs_cand_step) == CAND_STEP_BYTES, "gs_cand_host.hpp restates the record sizes");
static_assert(CAND_MAX == GS_CAND_MAX && CAND_FRAME_MAX == GS_NN_FRAME_MAX, "gs_cand_host.hpp restates the sizes");

extern "C" int gs_cand_params_default(gs_cand_params *p) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p)); p->struct_size = (int32_t)sizeof(*p);
    p->confirm_hits = 3; p->max_misses = 3; p->spawn_range = 67.0; p->view_range = 12.0; p->view_cos = 0.5;
    return GS_OK;
}
namespace {
struct CdParams { int confirm_hits, max_misses; double spawn_range, view2, view_cos; };
// what a run is made of, in device memory: the frames, a pose (and covariance) per step, the explanation, the table, where the outputs go
struct CandRun {
    int n, cap; const double *obs; const int32_t *fs; const double *poses, *covs; const int32_t *in_idx;
    CdTable tab; gs_cand_step *rec; int32_t *out_id, *out_slot;
    NnDev nd; CdParams cp;
};
}
static int cand_params_check(const gs_cand_params *p, CdParams &c) {
    if (!p) return fail(GS_ERR_INVALID, "null params");
    if (p->struct_size != (int32_t)sizeof(gs_cand_params)) return fail(GS_ERR_INVALID, "gs_cand_params: wrong struct_size");
    if (p->confirm_hits < 1 || p->max_misses < 1) return fail(GS_ERR_INVALID, "gs_cand_params: confirm_hits and max_misses must be at least 1");
    if (!std::isfinite(p->spawn_range) || p->spawn_range <= 0.0 || !std::isfinite(p->view_range) || p->view_range <= 0.0)
        return fail(GS_ERR_INVALID, "gs_cand_params: spawn_range and view_range must be finite and positive");
    if (!(p->view_cos >= -1.0 && p->view_cos <= 1.0)) return fail(GS_ERR_INVALID, "gs_cand_params: view_cos outside [-1, 1]");
    c = CdParams{p->confirm_hits, p->max_misses, p->spawn_range, p->view_range * p->view_range, p->view_cos};
    return GS_OK;
}
// the two parameter blocks of a candidate call, decided before the device is touched
static int cand_checks(const gs_nn_params *params, const gs_cand_params *cand, CandRun &R) {
    const int rc = nn_params_check(params, R.nd); if (rc != GS_OK) return rc;
    return cand_params_check(cand, R.cp);
}
static int cand_records_check(int32_t n_in, const gs_cand *rec) {
    if (n_in < 0 || n_in > GS_CAND_MAX || (n_in > 0 && !rec)) return fail(GS_ERR_INVALID, "n_in outside 0 .. GS_CAND_MAX, or no records");
    for (int s = 0; s < n_in; ++s) if (rec[s].state < 0 || rec[s].state > 2) return fail(GS_ERR_INVALID, "a candidate record's state is outside 0 .. 2");
    return GS_OK;
}
static CdTable cand_table(const gs_graph *g, const CandLayout &L, bool live) {
    char *t = g->fe.cd_mem.at(L.table[live ? 0 : 1]);
    return CdTable{(double *)(t + L.xy), (int32_t *)(t + L.type), (double *)(t + L.cov), (gs_cand *)(t + L.rec), (int32_t *)(t + L.meta)};
}
// the tables and the stage (one allocation of a fixed size, made here once), the live table empty until it is set
static int cand_reserve(gs_graph *g, CandLayout &L) {
    auto &fe = g->fe;
    cand_layout(L);
    const int rc = arena_reserve(g, fe.cd_mem, L.bytes); if (rc != GS_OK) return rc;
    if (!fe.cd_live) { launch_cand_init(0, nullptr, cand_table(g, L, true), g->stream); fe.cd_live = true; }
    return GS_OK;
}
void gs_cand_release(gs_graph *g) {
    arena_release(g->fe.cd_mem); arena_release(g->fe.cd_batch); g->fe.cd_io.release(); g->fe.cd_live = false;
}
static int cand_launch_error(const char *what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? GS_OK : fail(GS_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
// one step enqueued: the stage, the association against the table as the map (not for a frame the host knows to be empty), the update.
// step: its place in the run's frame bounds, poses and records; k: the frame's size, or -1 where only the device knows it
static void cand_step_enqueue(gs_graph *g, const CandRun &R, const CandLayout &L, int step, int k, hipEvent_t start, hipEvent_t stop) {
    char *m = (char *)g->fe.cd_mem.mem;
    CdArgs A{};
    A.n = R.n; A.cap = R.cap; A.fs = R.fs + step; A.obs = R.obs; A.in_idx = R.in_idx;
    A.pose = R.poses + 3 * (size_t)step; A.pose_cov = R.covs ? R.covs + 9 * (size_t)step : nullptr;
    A.tab = R.tab;
    A.st_obs = (double *)(m + L.st_obs); A.st_pose_of_obs = (int32_t *)(m + L.st_pose_of_obs); A.st_fs = (int32_t *)(m + L.st_fs);
    int32_t *as_idx = (int32_t *)(m + L.as_idx), *as_na = (int32_t *)(m + L.as_na); double *as_d2 = (double *)(m + L.as_d2);
    A.as_idx = as_idx; A.as_na = as_na;
    A.confirm_hits = R.cp.confirm_hits; A.max_misses = R.cp.max_misses; A.spawn_range = R.cp.spawn_range; A.view2 = R.cp.view2; A.view_cos = R.cp.view_cos;
    A.lidar = g->cfg.lidar_to_cog; A.p = R.nd;
    A.rec = R.rec ? R.rec + step : nullptr; A.out_id = R.out_id; A.out_slot = R.out_slot;
    const int kk = k >= 0 ? k : R.cap;
    launch_cand_stage(A, g->stream, start, nullptr);
    if (kk > 0)
        launch_assign_opt(ObsRef{kk, A.pose, 1, A.st_pose_of_obs, A.st_obs, 1, A.st_fs, A.pose_cov}, MapRef{GS_CAND_MAX, R.tab.xy, R.tab.type, R.tab.cov, 0, nullptr, nullptr},
                          A.lidar, R.nd, as_idx, as_d2, as_na, nullptr, nullptr, Launch{g->stream});
    launch_cand_update(A, g->stream, nullptr, stop);
}

extern "C" int gs_cand_batch(gs_graph *g, int32_t n_steps, int32_t n, const double *obs, const int32_t *frame_start, const double *poses, const double *pose_covs,
                             const int32_t *in_idx, int32_t n_in, const gs_cand *in_table, const gs_nn_params *params, const gs_cand_params *cand,
                             gs_cand_step *out_steps, int32_t *out_cand_id, int32_t *out_cand_slot, gs_cand *out_table, int32_t *out_n_live) {
    if (!g || n_steps < 0 || n < 0 || (n > 0 && !obs) || (n_steps > 0 && !poses)) return fail(GS_ERR_INVALID, "bad argument");
    CandRun R{}; int rc = cand_checks(params, cand, R); if (rc != GS_OK) return rc;
    if ((rc = cand_records_check(n_in, in_table)) != GS_OK) return rc;
    if ((rc = frame_start_check(n, n_steps, frame_start)) != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    CandBatch B; if (!cand_batch_layout(n_steps, n, n_in, B)) return fail(GS_ERR_INVALID, "cone candidates: bad sizes");
    if ((rc = arena_reserve(g, fe.cd_batch, B.bytes)) != GS_OK) return rc;
    const size_t ns = (size_t)n_steps, no = (size_t)n;
    hipError_t e = hipSuccess;
    HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.obs, obs, no * 32));
    HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.fs, frame_start, (ns + 1) * 4));
    HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.pose, poses, ns * 24));
    if (pose_covs) HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.cov, pose_covs, ns * 72));
    if (in_idx) HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.in_idx, in_idx, no * 4));
    HIP_NEXT(e, arena_upload(g, fe.cd_batch, B.in_table, in_table, (size_t)n_in * sizeof(gs_cand)));
    if (e != hipSuccess) { (void)hipStreamSynchronize(g->stream); return fail(GS_ERR_HIP, std::string("cone candidates: upload: ") + hipGetErrorString(e)); }
    const DevArena &a = fe.cd_batch;
    R.n = n; R.cap = 0; for (int t = 0; t < n_steps; ++t) R.cap = std::max(R.cap, frame_start[t + 1] - frame_start[t]);
    R.obs = (const double *)a.at(B.obs); R.fs = (const int32_t *)a.at(B.fs); R.poses = (const double *)a.at(B.pose);
    R.covs = pose_covs ? (const double *)a.at(B.cov) : nullptr; R.in_idx = in_idx ? (const int32_t *)a.at(B.in_idx) : nullptr;
    R.tab = cand_table(g, L, false); R.rec = (gs_cand_step *)a.at(B.steps);
    R.out_id = out_cand_id ? (int32_t *)a.at(B.out_id) : nullptr; R.out_slot = out_cand_slot ? (int32_t *)a.at(B.out_slot) : nullptr;
    launch_cand_init(n_in, (const gs_cand *)a.at(B.in_table), R.tab, g->stream);
    for (int t = 0; t < n_steps; ++t)                               // back to back: no host decision between the frames
        cand_step_enqueue(g, R, L, t, frame_start[t + 1] - frame_start[t], nullptr, nullptr);
    auto fetch = [&](void *dst, const void *src, size_t bytes) { if (dst && bytes) HIP_NEXT(e, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, g->stream)); };
    int32_t meta[4] = {0, 0, 0, 0};
    fetch(out_steps, R.rec, ns * sizeof(gs_cand_step)); fetch(out_cand_id, R.out_id, no * 4); fetch(out_cand_slot, R.out_slot, no * 4);
    fetch(out_table, R.tab.rec, (size_t)GS_CAND_MAX * sizeof(gs_cand)); fetch(meta, R.tab.meta, sizeof(meta));
    e = sync_keep_first(e, g->stream);                              // the one wait of the call
    fe.pin_map_busy = false;
    if (e != hipSuccess) return fail(GS_ERR_HIP, std::string("cone candidates: ") + hipGetErrorString(e));
    if (out_n_live) *out_n_live = meta[2];
    return cand_launch_error("cone candidates");
}
extern "C" int gs_cand_resident(gs_graph *g, int32_t n_steps, int32_t n, const double *dev_obs, const int32_t *dev_frame_start, int32_t frame_cap,
                                const double *dev_poses, const double *dev_pose_covs, const int32_t *dev_in_idx, int32_t n_in, const gs_cand *dev_in_table,
                                const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *dev_out_steps, int32_t *dev_out_cand_id,
                                int32_t *dev_out_cand_slot, gs_cand *dev_out_table, int32_t *dev_out_meta_4) {
    if (!g || n_steps < 0 || n < 0 || !dev_frame_start || (n > 0 && !dev_obs) || (n_steps > 0 && !dev_poses)) return fail(GS_ERR_INVALID, "bad argument");
    CandRun R{}; int rc = cand_checks(params, cand, R); if (rc != GS_OK) return rc;
    if (n_in < 0 || n_in > GS_CAND_MAX || (n_in > 0 && !dev_in_table)) return fail(GS_ERR_INVALID, "n_in outside 0 .. GS_CAND_MAX, or no records");
    if (frame_cap < 0 || frame_cap > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "frame_cap outside 0 .. GS_NN_FRAME_MAX");
    if (((uintptr_t)dev_obs & 31) != 0) return fail(GS_ERR_INVALID, "dev_obs must be 32-byte aligned (an observation is read in one load)");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    R.n = n; R.cap = frame_cap; R.obs = dev_obs; R.fs = dev_frame_start; R.poses = dev_poses; R.covs = dev_pose_covs; R.in_idx = dev_in_idx;
    R.tab = cand_table(g, L, false); R.rec = dev_out_steps; R.out_id = dev_out_cand_id; R.out_slot = dev_out_cand_slot;
    launch_cand_init(n_in, dev_in_table, R.tab, g->stream, g->ev_lin[0], n_steps == 0 ? g->ev_lin[1] : nullptr);
    for (int t = 0; t < n_steps; ++t) cand_step_enqueue(g, R, L, t, -1, nullptr, t == n_steps - 1 ? g->ev_lin[1] : nullptr);
    if (dev_out_table) HIP_TRY(hipMemcpyAsync(dev_out_table, R.tab.rec, (size_t)GS_CAND_MAX * sizeof(gs_cand), hipMemcpyDeviceToDevice, g->stream));
    if (dev_out_meta_4) HIP_TRY(hipMemcpyAsync(dev_out_meta_4, R.tab.meta, 4 * sizeof(int32_t), hipMemcpyDeviceToDevice, g->stream));
    return cand_launch_error("cone candidates");
}

// ---- the live table: it stays on the handle between frames
extern "C" int gs_cand_set(gs_graph *g, int32_t n_in, const gs_cand *records) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = cand_records_check(n_in, records); if (rc != GS_OK) return rc;
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    CandBatch B; if (!cand_batch_layout(0, 0, n_in, B)) return fail(GS_ERR_INVALID, "cone candidates: bad sizes");
    if ((rc = arena_reserve(g, fe.cd_batch, B.bytes)) != GS_OK) return rc;
    HIP_TRY(arena_upload(g, fe.cd_batch, B.in_table, records, (size_t)n_in * sizeof(gs_cand)));
    launch_cand_init(n_in, (const gs_cand *)fe.cd_batch.at(B.in_table), cand_table(g, L, true), g->stream);
    HIP_TRY(hipStreamSynchronize(g->stream));                       // pageable source
    fe.pin_map_busy = false;
    return cand_launch_error("gs_cand_set");
}
extern "C" int gs_cand_clear(gs_graph *g) { return gs_cand_set(g, 0, nullptr); }
extern "C" int gs_cand_get(gs_graph *g, gs_cand *out_table, int32_t *out_next_id, int32_t *out_step, int32_t *out_n_live) {
    if (!g) return fail(GS_ERR_INVALID, "null graph");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    const CdTable T = cand_table(g, L, true);
    int32_t meta[4] = {0, 0, 0, 0};
    if (out_table) HIP_TRY(hipMemcpyAsync(out_table, T.rec, (size_t)GS_CAND_MAX * sizeof(gs_cand), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(meta, T.meta, sizeof(meta), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->fe.pin_map_busy = false;
    if (out_next_id) *out_next_id = meta[0];
    if (out_step) *out_step = meta[1];
    if (out_n_live) *out_n_live = meta[2];
    return GS_OK;
}
// host side: read the records, free the confirmed slots in every form the table keeps them, write those slots back.  next_id and t stay
extern "C" int gs_cand_take_confirmed(gs_graph *g, int32_t cap, gs_cand *out_records, int32_t *out_n) {
    if (!g || cap < 0 || (cap > 0 && !out_records) || !out_n) return fail(GS_ERR_INVALID, "bad argument");
    int rc = ensure_device(g); if (rc != GS_OK) return rc;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    const CdTable T = cand_table(g, L, true);
    std::vector<gs_cand> rec((size_t)GS_CAND_MAX); int32_t meta[4] = {0, 0, 0, 0};
    HIP_TRY(hipMemcpyAsync(rec.data(), T.rec, rec.size() * sizeof(gs_cand), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipMemcpyAsync(meta, T.meta, sizeof(meta), hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));
    g->fe.pin_map_busy = false;
    std::vector<int> slots;
    for (int s = 0; s < GS_CAND_MAX; ++s) if (rec[s].state == 2) slots.push_back(s);
    if ((int)slots.size() > cap) return fail(GS_ERR_INVALID, "gs_cand_take_confirmed: more confirmed candidates than cap");
    std::sort(slots.begin(), slots.end(), [&](int a, int b) { return rec[a].id < rec[b].id; });
    *out_n = (int32_t)slots.size();
    if (slots.empty()) return GS_OK;
    gs_cand freed; std::memset(&freed, 0, sizeof(freed));
    freed.xy[0] = freed.xy[1] = std::nan(""); freed.id = -1; freed.confirm_step = -1;
    const double zero4[4] = {0.0, 0.0, 0.0, 0.0}; const int32_t zero = 0;
    for (size_t r = 0; r < slots.size(); ++r) { const int s = slots[r];
        out_records[r] = rec[s];
        HIP_TRY(hipMemcpyAsync(T.rec + s, &freed, sizeof(freed), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipMemcpyAsync(T.xy + 2 * (size_t)s, freed.xy, 2 * sizeof(double), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipMemcpyAsync(T.cov + 4 * (size_t)s, zero4, sizeof(zero4), hipMemcpyHostToDevice, g->stream));
        HIP_TRY(hipMemcpyAsync(T.type + s, &zero, sizeof(zero), hipMemcpyHostToDevice, g->stream)); }
    meta[2] -= (int32_t)slots.size();
    HIP_TRY(hipMemcpyAsync(T.meta, meta, sizeof(meta), hipMemcpyHostToDevice, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // pageable sources
    return GS_OK;
}
extern "C" int gs_frame_frontend_candidates(gs_graph *g, const double *pose, const double *pose_cov, const double *obs, int32_t k, const int32_t *in_idx,
                                            const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *out_step, int32_t *out_cand_id,
                                            int32_t *out_cand_slot) {
    if (!g || !pose || k < 0 || (k > 0 && !obs)) return fail(GS_ERR_INVALID, "bad argument");
    CandRun R{}; int rc = cand_checks(params, cand, R); if (rc != GS_OK) return rc;
    if (k > GS_NN_FRAME_MAX) return fail(GS_ERR_INVALID, "a frame holds more than GS_NN_FRAME_MAX observations");
    rc = ensure_device(g); if (rc != GS_OK) return rc;
    auto &fe = g->fe;
    CandLayout L; if ((rc = cand_reserve(g, L)) != GS_OK) return rc;
    using Io = CandFrameIo;
    if ((rc = fe.cd_io.reserve(g, Io::BYTES)) != GS_OK) return rc;                // once per handle: a fixed size
    char *pi = fe.cd_io.pin, *dv = fe.cd_io.dev;
    std::memset(pi, 0, Io::IN_IDX);
    std::memcpy(pi + Io::IN_POSE, pose, 3 * sizeof(double));
    if (pose_cov) std::memcpy(pi + Io::IN_COV, pose_cov, 9 * sizeof(double));
    ((int32_t *)(pi + Io::IN_FS))[1] = k;
    if (in_idx && k > 0) std::memcpy(pi + Io::IN_IDX, in_idx, (size_t)k * sizeof(int32_t));
    if (k > 0) std::memcpy(pi + Io::IN_OBS, obs, 4 * (size_t)k * sizeof(double));
    HIP_TRY(hipMemcpyAsync(dv, pi, Io::in_bytes(k), hipMemcpyHostToDevice, g->stream));
    R.n = k; R.cap = k; R.obs = (const double *)(dv + Io::IN_OBS); R.fs = (const int32_t *)(dv + Io::IN_FS);
    R.poses = (const double *)(dv + Io::IN_POSE); R.covs = pose_cov ? (const double *)(dv + Io::IN_COV) : nullptr;
    R.in_idx = in_idx ? (const int32_t *)(dv + Io::IN_IDX) : nullptr;
    R.tab = cand_table(g, L, true); R.rec = (gs_cand_step *)(dv + Io::OUT_STEP);
    R.out_id = (int32_t *)(dv + Io::OUT_ID); R.out_slot = (int32_t *)(dv + Io::OUT_SLOT);
    cand_step_enqueue(g, R, L, 0, k, nullptr, nullptr);
    HIP_TRY(hipMemcpyAsync(pi + Io::OUT_STEP, dv + Io::OUT_STEP, Io::OUT_ID - Io::OUT_STEP + 2 * (size_t)CAND_FRAME_MAX * 4, hipMemcpyDeviceToHost, g->stream));
    HIP_TRY(hipStreamSynchronize(g->stream));                       // the one wait of the call
    fe.pin_map_busy = false;
    if ((rc = cand_launch_error("cone candidates")) != GS_OK) return rc;
    if (out_step) std::memcpy(out_step, pi + Io::OUT_STEP, sizeof(gs_cand_step));
    if (out_cand_id && k > 0) std::memcpy(out_cand_id, pi + Io::OUT_ID, (size_t)k * sizeof(int32_t));
    if (out_cand_slot && k > 0) std::memcpy(out_cand_slot, pi + Io::OUT_SLOT, (size_t)k * sizeof(int32_t));
    return GS_OK;
}
