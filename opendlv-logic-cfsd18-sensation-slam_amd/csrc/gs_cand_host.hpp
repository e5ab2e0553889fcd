// gs_cand_host.hpp — where the cone candidates keep things (host arithmetic only, no HIP: tests/cand_layout_san.cpp compiles it alone).
//   CandLayout    the two tables (the live one, a batch or resident run's) and the per-step stage and association buffers, as byte offsets
//                 into one device allocation; every piece starts on a 256-byte boundary (the observation records need 32)
//   CandFrameIo   the frame call's pinned / device staging, fixed sizes: one frame in, one step's outputs behind it
//   CandBatch     a batch call's uploads and outputs for n_steps steps over n observations, as byte offsets into its own arena
#pragma once
#include <cstddef>
#include <cstdint>

namespace gs {

static constexpr int CAND_MAX = 1024;                                          // GS_CAND_MAX
static constexpr int CAND_FRAME_MAX = 256;                                     // GS_NN_FRAME_MAX
static constexpr size_t CAND_REC_BYTES = 80, CAND_STEP_BYTES = 48;             // sizeof(gs_cand), sizeof(gs_cand_step)

inline size_t cand_pad(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

struct CandLayout {
    size_t xy, type, cov, rec, meta, table_bytes;                              // inside a table; meta = {next_id, t, n_live, 0}
    size_t table[2];                                                           // the live table, a run's
    size_t st_obs, st_pose_of_obs, st_fs, as_idx, as_d2, as_na;                // the stage and what the association leaves
    size_t bytes;
};
inline void cand_layout(CandLayout &L) {
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += cand_pad(bytes); return at; };
    L.xy = take((size_t)CAND_MAX * 16); L.type = take((size_t)CAND_MAX * 4); L.cov = take((size_t)CAND_MAX * 32);
    L.rec = take((size_t)CAND_MAX * CAND_REC_BYTES); L.meta = take(16); L.table_bytes = off;
    L.table[0] = 0; L.table[1] = L.table_bytes; off = 2 * L.table_bytes;
    L.st_obs = take((size_t)CAND_FRAME_MAX * 32); L.st_pose_of_obs = take((size_t)CAND_FRAME_MAX * 4); L.st_fs = take(8);
    L.as_idx = take((size_t)CAND_FRAME_MAX * 4); L.as_d2 = take((size_t)CAND_FRAME_MAX * 8); L.as_na = take((size_t)CAND_FRAME_MAX * 4);
    L.bytes = off;
}

// in: the pose at 0, Sigma_p [9] at 32, the two frame bounds at 128, in_idx [256] at 160, the observations at 1184 (32-byte aligned, last:
// a frame of k sends in_bytes(k)).  out, behind IN_BYTES: the step's record, out_cand_id [256], out_cand_slot [256]
struct CandFrameIo {
    static constexpr size_t IN_POSE = 0, IN_COV = 32, IN_FS = 128, IN_IDX = 160, IN_OBS = IN_IDX + (size_t)CAND_FRAME_MAX * 4,
                            IN_BYTES = IN_OBS + (size_t)CAND_FRAME_MAX * 32;
    static constexpr size_t OUT_STEP = IN_BYTES, OUT_ID = OUT_STEP + 64, OUT_SLOT = OUT_ID + (size_t)CAND_FRAME_MAX * 4,
                            BYTES = OUT_SLOT + (size_t)CAND_FRAME_MAX * 4;
    static size_t in_bytes(int k) { return IN_OBS + (size_t)k * 32; }
};
static_assert(CandFrameIo::IN_OBS % 32 == 0, "an observation is read in one 32-byte load");

struct CandBatch {
    size_t obs, fs, pose, cov, in_idx, in_table, steps, out_id, out_slot, bytes;
};
// false (and nothing set) outside n_steps >= 0, n >= 0, 0 <= n_in <= 1024
inline bool cand_batch_layout(long long n_steps, long long n, long long n_in, CandBatch &B) {
    if (n_steps < 0 || n < 0 || n_in < 0 || n_in > CAND_MAX) return false;
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += cand_pad(bytes ? bytes : 1); return at; };
    const size_t ns = (size_t)n_steps, no = (size_t)n;
    B.obs = take(no * 32); B.fs = take((ns + 1) * 4); B.pose = take(ns * 24); B.cov = take(ns * 72); B.in_idx = take(no * 4);
    B.in_table = take((size_t)n_in * CAND_REC_BYTES); B.steps = take(ns * CAND_STEP_BYTES); B.out_id = take(no * 4); B.out_slot = take(no * 4);
    B.bytes = off;
    return true;
}

}  // namespace gs
