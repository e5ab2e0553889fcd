// gs_follow_host.hpp — where frame following keeps things (host arithmetic only, no HIP: tests/follow_layout_san.cpp compiles it alone).
//   FollowLayout   the per-step stage and chain buffers of a run of n_hyp hypotheses with room for `cap` observations each, as byte
//                  offsets into one device allocation; every piece starts on a 256-byte boundary (the observation records need 32)
//   FollowFrameIo  the frame call's pinned / device staging, fixed sizes: one frame in, one step's records out
#pragma once
#include <cstddef>
#include <cstdint>

namespace gs {

static constexpr int FOLLOW_HYP_MAX = 64;                                      // GS_FOLLOW_HYP_MAX
static constexpr int FOLLOW_FRAME_MAX = 256;                                   // GS_NN_FRAME_MAX
static constexpr size_t FOLLOW_STEP_BYTES = 224, FOLLOW_STATE_BYTES = 136;     // sizeof(gs_follow_step), sizeof(gs_follow_state)

struct FollowLayout {
    size_t obs, pose_of_obs, frame_start, pose, cov;                           // the stage
    size_t as_idx, as_d2, jc_idx, jc_kept, lo_pose, lo_cov, lo_chi2, lo_pairs, lo_iters, lo_status;   // the chain's outputs
    size_t bytes;
};
// false (and nothing set) outside 1 <= n_hyp <= 64, 0 <= cap <= 256
inline bool follow_layout(int n_hyp, int cap, FollowLayout &L) {
    if (n_hyp < 1 || n_hyp > FOLLOW_HYP_MAX || cap < 0 || cap > FOLLOW_FRAME_MAX) return false;
    const size_t nh = (size_t)n_hyp, no = nh * (size_t)(cap > 0 ? cap : 1);
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t at = off; off += (bytes + 255) & ~(size_t)255; return at; };
    L.obs = take(no * 32); L.pose_of_obs = take(no * 4); L.frame_start = take((nh + 1) * 4); L.pose = take(nh * 24); L.cov = take(nh * 72);
    L.as_idx = take(no * 4); L.as_d2 = take(no * 8); L.jc_idx = take(no * 4); L.jc_kept = take(nh * 4);
    L.lo_pose = take(nh * 24); L.lo_cov = take(nh * 72); L.lo_chi2 = take(nh * 8); L.lo_pairs = take(nh * 4); L.lo_iters = take(nh * 4); L.lo_status = take(nh * 4);
    L.bytes = off;
    return true;
}

// in: motion u[3] at 0, Qu[9] at 32, the two frame bounds at 128, the observations at 160 (32-byte aligned).
// out: the step's n_hyp records at 0, {best, n_tracking} behind them, then the pruned index [n_hyp x k]
struct FollowFrameIo {
    static constexpr size_t IN_MOTION = 0, IN_COV = 32, IN_FS = 128, IN_OBS = 160, IN_BYTES = IN_OBS + (size_t)FOLLOW_FRAME_MAX * 32;
    static constexpr size_t OUT_REC = 0, OUT_BEST = (size_t)FOLLOW_HYP_MAX * FOLLOW_STEP_BYTES, OUT_N_TRACKING = OUT_BEST + 4, OUT_IDX = OUT_BEST + 32,
                            OUT_BYTES = OUT_IDX + (size_t)FOLLOW_HYP_MAX * FOLLOW_FRAME_MAX * 4;
    static size_t in_bytes(int k) { return IN_OBS + (size_t)k * 32; }
};

}  // namespace gs
