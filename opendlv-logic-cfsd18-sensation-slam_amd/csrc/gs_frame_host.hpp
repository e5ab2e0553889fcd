// gs_frame_host.hpp — where the live frame calls (gs_frame_frontend_*) keep things in their pinned / device staging (host arithmetic only, no
// HIP: tests/frame_layout_san.cpp compiles it alone).
//   JcRec, LoRec, ChainRec   the joint test's and the localisation's record of one frame, and the two as the chain's record buffer holds them
//   RelocRec                 the search's record of gs_frame_frontend_relocalize
//   FrameLayout              a frame of k observations in the input buffer, its per-observation results in the output buffer, as byte
//                            offsets: the three input formats the kernels define
// A device pointer is a member's address in one of these; the host reads the same member of the pinned copy.
#pragma once
#include <cstddef>
#include <cstdint>

namespace gs {

static constexpr int FRAME_MAX = 256;                                          // GS_NN_FRAME_MAX

struct JcRec { double j, delta[3]; int32_t kept, dropped, untestable, pad_; int32_t index[FRAME_MAX]; };
struct LoRec { double pose[3], cov[9], chi2; int32_t pairs, iterations, status, pad_; };
struct ChainRec { JcRec jc; LoRec lo; };
struct RelocRec { double pose[3], second_pose[3], cost; long long n_seeds; int32_t seed[4], count, second_count, status, pad_;
                  int32_t index[FRAME_MAX]; double e2[FRAME_MAX]; };
static_assert(offsetof(JcRec, j) == 0 && offsetof(JcRec, delta) == 8 && offsetof(JcRec, kept) == 32 && offsetof(JcRec, dropped) == 36 &&
              offsetof(JcRec, untestable) == 40 && offsetof(JcRec, index) == 48 && sizeof(JcRec) == 48 + 4 * FRAME_MAX, "the joint test's record");
static_assert(offsetof(LoRec, pose) == 0 && offsetof(LoRec, cov) == 24 && offsetof(LoRec, chi2) == 96 && offsetof(LoRec, pairs) == 104 &&
              offsetof(LoRec, iterations) == 108 && offsetof(LoRec, status) == 112 && sizeof(LoRec) == 120, "the localisation's record");
static_assert(offsetof(ChainRec, jc) == 0 && offsetof(ChainRec, lo) == 1072 && sizeof(ChainRec) == 1192, "the chain's records");
static_assert(offsetof(RelocRec, pose) == 0 && offsetof(RelocRec, second_pose) == 24 && offsetof(RelocRec, cost) == 48 && offsetof(RelocRec, n_seeds) == 56 &&
              offsetof(RelocRec, seed) == 64 && offsetof(RelocRec, count) == 80 && offsetof(RelocRec, second_count) == 84 && offsetof(RelocRec, status) == 88 &&
              offsetof(RelocRec, index) == 96 && offsetof(RelocRec, e2) == 1120 && sizeof(RelocRec) == 1120 + 8 * FRAME_MAX, "the search's record");

// in: the pose at 0, then what the format has of cov[9], obs[k][4], frame_start[2], pose_of_obs[k].  out: z[k][2] at 0, g[k][2], then what the
// format has of d2[k], second[k], idx[k], na[k].  NONE: the format has no such piece
struct FrameLayout {
    static constexpr size_t NONE = ~(size_t)0;
    size_t pose = 0, cov = NONE, obs = NONE, frame_start = NONE, pose_of_obs = NONE, in_bytes = 0;
    size_t z = 0, g = NONE, d2 = NONE, second = NONE, idx = NONE, na = NONE, out_bytes = 0;
};
// gs_frame_frontend (k_frame_frontend): the pose, then the observations at 24; z, g, idx
inline FrameLayout frame_layout_plain(size_t k) {
    FrameLayout L; L.obs = 24; L.in_bytes = L.obs + 32 * k;
    L.g = 16 * k; L.idx = 32 * k; L.out_bytes = L.idx + 4 * k;
    return L;
}
// gs_frame_frontend_nn (k_frame_nn): the pose's covariance at 24, the observations at 96 (32-byte aligned); z, g, d2, second, idx
inline FrameLayout frame_layout_nn(size_t k) {
    FrameLayout L; L.cov = 24; L.obs = 96; L.in_bytes = L.obs + 32 * k;
    L.g = 16 * k; L.d2 = 32 * k; L.second = 40 * k; L.idx = 48 * k; L.out_bytes = L.idx + 4 * k;
    return L;
}
// the assignment chain (gs_frame_frontend_assign .. _relocalize): the batch kernels' arrays for one pose and one frame — the covariance at 32,
// the observations at 128 (32-byte aligned), then frame_start {0, k} and pose_of_obs (zeros); z, g, d2, idx, and behind them (so that the
// greedy assignment, which has none, copies [0, na) back) the admissible counts
inline FrameLayout frame_layout_chain(size_t k) {
    FrameLayout L; L.cov = 32; L.obs = 128; L.frame_start = L.obs + 32 * k; L.pose_of_obs = L.frame_start + 8; L.in_bytes = L.pose_of_obs + 4 * k;
    L.g = 16 * k; L.d2 = 32 * k; L.idx = 40 * k; L.na = 44 * k; L.out_bytes = L.na + 4 * k;
    return L;
}

}  // namespace gs
