// gs_follow.hpp — launchers of frame following (gs_follow.hip): pose hypotheses carried from frame to frame on the device.  A step is
// launch_follow_stage -> launch_assign_opt -> launch_joint_compat -> launch_localize (gs_assoc_nn.hpp, every hypothesis a frame of its own)
// -> launch_follow_update.  Host side: gs_frontend.cpp (gs_follow_*, gs_frame_frontend_follow); the buffers' layout: gs_follow_host.hpp.
#pragma once
#include "../../include/graphslam.h"
#include "gs_assoc_nn.hpp"

namespace gs {

// one step as both kernels take it.  Everything is device memory.  The step's frame is [fs[0], fs[1]) of obs; it is a frame of this call iff
// 0 <= fs[0] <= fs[1] <= n and fs[1] - fs[0] <= cap — otherwise both kernels leave the state and every output alone (the stage's own frame
// bounds become empty, so that the chain between them touches nothing)
struct FoArgs {
    int n_hyp, t, n, cap;                   // hypotheses (1 .. 64), the step's number (state_step), the call's observations, the stage's room per hypothesis
    const int32_t *fs;                      // the step's two frame bounds
    const double *obs;                      // the call's observations (4 x n, 32-byte aligned)
    const double *motion, *motion_cov;      // the step's u [3] (null: no prediction) and Qu [9] (null: zeros)
    gs_follow_state *state;                 // [n_hyp], read and written
    // the stage: what the chain reads as n_hyp ordinary frames
    double *st_obs; int32_t *st_pose_of_obs, *st_frame_start; double *st_pose, *st_cov;
    // the chain's results (the update reads them)
    const int32_t *jc_idx, *jc_kept; const double *lo_pose, *lo_cov, *lo_chi2; const int32_t *lo_pairs, *lo_iters, *lo_status;
    int min_pairs, max_misses; double merge2, merge_theta;      // gs_follow_params, merge2 = merge_xy merge_xy formed once on the host
    gs_follow_step *rec;                    // [n_hyp] records of this step, may be null
    int32_t *out_index;                     // [n_hyp x n] (hypothesis-major), may be null
    int32_t *best2;                         // {best, n_tracking}
};
// state[h] = tracking at (poses[3 h ..], covs[9 h ..] upper triangle mirrored, or zeros), every counter 0; best2 = {0, n_hyp}
void launch_follow_init(int n_hyp, const double *poses, const double *covs, gs_follow_state *state, int32_t *best2, hipStream_t st,
                        hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// the prediction (a lane per hypothesis) and the frame laid out once per hypothesis.  k_max: the largest the step's frame can be (its size
// where the host knows it, else A.cap): it sizes the grid only
void launch_follow_stage(const FoArgs &A, int k_max, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// accept / reject, the counters, the duplicate pass, best and n_tracking (one wave), and the pruned index per hypothesis
void launch_follow_update(const FoArgs &A, const JcGate &gate, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace gs
