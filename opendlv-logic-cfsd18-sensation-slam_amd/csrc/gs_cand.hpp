// gs_cand.hpp — launchers of the cone candidates (gs_cand.hip): unmatched observations tracked into new map cones on the device.  A step is
// launch_cand_stage -> launch_assign_opt (gs_assoc_nn.hpp, the table as the map) -> launch_cand_update.  Host side: gs_cand_api.cpp
// (gs_cand_*, gs_frame_frontend_candidates); the buffers' layout: gs_cand_host.hpp.
#pragma once
#include "../../include/graphslam.h"
#include "gs_assoc_nn.hpp"

namespace gs {

// a table in device memory, stored as a map is stored plus a record per slot; meta = {next_id, t, n_live, 0}
struct CdTable { double *xy; int32_t *type; double *cov; gs_cand *rec; int32_t *meta; };

// one step as both kernels take it.  Everything is device memory.  The step's frame is [fs[0], fs[1]) of obs; it is a frame of this call iff
// 0 <= fs[0] <= fs[1] <= n and fs[1] - fs[0] <= cap — otherwise both kernels leave the table and every output alone (the stage's own frame
// bounds become empty, so that the association between them touches nothing)
struct CdArgs {
    int n, cap;                             // the call's observations, the stage's room
    const int32_t *fs;                      // the step's two frame bounds
    const double *obs;                      // the call's observations (4 x n, 32-byte aligned)
    const int32_t *in_idx;                  // [n] the map cone that explains an observation, -1: none; null: nothing is explained
    const double *pose, *pose_cov;          // the step's pose [3] and Sigma_p [9] (null: none)
    CdTable tab;
    double *st_obs; int32_t *st_pose_of_obs, *st_fs;            // the stage: what the association reads as one frame of one pose
    const int32_t *as_idx, *as_na;          // the association's slot and n_admissible per staged observation
    int confirm_hits, max_misses; double spawn_range, view2, view_cos;      // gs_cand_params, view2 = view_range view_range formed once on the host
    double lidar; NnDev p;
    gs_cand_step *rec;                      // the step's record, may be null
    int32_t *out_id, *out_slot;             // [n] each, may be null
};
// tab = the n_in records of `in` (null with n_in == 0) in slots 0 .. n_in - 1, the rest free; next_id, t, n_live from them
void launch_cand_init(int n_in, const gs_cand *in, const CdTable &tab, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// the frame with the explained observations' azimuth replaced by NaN, pose index 0 each, bounds {0, k}
void launch_cand_stage(const CdArgs &A, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// fusion (a lane per observation), visibility / retirement / confirmation (four slots a thread), spawning by ballots and prefix counts, the counters
void launch_cand_update(const CdArgs &A, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace gs
