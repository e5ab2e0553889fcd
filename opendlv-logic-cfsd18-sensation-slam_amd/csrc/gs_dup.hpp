// gs_dup.hpp — launchers of the map twins (gs_dup.hip): duplicate cones found among all pairs of a map, fused and compacted on the device.
// A query is launch_dup_nearest; a consolidation is launch_dup_nearest -> launch_dup_fuse -> launch_dup_scan -> launch_dup_scatter.
// Host side: gs_dup_api.cpp (gs_map_twins_*, gs_map_merge_twins*); the buffers' layout and the graph merge: gs_dup_host.hpp.
#pragma once
#include "../../include/graphslam.h"
#include <hip/hip_runtime.h>

namespace gs {

// gs_dup_params as the kernels take it: s2 = sigma_floor sigma_floor and md2_hi, a bound above every (n0 n0) + (n1 n1) whose square root is
// below max_distance (a cheap first look that never decides; +inf where max_distance's square is not a normal number), both formed once on
// the host
struct DupDev { int same_type, exclusive; double gate_chi2, max_distance, md2_hi, s2; };

// a map in device memory; cov may be null: zeros
struct DupMap { int n; const double *xy; const int32_t *type; const double *cov; };

// what the consolidation's kernels pass on, all [n] but blk [3][blocks], blk_off [blocks] and info
struct DupWork {
    const int32_t *twin, *nadm;
    int32_t *slot; double *f_xy, *f_cov;
    int32_t *blk, *blk_off; gs_dup_info *info;
    double *out_xy; int32_t *out_type; double *out_cov; int32_t *remap;        // out_cov is null with a map without covariances
};

// twin / d2 / second_d2 / n_admissible of every cone; d2, second and nadm may be null
void launch_dup_nearest(const DupMap &m, const DupDev &p, int32_t *twin, double *d2, double *second, int32_t *nadm, hipStream_t st,
                        hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// the mutual test, the fusion for keepers, the keep flag as a rank within the block, the per-block counts
void launch_dup_fuse(const DupMap &m, const DupDev &p, const DupWork &w, hipStream_t st);
// one workgroup: the exclusive scan of the blocks' kept counts, and gs_dup_info
void launch_dup_scan(int n, const DupWork &w, hipStream_t st);
// every kept cone to its place in the second buffer, remap for all
void launch_dup_scatter(const DupMap &m, const DupWork &w, hipStream_t st, hipEvent_t stop = nullptr);

}  // namespace gs
