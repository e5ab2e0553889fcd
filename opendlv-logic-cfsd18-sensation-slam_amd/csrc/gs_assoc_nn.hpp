// gs_assoc_nn.hpp — launchers of the covariance-gated association (gs_assoc_nn.hip): nearest cone by Mahalanobis distance inside a
// chi-square gate, against a map with a 2x2 covariance per cone.  Host side: gs_frontend.cpp (gs_associate_nn_*, gs_frame_frontend_nn,
// gs_map_set_cov*).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gs {

// gs_nn_params as the kernels take it (the sigmas are squared on the device, inside the one function all kernels share)
struct NnDev { double gate_chi2, max_distance, type_tol, sigma_range, sigma_bearing, sigma_xy; };

// a thread per observation, the map through LDS in tiles of 1024.  map_cov (n_map x 4) and pose_cov (n_poses x 9) may be null: zeros.
// out_d2 / out_second may be null.  start / stop: events on the dispatch (timing hook), may be null.
void launch_assoc_nn(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, double lidar, int n_map,
                     const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                     int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// the same against the hashed grid of launch_grid_build (cell edge from max_distance): nine buckets per observation
void launch_assoc_nn_grid(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, double lidar,
                          const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                          long long buckets, const int32_t *cell_start, const int32_t *cell_items,
                          int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// one frame: in = {pose x, y, theta, pose_cov[9], obs[4 * k]} (has_pose_cov == 0: the nine are not read), a workgroup per observation
void launch_frame_nn(int k, const double *in, int has_pose_cov, double lidar, int n_map, const double *map_xy, const int32_t *map_type,
                     const double *map_cov, NnDev p, double *out_z, double *out_g, int32_t *out_idx, double *out_d2, double *out_second, hipStream_t st);
// map_cov[4 * (first + k) + c] = src[k] < 0 ? 0 : values[src[k] + c], k < n, c < 4
void launch_map_cov_gather(int n, const int64_t *src, const double *values, double *map_cov_first, hipStream_t st);
// one-to-one association inside frames [frame_start[f], frame_start[f + 1]), f < n_frames (everything in device memory): a wave per 1 .. 8 frames, by their mean size.
// cell_start != null: the nine buckets of the hashed grid (buckets, cell_start, cell_items); null: brute force over the map.
// A frame whose bounds are not 0 <= a <= b <= n touches nothing; one above GS_NN_FRAME_MAX gets -1 / +inf.  out_d2 may be null;
// out_z / out_g (both or neither): every covered observation's CoG-frame and global XY, as launch_frame_nn writes them.
void launch_assign_nn(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, int n_frames, const int32_t *frame_start,
                      double lidar, int n_map, const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                      long long buckets, const int32_t *cell_start, const int32_t *cell_items, int32_t *out_idx, double *out_d2, double *out_z, double *out_g,
                      hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// minimum-cost association inside the same frames, same arguments and defences; out_na (may be null): every covered observation's count of
// admissible cones, uncapped (0 in a frame above GS_NN_FRAME_MAX).  One or two dispatches: start on the first, stop on the last.
void launch_assign_opt(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, int n_frames, const int32_t *frame_start,
                       double lidar, int n_map, const double *map_xy, const int32_t *map_type, const double *map_cov, const double *pose_cov, NnDev p,
                       long long buckets, const int32_t *cell_start, const int32_t *cell_items, int32_t *out_idx, double *out_d2, int32_t *out_na,
                       double *out_z, double *out_g, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// joint compatibility of the hypothesis in_idx (cone or -1 per observation) inside the same frames: out_idx per observation (the cone while
// its pair is kept, else -1), and per frame J, the kept / dropped / untestable counts and delta[3] (each may be null).  gate: gs_jc_params'
// table, passed by value (the call needs no device copy of it).  Only p's sigmas are read.  Defences as launch_assign_opt, and a frame whose
// in-range pose indices differ is refused like one above GS_NN_FRAME_MAX: -1 per observation, J = +inf, counts and delta 0.
struct JcGate { double g[257]; };                                             // GS_NN_FRAME_MAX + 1
void launch_joint_compat(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, int n_frames, const int32_t *frame_start,
                         double lidar, int n_map, const double *map_xy, const double *map_cov, const double *pose_cov, NnDev p, const JcGate &gate,
                         const int32_t *in_idx, int32_t *out_idx, double *out_j, int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable,
                         double *out_delta, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);
// frame localisation under the hypothesis in_idx inside the same frames: per frame the pose [3], its covariance [9], chi2, the pairs counted,
// the solves made and the status (each may be null); step: d_f [3] per frame (gs_debug_localize's output, null as a rule).  Only p's sigmas are
// read.  Defences as launch_joint_compat: a frame above GS_NN_FRAME_MAX or with two pose indices gets status 4.  kernel: -1 by the mean frame
// size, 0 / 1 forces the small / the large kernel (results do not depend on it)
struct LoParams { int max_iterations; double tol_xy, tol_theta; };
struct LoOut { double *pose, *cov, *chi2; int32_t *n_pairs, *iterations, *status; double *step; };
void launch_localize(int n, const double *poses, int n_poses, const int32_t *pose_of_obs, const double *obs, int n_frames, const int32_t *frame_start,
                     double lidar, int n_map, const double *map_xy, const double *map_cov, const double *pose_cov, NnDev p, const LoParams &lp,
                     const int32_t *in_idx, const LoOut &o, int kernel, hipStream_t st, hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

// ---- relocalisation (gs_reloc.hip): a frame's pose found on the map without a prior, inside the same frames (no pose is read).
// gs_reloc_params as the kernels take it: inlier_r2 = inlier_radius^2 and distinct_d2 = distinct_xy^2, formed once on the host
struct RlDev { int seed_obs, min_inliers; double min_baseline, length_tol, inlier_radius, inlier_r2, type_tol, distinct_d2, distinct_cos; };
// what a workgroup of the seed kernel leaves behind, and what the pick kernel keeps of a frame's winner: count < 0 = none
struct RlRec { double cost, c, s, tx, ty; long long n_seeds; int32_t count, u, v, p, q, pad; };
struct RlOut { double *pose, *cost; int32_t *count, *seed, *second_count; double *second_pose; long long *n_seeds; int32_t *status, *index; double *e2; };
// a workgroup enumerates `slice` cones p against the whole map: n_slices records a frame (forced > 0: gs_debug_relocalize's slice)
int reloc_slices(int n_frames, int n_map, int forced, int &slice);
inline size_t reloc_rec_bytes(int n_frames, int n_slices) { return ((size_t)n_frames * (size_t)n_slices + (size_t)n_frames) * sizeof(RlRec); }
// seed kernel -> pick kernel, and both once more with the winner excluded when o.second_count or o.second_pose is set.  rec: reloc_rec_bytes
// of device memory.  cell_start != null: the score walks the nine buckets of the hashed grid (cell edge from inlier_radius); null: the whole
// map.  chain_pose / chain_frame_end (both or neither, one frame): the first pick kernel writes the pose there and, with status >= 2, a zero
// to chain_frame_end.  Defences as launch_assign_nn: bad bounds touch nothing, a frame above GS_NN_FRAME_MAX gets status 4.
void launch_relocalize(int n, const double *obs, int n_frames, const int32_t *frame_start, double lidar, int n_map, const double *map_xy,
                       const int32_t *map_type, RlDev p, long long buckets, const int32_t *cell_start, const int32_t *cell_items, int slice,
                       int n_slices, RlRec *rec, const RlOut &o, double *chain_pose, int32_t *chain_frame_end, hipStream_t st,
                       hipEvent_t start = nullptr, hipEvent_t stop = nullptr);

}  // namespace gs
