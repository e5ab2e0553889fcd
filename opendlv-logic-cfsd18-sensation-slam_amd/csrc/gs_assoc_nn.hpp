// gs_assoc_nn.hpp — launchers of the covariance-gated association (gs_assoc_nn.hip): nearest cone by Mahalanobis distance inside a
// chi-square gate, against a map with a 2x2 covariance per cone.  Host side: gs_frontend.cpp (gs_associate_nn_*, gs_frame_frontend_nn,
// gs_map_set_cov*).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace gs {

// gs_nn_params as the kernels take it (the sigmas are squared on the device, inside the one function all kernels share)
struct NnDev { double gate_chi2, max_distance, type_tol, sigma_range, sigma_bearing, sigma_xy; };

// what a launcher is given, in three parts (all device pointers; the views live on the caller's stack).
// The observations: n of them (4 doubles each, 32-byte aligned), the pose each was taken at, the frames [frame_start[f], frame_start[f + 1])
// they fall into (n_frames == 0: the launcher reads no frames), a 3x3 covariance per pose (n_poses x 9; null: zeros).  Relocalisation reads
// no poses: its pose fields are null
struct ObsRef { int n; const double *poses; int n_poses; const int32_t *pose_of_obs; const double *obs; int n_frames; const int32_t *frame_start; const double *pose_cov; };
// The map: n cones, a 2x2 covariance per cone (n x 4; null: zeros), and the search: cell_start != null: the nine buckets of the hashed grid of
// launch_grid_build (buckets, cell_start, cell_items; its cell edge is the launcher's own distance); null: the whole map is walked
struct MapRef { int n; const double *xy; const int32_t *type; const double *cov; long long buckets; const int32_t *cell_start, *cell_items; };
// The stream, and the timing hook's events: start on the launcher's first dispatch, stop on its last (null: none)
struct Launch { hipStream_t st; hipEvent_t start = nullptr, stop = nullptr; };

// a thread per observation: the map through LDS in tiles of 1024, or nine buckets of the grid (cell edge from max_distance).
// out_d2 / out_second may be null
void launch_assoc_nn(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, double *out_second, Launch L);
// one frame: in = {pose x, y, theta, pose_cov[9], obs[4 * k]} (has_pose_cov == 0: the nine are not read), a workgroup per observation
// (m's search is not read: the workgroup walks the map)
void launch_frame_nn(int k, const double *in, int has_pose_cov, const MapRef &m, double lidar, NnDev p, double *out_z, double *out_g, int32_t *out_idx,
                     double *out_d2, double *out_second, hipStream_t st);
// map_cov[4 * (first + k) + c] = src[k] < 0 ? 0 : values[src[k] + c], k < n, c < 4
void launch_map_cov_gather(int n, const int64_t *src, const double *values, double *map_cov_first, hipStream_t st);
// one-to-one association inside o's frames: a wave per 1 .. 8 frames, by their mean size.
// A frame whose bounds are not 0 <= a <= b <= n touches nothing; one above GS_NN_FRAME_MAX gets -1 / +inf.  out_d2 may be null;
// out_z / out_g (both or neither): every covered observation's CoG-frame and global XY, as launch_frame_nn writes them.
void launch_assign_nn(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, double *out_z, double *out_g, Launch L);
// minimum-cost association inside the same frames, same arguments and defences; out_na (may be null): every covered observation's count of
// admissible cones, uncapped (0 in a frame above GS_NN_FRAME_MAX).  One or two dispatches: start on the first, stop on the last.
void launch_assign_opt(const ObsRef &o, const MapRef &m, double lidar, NnDev p, int32_t *out_idx, double *out_d2, int32_t *out_na, double *out_z, double *out_g,
                       Launch L);
// joint compatibility of the hypothesis in_idx (cone or -1 per observation) inside the same frames: out_idx per observation (the cone while
// its pair is kept, else -1), and per frame J, the kept / dropped / untestable counts and delta[3] (each may be null).  gate: gs_jc_params'
// table, passed by value (the call needs no device copy of it).  Only p's sigmas are read.  Defences as launch_assign_opt, and a frame whose
// in-range pose indices differ is refused like one above GS_NN_FRAME_MAX: -1 per observation, J = +inf, counts and delta 0.
struct JcGate { double g[257]; };                                             // GS_NN_FRAME_MAX + 1
void launch_joint_compat(const ObsRef &o, const MapRef &m, double lidar, NnDev p, const JcGate &gate, const int32_t *in_idx, int32_t *out_idx, double *out_j,
                         int32_t *out_kept, int32_t *out_dropped, int32_t *out_untestable, double *out_delta, Launch L);
// frame localisation under the hypothesis in_idx inside the same frames: per frame the pose [3], its covariance [9], chi2, the pairs counted,
// the solves made and the status (each may be null); step: d_f [3] per frame (gs_debug_localize's output, null as a rule).  Only p's sigmas are
// read.  Defences as launch_joint_compat: a frame above GS_NN_FRAME_MAX or with two pose indices gets status 4.  kernel: -1 by the mean frame
// size, 0 / 1 forces the small / the large kernel (results do not depend on it)
struct LoParams { int max_iterations; double tol_xy, tol_theta; };
struct LoOut { double *pose, *cov, *chi2; int32_t *n_pairs, *iterations, *status; double *step; };
void launch_localize(const ObsRef &o, const MapRef &m, double lidar, NnDev p, const LoParams &lp, const int32_t *in_idx, const LoOut &out, int kernel, Launch L);

// ---- relocalisation (gs_reloc.hip): a frame's pose found on the map without a prior, inside the same frames (no pose is read).
// gs_reloc_params as the kernels take it: inlier_r2 = inlier_radius^2 and distinct_d2 = distinct_xy^2, formed once on the host
struct RlDev { int seed_obs, min_inliers; double min_baseline, length_tol, inlier_radius, inlier_r2, type_tol, distinct_d2, distinct_cos; };
// what a workgroup of the seed kernel leaves behind, and what the pick kernel keeps of a frame's winner: count < 0 = none
struct RlRec { double cost, c, s, tx, ty; long long n_seeds; int32_t count, u, v, p, q, pad; };
struct RlOut { double *pose, *cost; int32_t *count, *seed, *second_count; double *second_pose; long long *n_seeds; int32_t *status, *index; double *e2; };
// a workgroup enumerates `slice` cones p against the whole map: n_slices records a frame (forced > 0: gs_debug_relocalize's slice)
int reloc_slices(int n_frames, int n_map, int forced, int &slice);
inline size_t reloc_rec_bytes(int n_frames, int n_slices) { return ((size_t)n_frames * (size_t)n_slices + (size_t)n_frames) * sizeof(RlRec); }
// seed kernel -> pick kernel, and both once more with the winner excluded when out.second_count or out.second_pose is set.  rec: reloc_rec_bytes
// of device memory.  The score walks the nine buckets of m's grid (cell edge from inlier_radius) or, without one, the whole map; o's pose
// fields are not read.  chain_pose / chain_frame_end (both or neither, one frame): the first pick kernel writes the pose there and, with status >= 2, a zero
// to chain_frame_end.  Defences as launch_assign_nn: bad bounds touch nothing, a frame above GS_NN_FRAME_MAX gets status 4.
void launch_relocalize(const ObsRef &o, const MapRef &m, double lidar, RlDev p, int slice, int n_slices, RlRec *rec, const RlOut &out, double *chain_pose,
                       int32_t *chain_frame_end, Launch L);

}  // namespace gs
