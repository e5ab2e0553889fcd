/*
 * graphslam_debug.h — tuning, fault-injection and measurement hooks of the MI355X GraphSLAM back-end.
 *
 * NOT part of the drop-in boundary (include/graphslam.h): nothing here has a counterpart in the reference (its optimiser is a
 * g2o::SparseOptimizer with no such knobs, reference src/slam.cpp:53-65; it has no fault injection).  The tests, bench.py
 * and the scripts under scripts/ use these entry points for A/B timing, for the parity checks of every launch mode and for the
 * failure-semantics tests.  A consumer of the library (the microservice) never needs this header.
 */
#ifndef GRAPHSLAM_DEBUG_H
#define GRAPHSLAM_DEBUG_H

#include "graphslam.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Every tuning switch of a handle in ONE place.  gs_create fills it once from the environment variable named with each field (so a
 * script can still steer a whole process without code) and never looks at the environment again; gs_debug_set_options replaces it.
 * -1 (or 0 where stated) = the library's default.  "plan" fields act at the next structure phase (gs_initialize_optimization /
 * the first gs_optimize after a graph change), "call" fields at the next call that consults them.
 *
 *   launch shape of the solver — numerically neutral: the GPU suite asserts bitwise equal results across them
 *     tree            GS_TREE          plan  1 whole-tree launches (fronts wait for their children's flags); 0 one launch per level
 *     block_fronts    GS_BLOCK_FRONTS  plan  levels of at most this many fronts run a WORKGROUP per front (default 512)
 *     leaf_kernel     GS_LEAF_KERNEL   plan  0 never a separate leaf launch, 2 always, -1 by leaf_min
 *     leaf_min        GS_LEAF_MIN      plan  separate leaf launches only above this many leaves (default 2048)
 *     bs_wide         GS_BS_WIDE       plan  backward solve: levels wider than this leave the flagged launch for the light one(s) (default 1024)
 *     bs_low          GS_BS_LOW        plan  backward solve: 1 (default) the wide levels below the flagged launch share ONE light launch whose fronts
 *                                      poll their boundary rows; 0 one light launch per level (the launches before that one existed)
 *     leaf_nt3        GS_LEAF_NT3      plan  1 three-tile-row leaf instance when every leaf has <= 47 scalars (default), 0 off
 *     f3_lds_kb       GS_F3_LDS_KB     plan  occupancy experiments: LDS per workgroup of the per-level factor launches, KB (0 = need)
 *     subtree         GS_SUBTREE       plan  1: a level-1 front and the leaves below it run in ONE workgroup (k_factor3_sub: the leaves'
 *                                      update matrices stay in LDS; measured slower); 0 (default): leaf launch + flagged
 *                                      launch from level 1 up
 *     tickets         GS_TICKETS       plan  1: a workgroup of a whole-tree launch takes its number from a counter in HBM — the launch's own order,
 *                                      whatever order the hardware dispatches in (measured: -2.4 % iterations/s at 100k poses, -5 % at 10k, -9 % on
 *                                      24-cones-in-view tracks: one same-address atomic per workgroup); 0 (default): blockIdx — grid-order dispatch,
 *                                      with the bounded polls, the per-level fallback and the retry behind it
 *   plan shape — changes the elimination order, hence the last bits of the result (all are exact factorisations)
 *     leaf_poses      GS_LEAF_POSES    plan  nested-dissection leaf size in poses (0 = gs_config.leaf_poses / default 8)
 *     cluster_ways    GS_CLUSTER_WAYS  plan  fan-out of the multi-way split above the leaves (0 = default 8; 2 = binary)
 *     ell_lanes       GS_ELL_LANES     plan  lanes per pose of the observation-edge layout (0 = by size)
 *     big_cluster     GS_BIG_CLUSTER   plan  second-pass bound of a cluster front (-1 = by the view; 0 = wave fronts only)
 *     grow_headroom   GS_GROW_HEADROOM plan  scalars a cluster front stays below a wave's 63 (-1 = default 6)
 *     factor_variant  GS_FACTOR_VARIANT plan 0 = gs_config.factor_variant; 3 matrix-core LDL^T fronts, 4 block-per-front VALU
 *   append-only growth
 *     grow            GS_GROW          call  0: every graph change is a full structure phase (default 1)
 *     grow_min_poses  GS_GROW_MIN_POSES call graphs below this many poses always rebuild (default 128)
 *   front end
 *     assoc_grid      GS_ASSOC_GRID    call  batched association: 1 uniform grid, 0 brute force, -1 by map size (default)
 *   multi-GPU
 *     force_shared_top GS_FORCE_SHARED_TOP plan  world 1 only: the top k levels of the tree are treated as the SHARED top of a sharded
 *                                      graph (contribution -> exchange buffer -> all-reduce -> redundant top), so that the collective
 *                                      path runs with a non-empty exchange buffer on one GPU (default 0 = off)
 *     shard_by_window GS_SHARD_BY_WINDOW plan 1 (default): a rank builds the top of the tree from per-landmark window masks and touches only its own
 *                                      window's edges beyond one pass (gs_plan.cpp, nd_top); 0: the general recursion over every edge (the same plan
 *                                      for equal windows, a power of two of them)
 *   experiments / diagnostics
 *     host_trig       GS_HOST_TRIG     plan  1: cos / sin of the INITIAL pose angles from the host's libm (scripts/parity_spread.py)
 *     pool_poison     GS_POOL_POISON   plan  1: device chunks are filled with 0xFF when taken and when released
 *     plan_timing     GS_PLAN_TIMING   plan  1: per-step wall times of the structure phase on stderr, one line "<phase> <step> <ms> ms" each: phase
 *                                      "structure" (the driver), "plan" (the host's plan build, e.g. "plan symbolic  1.93 ms") and "upload"
 *     dbg             GS_DBG           plan  in-kernel phase timestamps: 8 | level_count << 8, 16 | level_position << 8
 * Two process-wide variables remain outside the struct: GS_THREADS (host threads of the plan build) and, Python binding only, GS_LIB. */
typedef struct gs_debug_options {
    int32_t struct_size;
    int32_t tree, block_fronts, leaf_kernel, leaf_min, bs_wide, leaf_nt3, f3_lds_kb, bs_low;
    int32_t leaf_poses, cluster_ways, ell_lanes, big_cluster, grow_headroom, factor_variant;
    int32_t grow, grow_min_poses;
    int32_t assoc_grid;
    int32_t force_shared_top;
    int32_t host_trig, pool_poison, plan_timing, dbg;
    int32_t subtree;
    int32_t tickets;
    int32_t shard_by_window;
    int32_t reserved[5];
} gs_debug_options;

int gs_debug_options_default(gs_debug_options *o);                     /* the library's defaults (the environment is NOT consulted) */
int gs_debug_get_options(gs_graph *g, gs_debug_options *o);            /* what the handle runs with */
int gs_debug_set_options(gs_graph *g, const gs_debug_options *o);      /* "plan" fields: the next structure phase is a full one */

/* Tuning aid: with dbg = 8 | (count << 8), the factor / backsolve kernels of the level that holds `count` fronts record 100 MHz
 * timestamps at their phase boundaries for that level's first front (factor: slots 0.., backsolve: slots 32..).  Copies the 64 slots out. */
int gs_debug_timestamps(gs_graph *g, int64_t *out64);
/* Tuning aid (F3_DONE_TS builds of the library only, zeros otherwise): 100 MHz completion time of every front in the
 * last factor launch ([0, n)) and the last backward-solve launch ([n, 2n)); returns n. */
int gs_debug_front_times(gs_graph *g, int64_t *out, int64_t capacity);
/* Fault injection (tests of the failure semantics; the reference has none): the k-th iteration enqueued after
 * this call reports `code` (1 = zero pivot, 2 = front-flag timeout) from its first front; k = 0 disarms. */
int gs_debug_fail_at_iteration(gs_graph *g, int32_t k, int32_t code);
/* Measurement hook of the batched association (bench.py's `association` entry): `reps` launches of gs_associate_resident, each with a HIP
 * start / stop event pair attached to the query kernel's dispatch (its own begin -> end, on the handle's stream); mean ms per launch. */
int gs_debug_time_associate_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                     const double *dev_obs_4xn, double threshold, double type_tol, int32_t *dev_out_index, int32_t reps, double *out_ms);
/* Its twin for the covariance-gated association: `reps` launches of gs_associate_nn_resident, timed the same way. */
int gs_debug_time_associate_nn_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                        const double *dev_obs_4xn, const double *dev_pose_cov_3x3, const gs_nn_params *params, int32_t *dev_out_index,
                                        double *dev_out_d2, double *dev_out_second_d2, int32_t reps, double *out_ms);
/* And for the one-to-one association: `reps` launches of gs_assign_nn_resident, events on the assignment kernel's dispatch. */
int gs_debug_time_assign_nn_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                     const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                                     const gs_nn_params *params, int32_t *dev_out_index, double *dev_out_d2, int32_t reps, double *out_ms);
/* And for the minimum-cost association: `reps` launches of gs_assign_opt_resident, events from its first dispatch to its last. */
int gs_debug_time_assign_opt_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                      const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                                      const gs_nn_params *params, int32_t *dev_out_index, double *dev_out_d2, int32_t *dev_out_n_admissible,
                                      int32_t reps, double *out_ms);
/* And for the joint compatibility test: `reps` launches of gs_joint_compat_resident, events from its first dispatch to its last. */
int gs_debug_time_joint_compat_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                        const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                                        const gs_nn_params *params, const gs_jc_params *jc, const int32_t *dev_in_index, int32_t *dev_out_index,
                                        double *dev_out_joint_d2, int32_t *dev_out_n_kept, int32_t *dev_out_n_dropped, int32_t *dev_out_n_untestable,
                                        double *dev_out_delta_3, int32_t reps, double *out_ms);
/* Frame localisation.  gs_debug_localize: kernel = 0 forces k_localize (k_localize_big behind it for the frames above 64 observations), 1 forces
 * k_localize_big alone, -1 (default) chooses by the mean frame size — in all three calls; results do not depend on it.  dev_out_step_3: a DEVICE
 * buffer of 3 doubles per frame that every later gs_localize_resident call fills with d_f (zeros where no solve was made or the status is 2, 3
 * or 4), until it is set back to NULL; the batch and the frame call do not write it.  gs_debug_time_localize_resident: `reps` launches of
 * gs_localize_resident, events from its first dispatch to its last. */
int gs_debug_localize(gs_graph *g, int32_t kernel, double *dev_out_step_3);
int gs_debug_time_localize_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                                    const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                                    const gs_nn_params *params, const gs_loc_params *loc, const int32_t *dev_in_index, double *dev_out_pose_3,
                                    double *dev_out_cov_3x3, double *dev_out_chi2, int32_t *dev_out_n_pairs, int32_t *dev_out_iterations,
                                    int32_t *dev_out_status, int32_t reps, double *out_ms);
/* Relocalisation.  gs_debug_relocalize: slice_cones > 0 forces how many cones p a workgroup of the seed kernel enumerates (a frame then has
 * ceil(map size / slice_cones) records for the pick kernel to reduce), 0 (default) lets the launcher choose — in all three calls; results do
 * not depend on it.  gs_debug_time_relocalize_resident: `reps` launches of gs_relocalize_resident (the grid built before), events from its
 * first dispatch to its last; mean milliseconds per call. */
int gs_debug_relocalize(gs_graph *g, int32_t slice_cones);
int gs_debug_time_relocalize_resident(gs_graph *g, int32_t n, const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start,
                                      const gs_reloc_params *params, double *dev_out_pose_3, int32_t *dev_out_count, double *dev_out_cost,
                                      int32_t *dev_out_seed_4, int32_t *dev_out_second_count, double *dev_out_second_pose_3,
                                      int64_t *dev_out_n_seeds, int32_t *dev_out_status, int32_t *dev_out_index, double *dev_out_e2,
                                      int32_t reps, double *out_ms);
/* Frame following.  gs_debug_time_follow_resident: `reps` calls of gs_follow_resident (the grid built before), events from the run's first
 * dispatch (the kernel that sets the hypotheses up) to its last (the last step's update); mean milliseconds per run. */
int gs_debug_time_follow_resident(gs_graph *g, int32_t n_hyp, const double *dev_poses_xytheta, const double *dev_covs_3x3, int32_t n_steps, int32_t n,
                                  const double *dev_obs_4xn, const int32_t *dev_frame_start, int32_t frame_cap, const double *dev_motion_3,
                                  const double *dev_motion_cov_3x3, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                                  const gs_follow_params *follow, gs_follow_step *dev_out_steps, int32_t *dev_out_index, gs_follow_state *dev_out_state,
                                  int32_t *dev_out_best_2, int32_t reps, double *out_ms);
/* Cone candidates.  gs_debug_time_cand_resident: `reps` calls of gs_cand_resident, events from the run's first dispatch (the kernel that sets
 * the table up) to its last (the last step's update); mean milliseconds per run. */
int gs_debug_time_cand_resident(gs_graph *g, int32_t n_steps, int32_t n, const double *dev_obs_4xn, const int32_t *dev_frame_start, int32_t frame_cap,
                                const double *dev_poses_xytheta, const double *dev_pose_covs_3x3, const int32_t *dev_in_idx, int32_t n_in,
                                const gs_cand *dev_in_table, const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *dev_out_steps,
                                int32_t *dev_out_cand_id, int32_t *dev_out_cand_slot, gs_cand *dev_out_table, int32_t *dev_out_meta_4,
                                int32_t reps, double *out_ms);
/* Map twins.  gs_debug_time_map_twins_resident: `reps` calls of gs_map_twins_resident, events on its one dispatch.
 * gs_debug_time_map_merge_twins: `reps` times the four dispatches of gs_map_merge_twins over the resident map into the second buffer, events
 * from the first to the last; the map itself is left as it is, so every run sees the same twins.  Mean milliseconds per run. */
int gs_debug_time_map_twins_resident(gs_graph *g, const gs_dup_params *params, int32_t *dev_out_twin, double *dev_out_d2, double *dev_out_second_d2,
                                     int32_t *dev_out_n_admissible, int32_t reps, double *out_ms);
int gs_debug_time_map_merge_twins(gs_graph *g, const gs_dup_params *params, int32_t reps, double *out_ms);
/* Measurement hook of the sharded iteration (bench.py's `ms_exchange`): `reps` RCCL all-reduces of the exchange buffer back to back on the
 * handle's stream, HIP events around them; mean ms per all-reduce.  Collective: every rank of the communicator calls it. */
int gs_debug_time_exchange(gs_graph *g, int32_t reps, double *out_ms);
/* The factor-kernel variant a plan with the given largest front and H-arena size (doubles) is given for a requested variant
 * (gs_config.factor_variant; 0 = default): 3 = matrix-core LDL^T fronts with 32-bit byte offsets into the arena (a wave per front of
 * <= 63 scalars, a workgroup per front of 64 .. 159; arena < 2^29 doubles), 4 = block-per-front kernel with 64-bit addressing
 * (anything else).  Pure function; what gs_initialize_optimization applies. */
int gs_debug_select_factor_variant(int32_t requested, int32_t max_front, int64_t arena_doubles);
/* The solver launches of the current plan, as decided once with the plan (a function of the plan and the options: no call history).
 * Same calling convention as gs_plan_export (out == NULL: *out_len = the length); works on a host-only handle after gs_plan_build_host.
 * int32 record, n_levels = L, own / shared level positions n_own / n_shared (a position indexes the device's level list: own fronts,
 * then the shared top of a sharded plan from shared_base):
 *   [0..20)  0x47535331, L, n_own, n_shared, shared_base, factor_variant (3, or 0 = the C-ABI's 4), tables (1: the plan holds a front of
 *            more than 63 scalars, launches are table-driven), leaf_n, leaf_slot, leaf_max_f, n_subtrees, sub_first, sub_free, block_n,
 *            bs_l0 (first level of the flagged backward-solve launch), small_max_npiv, small_max_f, 0, 0, 0
 *   own_start[L + 1], shared_start[L + 1], own_fronts[n_own], shared_fronts[n_shared]  (position -> front, positions relative to the list)
 *   five tables (own factor, own backward solve, shared contributions, shared top, shared backward solve), each: n, then n entries
 *            {position, kind | count << 8}: kind 0 = `count` small fronts a wave each (factor: position upwards, backward solve: downwards),
 *            1 = a small front on four waves, 4 / 2 / 3 = a front of 64-79 / 80-111 / 112-159 scalars on a workgroup
 *   the launches of one iteration in whole-tree mode, then with one launch per level (after a flag timeout), each: n, then n records
 *            {kind, first, count, LDS bytes (0: chosen inside the launcher), kernel class or mode, table (-1: none)}
 *            kind 1 whole-tree factor launch over positions [first, first + count) (leaf instance, bottom subtrees and flagged levels as
 *            the header says), 2 the leaf instance alone, 3 one factor launch over positions of one level (class = mode: 0 own, 1
 *            contributions, 2 shared top), 4 the shared top's flagged launch, 5 table-driven factor launch: entries [first, first + count)
 *            of `table` (0 .. 4 in the order above), 6 flagged backward-solve launch, 7 backward-solve launch of one level, 8 table-driven
 *            backward-solve launch.  A launch over no fronts (an empty level of a list) is none: left out.  The light polling launch
 *            over the wide levels (bs_low) is recorded with kind 6 as well — its fronts order themselves — with its LDS bytes. */
int gs_debug_schedule_export(gs_graph *g, int32_t *out, int64_t *out_len);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHSLAM_DEBUG_H */
