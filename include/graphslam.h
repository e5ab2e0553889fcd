/*
 * graphslam.h — C-ABI of the MI355X-native GraphSLAM back-end.
 *
 * Drop-in boundary for the ONE hot path of cfsd/opendlv-logic-cfsd18-sensation-slam:
 * every call `Slam` makes on its private `g2o::SparseOptimizer m_optimizer`
 * (reference src/slam.hpp:98) plus the batched front-end arithmetic that feeds
 * it (polar->XY, cone->map association).  The reference has no FFI of its own;
 * each entry point below cites the reference call site it replaces.
 *
 * Conventions
 *  - plain C, opaque handles, caller-owned buffers, all inputs copied (g2o takes
 *    ownership of new-ed vertices/edges, we copy instead: src/slam.cpp:434-438).
 *  - every function returns an int status (GS_OK == 0, negative == error) except
 *    gs_optimize / gs_iterate which follow g2o's convention of returning the
 *    number of iterations performed (0 == factorisation failed) or a negative
 *    error code.  Nothing throws, nothing aborts.
 *  - all arithmetic is IEEE fp64, all indices int32.
 *  - pose ids and landmark ids live in SEPARATE id spaces (the reference's
 *    single namespace, cones 0.., poses 1000.., collides beyond 1000 cones:
 *    src/slam.hpp:118, src/slam.cpp:556,610).
 *  - a handle is externally synchronised (the reference holds m_optimizerMutex
 *    around every optimiser call: src/slam.cpp:324,372,402,560,586,614,627).
 *  - the compute path is HIP on gfx950 only.  There is no CPU fallback: without
 *    a usable device gs_create fails with GS_ERR_NO_DEVICE.
 */
#ifndef GRAPHSLAM_H
#define GRAPHSLAM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_VERSION_MAJOR 0
#define GS_VERSION_MINOR 1

/* ---- status codes ------------------------------------------------------- */
#define GS_OK                    0
#define GS_ERR_INVALID          -1  /* null pointer / bad argument              */
#define GS_ERR_DUPLICATE_ID     -2  /* g2o addVertex returns false on dup id    */
#define GS_ERR_UNKNOWN_ID       -3  /* g2o vertex(id) returns nullptr           */
#define GS_ERR_NO_DEVICE        -4  /* no gfx950 device / HIP runtime unusable  */
#define GS_ERR_HIP              -5  /* a HIP call failed (see gs_last_error)    */
#define GS_ERR_NOT_INITIALIZED  -6  /* gs_iterate before gs_initialize_optimization */
#define GS_ERR_EMPTY            -7  /* nothing to optimise (no free vertex)     */
#define GS_ERR_NUMERIC          -8  /* zero pivot: H singular (see gs_optimize) */
#define GS_ERR_CAPACITY         -9  /* output buffer too small                  */
#define GS_ERR_TIMEOUT         -10  /* a whole-tree solver launch gave up waiting for a front (see gs_stream_synchronize) */
#define GS_ERR_OUT_OF_PATTERN  -11  /* covariance block of a pair outside the factor's pattern (see gs_get_covariance_block) */

typedef struct gs_graph gs_graph;   /* replaces g2o::SparseOptimizer (src/slam.hpp:98) */
typedef struct gs_slam  gs_slam;    /* replaces the graph-side state of class Slam     */

/* ---- configuration ------------------------------------------------------ */
typedef struct gs_config {
    int32_t struct_size;        /* sizeof(gs_config), for ABI evolution                     */
    int32_t device;             /* HIP device ordinal; -1 = current device; -2 = host-only
                                   handle (graph container + plan inspection, every compute
                                   entry point returns GS_ERR_NO_DEVICE)                    */
    int32_t verbose;            /* 1: print g2o-style "iteration= i chi2= ..." to stderr
                                   (reference: setVerbose(true), src/slam.cpp:63)          */
    int32_t leaf_poses;         /* nested-dissection leaf size in poses; 0 = default        */
    int32_t factor_variant;     /* front factorisation kernel: 0 = default (3 when every front has <= 159
                                   scalars and the H arena fits 32-bit byte offsets, else 4); 3 = LDL^T on the fp64
                                   matrix cores (v_mfma_f64_16x16x4_f64), chosen PER FRONT: a wave for a front of <= 63
                                   scalars, a workgroup for one of 64 .. 159; update matrices moved in storage order;
                                   4 = block-per-front VALU Cholesky, any front size                 */
    int32_t linearize_gather;   /* 1: force the general gather kernels instead of the fused tiled
                                   linearisation kernel (both are HIP; for tests and A/B timing)   */
    /* Slam-level constants, defaults are the reference's hard-coded values */
    double  odometry_information;   /* 5.0   (src/slam.cpp:456)                             */
    double  cone_information;       /* 0.01  (src/slam.cpp:546)                             */
    double  same_cone_threshold;    /* --sameConeThreshold, m_newConeThreshold (slam.cpp:740) */
    double  cone_mapping_threshold; /* --coneMappingThreshold (slam.cpp:744)                */
    double  lidar_to_cog;           /* 1.5 m (src/slam.cpp:514)                             */
    double  loop_closing_radius;    /* 1.0 m (src/slam.cpp:702)                             */
    int32_t loop_closing_min_index; /* 20    (src/slam.cpp:702)                             */
    int32_t optimize_iterations;    /* 10    (src/slam.cpp:481)                             */
    int32_t reference_quirks;       /* 1: keep SURVEY §8-B quirks 1-2 (duplicate first edge,
                                       re-optimise per remaining observation)              */
    int32_t optimize_every_keyframe; /* 0 (the reference): the graph is optimised once, at loop closure.  1 (NOT the reference's behaviour):
                                        gs_slam_perform also runs optimizeGraph + updateMap at the end of every keyframe that did not run
                                        them already.  The reference carries optimizeGraph() calls commented out at src/slam.cpp:594 and
                                        :620-621 (with updateMap) and at :403 (localizer: optimizeGraph ONLY, no updateMap); with this flag
                                        localizer-mode keyframes also run updateMap — the map and the resident association map are
                                        rewritten after loop closure, which restoring the reference's comments would not do.  One more
                                        keyframe does not rebuild the structure here (append-only growth), so the call costs about a
                                        millisecond at lap size; in localizer mode the published pose is then the optimised one. */
    /* robust kernels, applied by gs_create (see gs_set_robust_kernel); the defaults, none on both kinds, are the reference's behaviour */
    int32_t odometry_robust_kernel;     /* GS_ROBUST_*, 0 = none                                */
    double  odometry_robust_delta;      /* 1.0                                                  */
    int32_t observation_robust_kernel;  /* GS_ROBUST_*, 0 = none                                */
    double  observation_robust_delta;   /* 1.0                                                  */
} gs_config;

/* per-call statistics of gs_optimize / gs_iterate (all times from HIP events on
 * the handle's stream, milliseconds, summed over the iterations of the call) */
typedef struct gs_stats {
    int32_t struct_size;
    int32_t iterations;         /* iterations whose update was applied (== requested unless the solve failed) */
    int32_t n_free_poses, n_free_landmarks;
    int32_t n_odometry_edges, n_observation_edges;
    int32_t n_fronts, n_levels, max_front;   /* multifrontal plan                          */
    int32_t numeric_failure;    /* 0 ok; 1 zero pivot; 2 front-flag timeout; 3 failure reported by another rank */
    double  chi2_initial;       /* chi2 at the linearisation point of the first iteration   */
    double  chi2_final;         /* chi2 at the linearisation point of the last iteration    */
    double  ms_structure;       /* host: ordering + symbolic + upload (iteration-0 work)   */
    double  ms_linearize;       /* A5+A6+A7 kernel(s)                                       */
    double  ms_factor;          /* multifrontal numeric factorisation + forward solve       */
    double  ms_backsolve;       /* backward solve                                           */
    double  ms_update;          /* A9                                                       */
    double  ms_total;           /* whole call, events                                       */
    int64_t factor_flops;       /* model flops of one factorisation                         */
    int64_t factor_bytes;       /* L + update-matrix storage, bytes                         */
    double  ms_event_overhead;  /* gs_time_iterations: an empty event-to-event interval on the
                                   stream, i.e. the share of every phase time that is measurement */
    int32_t fell_back;          /* 1: the handle runs one launch per level (the slow path) because a whole-tree launch gave
                                   up on a front's completion flag — in this call or an earlier one; 0: whole-tree launches.
                                   Not for good: the 4th gs_optimize call after a fallback tries the whole-tree launches again
                                   (then the 16th, 64th ... after each further timeout), and a new plan starts afresh */
    int32_t first_failure;      /* the first failure code this call met (0 none): a flag timeout (2) that the per-level
                                   fallback then repaired leaves numeric_failure 0 and first_failure 2 */
    int32_t factor_variant;     /* the front kernels this plan runs on (gs_config.factor_variant after the per-plan rules): 3 = LDL^T on
                                   the fp64 matrix cores (a wave per front up to 63 scalars, a workgroup per front up to 159), 4 = block VALU */
    int32_t n_big_fronts;       /* fronts of more than 63 scalars (variant 3: the ones that get a workgroup) */
    int64_t device_bytes;       /* HBM this handle's plan and graph occupy (the chunks its arrays are carved from) */
    int32_t n_own_fronts, n_shared_fronts;   /* pose-window shards: fronts this rank factorises / the shared top (world 1: all, 0) */
    double  ms_plan_host;       /* share of ms_structure spent building the plan on the host */
    double  ms_linearize_kernel; /* gs_time_iterations: the A5-A7 kernel's own begin -> end per launch, from events attached to its dispatch (ms_linearize
                                    is event to event on the stream: it also holds the hand-over from the previous kernel) */
    int32_t n_growths;          /* append-only growth steps the current plan has absorbed since the last full structure phase (0: none) */
    int32_t n_subtrees;         /* level-1 fronts that run with the leaves below them in ONE workgroup (k_factor3_sub; known after the first iteration of a plan) */
    int32_t n_pose_priors, n_landmark_priors;   /* prior edges the handle holds (gs_add_*_prior; XY priors count as pose priors).  The last fields so far:
                                   present when the struct_size the library writes is >= offsetof(gs_stats, n_landmark_priors) + 4 */
} gs_stats;

int  gs_version(void);                               /* major*100+minor */
const char *gs_last_error(void);                      /* thread-local message of the last failure */
int  gs_config_default(gs_config *cfg);
int  gs_device_count(void);                           /* number of usable gfx950 devices, 0 if none */

/* ---- lifetime: replaces Slam::setupOptimizer (src/slam.cpp:53-65) -------- */
int  gs_create(const gs_config *cfg, gs_graph **out);
int  gs_destroy(gs_graph *g);
int  gs_clear(gs_graph *g);                           /* drop all vertices, edges and priors */
/* use an externally owned hipStream_t (e.g. torch's current stream); NULL = own stream */
int  gs_set_stream(gs_graph *g, void *hip_stream);
/* Device memory for the first structure phase, taken (and touched) now — e.g. at start-up, where the reference constructs its
 * optimizer (src/slam.cpp:36-65) — instead of inside the first gs_optimize: chunks of 8, 16, 32 ... MB until `bytes` are held.  A handle
 * keeps its device memory across structure phases anyway (a re-plan allocates nothing); this only moves the FIRST allocations out of
 * the first optimize(): 0.05 ms for a lap-sized graph, up to ~12 ms at 10k poses on machines where fresh allocations are slow.
 * gs_slam_create reserves 24 MB (a lap-sized graph needs 3-8 MB). */
int  gs_reserve_device(gs_graph *g, int64_t bytes);

/* ---- graph construction (A2) --------------------------------------------
 * gs_add_pose             <- new VertexSE2; setId; setEstimate; addVertex        (src/slam.cpp:434-438)
 * gs_add_landmark         <- new VertexPointXY; setId; setEstimate; addVertex    (src/slam.cpp:527-531)
 * gs_add_odometry_edge    <- new EdgeSE2; vertices; setMeasurement; setInformation; addEdge (src/slam.cpp:447-457)
 * gs_add_observation_edge <- new EdgeSE2PointXY; ...                              (src/slam.cpp:538-547)
 * information matrices are row-major full (9 resp. 4 doubles) and must be symmetric. */
int  gs_add_pose(gs_graph *g, int32_t pose_id, const double est_xytheta[3]);
int  gs_add_landmark(gs_graph *g, int32_t lm_id, const double est_xy[2]);
int  gs_add_odometry_edge(gs_graph *g, int32_t pose_id_i, int32_t pose_id_j,
                          const double z_xytheta[3], const double information[9]);
int  gs_add_observation_edge(gs_graph *g, int32_t pose_id, int32_t lm_id,
                             const double z_xy[2], const double information[4]);
/* bulk SoA/AoS variants (count records, arrays tightly packed, row-major per record) */
int  gs_add_poses(gs_graph *g, int32_t count, const int32_t *pose_ids, const double *est_xytheta);
int  gs_add_landmarks(gs_graph *g, int32_t count, const int32_t *lm_ids, const double *est_xy);
int  gs_add_odometry_edges(gs_graph *g, int32_t count, const int32_t *pose_ids_i,
                           const int32_t *pose_ids_j, const double *z_xytheta,
                           const double *information /* count*9, or NULL -> cfg.odometry_information*I */);
int  gs_add_observation_edges(gs_graph *g, int32_t count, const int32_t *pose_ids,
                              const int32_t *lm_ids, const double *z_xy,
                              const double *information /* count*4, or NULL -> cfg.cone_information*I */);

/* gs_set_fixed_* <- dynamic_cast<...>(vertex(id))->setFixed(true)                 (src/slam.cpp:464-474) */
int  gs_set_fixed_pose(gs_graph *g, int32_t pose_id, int32_t fixed);
int  gs_set_fixed_landmark(gs_graph *g, int32_t lm_id, int32_t fixed);
int  gs_set_pose_estimate(gs_graph *g, int32_t pose_id, const double est_xytheta[3]);
int  gs_set_landmark_estimate(gs_graph *g, int32_t lm_id, const double est_xy[2]);

/* ---- read-back (A11) -----------------------------------------------------
 * gs_get_pose     <- static_cast<VertexSE2*>(vertex(id))->estimate().toVector()   (src/slam.cpp:418-420,451-452)
 * gs_get_landmark <- static_cast<VertexPointXY*>(vertex(j))->estimate()           (src/slam.cpp:719-720) */
int  gs_get_pose(gs_graph *g, int32_t pose_id, double out_xytheta[3]);
int  gs_get_landmark(gs_graph *g, int32_t lm_id, double out_xy[2]);
int  gs_num_poses(gs_graph *g);
int  gs_num_landmarks(gs_graph *g);
int  gs_num_odometry_edges(gs_graph *g);
int  gs_num_observation_edges(gs_graph *g);
/* all vertices in insertion order; ids may be NULL */
int  gs_get_poses(gs_graph *g, int32_t capacity, int32_t *out_ids, double *out_xytheta);
int  gs_get_landmarks(gs_graph *g, int32_t capacity, int32_t *out_ids, double *out_xy);

/* ---- optimisation (A3-A10) ------------------------------------------------
 * gs_initialize_optimization <- m_optimizer.initializeOptimization()              (src/slam.cpp:480)
 *      + g2o BlockSolver::buildStructure: index maps, ordering, symbolic plan, upload to HBM.
 * gs_optimize                <- m_optimizer.optimize(10)                          (src/slam.cpp:481)
 *      runs `iterations` x (computeActiveErrors, buildSystem, solve, update) on the device,
 *      no damping, no line search, no convergence test; returns iterations done (damped: gs_optimize_lm, below).
 *      Failure semantics are g2o's: when the factorisation of an iteration fails, that iteration's
 *      update and all later ones are NOT applied — the estimates stay at the last good iterate —
 *      and the call returns 0 (stats->iterations = updates applied, stats->numeric_failure = code).
 *      The default solver is an LDL^T like the Eigen 3.3.4 SimplicialLDLT behind g2o's
 *      LinearSolverEigen and fails like it on a pivot d == 0 only
 *      (thirdparty/Eigen/src/SparseCholesky/SimplicialCholesky_impl.h:172-176), plus on NaN;
 *      the Cholesky fallback kernel (factor_variant 4) fails on d <= 0 like SimplicialLLT.
 * gs_iterate                 one Gauss-Newton iteration, asynchronous on the handle's stream
 *      (the bench's "step"); estimates stay in HBM until gs_sync_estimates / gs_optimize.
 *      A failed iteration applies no update either; gs_stream_synchronize / gs_sync_estimates
 *      report it (GS_ERR_NUMERIC, or GS_ERR_TIMEOUT when a whole-tree launch gave up waiting for
 *      a front: the handle then switches to one launch per level) once and clear the condition.
 * gs_optimize_until          config 2 of BASELINE.json ("optimise to convergence"): the reference has no
 *      stop rule, this is the build-defined one.  Iterates until the chi2 at two
 *      consecutive linearisation points differs by <= rel_chi2_tol * chi2 (checked on the device
 *      value every iteration), at most max_iterations; returns the iterations whose update
 *      was applied, 0 on failure as gs_optimize.
 * With a robust kernel set (gs_set_robust_kernel) every chi2 these calls report (gs_chi2, gs_stats.chi2_initial / chi2_final, the
 *      verbose line) is the sum of rho(s) over the edges (g2o activeRobustChi2), and the stop rule of gs_optimize_until compares
 *      that sum. */
int  gs_initialize_optimization(gs_graph *g);
int  gs_optimize(gs_graph *g, int32_t iterations, gs_stats *stats /* may be NULL */);
int  gs_optimize_until(gs_graph *g, int32_t max_iterations, double rel_chi2_tol, gs_stats *stats /* may be NULL */);
int  gs_iterate(gs_graph *g);
int  gs_sync_estimates(gs_graph *g);      /* device -> host estimates, waits for the stream   */
int  gs_stream_synchronize(gs_graph *g);
/* computeActiveErrors + activeChi2 at the current estimates (device); with a robust kernel set: activeRobustChi2, the sum of rho(s) */
int  gs_chi2(gs_graph *g, double *out_chi2);
int  gs_get_stats(gs_graph *g, gs_stats *stats);      /* plan statistics after initialize */

/* ---- Levenberg-Marquardt ------------------------------------------------------
 * gs_optimize_lm <- g2o OptimizationAlgorithmLevenberg, the one-line swap at the reference's call site (src/slam.cpp:61 constructs
 * OptimizationAlgorithmGaussNewton).  g2o is not part of this project's checkers: the rule is restated from g2o's published text and is
 * not pinned against a g2o build.  State lambda, nu (2 at the start).  Per iteration, at the accepted estimates x:
 *   1. chi_old = chi2(x) (with a robust kernel set: the sum of rho(s), as everywhere else); H and b linearised at x.
 *   2. first iteration, no lambda given: lambda = tau * max_j |H_jj| over the free scalars.
 *   3. trials, at most max_trials_after_failure: solve (H + lambda I) D = b — lambda added to EVERY free diagonal scalar (g2o setLambda),
 *      not Marquardt's scaling —; x_try = x [+] D (the update of gs_iterate, angle normalisation included); chi_new = chi2(x_try);
 *      scale = sum_j D_j (lambda D_j + b_j) + 1e-3; rho = (chi_old - chi_new) / scale.
 *      rho > 0 and chi_new finite: ACCEPT, lambda *= max(1/3, min(1 - (2 rho - 1)^3, 2/3)), nu = 2, next iteration.
 *      otherwise REJECT: x is put back bit for bit, lambda *= nu, nu *= 2, next trial.  A zero pivot in a trial's factorisation is a
 *      rejected trial (g2o sets rho = -1), not the end of the call.
 *   4. every trial of an iteration rejected: the call ends ("terminate"), the estimates are the last accepted ones.
 * The whole call runs on the handle's stream with no host decision inside a trial: a trial is the launch sequence of gs_iterate with
 * five more launches around it — damp + base copy of the estimates, scale, the chi2 pass (two launches: per-pose sums, total) and step;
 * a max-diagonal kernel once per call when no lambda is given —; lambda, nu, the counters and the verdict live in a device record the
 * host reads between chunks of trials.  A retrial linearises again at the restored estimates.
 * Returns the number of ACCEPTED iterations (like gs_optimize: the updates that stayed); a call that ends by "terminate" returns the
 * count so far with info->terminated = 1 — not an error.  A flag timeout of a whole-tree launch is repaired by the per-level fallback
 * as in gs_optimize.  gs_stats: chi2_initial / chi2_final are the values at the first / last accepted point, iterations the accepted
 * count.  Works with robust kernels, grown plans, factor_variant 3 and 4, workgroup fronts, both linearisation paths; makes the
 * marginals stale like an iteration; leaves no failure, stop or LM state behind that gates a later gs_iterate / gs_optimize.
 * gs_export_system afterwards returns the system of the LAST TRIAL AS IT WAS FACTORISED: H at that trial's starting point with its
 * lambda on the free diagonal scalars (b and the off-diagonal blocks undamped).  On a grown plan as well: lambda is on the
 * diagonal scalars of tail poses and tail cones as on those of old vertices (a trial's chi2 at its trial point writes nothing of H or b).
 * Errors: iterations < 0, a tau or initial_lambda that is not finite, tau <= 0, max_trials_after_failure < 1: GS_ERR_INVALID;
 * a host-only handle GS_ERR_NO_DEVICE.  A solver failure the step control cannot turn into a rejected trial ends the call with an
 * error code, NOT with gs_optimize's "return 0" (0 is a regular result here: no trial accepted): GS_ERR_TIMEOUT when a front's flag
 * did not arrive with one launch per level either, GS_ERR_NUMERIC for any other failure code; the estimates are the last accepted
 * ones, stats and info are filled (stats->numeric_failure = the code), and the handle is clean for the next call.
 * NOT DONE: pose-window shards (a handle configured with gs_dist_configure(world > 1) returns GS_ERR_INVALID); Marquardt's diagonal
 * scaling; a convergence stop rule other than "terminate"; the Slam mirror keeps calling gs_optimize. */
typedef struct gs_lm_params {
    int32_t struct_size;                /* sizeof(gs_lm_params), for ABI evolution                           */
    int32_t max_trials_after_failure;   /* 10 (g2o's default)                                                */
    double  initial_lambda;             /* <= 0 (default): tau * max_j |H_jj| at the first linearisation      */
    double  tau;                        /* 1e-5 (g2o's default)                                              */
} gs_lm_params;
typedef struct gs_lm_info {
    int32_t struct_size;
    int32_t iterations;                 /* accepted                                                          */
    int32_t trials, rejected;           /* trials run, trials rejected                                       */
    int32_t terminated;                 /* 1: an iteration used up its trials without an accepted step       */
    int32_t reserved;
    double  lambda_initial, lambda_final;   /* of the first trial; the one a next trial would have used     */
    /* per ITERATION (the first 64): chi2 at the accepted point the iteration started from, lambda of its accepted (or last) trial,
       its number of trials.  A call that terminates has one more entry than accepted iterations. */
    double  chi2[64], lambda[64];
    int32_t n_trials[64];
} gs_lm_info;
int  gs_lm_params_default(gs_lm_params *p);
int  gs_optimize_lm(gs_graph *g, int32_t iterations, const gs_lm_params *p /* NULL: defaults */,
                    gs_stats *stats /* may be NULL */, gs_lm_info *info /* may be NULL */);

/* ---- Powell's dogleg -----------------------------------------------------------
 * gs_optimize_dogleg <- g2o OptimizationAlgorithmDogleg, the third algorithm at the reference's call site (src/slam.cpp:61).  g2o is not
 * part of this project's checkers: the rule is restated from g2o's published text and is not pinned against a g2o build.  State: the
 * trust radius delta (initial_delta at the start).  All vectors are over the free scalars.  Per iteration, at the accepted estimates x:
 *   1. chi_old = chi2(x) (with a robust kernel set: the sum of rho(s)); H and b linearised at x.
 *   2. steepest descent: alpha = (b^T b) / (b^T H b), h_sd = alpha b.  (Not g2o's: alpha = 0 when b^T H b is not finite or not > 0.)
 *   3. h_gn = the Gauss-Newton step: the factorisation and back-solve of gs_iterate, no damping.
 *   4. trials, at most max_trials_after_failure:
 *        |h_gn| < delta:       h_dl = h_gn                                (GS_DOGLEG_GN)
 *        else |h_sd| > delta:  h_dl = (delta / |h_sd|) h_sd               (GS_DOGLEG_SD)
 *        else:                 h_dl = h_sd + beta a                       (GS_DOGLEG_DL)  with a = h_gn - h_sd, c = h_sd^T a, q = a^T a,
 *                              m = delta^2 - |h_sd|^2, beta = (-c + sqrt(c^2 + q m)) / q if c <= 0, else m / (c + sqrt(c^2 + q m))
 *      gain = -h_dl^T (H h_dl) + 2 b^T h_dl (|gain| < 1e-12: 1e-12); x_try = x [+] h_dl (the update of gs_iterate, angle normalisation
 *      included); chi_new = chi2(x_try); rho = (chi_old - chi_new) / gain.  rho > 0 and chi_new finite: ACCEPT; otherwise x is put back
 *      bit for bit.  Either way rho > 0.75 sets delta = max(delta, 3 |h_dl|) and rho < 0.25 halves delta.
 *   5. every trial of an iteration rejected: the call ends ("terminate"), the estimates are the last accepted ones.
 * The whole call runs on the handle's stream with no host decision inside a trial, as gs_optimize_lm does: a trial is the launch sequence
 * of gs_iterate with the two Hessian-vector products (H b and H h_dl: the kernel behind gs_multiply_hessian), six vertex-parallel
 * kernels and the chi2 pass around it; delta, the counters and the verdict live in a device record the host reads between chunks of
 * trials.  A retrial runs the whole sequence again at the restored estimates.  gs_export_delta afterwards returns h_dl of the last trial.
 * Returns the number of ACCEPTED iterations; a call that ends by "terminate" returns the count so far with info->terminated = 1 — not an
 * error.  gs_stats: chi2_initial / chi2_final are the values at the first / last accepted point, iterations the accepted count.  Works
 * with robust kernels, priors, polar edges, inactive edges, grown plans, factor_variant 3 and 4, both linearisation paths; makes the
 * marginals stale like an iteration; leaves no failure, stop or dogleg state behind that gates a later gs_iterate / gs_optimize /
 * gs_optimize_lm.  A flag timeout of a whole-tree launch is repaired by the per-level fallback as in gs_optimize.
 * Errors: iterations < 0, an initial_delta that is not finite or <= 0, max_trials_after_failure < 1: GS_ERR_INVALID; a host-only handle
 * GS_ERR_NO_DEVICE.  A zero pivot in the Gauss-Newton solve is g2o's "Fail": the call ends with GS_ERR_NUMERIC (GS_ERR_TIMEOUT when a
 * front's flag did not arrive with one launch per level either), the estimates are the last accepted ones, stats and info are filled and
 * the handle is clean for the next call.
 * NOT DONE: g2o's lambda-damping of H when it was not positive definite; reuse of h_gn across the retrials of an iteration (a retrial
 * factorises again); pose-window shards (a handle configured with gs_dist_configure(world > 1) returns GS_ERR_INVALID); the Slam mirror
 * keeps calling gs_optimize. */
#define GS_DOGLEG_GN 0
#define GS_DOGLEG_SD 1
#define GS_DOGLEG_DL 2
typedef struct gs_dogleg_params {
    int32_t struct_size;                /* sizeof(gs_dogleg_params), for ABI evolution                       */
    int32_t max_trials_after_failure;   /* 100 (g2o's default)                                               */
    double  initial_delta;              /* 1e4 (g2o's default)                                               */
} gs_dogleg_params;
typedef struct gs_dogleg_info {
    int32_t struct_size;
    int32_t iterations;                 /* accepted                                                          */
    int32_t trials, rejected;           /* trials run, trials rejected                                       */
    int32_t terminated;                 /* 1: an iteration used up its trials without an accepted step       */
    int32_t reserved;
    int32_t n_gn, n_sd, n_dl;           /* accepted steps by kind                                            */
    double  delta_initial, delta_final; /* of the first trial; the one a next trial would have used          */
    /* per ITERATION (the first 64): chi2 at the accepted point the iteration started from, delta and kind (GS_DOGLEG_*) of its accepted
       (or last) trial, its number of trials.  A call that terminates has one more entry than accepted iterations. */
    double  chi2[64], delta[64];
    int32_t n_trials[64], step_kind[64];
} gs_dogleg_info;
int  gs_dogleg_params_default(gs_dogleg_params *p);
int  gs_optimize_dogleg(gs_graph *g, int32_t iterations, const gs_dogleg_params *p /* NULL: defaults */,
                        gs_stats *stats /* may be NULL */, gs_dogleg_info *info /* may be NULL */);

/* ---- robust kernels ---------------------------------------------------------
 * <- g2o OptimizableGraph::Edge::setRobustKernel with RobustKernelHuber / RobustKernelCauchy (the reference never sets one; the
 * formulas are restated from g2o's published text, not pinned against a g2o build).  For an edge with squared error
 * s = e^T Omega e (g2o's e->chi2()) and parameter delta, d2 = delta^2:
 *      none     rho(s) = s                                          w = rho'(s) = 1
 *      Huber    rho(s) = s if s <= d2, else 2 sqrt(s) delta - d2    w = 1 if s <= d2, else delta / sqrt(s)
 *      Cauchy   rho(s) = d2 log(1 + s / d2)                         w = 1 / (1 + s / d2)
 * The edge contributes w A^T Omega A, w A^T Omega B, w B^T Omega B to H, -w A^T Omega e, -w B^T Omega e to b (the second-order
 * term 2 rho'' (Omega e)(Omega e)^T is dropped, as g2o drops it) and rho(s) to chi2: one iteration is the plain Gauss-Newton
 * iteration of the same graph with every information matrix scaled by its edge's weight at the current estimates.
 * delta is in units of sqrt(s), i.e. it INCLUDES Omega: with the reference's cone_information = 0.01 a cone matched 3 m off has
 * sqrt(s) = 0.3, and the residuals at a clean optimum are near 0.01.  delta = 1, g2o's default, does nothing on this graph.
 * The kernel is set per edge KIND on the handle (all odometry edges / all observation edges), not per edge.  The setting belongs
 * to the handle: it survives gs_clear, growth and structure phases, costs no structure phase, may change between two gs_iterate
 * calls, and makes the marginals stale like any other change.  It can be set and read on a host-only handle.
 * Unknown kind or kernel, or (kernel other than none) a delta that is not finite and > 0: GS_ERR_INVALID.
 * NOT DONE: pose-window shards.  gs_set_robust_kernel(other than none) on a handle configured with gs_dist_configure(world > 1),
 * and gs_dist_configure(world > 1) on a handle with a kernel set, return GS_ERR_INVALID.
 * gs_get_edge_chi2: per edge of that kind, insertion order, at the CURRENT estimates: s = e^T Omega e and the weight rho'(s) of the
 *      kind's kernel (1 with GS_ROBUST_NONE).  Edges between two fixed vertices are reported too (they stay out of chi2).  Either
 *      pointer may be NULL; returns the number of edges (GS_ERR_CAPACITY when capacity is below it and a pointer is given);
 *      a host-only handle GS_ERR_NO_DEVICE, a sharded handle GS_ERR_INVALID. */
#define GS_ROBUST_NONE      0
#define GS_ROBUST_HUBER     1
#define GS_ROBUST_CAUCHY    2
#define GS_EDGE_ODOMETRY    0
#define GS_EDGE_OBSERVATION 1
int  gs_set_robust_kernel(gs_graph *g, int32_t edge_kind, int32_t kernel, double delta);
int  gs_get_robust_kernel(gs_graph *g, int32_t edge_kind, int32_t *out_kernel, double *out_delta);
int  gs_get_edge_chi2(gs_graph *g, int32_t edge_kind, int32_t capacity, double *out_chi2, double *out_weight);

/* ---- prior edges ------------------------------------------------------------
 * Unary edges: "this vertex is about HERE, with this uncertainty" — an absolute measurement (a GPS fix), or a soft gauge in place of a
 * fixed flag.  <- g2o EdgeSE2Prior, EdgeSE2XYPrior, EdgeXYPrior (the reference adds none; the formulas are restated from g2o's
 * published text, not pinned against a g2o build: g2o is not part of this project's checkers).
 *   gs_add_pose_prior      z = (zx, zy, ztheta), Omega 3x3:  e = vec(z^-1 o x), i.e. e_t = R_z^T (t - t_z), e_theta = normalize(theta - ztheta);
 *                          J = diag(R_z^T, 1) with the additive update of gs_iterate
 *   gs_add_pose_xy_prior   z = (zx, zy), Omega 2x2:  e = t - z (position only, no heading: the GPS case) — the pose prior with ztheta = 0
 *                          and Omega in the upper-left 2x2 of a 3x3 that is zero elsewhere, and stored as one
 *   gs_add_landmark_prior  z = (zx, zy), Omega 2x2:  e = l - z, J = I
 * A prior contributes J^T Omega J to the diagonal block of its vertex, -J^T Omega e to its right-hand side and e^T Omega e to chi2 —
 * nothing else: no off-diagonal block, so the plan, the fronts and the launch schedule do not change.  ADDING OR CLEARING PRIORS IS NOT
 * A STRUCTURAL CHANGE: it triggers no structure phase and does not turn a growth step into a full phase (a keyframe appended together
 * with its GPS prior is absorbed by growth); the prior tables travel whole to the device at the next call that computes.  Like any
 * change it makes the marginals stale.  A handle without priors runs exactly the launches it ran before.
 * A prior on a FIXED vertex is accepted and stays out of H, b and chi2 (g2o: an edge whose vertices are all fixed is inactive).
 * Several priors on one vertex are summed in insertion order.  Every chi2 the library reports includes the priors (gs_chi2,
 * gs_stats.chi2_*, the verbose line, the stop rule of gs_optimize_until, chi_old / chi_new of gs_optimize_lm); gs_export_system
 * returns H and b with them, gs_compute_marginals inverts that H — with a prior in place of a fixed flag every vertex has a covariance.
 * information: row-major full (9 resp. 4 doubles), symmetric, REQUIRED (also in the bulk forms).  Priors belong to their vertices:
 * gs_clear drops them; gs_clear_priors drops all of them and nothing else.
 * gs_num_pose_priors counts the XY priors too.
 * gs_get_prior_chi2: per prior of the kind (0 pose, 1 landmark), insertion order, e^T Omega e at the CURRENT estimates; priors on
 *      fixed vertices are reported too (they stay out of chi2).  out_chi2 may be NULL; returns the number of priors (GS_ERR_CAPACITY
 *      when capacity is below it and a pointer is given); a host-only handle GS_ERR_NO_DEVICE, a sharded handle GS_ERR_INVALID.
 * Errors: unknown id GS_ERR_UNKNOWN_ID; a null pointer, a z that is not finite, an information matrix that gs_add_*_edge would
 *      refuse: GS_ERR_INVALID.  On a host-only handle everything but gs_get_prior_chi2 works.
 * NOT DONE: robust kernels are not applied to priors (weight 1 whatever gs_set_robust_kernel says); pose-window shards — a gs_add_*_prior
 *      on a handle configured with gs_dist_configure(world > 1), and gs_dist_configure(world > 1) on a handle that holds priors, return
 *      GS_ERR_INVALID; a FREE landmark whose only measurement is a prior (the fused linearisation keeps a landmark's block in the
 *      partial-sum slots of its observation edges; without one there is no address for it): the next computing call returns
 *      GS_ERR_INVALID with a message, on both linearisation paths, until the prior is cleared or an observation edge is added;
 *      removal of single priors; the Slam mirror and the microservice shell add no priors. */
int  gs_add_pose_prior(gs_graph *g, int32_t pose_id, const double z_xytheta[3], const double information[9]);
int  gs_add_pose_xy_prior(gs_graph *g, int32_t pose_id, const double z_xy[2], const double information[4]);
int  gs_add_landmark_prior(gs_graph *g, int32_t lm_id, const double z_xy[2], const double information[4]);
int  gs_add_pose_priors(gs_graph *g, int32_t count, const int32_t *pose_ids, const double *z_xytheta, const double *information /* count*9 */);
int  gs_add_pose_xy_priors(gs_graph *g, int32_t count, const int32_t *pose_ids, const double *z_xy, const double *information /* count*4 */);
int  gs_add_landmark_priors(gs_graph *g, int32_t count, const int32_t *lm_ids, const double *z_xy, const double *information /* count*4 */);
int  gs_num_pose_priors(gs_graph *g);
int  gs_num_landmark_priors(gs_graph *g);
int  gs_clear_priors(gs_graph *g);
int  gs_get_prior_chi2(gs_graph *g, int32_t kind /* 0 pose, 1 landmark */, int32_t capacity, double *out_chi2);

/* ---- edge deactivation ------------------------------------------------------
 * Per-edge levels, restated from g2o's published text (OptimizableGraph::Edge::setLevel, initializeOptimization(level)); nothing
 * here is pinned against a g2o build.  An edge is active (level 0) or inactive (level 1); a new edge is active.  The standard outlier
 * workflow: optimise with a robust kernel, gs_deactivate_edges_above a gate, optimise without the kernel on the inliers.
 * Edges are named by kind (GS_EDGE_ODOMETRY / GS_EDGE_OBSERVATION) and insertion index within the kind — the indices gs_get_edge_chi2
 * reports in.
 * An inactive edge contributes nothing to H, b or any chi2 the library reports (gs_chi2, gs_stats.chi2_*, the verbose line, the stop
 * rule of gs_optimize_until, the step control of gs_optimize_lm); gs_export_system returns zeros for its blocks; gs_compute_marginals
 * inverts the H without it.  gs_get_edge_chi2 still reports its s, with the edge's own information at the current estimates (so that
 * the caller can reconsider it), and weight 0.  On a handle with no inactive edge every call returns what it returned before.
 * Changing a flag is NOT a structural change: no structure phase, a growth step stays a growth step.  It may happen between two
 * gs_iterate calls and is applied on the handle's stream at the next call that computes.  Like any change it makes the marginals
 * stale.  Flags survive growth steps and full structure phases; gs_clear drops them.
 * Isolated vertices: a FREE vertex that carries no prior and has no active edge (its diagonal block would be zero).
 * gs_find_isolated_vertex reports the first one — poses in insertion order, then landmarks — as kind (0 pose, 1 landmark) and id;
 * returns 1 when there is one, 0 when not (host only: works on every handle).  While a handle with inactive edges has one, every
 * call that computes returns GS_ERR_INVALID with a message naming the vertex, before anything is launched.  A graph that deactivation
 * cuts into a component without gauge is the caller's business, as any under-constrained graph is.
 * gs_set_edges_active: active == NULL switches all the listed edges off.  All or nothing: a bad index changes no flag.
 * gs_get_edges_active: one byte per edge of the kind (1 active); out_active may be NULL; returns the number of edges.
 * gs_deactivate_edges_above: the device computes s = e^T Omega e of every edge of the kind with the edge's own information at the
 *      current estimates and marks the ACTIVE edges with s > s_threshold; the host walks the marked edges in insertion order and
 *      switches each off — except, with keep_connected != 0, one that would leave a free, prior-less endpoint without an active edge,
 *      given the decisions taken so far.  Inactive edges stay inactive.  *out_deactivated (may be NULL) = edges newly switched off.
 *      Deterministic.  s_threshold must be finite and >= 0.
 * Errors: unknown kind, index out of range, a null pointer with count > 0: GS_ERR_INVALID; capacity below the edge count:
 *      GS_ERR_CAPACITY.  On a host-only handle everything works but gs_deactivate_edges_above (GS_ERR_NO_DEVICE).
 * NOT DONE: pose-window shards — a flag change to inactive (gs_deactivate_edges_above included) on a handle configured with
 *      gs_dist_configure(world > 1), and gs_dist_configure(world > 1) on a handle with inactive edges, return GS_ERR_INVALID; physical
 *      removal of edges or vertices; levels other than 0 / 1; pinning an isolated vertex instead of refusing it; the Slam mirror and
 *      the microservice shell deactivate nothing. */
int  gs_set_edge_active(gs_graph *g, int32_t edge_kind, int32_t index, int32_t active);
int  gs_set_edges_active(gs_graph *g, int32_t edge_kind, int32_t count, const int32_t *indices, const uint8_t *active /* NULL: all 0 */);
int  gs_get_edges_active(gs_graph *g, int32_t edge_kind, int32_t capacity, uint8_t *out_active);
int  gs_activate_all_edges(gs_graph *g);
int  gs_num_inactive_edges(gs_graph *g, int32_t edge_kind);
int  gs_find_isolated_vertex(gs_graph *g, int32_t *out_kind, int32_t *out_id);
int  gs_deactivate_edges_above(gs_graph *g, int32_t edge_kind, double s_threshold, int32_t keep_connected, int32_t *out_deactivated);

/* ---- polar observation edges -------------------------------------------------
 * The sensor's own measurement model: a cone detection is accurate in bearing and poor in range, and a camera-only cone is a bearing
 * with no range at all.  Two edge types between a pose and a landmark beside the Cartesian gs_add_observation_edge (<- g2o
 * EdgeSE2PointXYBearing for the bearing-only one; the formulas are restated, nothing here is pinned against a g2o build).
 * With d = x_p^-1 * l the landmark in the pose frame, r = |d| and beta = atan2(dy, dx):
 *   gs_add_range_bearing_edge  z = (z_r >= 0, z_beta in radians), Omega 2x2 symmetric in (range, bearing):
 *                              e = (r - z_r, normalize_theta(beta - z_beta))
 *   gs_add_bearing_edge        z_beta, omega >= 0: the range-bearing edge with z_r = 0 and Omega = [[0, 0], [0, omega]], and stored as one
 * g2o's EdgeSE2PointXYBearing takes z - beta; the sign changes neither H, b nor chi2.  z_beta is normalised when stored.  The bearing
 * is taken at the pose's origin.  Jacobians are analytic, for the additive update of gs_iterate: Jd = d(r, beta)/dd =
 * [[dx/r, dy/r], [-dy/r^2, dx/r^2]], B = Jd R^T for the landmark, A = [-B | (0, -1)^T] for the pose.  The edge contributes w A^T Omega A,
 * w A^T Omega B, w B^T Omega B to H, -w A^T Omega e and -w B^T Omega e to b and rho(s) to chi2, with s = e^T Omega e and w, rho from the
 * OBSERVATION kind's robust kernel.  An edge with r == 0 exactly contributes nothing in that pass and reports s = 0.  Fixed vertices as
 * for every edge: a fixed endpoint stays out of H, an edge between two fixed vertices out of chi2.
 * A POLAR EDGE IS AN OBSERVATION EDGE.  It takes the next observation-edge index, gs_num_observation_edges counts it, and that index
 * names it in gs_get_edge_chi2 (s with its own Omega, the kind's weight), gs_set_edge_active / gs_set_edges_active,
 * gs_export_system (its Hpl row) and gs_get_observation_edge_covariances.  Adding one is a structural change exactly like
 * gs_add_observation_edge: the same growth rules apply (a keyframe appended with polar edges to old cones is absorbed by growth).
 * gs_clear drops polar edges.  Everything that linearises or sums chi2 sees them: gs_iterate, gs_optimize, gs_optimize_until,
 * gs_optimize_lm, gs_chi2, gs_compute_marginals, gs_export_system, with robust kernels, priors and inactive edges.  A handle without
 * polar edges runs exactly the launches it ran before and allocates nothing new.
 * information is REQUIRED (also in the bulk forms: count*4 resp. count doubles).
 * gs_num_polar_edges / gs_get_polar_edges: the polar edges in insertion order as observation-edge index and model (GS_OBS_RANGE_BEARING /
 *      GS_OBS_BEARING; every other observation edge is GS_OBS_CARTESIAN); either pointer may be NULL; returns the count (GS_ERR_CAPACITY
 *      when capacity is below it and a pointer is given).
 * Errors: unknown id GS_ERR_UNKNOWN_ID; a null pointer, a z that is not finite, z_r < 0, an Omega that is not finite or not symmetric,
 *      omega < 0 or not finite: GS_ERR_INVALID — a refused edge leaves nothing behind.  On a host-only handle everything here works;
 *      the computing calls return GS_ERR_NO_DEVICE as before.
 * NOT DONE: pose-window shards — a polar add on a handle configured with gs_dist_configure(world > 1), and gs_dist_configure(world > 1)
 *      on a handle that holds polar edges, return GS_ERR_INVALID; gs_deactivate_edges_above never selects a polar edge (its gate sees the
 *      zero information the edge is carried with): gate on gs_get_edge_chi2 and use gs_set_edges_active; removal of single edges; a
 *      sensor offset; the Slam mirror and the microservice shell keep adding Cartesian edges; gs_time_linearize keeps timing the
 *      roofline kernel alone. */
#define GS_OBS_CARTESIAN      0
#define GS_OBS_RANGE_BEARING  1
#define GS_OBS_BEARING        2
int  gs_add_range_bearing_edge(gs_graph *g, int32_t pose_id, int32_t lm_id, const double z_rb[2], const double information[4]);
int  gs_add_bearing_edge(gs_graph *g, int32_t pose_id, int32_t lm_id, double z_bearing, double information);
int  gs_add_range_bearing_edges(gs_graph *g, int32_t count, const int32_t *pose_ids, const int32_t *lm_ids, const double *z_rb, const double *information /* count*4, required */);
int  gs_add_bearing_edges(gs_graph *g, int32_t count, const int32_t *pose_ids, const int32_t *lm_ids, const double *z_bearing, const double *information /* count, required */);
int  gs_num_polar_edges(gs_graph *g);
int  gs_get_polar_edges(gs_graph *g, int32_t capacity, int32_t *out_observation_index, int32_t *out_model);

/* ---- measurement / parity hooks (tuning, fault injection and timestamps: include/graphslam_debug.h) ----------
 * gs_linearize: one A5+A6+A7 pass (the roofline kernel) on the stream, nothing else.
 * gs_time_linearize: `reps` back-to-back passes bracketed by HIP events on the handle's
 *      stream; returns the mean milliseconds per pass in *out_ms_per_pass.
 * gs_linearize_bytes: algorithmic bytes of one pass, SURVEY §8(d):
 *      E_pp*152 + E_pl*96 + N*120 + M*64.
 * gs_export_system: copy the block-sparse H and b of the last linearisation to the host (gs_linearize, the last
 *      iteration of gs_optimize / gs_iterate: H and b at the estimates before its update, or gs_compute_marginals:
 *      H and b at the estimates of that call); with a robust kernel set: the WEIGHTED H and b (every edge's blocks scaled by rho'(s))
 *      (vertex arrays in insertion order, edge arrays in the order reported by *_edge_order):
 *      Hpp_diag [N*9], Hll_diag [M*4], Hpp_off [Epp*9] (= A^T Omega B), Hpl [Epl*6] (= A^T Omega B,
 *      3x2 row-major), b_pose [N*3], b_lm [M*2].  Any pointer may be NULL.
 *      A plan grown by appended keyframes exports the system of the WHOLE graph the handle holds: N, M, Epp and Epl count the
 *      appended poses, cones and edges too, in the same insertion order; an appended vertex's or edge's blocks come from the tail
 *      arenas, and an older vertex's entries hold the shares of the appended edges, summed as the solver's fronts read them.
 *      gs_chi2 changes nothing of it, on a grown plan either.
 * gs_export_delta: the last solve's increment, per vertex in insertion order
 *      (zeros for fixed vertices): dpose [N*3], dlm [M*2].
 * gs_multiply_hessian: y = H v on the device, H the system gs_export_system would return (the last linearisation as it lies in HBM:
 *      robust weights, priors, polar and inactive edges as they went in, the lambda of a preceding gs_optimize_lm trial on the diagonal
 *      included), on a grown plan as well: the two agree block by block there too.  v and y per vertex in insertion order; rows and
 *      columns of fixed vertices are zero: y is 0 there and v is not read there.  Either output may be NULL.  Changes no state; a
 *      handle that never calls it (or gs_optimize_dogleg) allocates and launches nothing for it.
 *      Errors: a null v, or a v entry on a free vertex that is not finite: GS_ERR_INVALID; a sharded handle GS_ERR_INVALID; a
 *      host-only handle GS_ERR_NO_DEVICE; nothing linearised since the last structure phase or growth step (or the graph changed
 *      since): GS_ERR_NOT_INITIALIZED. */
int  gs_linearize(gs_graph *g);
int  gs_time_linearize(gs_graph *g, int32_t reps, double *out_ms_per_pass);

int64_t gs_linearize_bytes(gs_graph *g);
int  gs_export_system(gs_graph *g, double *Hpp_diag, double *Hll_diag, double *Hpp_off,
                      double *Hpl, double *b_pose, double *b_lm,
                      int32_t *odometry_edge_order, int32_t *observation_edge_order);
int  gs_export_delta(gs_graph *g, double *dpose, double *dlm);
int  gs_multiply_hessian(gs_graph *g, const double *v_pose /* [n_poses*3] */, const double *v_lm /* [n_lms*2] */,
                         double *out_pose, double *out_lm);   /* insertion order, either output may be NULL */
/* per-phase timing of `reps` full iterations (events on the stream); fills stats->ms_* with
 * per-iteration means.  Estimates are restored afterwards. */
int  gs_time_iterations(gs_graph *g, int32_t reps, gs_stats *stats);

/* ---- plan export (host logic, no device work; for tests of the symbolic phase) ---- */
typedef struct gs_plan_info {
    int32_t n_scalar;        /* free scalar unknowns                                          */
    int32_t n_fronts;
    int32_t n_levels;
    int32_t max_front;
    int64_t l_doubles;       /* factor storage                                                */
    int64_t u_doubles;       /* update-matrix storage                                         */
    int64_t n_asm_blocks;    /* original-entry assembly records                               */
    int64_t n_child_map;     /* extend-add map entries                                        */
} gs_plan_info;
/* builds the plan on the host only (no HIP), usable without a device */
int  gs_plan_build_host(gs_graph *g, gs_plan_info *info);
/* Append-only growth.  Per keyframe the reference adds one pose vertex with its odometry edge (src/slam.cpp:433-459), observation edges
 * to cones of the map (:537-550) and the cones it is the first to see with their first observation (:525-535); g2o's
 * initializeOptimization rebuilds everything at the next optimize() (:480).  Here, when the only changes since the last structure phase
 * are of that kind — new poses, new landmarks, edges whose pose end is a new pose; at most 16 poses / 16 landmarks / 512 + 64 edges since
 * the last full phase; every front stays within its form (63 scalars, or 159 in a plan with workgroup fronts) — gs_initialize_optimization /
 * gs_optimize keep the plan: the new vertices become
 * pivots of the root front, the fronts between a neighbour's front and the root gain them as boundary rows, and only those fronts' tables
 * are rebuilt (csrc/gs_plan.cpp grow_plan, csrc/gs_upload.cpp upload_growth).  Anything else (a fixed flag, an edge between old vertices,
 * a graph below 128 poses, where there is nothing to gain; switches: gs_debug_options.grow / grow_min_poses, graphslam_debug.h) is a full structure phase.
 * gs_plan_growths: steps absorbed by the current plan; gs_growth_refusal: why the last change was NOT absorbed ("" if it was). */
int  gs_plan_growths(gs_graph *g);
const char *gs_growth_refusal(gs_graph *g);
/* flat int32 dump of the plan, see csrc/gs_plan.hpp for the layout; call with out==NULL
 * to get the required length in *out_len. */
int  gs_plan_export(gs_graph *g, int32_t *out, int64_t *out_len);

/* ---- marginal covariances --------------------------------------------------
 * gs_compute_marginals       <- g2o SparseOptimizer::computeMarginals (g2o/core/sparse_optimizer.h): the
 *      counterpart of what g2o offers; the reference itself never calls it.  Linearises H at the CURRENT
 *      estimates (the ones gs_get_* returns), factorises it with the iteration's kernels and launch sequence
 *      (no backward solve, no update) and runs a selected inversion of the factor (Takahashi recursion):
 *      Sigma = H^-1 on the pattern of L, kept on the device by the handle.  With a robust kernel set H is the weighted H
 *      (gs_set_robust_kernel), and a change of the setting makes the results stale like an iteration does.  g2o's computeMarginals reuses the
 *      last iteration's factor instead, taken at the estimates BEFORE that iteration's update.
 *      Nothing else moves: no estimate, no chi2 history, no stop / failure / fallback state of gs_optimize_until
 *      and gs_iterate; runs on the handle's stream.  It is a linearisation, though: gs_export_system afterwards
 *      returns the H and b of this call.  H must have a gauge (fixed vertices): without one it is singular in exact
 *      arithmetic, and only an exactly-zero pivot is reported.  Fixed vertices (the gauge) are not in H: their blocks, and
 *      every cross block that involves one, are zeros.  A zero pivot returns GS_ERR_NUMERIC (no results), a
 *      front-flag timeout GS_ERR_TIMEOUT (the handle falls back to one launch per level, as gs_optimize does);
 *      a host-only handle GS_ERR_NO_DEVICE; a sharded handle GS_ERR_INVALID.
 * getters: the results of the last gs_compute_marginals, which belong to the estimates and the graph of that
 *      call: after an iteration, a gs_set_*_estimate, any gs_add_*, a fixed flag or gs_clear they return
 *      GS_ERR_NOT_INITIALIZED until the next gs_compute_marginals.  Full blocks, row-major; each returns the
 *      number of blocks written (GS_ERR_CAPACITY when capacity is below it).
 * gs_get_pose_covariances         3x3 per pose, the order of gs_get_poses (out_ids may be NULL)
 * gs_get_landmark_covariances     2x2 per landmark, the order of gs_get_landmarks (out_ids may be NULL)
 * gs_get_odometry_edge_covariances    Sigma(x_i, x_j), 3x3 per odometry edge, insertion order
 * gs_get_observation_edge_covariances Sigma(x_p, l), 3x2 per observation edge, insertion order
 * gs_get_covariance_block         Sigma(a, b) of any two vertices (kind 0 pose, 1 landmark) whose block lies in
 *      the pattern of L — every pair joined by an edge does, and every vertex with itself; other pairs return
 *      GS_ERR_OUT_OF_PATTERN (no extra solves).  out: 3 or 2 rows (a) x 3 or 2 columns (b), row-major.
 * gs_slam_get_map_covariances     (below) the 2x2 block of every cone of the Slam mirror's map, map order: computes
 *      the marginals of gs_slam_graph on demand; what gs_slam_perform does or publishes does not change. */
typedef struct gs_marginals_info {
    int32_t struct_size;         /* sizeof(gs_marginals_info), for ABI evolution                         */
    int32_t numeric_failure;     /* as gs_stats: 0 ok, 1 zero pivot, 2 front-flag timeout                 */
    int32_t n_fronts, n_levels;
    int64_t sigma_bytes;         /* device bytes of the selected inverse kept by the handle              */
    double  ms_linearize_factor, ms_selinv, ms_extract, ms_total;   /* HIP events on the handle's stream */
} gs_marginals_info;
int  gs_compute_marginals(gs_graph *g, gs_marginals_info *info /* may be NULL */);
int  gs_get_pose_covariances(gs_graph *g, int32_t capacity, int32_t *out_ids, double *out_3x3);
int  gs_get_landmark_covariances(gs_graph *g, int32_t capacity, int32_t *out_ids, double *out_2x2);
int  gs_get_odometry_edge_covariances(gs_graph *g, int32_t capacity, double *out_3x3);
int  gs_get_observation_edge_covariances(gs_graph *g, int32_t capacity, double *out_3x2);
int  gs_get_covariance_block(gs_graph *g, int32_t kind_a, int32_t id_a, int32_t kind_b, int32_t id_b, double *out);

/* ---- front end (A0, A1) ----------------------------------------------------
 * gs_polar_to_xy_batch  <- Slam::Spherical2Cartesian + transformConeToCoG    (src/slam.cpp:637-654, 513-523)
 *      in : az_deg[n], zen_deg[n], dist[n]   out: xy[n*2] (CoG-frame x,y)
 *      The reference's formula, kept with its quirks: NaN at az == 0 (sign = az / |az|), and next to dist * cos(az) = -lidar_to_cog
 *      (the cone abeam of the CoG, where asin's argument is 1) NaN or an error of order sqrt(2^-53) * dist in x.
 * gs_cone_to_global_batch <- Slam::coneToGlobal                               (src/slam.cpp:499-510)
 *      in : pose_of_obs[n] index into poses[npose*3]; out: xy_global[n*2]
 * gs_associate_batch    <- association loop of Slam::addConesToMap against a FIXED map
 *      (src/slam.cpp:570-607; localizer variant :350-382): for each observation the LOWEST map
 *      index j with |type_j - type_i| < type_tol and Euclidean distance < threshold, else -1.
 *      obs is the reference's m_coneCollector layout, column-major 4 x n: (az, zen, dist, type).
 * All three run on the device of `g`. */
int  gs_polar_to_xy_batch(gs_graph *g, int32_t n, const double *az_deg, const double *zen_deg,
                          const double *dist, double *out_xy);
int  gs_cone_to_global_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses,
                             const int32_t *pose_of_obs, const double *obs_4xn, double *out_xy_global);
int  gs_associate_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses,
                        const int32_t *pose_of_obs, const double *obs_4xn,
                        int32_t n_map, const double *map_xy, const int32_t *map_type,
                        double threshold, double type_tol, int32_t *out_index);

/* gs_associate_resident: the same association with EVERYTHING resident — the map of gs_map_append (below; its hashed uniform grid is built on
 *      the device, once per map change), poses, observations and the result in DEVICE memory — asynchronous on the handle's stream:
 *      nothing crosses PCIe, nothing waits (gs_stream_synchronize when the caller needs the indices).  The batched form of the loop
 *      that SURVEY 8(a) calls the dominant front-end cost at scale (src/slam.cpp:570-607). */
int  gs_associate_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                           const double *dev_obs_4xn, double threshold, double type_tol, int32_t *dev_out_index);

/* ---- the per-keyframe front end: A0 + A1 fused, against a map that stays resident in HBM -------------------------
 * gs_map_clear / gs_map_append / gs_map_set_xy / gs_map_size: the device mirror of Slam::m_map (src/slam.hpp: std::vector<Cone>):
 *      cones are appended in map order (index = Cone id, src/slam.cpp:556,610) and their positions rewritten after
 *      updateMap (src/slam.cpp:713-732).  Appends are asynchronous on the handle's stream.
 * gs_frame_frontend <- the per-frame arithmetic of addConesToMap / localizer (src/slam.cpp:570-607, 350-382): for the k
 *      observations of ONE frame (collector layout, column-major 4 x k) the CoG-frame XY (edge measurement), the global XY
 *      seen from `pose`, and the LOWEST map index with a matching type within `threshold` (-1: none) — one launch, one wait,
 *      no allocation.  signed_type != 0 selects the localizer's test `(type_j - (int)type_i) < type_tol` (no fabs, :360). */
int  gs_map_clear(gs_graph *g);
int  gs_map_append(gs_graph *g, int32_t n, const double *xy, const int32_t *type);
int  gs_map_set_xy(gs_graph *g, int32_t first, int32_t n, const double *xy);
int  gs_map_size(gs_graph *g);
int  gs_frame_frontend(gs_graph *g, const double pose_xytheta[3], const double *obs_4xk, int32_t k, double threshold,
                       double type_tol, int32_t signed_type, double *out_zxy, double *out_gxy, int32_t *out_index);

/* ---- covariance-gated association: the nearest cone by Mahalanobis distance inside a chi-square gate --------------
 * The loops these replace are the same two as above (src/slam.cpp:570-607, the association of addConesToMap, and :350-382, the
 * localizer's), which take the LOWEST map index inside a fixed Euclidean radius.  Here every map cone carries a 2x2 covariance (from
 * gs_compute_marginals or the caller), the measurement carries a range / bearing noise model, and the winner is the admissible cone with
 * the SMALLEST Mahalanobis distance.  The reference has no noise model: the rule and the defaults of gs_nn_params are build-defined.
 *
 * Rule.  Observation i of pose p = pose_of_obs[i] = (t, theta):  z = its CoG-frame XY (the A0 formula above, quirks included),
 *      w = R(theta) z,  g = w + t,  r^2 = zx^2 + zy^2,  wp = (-w_y, w_x).
 *      Q = (sigma_range^2 / r^2) w w^T + sigma_bearing^2 wp wp^T + sigma_xy^2 I      range along the ray, bearing across it (the bearing
 *                                                                                     is taken at the pose's origin, as the polar edges do)
 *      P = G Sigma_p G^T,  G = [I2 | wp],  Sigma_p = the pose's 3x3 covariance, row-major, the upper triangle read; NULL = zero
 *      Q + P is computed once per observation.  Candidate cone j at l_j with covariance Sigma_j (row-major 2x2, entry [1] read):
 *      S = Sigma_j + (Q + P),  nu = l_j - g,  det = S00 S11 - S01^2,  d2 = (S11 nu0^2 - 2 S01 nu0 nu1 + S00 nu1^2) / det.
 *      j is admissible iff ALL of  |type_j - type_i| < type_tol,  sqrt(nu0^2 + nu1^2) < max_distance,  det > 0,  S00 > 0,  d2 < gate_chi2
 *      hold (positive tests: any NaN skips the candidate).
 *      index     = the admissible j with the smallest d2, exact ties to the lowest index; -1 when there is none
 *      d2        = its d2; +inf when there is none
 *      second_d2 = the smallest d2 among the OTHER admissible candidates, +inf when there is none (what counts as ambiguous is the caller's call)
 *      A query whose g is not finite (azimuth 0) or whose r is 0 gets -1.  The cross-covariance Sigma(pose, cone) is IGNORED: for a
 *      candidate pair without an edge it lies outside the pattern of the factor, so the selected inversion does not have it.
 *      All paths below (batch with either search, resident with either search, the frame call) return identical bits.
 *
 * gs_map_set_cov / gs_map_get_cov: row-major 2x2 blocks of the resident map's cones [first, first + n).  set refuses (GS_ERR_INVALID, all
 *      or nothing) a block that is not finite, not bitwise symmetric or has a negative diagonal, and a range beyond the end of the map.
 *      Cones of gs_map_append have zero covariance until one is set; gs_map_clear drops them, gs_map_set_xy leaves them, growth keeps them.
 *      The array exists from the first set call on: a handle that never sets one allocates and launches nothing for it.
 * gs_map_set_cov_from_marginals: map cone first + k takes the 2x2 block of landmark lm_ids[k] (-1: zeros) out of the last
 *      gs_compute_marginals — device to device, one gather kernel, no host round trip of the values.  Unknown id GS_ERR_UNKNOWN_ID; stale or
 *      missing marginals GS_ERR_NOT_INITIALIZED (the getters' test).
 * gs_associate_nn_batch: host arrays in gs_associate_batch's layout plus map_cov (n_map x 4, NULL = zeros) and pose_cov (n_poses x 9,
 *      NULL = zeros); out_d2 / out_second_d2 may be NULL.  Grid (cell edge from max_distance) from 2048 cones, LDS tiles below;
 *      gs_debug_options.assoc_grid forces either, as for gs_associate_batch.
 * gs_associate_nn_resident: everything in DEVICE memory against the resident map and its covariances, asynchronous on the handle's stream.
 *      dev_pose_cov, dev_out_d2, dev_out_second_d2 may be NULL.  A dev_obs that is not 32-byte aligned is GS_ERR_INVALID; an observation whose
 *      pose_of_obs lies outside [0, n_poses) gets -1 (nothing is read through it).
 * gs_frame_frontend_nn: one frame in one launch, as gs_frame_frontend; pose_cov_3x3 may be NULL.
 * Errors (before the device is touched): a null pointer, a parameter that is not finite, gate_chi2 <= 0, max_distance <= 0, a negative sigma,
 *      a wrong struct_size: GS_ERR_INVALID.  A host-only handle: GS_ERR_NO_DEVICE.
 * NOT DONE: the Slam mirror and the shell keep the Euclidean rule; these calls decide every observation on its own, so two observations
 *      of a frame may take the same cone (the one-to-one association below resolves that); no cross-covariance (above); no signed localizer
 *      type test (gs_frame_frontend's signed_type); sharded handles: nothing beyond what the Euclidean calls do (the map and the search are
 *      per handle). */
typedef struct gs_nn_params {
    int32_t struct_size;
    int32_t reserved;
    double gate_chi2;      /* 5.991464547107979: 95 %, 2 dof */
    double max_distance;   /* 3.0 m: Euclidean pre-gate and grid cell */
    double type_tol;       /* 1e-4 */
    double sigma_range;    /* 0.3 m */
    double sigma_bearing;  /* 0.02 rad */
    double sigma_xy;       /* 0.05 m */
} gs_nn_params;
int  gs_nn_params_default(gs_nn_params *p);
int  gs_map_set_cov(gs_graph *g, int32_t first, int32_t n, const double *cov_2x2);
int  gs_map_get_cov(gs_graph *g, int32_t first, int32_t n, double *out_cov_2x2);
int  gs_map_set_cov_from_marginals(gs_graph *g, int32_t first, int32_t n, const int32_t *lm_ids);
int  gs_associate_nn_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses, const int32_t *pose_of_obs, const double *obs_4xn,
                           int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov_2x2, const double *pose_cov_3x3,
                           const gs_nn_params *params, int32_t *out_index, double *out_d2, double *out_second_d2);
int  gs_associate_nn_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                              const double *dev_obs_4xn, const double *dev_pose_cov_3x3, const gs_nn_params *params,
                              int32_t *dev_out_index, double *dev_out_d2, double *dev_out_second_d2);
int  gs_frame_frontend_nn(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                          const gs_nn_params *params, double *out_zxy, double *out_gxy, int32_t *out_index, double *out_d2, double *out_second_d2);

/* ---- one-to-one association: each frame's cones matched by ascending d2 ------------------------------------------
 * The calls above decide every observation on its own, so two observations of one frame can take the same cone — which a lidar frame
 * cannot see twice.  These calls resolve that on the device, where the candidates are (the host only ever sees best and runner-up).
 *
 * Frame.  A frame is a consecutive run of observations [frame_start[f], frame_start[f + 1]).
 * Pair distance.  For observation i and cone j, d2(i, j) and "admissible" are exactly those of the covariance-gated association above:
 *      the same fp64 operations, no contraction.  Nothing about a pair changes.
 * Assignment.  Inside a frame a cone is given to at most one observation and an observation gets at most one cone: the GREEDY matching over
 *      the frame's admissible pairs in ascending order of the key (d2, observation index, cone index).  Walk the pairs in that order; take a
 *      pair when its observation is still unassigned and its cone still unclaimed in this frame.  The observation index in the key is the
 *      position in the call's arrays.  The order is strict and total, so the result is unique and does not depend on how the device gets
 *      there (it takes, round by round, the smallest pair still open).
 * Outputs, per observation.  index = the cone, or -1;  d2 = the d2 of the taken pair, or +inf.  An observation whose query is invalid
 *      (azimuth 0, r == 0, pose index out of range) gets -1 and takes part in nothing.
 * Scope.  Frames are independent: the same cone may be taken in two different frames.
 * Consequences.  In a frame where gs_associate_nn_* returns no cone twice the result equals it in index and d2, bit for bit.  The matching
 *      equals the fixed point of "mutual best" rounds (every unassigned observation proposes its best unclaimed cone by (d2, j); a proposal
 *      (i, c) commits iff no other UNASSIGNED observation i' of the frame — not only those that proposed c — has an admissible d2(i', c)
 *      with (d2, i') below (d2(i, c), i)).
 *
 * gs_assign_nn_batch: the layouts of gs_associate_nn_batch plus frame_start (n_frames + 1 entries): frame_start[0] == 0, ascending (empty
 *      frames allowed), frame_start[n_frames] == n, every frame of at most GS_NN_FRAME_MAX observations — anything else GS_ERR_INVALID
 *      before the device is touched, as are all the refusals of gs_associate_nn_batch.  out_d2 may be NULL.  The search is chosen as there.
 * gs_assign_nn_resident: everything in DEVICE memory against the resident map and its covariances, asynchronous on the handle's stream, no
 *      wait.  dev_pose_cov and dev_out_d2 may be NULL; dev_obs must be 32-byte aligned.  The host cannot see the offsets, so the kernel
 *      defends itself: a frame whose bounds are not 0 <= a <= b <= n reads and writes nothing; a frame longer than GS_NN_FRAME_MAX writes
 *      -1 / +inf for all its observations; OBSERVATIONS THAT NO FRAME COVERS ARE NOT WRITTEN (the outputs keep what they held); an
 *      observation that two frames cover is written by both, in no stated order.
 * gs_frame_frontend_assign: one frame of k <= GS_NN_FRAME_MAX observations in one launch against the resident map (the grid from 2048
 *      cones, brute force below; gs_debug_options.assoc_grid forces either); out_zxy / out_gxy are the bits gs_frame_frontend_nn returns.
 *      k above the cap: GS_ERR_INVALID.  Its staging buffers exist from the first call on and only grow.
 * A handle that never calls any of these allocates and launches nothing for them; the calls above are unchanged by them.
 * NOT DONE: this is NOT the minimum-sum assignment — a greedy matching can be beaten in total d2 (the minimum-cost association below is
 *      that assignment) — and NOT joint compatibility (a test of its own, further below); the Slam mirror and the shell keep the Euclidean lowest-index rule; no cross-covariance; no signed localizer type test; frames of
 *      more than GS_NN_FRAME_MAX observations; sharded handles: nothing beyond what the gs_associate_nn_* calls give. */
#define GS_NN_FRAME_MAX 256
int  gs_assign_nn_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses, const int32_t *pose_of_obs, const double *obs_4xn,
                        int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const int32_t *map_type,
                        const double *map_cov_2x2, const double *pose_cov_3x3, const gs_nn_params *params, int32_t *out_index, double *out_d2);
int  gs_assign_nn_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                           const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                           const gs_nn_params *params, int32_t *dev_out_index, double *dev_out_d2);
int  gs_frame_frontend_assign(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                              const gs_nn_params *params, double *out_zxy, double *out_gxy, int32_t *out_index, double *out_d2);

/* ---- minimum-cost association: a frame's cones matched at least total d2 ------------------------------------------
 * The greedy matching above takes the smallest pair first, so a cone grabbed early can push a neighbour to a worse cone or to none.  These
 * calls return the assignment of smallest total instead.
 *
 * Frames, pair distances, "admissible" and invalid queries are exactly those of the one-to-one association: frame_start, at most
 *      GS_NN_FRAME_MAX observations a frame, d2(i, j) by the same fp64 operations, no contraction.  Nothing about a pair changes.
 * Candidates.  Observation i competes with its GS_ASSIGN_CAND_MAX admissible cones of smallest (d2, cone index).  An observation with more
 *      admissible cones loses the rest: the cut is part of the rule, and n_admissible (below) reports where it applied.
 * Assignment.  Among all matchings of the frame over these candidate pairs — every observation at most one cone, every cone at most one
 *      observation — one that MAXIMISES the total gain  sum (gate_chi2 - d2(i, j))  over its pairs.  That is the same as minimising
 *      sum d2 + gate_chi2 * (unmatched observations): the usual gated assignment with one dummy column of cost gate_chi2 per observation.
 *      d2 < gate_chi2 holds strictly for an admissible pair, so every pair has positive gain and the result is MAXIMAL: no observation is
 *      left at -1 while a cone on its list is free.
 * Ties.  Where two matchings have the same total, which one is returned is not stated; all calls and both searches return the same one.
 *      The duals of the solver are fp64: the returned total is within  48 k^2 2^-53 gate_chi2  of the best (k = the frame's observations).
 * Outputs, per observation.  index = the cone, or -1;  d2 = the pair's d2 (the bits the covariance-gated association computes), or +inf;
 *      n_admissible (optional, int32) = how many admissible cones the search met, NOT capped: a value above GS_ASSIGN_CAND_MAX says that
 *      the cut applied to this observation.  An invalid query gets -1, +inf and 0 and takes part in nothing.
 * Consequences.  In a frame where gs_associate_nn_* returns no cone twice the result equals it in index and d2, bit for bit.  The total
 *      gain is never below that of the greedy matching (ascending (d2, observation, cone)) over the same candidate pairs.
 *
 * gs_assign_opt_batch / gs_assign_opt_resident / gs_frame_frontend_assign_opt: the arguments, layouts, refusals, search choice (the grid from
 *      2048 cones; gs_debug_options.assoc_grid forces either) and the resident kernel's defences of gs_assign_nn_batch /
 *      gs_assign_nn_resident / gs_frame_frontend_assign, plus out_n_admissible (may be NULL).  The defences with it: a frame with bad bounds
 *      reads and writes nothing; a frame longer than GS_NN_FRAME_MAX writes -1, +inf and 0 for all its observations; observations that no
 *      frame covers are not written, in any of the three outputs.
 * A handle that never calls any of these allocates and launches nothing for them; the calls above are unchanged by them.
 * NOT DONE: joint compatibility is a test of its own (below), not part of these calls; no cross-covariance; the Slam mirror and the shell keep the Euclidean lowest-index rule; frames of more than
 *      GS_NN_FRAME_MAX observations; more than GS_ASSIGN_CAND_MAX candidates per observation; no signed localizer type test; sharded
 *      handles: nothing beyond what the gs_associate_nn_* calls give. */
#define GS_ASSIGN_CAND_MAX 8
int  gs_assign_opt_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses, const int32_t *pose_of_obs, const double *obs_4xn,
                         int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const int32_t *map_type,
                         const double *map_cov_2x2, const double *pose_cov_3x3, const gs_nn_params *params, int32_t *out_index, double *out_d2,
                         int32_t *out_n_admissible);
int  gs_assign_opt_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                            const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                            const gs_nn_params *params, int32_t *dev_out_index, double *dev_out_d2, int32_t *dev_out_n_admissible);
int  gs_frame_frontend_assign_opt(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                                  const gs_nn_params *params, double *out_zxy, double *out_gxy, int32_t *out_index, double *out_d2,
                                  int32_t *out_n_admissible);

/* ---- joint compatibility: a frame's matches gated as one hypothesis ------------------------------------------------
 * The calls above gate every pair (i, j) alone: P = G Sigma_p G^T enters each pair's S as if the pose error were drawn afresh for every
 * observation.  All observations of a frame share ONE pose error.  A frame whose residuals all point the same way (a pose error explains
 * it) and one whose residuals contradict each other (nothing does) pass the same per-pair gates when Sigma_p is generous; only the joint
 * test tells them apart, and it yields the pose correction the matches imply.  The reference has no noise model: the rule is build-defined.
 *
 * Frames are those of gs_assign_*: frame_start, at most GS_NN_FRAME_MAX observations each.  A frame carries a HYPOTHESIS index[i] — a cone
 *      or -1 per observation, as any of gs_associate_nn_*, gs_assign_nn_* or gs_assign_opt_* returns it.  All observations of a frame share
 *      one pose index p; Sigma_p = that pose's 3x3 covariance (row-major, the upper triangle read), zero when pose_cov is NULL.
 * Pair.  Observation i with j = index[i] != -1:  z, w = R(theta) z, g, wp = (-w_y, w_x) and Q are exactly those of the covariance-gated
 *      association — the same device function, called WITHOUT a pose covariance, so that its Q + P is Q alone.
 *      D = Sigma_j + Q,  nu = l_j - g,  det = D00 D11 - D01^2,
 *      a_i = (((D11 nu0) nu0 - ((2 D01) nu0) nu1) + (D00 nu1) nu1) / det          the operations of the covariance-gated d2: with pose_cov == NULL
 *                                                                                  a_i is bitwise the d2 gs_associate_nn_* returns for (i, j)
 *      y = D^-1 nu:  y0 = (D11 nu0 - D01 nu1) / det,  y1 = (D00 nu1 - D01 nu0) / det
 *      c_i = (y0, y1, wp_x y0 + wp_y y1)
 *      E = D^-1:  E00 = D11 / det,  E01 = -(D01 / det),  E11 = D00 / det;   h = E wp:  h0 = E00 wp_x + E01 wp_y,  h1 = E01 wp_x + E11 wp_y
 *      M_i = G^T D^-1 G, G = [I2 | wp], symmetric 3x3, six entries:  (E00, E01, h0, E11, h1, wp_x h0 + wp_y h1) = (M00, M01, M02, M11, M12, M22)
 *      The pair enters the set K iff ALL of  the query is valid (as above: g finite, r > 0, pose index in range),  0 <= j < n_map,  det > 0,
 *      D00 > 0  hold (positive tests: any NaN excludes).  Otherwise the observation gets -1 and counts in n_untestable.  No type, distance or
 *      gate test is repeated: the hypothesis is the caller's.  An observation with index[i] == -1 has no pair: it gets -1 and counts nowhere.
 * Sums.  a, c, M over K in a FIXED order: with r = the observation's position in its frame, lane r mod 64 adds its pairs in ascending r
 *      starting from +0; then the 64 lane values are added pairwise at distance 32, 16, 8, 4, 2, 1 (lane l takes l + (l xor d)); a lane
 *      without a pair holds +0.  The sums of a round are formed from the kept pairs afresh, never carried over from the round before.
 * Joint distance.  A = I + M Sigma_p, every entry as ((M_r0 P_0s + M_r1 P_1s) + M_r2 P_2s), 1 added last on the diagonal;  C = the cofactors
 *      of A, each a difference of two products (C00 = A11 A22 - A12 A21, C01 = A12 A20 - A10 A22, C02 = A10 A21 - A11 A20, C10 = A02 A21 -
 *      A01 A22, C11 = A00 A22 - A02 A20, C12 = A01 A20 - A00 A21, C20 = A01 A12 - A02 A11, C21 = A02 A10 - A00 A12, C22 = A00 A11 - A01 A10);
 *      detA = (A00 C00 + A01 C01) + A02 C02  (>= 1 in exact arithmetic);  x_s = ((C0s c0 + C1s c1) + C2s c2) / detA;
 *      delta_r = (P_r0 x0 + P_r1 x1) + P_r2 x2;   J(K) = a - ((c0 delta0 + c1 delta1) + c2 delta2).
 *      In exact arithmetic delta = Sigma_p (I + M Sigma_p)^-1 c and J = nu^T (blockdiag(D) + G Sigma_p G^T)^-1 nu over the stacked pairs.
 *      delta is the correction of (x, y, theta) the kept matches imply, added to the pose as gs_iterate adds its update; the caller may apply
 *      it.  pose_cov == NULL: no solve, delta = 0 and J = a.  No contraction anywhere.
 * Gate.  gs_jc_params.gate[m], m = 0 .. GS_NN_FRAME_MAX: the `confidence` quantile of chi-square with 2 m degrees of freedom, gate[0] = 0,
 *      filled on the host by gs_jc_params_default (0.95) and gs_jc_params_set_confidence (bisection on 1 - e^(-x/2) sum_{k<m} (x/2)^k / k!;
 *      a confidence outside (0, 1): GS_ERR_INVALID).  The device reads the table as given — the rule is defined relative to the table's bits,
 *      a caller may edit it.  A table that is not finite, has a negative entry or decreases somewhere, or a wrong struct_size: GS_ERR_INVALID.
 * Pruning (backward elimination).  While K is not empty and NOT J(K) < gate[|K|]: remove the pair r of smallest J(K \ {r}), exact ties to the
 *      lowest observation; repeat.  J(K \ {r}) is formed from (the round's sums - the pair's own terms), entry by entry, by the same solve.
 * Outputs.  Per observation out_index: the cone while its pair is kept, else -1.  Per frame (each pointer may be NULL): joint_d2 = J of the
 *      kept set (0 when it is empty);  n_kept;  n_dropped = pairs removed by pruning;  n_untestable;  delta[3] (of the kept set).
 *      n_kept + n_dropped + n_untestable = the frame's observations with index != -1.
 * Consequences.  With pose_cov == NULL, J is the fixed-order sum of the pairs' own d2.  A frame with J < gate[m] at once keeps its hypothesis
 *      unchanged, index for index, after ONE round.  Frames are independent.  A cone named twice in a hypothesis is not checked: its two
 *      pairs are treated as independent.  Batch, resident and frame call return identical bits.
 *
 * gs_joint_compat_batch: the host layouts of gs_assign_opt_batch without map_type, plus in_index and the table.  Of gs_nn_params only
 *      struct_size and the three sigmas are read (the other fields may hold anything).  GS_ERR_INVALID before the device is touched:
 *      everything gs_assign_nn_batch refuses about frames and pointers, an in_index entry outside [-1, n_map), a frame whose observations
 *      do not share one pose index, a sigma that is negative or not finite, a bad table.
 * gs_joint_compat_resident: everything in DEVICE memory against the resident map and its covariances, asynchronous on the handle's stream,
 *      no wait.  dev_obs must be 32-byte aligned.  The kernel defends itself as the resident assign kernels do: a frame whose bounds are
 *      not 0 <= a <= b <= n reads and writes nothing; a frame longer than GS_NN_FRAME_MAX writes -1 per observation, joint_d2 = +inf, counts
 *      and delta 0; a frame whose observations name two different pose indices inside [0, n_poses) does the same; an index[i] outside
 *      [-1, map size) makes that pair untestable; observations that no frame covers are not written.
 * gs_frame_frontend_jc: one frame against the resident map — the minimum-cost assignment of gs_frame_frontend_assign_opt (all of
 *      gs_nn_params read and checked as there), then the joint test of its result, enqueued back to back on the handle's stream, one wait.
 *      out_zxy / out_gxy: the bits gs_frame_frontend_nn returns; out_index: the PRUNED index; out_d2 / out_n_admissible (may be NULL): the
 *      assignment's, for every pair it made, pruned or not; then the frame's record.  It shares the assignment call's staging and keeps a
 *      fixed record buffer of its own from the first call on: nothing is allocated per call after that.
 * A handle that never calls any of these allocates and launches nothing for them; the calls above are unchanged by them.
 * NOT DONE: pose-cone and cone-cone cross-covariances; JCBB's search over alternative cones — this PRUNES a given hypothesis, it does not
 *      re-match (a search over alternative cones WITHOUT a prior pose is "relocalisation", further below); the posterior pose covariance (frame localisation, below, returns it); frames of more than GS_NN_FRAME_MAX observations; sharded handles (nothing beyond what the
 *      gs_associate_nn_* calls give); the Slam mirror and the shell, which keep the Euclidean rule. */
typedef struct gs_jc_params {
    int32_t struct_size;
    int32_t reserved;
    double confidence;                      /* 0.95 */
    double gate[GS_NN_FRAME_MAX + 1];       /* gate[m]: the quantile at 2 m degrees of freedom; gate[0] = 0 */
} gs_jc_params;
int  gs_jc_params_default(gs_jc_params *p);
int  gs_jc_params_set_confidence(gs_jc_params *p, double confidence);
int  gs_joint_compat_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses, const int32_t *pose_of_obs, const double *obs_4xn,
                           int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const double *map_cov_2x2,
                           const double *pose_cov_3x3, const gs_nn_params *params, const gs_jc_params *jc, const int32_t *in_index,
                           int32_t *out_index, double *out_joint_d2, int32_t *out_n_kept, int32_t *out_n_dropped, int32_t *out_n_untestable,
                           double *out_delta_3);
int  gs_joint_compat_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                              const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                              const gs_nn_params *params, const gs_jc_params *jc, const int32_t *dev_in_index, int32_t *dev_out_index,
                              double *dev_out_joint_d2, int32_t *dev_out_n_kept, int32_t *dev_out_n_dropped, int32_t *dev_out_n_untestable,
                              double *dev_out_delta_3);
int  gs_frame_frontend_jc(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                          const gs_nn_params *params, const gs_jc_params *jc, double *out_zxy, double *out_gxy, int32_t *out_index, double *out_d2,
                          int32_t *out_n_admissible, double *out_joint_d2, int32_t *out_n_kept, int32_t *out_n_dropped, int32_t *out_n_untestable,
                          double *out_delta_3);

/* ---- frame localisation: iterated pose refinement against the map ------------------------------------------------------
 * The joint test's delta is ONE linear step from the prior pose.  The model is not linear in the heading (w = R(theta) z against w + dtheta wp
 * leaves r dtheta^2 / 2: 5 cm for a cone at 10 m and 0.1 rad), the joint test does not return the posterior covariance, and nothing says how
 * well the frame fits where it ends.  These calls compute the maximum-a-posteriori pose under the prior (x0, Sigma_p) and the frame's pairs
 * by iterated relinearisation on the device (the iterated EKF update: Gauss-Newton on three unknowns per frame), the posterior covariance
 * and the posterior chi2.  The reference has no noise model: the rule is build-defined.
 *
 * Frames, the hypothesis in_index (a cone or -1 per observation) and the pose are those of gs_joint_compat_*: all observations of a frame share
 *      one pose index; x0 = (t0, theta0) = that pose, Sigma_p = its 3x3 covariance (row-major, the upper triangle read).
 * Iterate.  d_0 = (+0, +0, +0).  x_0 = x0 itself; for k > 0  x_k = (t0 + d_k[0:2], theta0 + d_k[2]), NOT normalised (sincos is periodic).
 * Pair terms at x_k.  Observation i with j = in_index[i] != -1:  z by the A0 formula (it does not depend on k);  w = R(theta_k) z, g = w + t_k,
 *      wp = (-w_y, w_x) and Q exactly as the covariance-gated association forms them from the pose x_k WITHOUT a pose covariance — with k = 0 the
 *      bits the joint test uses;  D = Sigma_j + Q, nu = l_j - g, det, y, E, h, c_i and M_i exactly as listed under "joint compatibility".
 *      The pair COUNTS in iteration k iff ALL of  the query is valid (g finite, r > 0, pose index in range),  0 <= j < n_map,  det > 0,  D00 > 0,
 *      nu finite (a cone whose position is not finite never counts)  hold (positive tests, taken again in every iteration).  A pair that does
 *      not count contributes +0.
 * Sums.  c, M and the count m_k in the joint test's fixed order: lane r mod 64 adds its pairs in ascending r from +0, then the butterfly at
 *      distance 32, 16, 8, 4, 2, 1.
 * Right-hand side.  k = 0: b = c.  k > 0: b_r = c_r + ((M_r0 d_k0 + M_r1 d_k1) + M_r2 d_k2).
 * Solve.  The joint test's operations with b in place of c:  A = I + M Sigma_p, the nine cofactors C, detA = (A00 C00 + A01 C01) + A02 C02,
 *      x_s = ((C0s b0 + C1s b1) + C2s b2) / detA,  d_{k+1,r} = (P_r0 x0 + P_r1 x1) + P_r2 x2.  In exact arithmetic d_{k+1} = (Sigma_p^-1 + M)^-1
 *      (c + M d_k): the Gauss-Newton step of |x - x0|^2_{Sigma_p^-1} + sum |nu_i(x)|^2_{D_i^-1}, written so that Sigma_p is never inverted and
 *      may be singular or very wide.
 * Stop.  Converged iff ALL of |d_{k+1,0} - d_k0| <= tol_xy, |d_{k+1,1} - d_k1| <= tol_xy, |d_{k+1,2} - d_k2| <= tol_theta hold (positive
 *      tests).  Otherwise the next iteration runs, until max_iterations solves have been made.  No host decision between iterations.
 * Final pass at x_f = x0 + d_f, d_f = the last d (x_f = x0 itself when no solve was made): the pair terms once more, with
 *      a_i = (((D11 nu0) nu0 - ((2 D01) nu0) nu1) + (D00 nu1) nu1) / det, summed with M and the count as above;  A, C, detA of this pass;
 *      cov_rs = ((P_r0 C_s0 + P_r1 C_s1) + P_r2 C_s2) / detA for r <= s, mirrored  (exactly: Sigma_p (I + M Sigma_p)^-1 = (Sigma_p^-1 + M)^-1);
 *      chi2 = a + ((x0 d_f0 + x1 d_f1) + x2 d_f2), x of the LAST solve (the second term is d_f^T Sigma_p^-1 d_f without an inverse); it has
 *      2 n_pairs degrees of freedom: hold it against gs_jc_params.gate[n_pairs];
 *      pose = (t0x + d_f0, t0y + d_f1, normalize_theta(theta0 + d_f2)) — gs_iterate's addition and normalisation;
 *      n_pairs = the pairs counted in this pass;  iterations = the solves made.
 * Status.  0 converged.  1 the iteration limit was reached.  2 no pair counted in iteration 0: pose = x0's bits, cov = Sigma_p's (upper triangle,
 *      mirrored), chi2 0, n_pairs 0, iterations 0 — an EMPTY frame has no pose: zeros.  3 some d or detA (of a solve or of the final pass) was
 *      not finite: pose and cov as for 2, chi2 +inf, n_pairs 0.  4 the frame was refused (resident defences): zeros, chi2 +inf, counts 0.
 *      pose_cov == NULL: the prior has zero covariance; no solve: status 0, iterations 0, pose = (t0, normalize_theta(theta0)), cov zeros,
 *      chi2 = a at x0 (the fixed-order sum of the bits gs_associate_nn_* returns as d2 for the pairs), n_pairs as counted.
 * Outputs per frame, each pointer may be NULL: out_pose[3], out_cov[9], out_chi2, out_n_pairs, out_iterations, out_status.  No contraction anywhere.
 * Consequences.  With max_iterations = 1, d_f is BITWISE the delta of gs_joint_compat_* for a hypothesis that call keeps whole.  A frame's
 *      result does not depend on the lanes it was given, on the kernel, or on its neighbours in the wave.  Batch, resident and frame call return
 *      identical bits (the frame call with k == 0 makes no launch and returns status 2 with the GIVEN pose and covariance).
 *
 * gs_localize_batch: the host layouts of gs_joint_compat_batch (of gs_nn_params only struct_size and the three sigmas are read).  GS_ERR_INVALID
 *      before the device is touched: everything gs_joint_compat_batch refuses, a wrong gs_loc_params.struct_size, max_iterations outside
 *      1 .. GS_LOC_ITER_MAX, a tolerance that is negative or not finite.  A host-only handle: GS_ERR_NO_DEVICE.
 * gs_localize_resident: everything in DEVICE memory against the resident map and its covariances, asynchronous on the handle's stream, no wait.
 *      dev_obs must be 32-byte aligned.  A frame whose bounds are not 0 <= a <= b <= n reads and writes nothing; a frame longer than
 *      GS_NN_FRAME_MAX, or one whose observations name two different pose indices inside [0, n_poses), gets status 4; an index[i] outside
 *      [-1, map size) is a pair that never counts; nothing is written per observation.
 * gs_frame_frontend_localize: gs_frame_frontend_jc (same arguments, same outputs, same bits), then the localisation under the PRUNED index,
 *      enqueued back to back on the handle's stream, one wait.  It shares the assignment call's staging and keeps a fixed record buffer of its
 *      own from the first call on.  To chain frames, the caller adds its motion noise to out_cov before it is the next frame's pose_cov.
 *      gs_follow_* and gs_frame_frontend_follow ("frame following", below) do that chaining on the device, for up to 64 poses at once.
 * A handle that never calls any of these allocates and launches nothing for them; the calls above are unchanged by them.
 * NOT DONE: the Slam mirror and the shell stay as they are (the reference's localizer reports the raw odometry pose); no prior-free (maximum-
 *      likelihood) solve — a wide Sigma_p serves, and "relocalisation" (below) finds a pose from the frame and the map alone; no cross-covariances;
 *      no re-matching (the hypothesis is the caller's throughout; relocalisation, below, searches the cones for one); no sharded
 *      handles; no frames above GS_NN_FRAME_MAX observations. */
#define GS_LOC_ITER_MAX 16
typedef struct gs_loc_params {
    int32_t struct_size;
    int32_t max_iterations;                 /* 5; 1 .. GS_LOC_ITER_MAX */
    double tol_xy;                          /* 1e-6 m */
    double tol_theta;                       /* 1e-8 rad */
} gs_loc_params;
int  gs_loc_params_default(gs_loc_params *p);
int  gs_localize_batch(gs_graph *g, int32_t n, const double *poses_xytheta, int32_t n_poses, const int32_t *pose_of_obs, const double *obs_4xn,
                       int32_t n_frames, const int32_t *frame_start, int32_t n_map, const double *map_xy, const double *map_cov_2x2,
                       const double *pose_cov_3x3, const gs_nn_params *params, const gs_loc_params *loc, const int32_t *in_index,
                       double *out_pose_3, double *out_cov_3x3, double *out_chi2, int32_t *out_n_pairs, int32_t *out_iterations, int32_t *out_status);
int  gs_localize_resident(gs_graph *g, int32_t n, const double *dev_poses_xytheta, int32_t n_poses, const int32_t *dev_pose_of_obs,
                          const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start, const double *dev_pose_cov_3x3,
                          const gs_nn_params *params, const gs_loc_params *loc, const int32_t *dev_in_index, double *dev_out_pose_3,
                          double *dev_out_cov_3x3, double *dev_out_chi2, int32_t *dev_out_n_pairs, int32_t *dev_out_iterations, int32_t *dev_out_status);
int  gs_frame_frontend_localize(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                                const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, double *out_zxy, double *out_gxy,
                                int32_t *out_index, double *out_d2, int32_t *out_n_admissible, double *out_joint_d2, int32_t *out_n_kept,
                                int32_t *out_n_dropped, int32_t *out_n_untestable, double *out_delta_3, double *out_pose_3, double *out_cov_3x3,
                                double *out_chi2, int32_t *out_n_pairs, int32_t *out_iterations, int32_t *out_status);

/* ---- relocalisation: a frame's pose found on the map without a prior ---------------------------------------------------
 * Every call above starts from a pose that is roughly right: max_distance and the chi-square gate only admit a cone near where the prior puts
 * it.  After a restart on a saved map, a GPS jump, a spin or drift at the loop closure the prior is wrong and the chain matches nothing, or
 * the neighbouring cones of a self-similar track.  These calls find, from ONE frame and the map alone, the rigid pose under which the most
 * observations land on type-compatible cones, and report the best count at a clearly DIFFERENT pose, because tracks repeat themselves and
 * the caller must be able to see that.  The reference's localizer (src/slam.cpp:340-414) trusts the odometry pose: the rule is build-defined.
 * No contraction anywhere; only + - * / sqrt and comparisons, up to the one final atan2.
 *
 * Frames and observations.  Frames are runs of observations (frame_start), at most GS_NN_FRAME_MAX each, collector layout 4 x n.  z_i = the
 *      CoG-frame XY by the A0 formula (quirks included), r2_i = zx zx + zy zy, ty_i = the type.  An observation is VALID iff zx and zy are
 *      finite and r2 > 0.  No pose is read: there is no poses or pose_of_obs argument.
 * Seed observations.  The frame's valid observations with the seed_obs smallest keys (r2, index): the closest cones are the best measured.
 * Seed pairs.  All (u, v) with u < v (positions in the call's arrays) among the seed observations:  dz = z_v - z_u,
 *      L2 = (dzx dzx) + (dzy dzy),  L = sqrt(L2).  The pair is kept iff L >= min_baseline.
 * Seeds.  For every kept (u, v), every ordered map pair (p, q), p != q, with |type_p - ty_u| < type_tol and |type_q - ty_v| < type_tol:
 *      dl = l_q - l_p,  M2 = (dlx dlx) + (dly dly),  M = sqrt(M2);  the lengths must match: |M - L| <= length_tol.  Then
 *      den = sqrt(L2 M2),  c = ((dzx dlx) + (dzy dly)) / den,  s = ((dzx dly) - (dzy dlx)) / den,
 *      mz = (0.5 (zx_u + zx_v), 0.5 (zy_u + zy_v)),  ml = (0.5 (lx_p + lx_q), 0.5 (ly_p + ly_q)),
 *      t = (mlx - ((c mzx) - (s mzy)),  mly - ((s mzx) + (c mzy))).
 *      The seed EXISTS iff den > 0 and c, s, tx, ty are all finite.  All tests are positive tests: a NaN cone or query takes part in nothing.
 * Score of a seed.  For every valid observation i of the frame (not only the seed observations), in ascending i:
 *      w = (((c zx) - (s zy)) + tx,  ((s zx) + (c zy)) + ty);  among the cones j with |type_j - ty_i| < type_tol the one of smallest
 *      e2 = (ex ex) + (ey ey), ex = lx - wx, ey = ly - wy, exact ties to the lowest j;  i is an INLIER iff that e2 < inlier_radius inlier_radius
 *      (the product formed once, on the host).  count = the inliers;  cost = their e2 added from +0 in ascending i.
 *      A cone may serve two observations: uniqueness is the job of the assignment calls that follow, not of the score.
 * Winner.  The seed with the smallest key (-count, cost, u, v, p, q).  The key is strict and total: the result does not depend on how the
 *      device gets there.
 * Runner-up.  The smallest key among the seeds that are NOT NEAR the winner (c*, s*, t*).  A seed is near iff
 *      ((dx dx) + (dy dy)) < distinct_xy distinct_xy, dx = tx - tx*, dy = ty - ty*,  AND  ((c c*) + (s s*)) > distinct_cos.
 *      The angle is passed as a cosine so that no libm call sits between the caller's number and the comparison.
 * Outputs per frame, each pointer may be NULL:  pose[3] = (tx, ty, atan2(s, c));  count;  cost;  seed[4] = (u, v, p, q);
 *      second_count and second_pose[3] (0 and zeros when there is none);  n_seeds (int64) = the seeds that existed;  status:
 *      0 found, count >= min_inliers.  1 the best seed is below min_inliers; the record is written all the same.  2 no seed: pose zeros, counts
 *      0, cost +inf, seed (-1, -1, -1, -1).  4 refused (resident defences): as 2.
 * Outputs per observation (may be NULL):  index = the inlier's cone under the winner, else -1;  e2 = its e2, else +inf.
 * Consequences.  Frames are independent.  Batch, resident and frame call, with either scoring search, return identical bits.
 *
 * gs_reloc_params_default fills the struct.  Refused (GS_ERR_INVALID) before the device is touched: a wrong struct_size; seed_obs outside
 *      2 .. GS_RELOC_SEED_MAX; min_inliers < 2; min_baseline, length_tol, inlier_radius or distinct_xy not finite or not positive; type_tol not
 *      finite; distinct_cos outside [-1, 1].
 * gs_relocalize_batch: host arrays; frame_start as gs_assign_nn_batch checks it (begins at 0, ascends, ends at n, no frame above
 *      GS_NN_FRAME_MAX).  The score searches the hashed grid (cell edge from inlier_radius, nine buckets) from 2048 cones and the whole map
 *      below; gs_debug_options.assoc_grid forces either.  A host-only handle: GS_ERR_NO_DEVICE.
 * gs_relocalize_resident: everything in DEVICE memory against the resident map, asynchronous on the handle's stream, no wait.  dev_obs must
 *      be 32-byte aligned.  The kernels defend themselves: a frame whose bounds are not 0 <= a <= b <= n reads and writes nothing; a frame
 *      above GS_NN_FRAME_MAX gets status 4 and -1 / +inf per observation; observations that no frame covers are not written.  The grid (a
 *      second one beside the association's, so that the two cell edges do not evict each other) is used unless assoc_grid == 0.
 * gs_frame_frontend_relocalize: one frame: the search, then the chain of gs_frame_frontend_localize (assignment -> joint test ->
 *      localisation) from the found pose under the prior covariance diag(prior_sigma_xy^2, prior_sigma_xy^2, prior_sigma_theta^2) — all
 *      enqueued back to back, one wait: the search's last kernel writes the pose into the frame record the chain reads.  It returns the search
 *      record and every output of gs_frame_frontend_localize, bitwise what that call returns for the returned pose and this prior.  With
 *      status 2 the search's last kernel EMPTIES the frame the chain reads, so the chain touches no observation: its per-observation outputs are
 *      then zeros / -1 / +inf / 0 and its records those of an empty frame.  k == 0: nothing is launched, status 2.  k above GS_NN_FRAME_MAX,
 *      a sigma that is negative or not finite: GS_ERR_INVALID.  pose and second_pose are what gs_follow_set / gs_follow_batch ("frame
 *      following", below) take as two hypotheses: the next frames decide between them.
 * A handle that never calls any of these allocates and launches nothing for them; the calls above are unchanged by them.  The record buffers
 *      exist from the first call on and only grow.
 * NOT DONE: one-to-one inside the score (above); cross-covariances; pruning the map-pair enumeration with a coarse grid (every ordered cone
 *      pair is met: n_map^2 length tests a frame); the Slam mirror and the shell; sharded handles; frames above GS_NN_FRAME_MAX. */
#define GS_RELOC_SEED_MAX 16
typedef struct gs_reloc_params {
    int32_t struct_size;
    int32_t seed_obs;        /* 12; 2 .. GS_RELOC_SEED_MAX */
    int32_t min_inliers;     /* 4; >= 2 */
    int32_t reserved;
    double min_baseline;     /* 2.0 m */
    double length_tol;       /* 0.3 m */
    double inlier_radius;    /* 0.5 m */
    double type_tol;         /* 1e-4 */
    double distinct_xy;      /* 2.0 m */
    double distinct_cos;     /* 0.98006657784124163 = cos 0.2 */
} gs_reloc_params;
int  gs_reloc_params_default(gs_reloc_params *p);
int  gs_relocalize_batch(gs_graph *g, int32_t n, const double *obs_4xn, int32_t n_frames, const int32_t *frame_start, int32_t n_map,
                         const double *map_xy, const int32_t *map_type, const gs_reloc_params *params, double *out_pose_3, int32_t *out_count,
                         double *out_cost, int32_t *out_seed_4, int32_t *out_second_count, double *out_second_pose_3, int64_t *out_n_seeds,
                         int32_t *out_status, int32_t *out_index, double *out_e2);
int  gs_relocalize_resident(gs_graph *g, int32_t n, const double *dev_obs_4xn, int32_t n_frames, const int32_t *dev_frame_start,
                            const gs_reloc_params *params, double *dev_out_pose_3, int32_t *dev_out_count, double *dev_out_cost,
                            int32_t *dev_out_seed_4, int32_t *dev_out_second_count, double *dev_out_second_pose_3, int64_t *dev_out_n_seeds,
                            int32_t *dev_out_status, int32_t *dev_out_index, double *dev_out_e2);
int  gs_frame_frontend_relocalize(gs_graph *g, const double *obs_4xk, int32_t k, const gs_reloc_params *reloc, double prior_sigma_xy,
                                  double prior_sigma_theta, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                                  double *out_reloc_pose_3, int32_t *out_reloc_count, double *out_reloc_cost, int32_t *out_reloc_seed_4,
                                  int32_t *out_second_count, double *out_second_pose_3, int64_t *out_n_seeds, int32_t *out_reloc_status,
                                  int32_t *out_reloc_index, double *out_reloc_e2, double *out_zxy, double *out_gxy, int32_t *out_index,
                                  double *out_d2, int32_t *out_n_admissible, double *out_joint_d2, int32_t *out_n_kept, int32_t *out_n_dropped,
                                  int32_t *out_n_untestable, double *out_delta_3, double *out_pose_3, double *out_cov_3x3, double *out_chi2,
                                  int32_t *out_n_pairs, int32_t *out_iterations, int32_t *out_status);

/* ---- frame following: pose hypotheses carried from frame to frame on the device ----------------------------------------------------
 * Every call above treats a frame as an island.  These calls carry n_hyp pose hypotheses (1 .. GS_FOLLOW_HYP_MAX) through a run of frames
 * without a host decision between the frames: per step a motion prediction, the chain minimum-cost assignment -> joint test -> localisation
 * once per hypothesis, and an update that accepts or rejects the fit, counts, and retires hypotheses that lost the map or converged onto a
 * lower-numbered one.  It is the reference's localizer (src/slam.cpp:340-414) with a noise model, and the consumer of relocalisation's
 * pose / second_pose: a wrong place on a self-similar track stops matching once the car has moved.  No contraction anywhere: every product
 * and sum below is rounded once, in the order the parentheses give.
 *
 * Inputs.  n_hyp poses (x, y, theta) and 3x3 covariances (row-major, the upper triangle read; covs == NULL: zeros).  n_steps frames as runs of
 *      observations (frame_start, n_steps + 1 bounds, collector layout 4 x n), at most GS_NN_FRAME_MAX each, an empty frame is legal.
 *      n_steps - 1 motion records u = (ux, uy, utheta): record t - 1 is the step from frame t - 1 to frame t in the body frame of t - 1 (the
 *      measurement of an odometry edge), and per record a 3x3 covariance Qu in that body frame (upper triangle read; motion_cov == NULL: zeros).
 * State per hypothesis (gs_follow_state): pose, cov (full, symmetric), hits = the n_pairs of the accepted steps summed, sum_chi2 = their chi2
 *      added from +0 in step order, frames_hit, frames_missed, misses = the current run of missed frames, state (0 tracking, 1 lost,
 *      2 duplicate), state_step (the step that retired it, -1 while tracking), duplicate_of (-1 unless a duplicate).  At the start: the given
 *      pose's bits, the given covariance with its upper triangle mirrored, every counter 0, tracking.
 * Prior of step t, per tracking hypothesis with state (x, y, theta, P).  t == 0 (no motion record): the state's bits.  t > 0:
 *      (s, c) = sincos(theta), the device call the association's query side makes;  p = (c ux) - (s uy),  q = (s ux) + (c uy);
 *      x- = x + p,  y- = y + q,  theta- = normalize_theta(theta + utheta) — gs_iterate's normalisation (the floor form, no libm);
 *      with a = -q, b = p:   S00 = (P00 + a P02) + a (P02 + a P22)      S01 = (P01 + a P12) + b (P02 + a P22)      S02 = P02 + a P22
 *                            S11 = (P11 + b P12) + b (P12 + b P22)      S12 = P12 + b P22                          S22 = P22
 *      (F P F^T, F = [1 0 a; 0 1 b; 0 0 1]);  W Qu W^T, W = blockdiag(R(theta), 1) (all zeros with motion_cov == NULL):
 *                            N00 = c (c q00 - s q01) - s (c q01 - s q11)      N01 = s (c q00 - s q01) + c (c q01 - s q11)
 *                            N11 = s (s q00 + c q01) + c (s q01 + c q11)      N02 = c q02 - s q12      N12 = s q02 + c q12      N22 = q22
 *      Sigma- = S + N entry by entry, upper triangle, mirrored.
 * Chain of step t.  All n_hyp hypotheses at once, each a frame of its own holding the step's observations: the minimum-cost assignment with
 *      pose = prior and pose_cov = Sigma- (ALWAYS an array, zeros where nothing was given: localisation then solves, it does not take its
 *      pose_cov == NULL path), the joint test of its result, the localisation under the pruned index.  Per hypothesis the results are bitwise
 *      what gs_assign_opt_* -> gs_joint_compat_* -> gs_localize_* return for that prior and that frame.  An EMPTY frame launches no chain:
 *      its record is pose = the prior's bits, cov = Sigma-, chi2 0, n_pairs 0, iterations 0, status 2, n_kept 0.
 * Update, per tracking hypothesis.  ACCEPTED iff ALL of  status <= 1,  n_pairs >= min_pairs,  chi2 <= gs_jc_params.gate[n_pairs]  hold
 *      (positive tests: a NaN fails).  Accepted: pose, cov = the posterior; hits += n_pairs; sum_chi2 = sum_chi2 + chi2; frames_hit += 1;
 *      misses = 0.  Otherwise: pose, cov = the prior (dead reckoning); frames_missed += 1; misses += 1; if misses >= max_misses: state = 1,
 *      state_step = t.
 * Duplicates, after every update of the step, for h = 1, 2, ... in ascending order.  Hypothesis h, if it tracks, becomes a duplicate of the
 *      SMALLEST d < h that tracks (and was not made a duplicate earlier in this pass) with BOTH
 *      ((dx dx) + (dy dy)) < merge_xy merge_xy  (dx = x_h - x_d, dy = y_h - y_d; the right side formed once, on the host)  and
 *      |normalize_theta(theta_h - theta_d)| < merge_theta:  state = 2, duplicate_of = d, state_step = t.  The rule is sequential: a
 *      hypothesis retired in this step or before is compared with nobody.  merge_xy == 0 switches the pass off.
 * Retired hypotheses are frozen: no prediction, no update.  Their step records repeat the frozen pose and covariance as prior and posterior,
 *      with chi2 0, n_pairs 0, iterations 0, status -1, n_kept 0, accepted 0; their pruned index is -1.
 * Best.  The tracking hypothesis of smallest key (-hits, sum_chi2, h); -1 when none tracks.  n_tracking = how many track.
 * Outputs, each pointer may be NULL.  out_steps[t n_hyp + h] (gs_follow_step): the prior, the chain's record as it came (also when it was
 *      rejected), accepted, and the state after the step's duplicate pass.  out_index[h n + i]: observation i's cone under hypothesis h after
 *      the joint test, or -1.  out_state[h]: the state after the last step.  out_best, out_n_tracking.
 * Consequences.  A hypothesis does not depend on its neighbours except through the duplicate pass: with merge_xy = 0, n_hyp hypotheses in
 *      one call equal each of them alone.  Batch, resident and a sequence of frame calls return identical bits, with either search.
 *
 * gs_follow_params_default fills the struct.  Refused (GS_ERR_INVALID) before the device is touched, by every call below: a wrong struct_size
 *      of any of the four parameter blocks and whatever the chain's calls refuse of them; min_pairs < 1; max_misses < 1; a merge value that
 *      is negative or not finite; n_hyp outside 1 .. GS_FOLLOW_HYP_MAX.  A host-only handle: GS_ERR_NO_DEVICE.
 * gs_follow_batch: host arrays, the map as gs_localize_batch takes it plus map_type; frame_start as gs_assign_nn_batch checks it.  Everything
 *      is uploaded once, all steps are enqueued back to back on the handle's stream, one wait.  The search as gs_assign_opt_batch chooses it.
 * gs_follow_resident: everything in DEVICE memory against the resident map, asynchronous on the handle's stream, no wait.  dev_obs must be
 *      32-byte aligned.  frame_cap (0 .. GS_NN_FRAME_MAX): the caller's bound on a frame's size — the host does not see dev_frame_start; it
 *      sizes the buffers and chooses the chain's kernels, never a result.  The kernels defend themselves: a step whose bounds are not
 *      0 <= a <= b <= n, or whose frame is above frame_cap, is no step: nothing of it is read, no state changes and no output of it is written.
 *      dev_out_best_2: {best, n_tracking}.
 * gs_follow_set / gs_frame_frontend_follow / gs_follow_get: the live run.  gs_follow_set puts n_hyp hypotheses on the handle (one wait);
 *      each gs_frame_frontend_follow is one step on them, one wait, and returns that step's records (out_steps[n_hyp], out_index[h k + i]);
 *      gs_follow_get reads the state.  motion must be NULL on the first frame after gs_follow_set ("no prediction") and given on every later
 *      one; motion_cov may be NULL.  k above GS_NN_FRAME_MAX, a frame call or a get before gs_follow_set: GS_ERR_INVALID.  A sequence of
 *      these calls returns bitwise the records of gs_follow_batch over the same frames.
 * Per step: two dispatches of its own (gs_follow.hip: the prediction with the frame laid out once per hypothesis; the update) around the
 *      chain's three to six.  The stage and chain buffers (at most 64 x 256 observations) are allocated at the first call and only grow;
 *      stream order makes their reuse from step to step safe.  A handle that never calls any of these allocates and launches nothing for
 *      them; the calls above are unchanged by them.
 * NOT DONE: one fused kernel per hypothesis for the whole chain; branching (no re-matching, no hypotheses spawned on the device); feeding
 *      relocalisation's result in automatically (the caller passes pose and second_pose); the Slam mirror and the shell; cross-covariances;
 *      frames above GS_NN_FRAME_MAX; sharded handles; hipGraph capture of the step sequence. */
#define GS_FOLLOW_HYP_MAX 64
typedef struct gs_follow_params {
    int32_t struct_size;
    int32_t min_pairs;       /* 3; >= 1 */
    int32_t max_misses;      /* 3; >= 1 */
    int32_t reserved;
    double merge_xy;         /* 0.5 m; 0 switches the duplicate pass off */
    double merge_theta;      /* 0.1 rad */
} gs_follow_params;
typedef struct gs_follow_state {
    double pose[3];
    double cov[9];
    double sum_chi2;
    int32_t hits, frames_hit, frames_missed, misses;
    int32_t state;           /* 0 tracking, 1 lost, 2 duplicate */
    int32_t state_step;      /* -1 while tracking */
    int32_t duplicate_of;    /* -1 unless a duplicate */
    int32_t reserved;
} gs_follow_state;
typedef struct gs_follow_step {
    double prior_pose[3];
    double prior_cov[9];
    double pose[3];
    double cov[9];
    double chi2;
    int32_t n_pairs, iterations, status;    /* of the localisation; status -1: the hypothesis was retired before this step */
    int32_t n_kept;                         /* of the joint test */
    int32_t accepted;                       /* 0 / 1 */
    int32_t state;                          /* after the step */
} gs_follow_step;
int  gs_follow_params_default(gs_follow_params *p);
int  gs_follow_batch(gs_graph *g, int32_t n_hyp, const double *poses_xytheta, const double *covs_3x3, int32_t n_steps, int32_t n, const double *obs_4xn,
                     const int32_t *frame_start, const double *motion_3, const double *motion_cov_3x3, int32_t n_map, const double *map_xy,
                     const int32_t *map_type, const double *map_cov_2x2, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                     const gs_follow_params *follow, gs_follow_step *out_steps, int32_t *out_index, gs_follow_state *out_state, int32_t *out_best,
                     int32_t *out_n_tracking);
int  gs_follow_resident(gs_graph *g, int32_t n_hyp, const double *dev_poses_xytheta, const double *dev_covs_3x3, int32_t n_steps, int32_t n,
                        const double *dev_obs_4xn, const int32_t *dev_frame_start, int32_t frame_cap, const double *dev_motion_3,
                        const double *dev_motion_cov_3x3, const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc,
                        const gs_follow_params *follow, gs_follow_step *dev_out_steps, int32_t *dev_out_index, gs_follow_state *dev_out_state,
                        int32_t *dev_out_best_2);
int  gs_follow_set(gs_graph *g, int32_t n_hyp, const double *poses_xytheta, const double *covs_3x3);
int  gs_follow_get(gs_graph *g, gs_follow_state *out_state, int32_t *out_n_hyp, int32_t *out_best, int32_t *out_n_tracking);
int  gs_frame_frontend_follow(gs_graph *g, const double *motion_3, const double *motion_cov_3x3, const double *obs_4xk, int32_t k,
                              const gs_nn_params *params, const gs_jc_params *jc, const gs_loc_params *loc, const gs_follow_params *follow,
                              gs_follow_step *out_steps, int32_t *out_index, int32_t *out_best, int32_t *out_n_tracking);

/* ---- cone candidates: unmatched observations tracked into new map cones --------------------------------------------------------------
 * Every call above works against a finished map and returns -1 for an observation that no map cone explains.  These calls consume that -1:
 * a table of GS_CAND_MAX tentative cones on the device, into which such observations are fused or spawn an entry; an entry is confirmed
 * after enough sightings and retired after enough misses while it should have been visible; confirmed entries are handed to the caller,
 * who appends them to the map and the graph.  The reference's addConesToMap (src/slam.cpp:608-623) makes a map cone and a vertex of an
 * unmatched observation inside coneMappingThreshold on first sight, without a second look or a way back.  The rule is build-defined.  No
 * contraction anywhere: every product and sum below is rounded once, in the order the parentheses give.
 *
 * Table.  GS_CAND_MAX slots, stored as a map is stored (xy [2], type, cov [4] per slot) so that the association takes it as one, and a
 *      record (gs_cand) per slot that repeats those bits and adds: id (a serial number, unique over the table's life), state (0 free,
 *      1 tentative, 2 confirmed), hits, misses (the current run of misses), first_step, last_step, confirm_step (-1 until confirmed).  A FREE
 *      slot is xy = (NaN, NaN), type 0, cov 0, id -1, every counter 0, confirm_step -1: no admissibility test of the covariance-gated
 *      association holds for it.  The table also holds next_id and the step counter t.  Loading n_in records (gs_cand_set, the initial table
 *      of a batch or resident run) puts record s into slot s as it is — a record of state 0 becomes a free slot whatever else it holds — and
 *      frees the rest; next_id = 1 + the largest id and t = 1 + the largest last_step over the loaded records that are not free, 0 without one.
 * Step t.  One frame of k <= GS_NN_FRAME_MAX observations (collector layout 4 x k), a pose x = (tx, ty, theta), its covariance Sigma_p (NULL:
 *      none) and in_idx[i], the map cone that explains observation i (-1: none; in_idx == NULL: nothing is explained).
 *   1. Unexplained: U = { i : in_idx[i] < 0 }.
 *   2. Association.  The minimum-cost association above over this one frame, with the table AS IT STOOD BEFORE THE STEP as the map
 *      (n_map = GS_CAND_MAX, its cov array, brute force), the pose and Sigma_p of the step, and the azimuth of every observation outside U
 *      replaced by NaN (an invalid query: -1).  slot[i] and n_admissible[i] are bitwise what gs_assign_opt_batch returns for those arrays.
 *   3. Fusion, for every i with slot[i] = c >= 0.  g and A = Q + P are the query's of the covariance-gated association (Sigma_p NULL: A = Q);
 *      l = the slot's xy, C00 C01 C11 = its cov [0] [1] [3]:
 *            S00 = C00 + A00   S01 = C01 + A01   S11 = C11 + A11      det = (S00 S11) - (S01 S01)      n0 = gx - lx   n1 = gy - ly
 *            K00 = ((C00 S11) - (C01 S01)) / det      K01 = ((C01 S00) - (C00 S01)) / det
 *            K10 = ((C01 S11) - (C11 S01)) / det      K11 = ((C11 S00) - (C01 S01)) / det
 *            lx+ = lx + ((K00 n0) + (K01 n1))         ly+ = ly + ((K10 n0) + (K11 n1))
 *            C00+ = (K00 A00) + (K01 A01)             C01+ = (K00 A01) + (K01 A11)             C11+ = (K10 A01) + (K11 A11)
 *      (K = C S^-1, C+ = K A = the parallel sum C S^-1 A: no C - K C cancellation); cov+ = (C00+, C01+, C01+, C11+), the 01 entry formed once.
 *      hits += 1, misses = 0, last_step = t.  (An assigned pair is admissible, so det > 0 holds.)
 *   4. Misses, for every slot that is not free and was not fused in this step.  (s, c) = sincos(theta), the device call the association's
 *      query side makes;  ex = lx - tx,  ey = ly - ty;  dx = (c ex) + (s ey),  dy = (c ey) - (s ex);  r2 = (dx dx) + (dy dy).  The slot is
 *      VISIBLE iff BOTH  r2 < view_range view_range  (the right side formed once, on the host)  and  dx >= view_cos sqrt(r2)  hold (positive
 *      tests: a NaN fails).  Visible: misses += 1, and a TENTATIVE slot with misses >= max_misses becomes free.  A confirmed slot never
 *      retires.  A slot that is not visible is left alone.
 *   5. Confirmation.  A tentative slot (not retired in 4) with hits >= confirm_hits: state = 2, confirm_step = t.
 *   6. Spawning.  i in U with a valid query, slot[i] = -1 and n_admissible[i] == 0 SPAWNS iff its distance column < spawn_range (the
 *      reference's coneMappingThreshold test; positive: a NaN fails), else it is FAR.  Spawners are ranked in ascending observation index;
 *      rank r takes the r-th slot, in ascending slot index, of those that were FREE AT THE START OF THE STEP (a slot retired in 4 is reusable
 *      from the next step on).  The slot gets xy = g, cov = (A00, A01, A01, A11), type = (int) the observation's type (the C conversion of
 *      gs_slam's addConesToMap), id = next_id + r, hits 1, misses 0, first_step = last_step = t, state 1 and confirm_step -1 — or state 2 and
 *      confirm_step = t when confirm_hits == 1.  Spawners beyond the free slots are DROPPED.  next_id += the slots taken.
 *      i in U with a valid query, slot[i] = -1 and n_admissible[i] > 0 is CONTESTED: it neither fuses nor spawns.  An invalid query (g not
 *      finite, or r == 0) does nothing and is counted in none of fused, spawned, contested, far, dropped.
 *   7. Outputs.  out_cand_id[i] / out_cand_slot[i]: the id and the slot fused with or spawned into, else -1 / -1.  gs_cand_step: step = t,
 *      n_unexplained = |U|, n_fused, n_spawned (slots taken), n_contested, n_far, n_dropped, n_missed (visible slots of 4), n_retired,
 *      n_confirmed (newly confirmed: in 5, or spawned confirmed), n_live (slots not free after the step).  Then t += 1.
 *      An empty frame still runs 4 and 5.
 *
 * gs_cand_params_default fills the struct: confirm_hits 3, max_misses 3, view_cos 0.5 (the cosine of half the field of view, so that no host
 *      cos enters a decision; -1 is all-round); spawn_range 67 m = the reference's coneMappingThreshold default (src/slam.hpp:116; the Slam
 *      mirror's cone_mapping_threshold is compared with the same distance column); view_range 12 m = the forward bound of the lidar cone
 *      detector's region of interest in the reference's usecase (usecase/docker-compose.yml, yBoundary=12).
 *      Refused (GS_ERR_INVALID) before the device is touched, by every call below that takes the blocks: a wrong struct_size of either block
 *      and whatever the association refuses of gs_nn_params; confirm_hits < 1; max_misses < 1; spawn_range or view_range not finite or <= 0;
 *      view_cos outside [-1, 1] (a NaN included).  A host-only handle: GS_ERR_NO_DEVICE.
 * gs_cand_batch: host arrays; n_steps frames through frame_start (as gs_assign_nn_batch checks it), a pose and (pose_cov != NULL) a 3x3
 *      covariance per STEP, in_idx[n] (may be NULL), the initial table (n_in records, 0 .. GS_CAND_MAX; a record whose state is outside
 *      0 .. 2: GS_ERR_INVALID).  Outputs, each may be NULL: out_steps[n_steps], out_cand_id[n], out_cand_slot[n], out_table[GS_CAND_MAX]
 *      (slot s at [s]), out_n_live.  One upload, all steps enqueued back to back, one wait.
 * gs_cand_resident: everything in DEVICE memory, asynchronous on the handle's stream, no wait.  dev_obs must be 32-byte aligned.
 *      frame_cap (0 .. GS_NN_FRAME_MAX) sizes launches, never a result.  The kernels defend themselves: a step whose bounds are not
 *      0 <= a <= b <= n, or whose frame is above frame_cap, is no step: nothing of it is read, the table and t stay, no output of it is
 *      written.  Observations that no frame covers are not written.  dev_out_meta_4: {next_id, t, n_live, 0}.  A loaded record whose
 *      state is neither 1 nor 2 becomes a free slot (the host cannot see it to refuse it).
 *      A batch or resident run works in a table of its own and does not disturb the live one.
 * gs_cand_clear / gs_cand_set / gs_frame_frontend_candidates / gs_cand_get / gs_cand_take_confirmed: the live table, empty until set.
 *      gs_frame_frontend_candidates is one step on it, one wait.  gs_cand_get reads all GS_CAND_MAX records (slot s at [s]) and next_id,
 *      t, n_live (each may be NULL).  gs_cand_take_confirmed returns the confirmed records in ascending id and frees their slots (more
 *      than cap of them: GS_ERR_INVALID, nothing changes); it touches neither map nor graph: the caller runs gs_map_append,
 *      gs_map_set_cov and gs_add_landmark.  Batch, resident and a sequence of live calls return identical bits.
 * Per step: two dispatches of its own (gs_cand.hip: the masked frame laid out for the association; the update, one workgroup) around the
 *      association's one or two.  Everything (two tables, the stage) is one allocation made at the first call; a handle that never calls
 *      any of these allocates and launches nothing for them; the calls above are unchanged by them.
 * NOT DONE: one wait for localisation plus candidates (the caller chains gs_frame_frontend_follow or gs_frame_frontend_localize and this
 *      call); correlation of the pose error across frames (P is added afresh at every fusion, so the fused covariance is optimistic when
 *      Sigma_p is given — the counterpart of the association ignoring cross-covariances); merging two candidates spawned for one cone;
 *      observation edges for a candidate's earlier sightings (out_cand_id lets the caller keep that log); the Slam mirror and the shell;
 *      sharded handles; frames above GS_NN_FRAME_MAX and more than GS_CAND_MAX candidates. */
#define GS_CAND_MAX 1024
typedef struct gs_cand_params {
    int32_t struct_size;
    int32_t confirm_hits;    /* 3; >= 1 */
    int32_t max_misses;      /* 3; >= 1 */
    int32_t reserved;
    double spawn_range;      /* 67 m; finite, > 0 */
    double view_range;       /* 12 m; finite, > 0 */
    double view_cos;         /* 0.5; in [-1, 1] */
} gs_cand_params;
typedef struct gs_cand {
    double xy[2];
    double cov[4];
    int32_t type;
    int32_t id;              /* -1 in a free slot */
    int32_t state;           /* 0 free, 1 tentative, 2 confirmed */
    int32_t hits, misses;
    int32_t first_step, last_step;
    int32_t confirm_step;    /* -1 until confirmed */
} gs_cand;
typedef struct gs_cand_step {
    int32_t step;
    int32_t n_unexplained, n_fused, n_spawned, n_contested, n_far, n_dropped, n_missed, n_retired, n_confirmed, n_live;
    int32_t reserved;
} gs_cand_step;
int  gs_cand_params_default(gs_cand_params *p);
int  gs_cand_batch(gs_graph *g, int32_t n_steps, int32_t n, const double *obs_4xn, const int32_t *frame_start, const double *poses_xytheta,
                   const double *pose_covs_3x3, const int32_t *in_idx, int32_t n_in, const gs_cand *in_table, const gs_nn_params *params,
                   const gs_cand_params *cand, gs_cand_step *out_steps, int32_t *out_cand_id, int32_t *out_cand_slot, gs_cand *out_table,
                   int32_t *out_n_live);
int  gs_cand_resident(gs_graph *g, int32_t n_steps, int32_t n, const double *dev_obs_4xn, const int32_t *dev_frame_start, int32_t frame_cap,
                      const double *dev_poses_xytheta, const double *dev_pose_covs_3x3, const int32_t *dev_in_idx, int32_t n_in,
                      const gs_cand *dev_in_table, const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *dev_out_steps,
                      int32_t *dev_out_cand_id, int32_t *dev_out_cand_slot, gs_cand *dev_out_table, int32_t *dev_out_meta_4);
int  gs_cand_clear(gs_graph *g);
int  gs_cand_set(gs_graph *g, int32_t n_in, const gs_cand *records);
int  gs_cand_get(gs_graph *g, gs_cand *out_table, int32_t *out_next_id, int32_t *out_step, int32_t *out_n_live);
int  gs_cand_take_confirmed(gs_graph *g, int32_t cap, gs_cand *out_records, int32_t *out_n);
int  gs_frame_frontend_candidates(gs_graph *g, const double pose_xytheta[3], const double *pose_cov_3x3, const double *obs_4xk, int32_t k,
                                  const int32_t *in_idx, const gs_nn_params *params, const gs_cand_params *cand, gs_cand_step *out_step,
                                  int32_t *out_cand_id, int32_t *out_cand_slot);

/* ---- map twins: duplicate cones found, fused and merged in the graph -------------------------------------------------------------------
 * Every call above assumes that one physical cone is one map entry.  The reference's addConesToMap (src/slam.cpp:570-623) makes a new cone
 * whenever no map cone of the same type lies within m_newConeThreshold (1 m, src/slam.hpp:113), so drift at the end of a lap maps the first
 * cones a second time beside themselves, and loopClosing only ever looks at cone 0; the cone candidates above can spawn two entries for one
 * cone.  These calls find such twins among ALL cone pairs of a map, fuse each pair into one cone, compact the map, and merge the two
 * landmark vertices in the graph (g2o's OptimizableGraph::mergeVertices).  The rule is build-defined.  No contraction anywhere: every
 * product and sum below is rounded once, in the order the parentheses give.
 *
 * Map.  What the association calls take: xy [n][2], type [n] (int32) and cov [n][4] (row-major 2x2, entry [1] read; NULL or never set: zeros).
 * Pair.  The quantities of cones i != j are ALWAYS formed from a = min(i, j) and b = max(i, j), so both ends of a pair see identical bits:
 *            s2 = sigma_floor sigma_floor  (formed once, on the host)
 *            A00 = Ca00 + s2   A01 = Ca01   A11 = Ca11 + s2         B00 = Cb00 + s2   B01 = Cb01   B11 = Cb11 + s2
 *            S00 = A00 + B00   S01 = A01 + B01   S11 = A11 + B11     n0 = xb - xa   n1 = yb - ya
 *            det = (S00 S11) - (S01 S01)
 *            d2  = ((((S11 n0) n0) - (((2 S01) n0) n1)) + ((S00 n1) n1)) / det          (the covariance-gated association's order)
 *      The pair is ADMISSIBLE iff ALL of   type_a == type_b (only when require_same_type),   sqrt((n0 n0) + (n1 n1)) < max_distance,
 *      det > 0,   S00 > 0,   d2 < gate_chi2   hold.  Positive tests: any NaN skips the pair, so a cone whose xy is not finite is invisible
 *      (as a free candidate slot is).  A cone is never its own partner.
 * Per cone i.  twin[i] = the admissible j with the smallest d2, exact ties to the lowest j, -1 when there is none; d2[i] = that d2, +inf
 *      when there is none; second_d2[i] = the smallest d2 among the OTHER admissible cones, +inf when there is none; n_admissible[i] = how
 *      many cones are admissible.
 * Twin pair.  (a, b), a < b, is a twin pair iff twin[a] == b and twin[b] == a — with `exclusive` also n_admissible == 1 at both ends.  Twin
 *      pairs are disjoint by construction.  Of a triplet the closest two are a pair in one round and the third finds the fused cone in the
 *      next: the caller repeats until n_pairs == 0.
 * Fusion of a twin pair.  The keeper is a.  With A, B, S, det, n0, n1 of the pair as above:
 *            K00 = ((A00 S11) - (A01 S01)) / det      K01 = ((A01 S00) - (A00 S01)) / det
 *            K10 = ((A01 S11) - (A11 S01)) / det      K11 = ((A11 S00) - (A01 S01)) / det
 *            x+ = xa + ((K00 n0) + (K01 n1))          y+ = ya + ((K10 n0) + (K11 n1))
 *            C00+ = (K00 B00) + (K01 B01)             C01+ = (K00 B01) + (K01 B11)             C11+ = (K10 B01) + (K11 B11)
 *      (K = A S^-1, C+ = K B = the parallel sum (A^-1 + B^-1)^-1: no C - K C cancellation); cov+ = (C00+, C01+, C01+, C11+), the 01 entry
 *      formed once; the type is a's.  THE FLOOR IS PART OF C+: A and B carry s2, so two cones of zero covariance fuse to (s2 / 2) I and
 *      every fused cone's covariance includes what the floor stood for.
 * Consolidated map.  Every b of a twin pair is dropped; every other cone keeps its relative order; a cone in no pair keeps its bits (a NaN
 *      cone included); a keeper takes x+, y+, cov+.  remap[old] = the new index, remap[b] = remap[a].  n_out = n_in - n_pairs.
 *
 * gs_dup_params_default fills the struct: require_same_type 1, exclusive 0, gate_chi2 5.991464547107979 (95 %, 2 dof, as gs_nn_params),
 *      max_distance 1.0 m (the reference's m_newConeThreshold), sigma_floor 0.05 m (gs_nn_params.sigma_xy's default).
 *      Refused (GS_ERR_INVALID) before the device is touched, by every call below that takes the block: a null block, a wrong struct_size,
 *      a parameter that is not finite, gate_chi2 <= 0, max_distance <= 0, sigma_floor < 0, require_same_type or exclusive outside {0, 1};
 *      a map of more than GS_DUP_MAP_MAX cones; a null array where one is required.  A host-only handle: GS_ERR_NO_DEVICE.
 * gs_dup_info: n_in, n_out, n_pairs, n_ambiguous = the cones of the INPUT map with n_admissible > 1.
 * gs_map_twins_batch: a query over host arrays; map_cov and every output but out_twin may be NULL.
 * gs_map_twins_resident: the same over the resident map and its covariances; outputs in DEVICE memory ([map size] each, every one but
 *      dev_out_twin may be NULL), asynchronous on the handle's stream.  Nothing is changed.
 * gs_map_merge_twins_batch: host map in, consolidated host map out (each output array has room for n_map cones and is written whole: entries from n_out
 *      on are free cones, xy = (NaN, NaN), type 0, zero covariance); out_cov is written when map_cov is given and may be NULL; out_remap [n_map] and out_info may be NULL.
 * gs_map_merge_twins: consolidates the RESIDENT map in place, device to device (compacted into a second buffer and copied back), with the
 *      one wait at its end that the new map size needs: a maintenance call, not a per-frame one.  It invalidates what gs_map_clear
 *      invalidates (the grids of the resident searches).  out_remap is a host array of `capacity` entries, capacity >= the map size before
 *      the call (else GS_ERR_CAPACITY, nothing changes), and may be NULL (capacity is then ignored).  A handle that never set a covariance
 *      runs with Sigma = 0, stores no C+ and creates no covariance array.
 * gs_map_get_xy: positions and types of the resident map's cones [first, first + n) back to the host (either output may be NULL): after a
 *      consolidation the caller's own copy of the map is stale.
 * All four twins calls return identical bits for identical maps.  Four dispatches for a consolidation (gs_dup.hip: the search, the mutual
 *      test with the fusion and per-block counts, a one-workgroup scan of the block counts, the scatter), one for a query; no atomics, no
 *      spin, no cross-workgroup wait.  A handle that never calls these allocates and launches nothing for them.
 * gs_merge_landmarks(keep, drop) = g2o's mergeVertices(keep, drop, erase = true) on the handle's graph: every observation edge of `drop`
 *      (polar edges are observation edges and follow) and every landmark prior of `drop` is re-attached to `keep`, activity flags stay with
 *      their edge, `drop` is erased, later landmarks move down by one (in the graph, in the priors' and in the polar edges' tables alike).
 *      The next optimisation runs a full structure phase; marginals become stale.  keep's estimate and fixed flag are untouched: the caller sets the fused position with gs_set_landmark_estimate.  Estimates
 *      that are newer on the device are brought to the host first (as gs_add_landmark does).  Afterwards the handle is indistinguishable
 *      from a fresh one given the same insertions without `drop` and with those edges pointing at `keep`.
 *      Unknown id: GS_ERR_UNKNOWN_ID.  keep == drop, `drop` fixed while `keep` is free, a handle configured with
 *      gs_dist_configure(world > 1): GS_ERR_INVALID.
 * NOT DONE: twins inside the candidate table (the search kernel takes plain (xy, type, cov, n) pointers so that it can be handed the table);
 *      a grid instead of the walk over all pairs; cone-cone cross-covariances (outside the factor's pattern, as the association ignores
 *      them); chains merged in one round; sharded handles; the Slam mirror and the shell. */
#define GS_DUP_MAP_MAX 262144
typedef struct gs_dup_params {
    int32_t struct_size;
    int32_t require_same_type;  /* 1; 0 or 1 */
    int32_t exclusive;          /* 0; 0 or 1 */
    int32_t reserved;
    double gate_chi2;           /* 5.991464547107979: 95 %, 2 dof */
    double max_distance;        /* 1.0 m: Euclidean pre-gate */
    double sigma_floor;         /* 0.05 m; >= 0 */
} gs_dup_params;
typedef struct gs_dup_info {
    int32_t n_in, n_out, n_pairs, n_ambiguous;
} gs_dup_info;
int  gs_dup_params_default(gs_dup_params *p);
int  gs_map_twins_batch(gs_graph *g, int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov_2x2,
                        const gs_dup_params *params, int32_t *out_twin, double *out_d2, double *out_second_d2, int32_t *out_n_admissible);
int  gs_map_twins_resident(gs_graph *g, const gs_dup_params *params, int32_t *dev_out_twin, double *dev_out_d2, double *dev_out_second_d2,
                           int32_t *dev_out_n_admissible);
int  gs_map_merge_twins_batch(gs_graph *g, int32_t n_map, const double *map_xy, const int32_t *map_type, const double *map_cov_2x2,
                              const gs_dup_params *params, double *out_xy, int32_t *out_type, double *out_cov_2x2, int32_t *out_remap,
                              gs_dup_info *out_info);
int  gs_map_merge_twins(gs_graph *g, const gs_dup_params *params, int32_t capacity, int32_t *out_remap, gs_dup_info *out_info);
int  gs_map_get_xy(gs_graph *g, int32_t first, int32_t n, double *out_xy, int32_t *out_type);
int  gs_merge_landmarks(gs_graph *g, int32_t keep_id, int32_t drop_id);

/* ---- multi-GPU: pose-window shards -----------------------------
 * Each rank owns a contiguous pose window and builds the SAME global plan; it linearises and
 * factorises only its own subtrees, exports the update contributions to the shared top of the
 * assembly tree into a dense exchange buffer (device memory), the caller all-reduces that
 * buffer (RCCL sum, fp64), and every rank finishes the top of the tree redundantly. */
int  gs_dist_configure(gs_graph *g, int32_t rank, int32_t world_size);   /* before gs_initialize_optimization */
/* Rank-local ingestion (optional).  By default every rank is given the WHOLE graph and finds out in one pass over all observation edges which
 * windows see which landmark.  A rank that is told so need not hold the other windows' observation edges at all: its plan is built from the edges
 * of its own window's poses, of every window's FIRST pose (the separators of the shared top) and of the fixed poses; everything else of the other
 * windows enters through two 64-bit masks per landmark — bit w set: an interior pose / the first pose of window w observes it.  Vertices and
 * odometry edges are still added on every rank (they carry the global indices the exchange slots are agreed on), observation edges grouped by pose.
 *   gs_dist_window_starts           insertion index of the first free pose of each window, world + 1 entries (the last: n_poses): which poses are whose
 *   gs_dist_local_landmark_windows  this rank's OWN bits, from the edges it holds (the ranks' bits are disjoint: an all-reduce SUM over the ranks —
 *                                   or an OR in a single process — gives the masks of the whole graph)
 *   gs_dist_share_landmark_windows  the two steps around the exchange in one call, over the handle's own RCCL communicator (gs_dist_comm_init first): own bits ->
 *                                   ncclAllReduce(uint64, sum) -> gs_dist_set_landmark_windows.  Collective: every rank calls it.
 *   gs_dist_set_landmark_windows    hands the whole-graph masks to the handle (n_landmarks = 0: back to the default); the next structure phase
 *                                   uses them and fails if an edge it holds contradicts them, or if the graph cannot be planned by windows
 *                                   (more than 64 ranks, fewer than 4 free poses per window, odometry edges between two windows' interiors).
 * The reference has no counterpart (one process, one optimiser: src/slam.cpp:53-65); SURVEY 8e's pose windows, without "every rank ingests everything". */
int  gs_dist_window_starts(gs_graph *g, int32_t *out_first_pose, int32_t capacity);
int  gs_dist_local_landmark_windows(gs_graph *g, uint64_t *seen_interior, uint64_t *seen_first, int32_t n_landmarks);
int  gs_dist_set_landmark_windows(gs_graph *g, const uint64_t *seen_interior, const uint64_t *seen_first, int32_t n_landmarks);
int  gs_dist_share_landmark_windows(gs_graph *g);
int64_t gs_dist_exchange_doubles(gs_graph *g);         /* length of the exchange buffer (after initialize)   */
int  gs_dist_set_exchange_buffer(gs_graph *g, void *device_ptr);   /* NULL: the library allocates its own   */
int  gs_dist_iterate_local(gs_graph *g);               /* linearise own edges + own subtrees + contribution  */
int  gs_dist_iterate_finish(gs_graph *g);              /* after the all-reduce: shared top, solve, update    */
/* The all-reduce INSIDE the library (the host side stays C++: the microservice needs no Python and no torch): RCCL is resolved at run
 * time (the copy the process has loaded already, else librccl.so), never linked.
 * gs_dist_unique_id        ncclGetUniqueId: 128 bytes, made by one rank and handed to the others by whatever channel the ranks share
 *                          (the microservices share an OD4 session: reference src/opendlv-logic-cfsd18-sensation-slam.cpp:62).
 * gs_dist_comm_init        ncclCommInitRank on the handle's device (collective: every rank calls it); the handle owns the communicator.
 * gs_dist_set_communicator adopt a caller-owned ncclComm_t instead.
 * gs_dist_iterate          one sharded Gauss-Newton iteration, all enqueued from C++ on the handle's stream: local half ->
 *                          ncclAllReduce(sum, fp64) of the exchange buffer (the shared rows of Omega / xi) -> shared top, solve, update.
 * gs_dist_optimize         Slam's optimize(10) (src/slam.cpp:481) on a sharded graph: `iterations` x gs_dist_iterate, g2o's failure rule
 *                          across ranks; returns the updates applied (0: a factorisation failed on some rank).  A whole-tree launch that gives up on a
 *                          front's flag on some rank (no property of H) is repaired inside the call: that rank switches to one launch per level, every rank
 *                          runs the iterations that were not applied again; gs_stats.first_failure = 2 / 4 says it happened (here / on another rank).  If the
 *                          launch gave up BEHIND the exchange the ranks have applied different numbers of updates: all return GS_ERR_TIMEOUT (estimates to be set again). */
int  gs_dist_unique_id(void *out_128_bytes);
int  gs_dist_comm_init(gs_graph *g, const void *unique_id_128_bytes, int32_t rank, int32_t world_size);
int  gs_dist_set_communicator(gs_graph *g, void *nccl_comm);
int  gs_dist_iterate(gs_graph *g);
int  gs_dist_optimize(gs_graph *g, int32_t iterations, gs_stats *stats /* may be NULL */);
/* host copies of the exchange buffer (tests; all-reduce over a CPU backend when ranks share one GPU) */
int  gs_dist_read_exchange(gs_graph *g, double *host_out);
int  gs_dist_write_exchange(gs_graph *g, const double *host_in);
/* per vertex (insertion order): known = this rank tracks its estimate; primary = exactly one rank per vertex
 * (shared and fixed vertices: rank 0), so summing primary-masked estimates over the ranks merges them */
int  gs_dist_known(gs_graph *g, uint8_t *pose_known, uint8_t *lm_known, uint8_t *pose_primary, uint8_t *lm_primary);

/* ---- Slam-level host mirror (rows f-1/f-2 of SURVEY §8f) ----------------------
 * gs_slam_perform <- Slam::performSLAM (src/slam.cpp:298-338): the 200 m odometry guard, the heading compensated by
 *      yawRate * dt (0 < dt < 1 s, dt from gs_slam_set_sample_times), addPoseToGraph, then — two independent ifs as in
 *      the reference (:329-334) — addConesToMap (loop-closure trigger, optimizeGraph, updateMap) while the loop is open
 *      and the localizer once it is closed, i.e. BOTH in the frame that closes it. */
int  gs_slam_create(const gs_config *cfg, gs_slam **out);
int  gs_slam_destroy(gs_slam *s);
int  gs_slam_perform(gs_slam *s, const double odometry_xytheta[3], const double *cones_4xk, int32_t k);
int  gs_slam_map_size(gs_slam *s);
int  gs_slam_get_map(gs_slam *s, int32_t capacity, double *out_xy, int32_t *out_type);
int  gs_slam_get_map_covariances(gs_slam *s, int32_t capacity, double *out_2x2);   /* see gs_compute_marginals; a map cone that is not in the graph: zeros;
                                                                                      GS_ERR_NOT_INITIALIZED until the mirror has fixed its gauge (first optimizeGraph) */
int  gs_slam_loop_closed(gs_slam *s);
int  gs_slam_current_cone_index(gs_slam *s);
int  gs_slam_get_send_pose(gs_slam *s, double out_xytheta[3]);
gs_graph *gs_slam_graph(gs_slam *s);
/* ---- frame collector and output encoders (row f-2) ---------------------------
 * gs_slam_collect_direction / _distance / _type <- Slam::nextCone (src/slam.cpp:67-152): one field of column objectId of
 *      the 4 x 1000 collector; returns 1 when the message opened a new frame, 0 otherwise, < 0 on error
 *      (objectId >= 1000 is refused; the reference indexes unchecked).
 * gs_slam_collect_flush <- Slam::initializeCollection (src/slam.cpp:221-257) after its wait, without the keyframe gate:
 *      extracts the leftmost lastObjectId + 1 columns (also copied to cones_out_4xk when not NULL, count in *k_out),
 *      resets the collector and runs gs_slam_perform on them with the given odometry pose.
 * gs_slam_encode_cones <- Slam::sendCones + Cone::getDirection / getDistance (src/slam.cpp:656-677, src/cone.cpp:34-53):
 *      conesPerPacket cones from currentConeIndex on, wrapping around the map, seen from the send pose; float32 fields
 *      as in the messages (azimuth in degrees, zenith is always 0).  cfg.reference_quirks keeps the reference's heading
 *      unit slip. */
int  gs_slam_collect_direction(gs_slam *s, uint32_t object_id, double azimuth_deg, double zenith_deg);
int  gs_slam_collect_distance(gs_slam *s, uint32_t object_id, double distance);
int  gs_slam_collect_type(gs_slam *s, uint32_t object_id, uint32_t type);
int  gs_slam_collect_flush(gs_slam *s, const double pose_xytheta[3], int32_t *k_out, double *cones_out_4xk);
/* the first half of gs_slam_collect_flush alone: extract the leftmost lastObjectId + 1 columns and reset the collector */
int  gs_slam_collect_extract(gs_slam *s, int32_t *k_out, double *cones_out_4xk);
int  gs_slam_encode_cones(gs_slam *s, int32_t cones_per_packet, float *azimuth_deg, float *distance, int32_t *type);
/* gs_cone_encode <- Cone::getDirection / Cone::getDistance (src/cone.cpp:34-53) for ONE cone seen from `pose`: the float32
 * azimuthAngle (degrees) and distance fields (zenithAngle is always 0).  reference_quirks != 0 keeps the reference's unit slip
 * (heading * 1 / RAD2DEG, src/cone.cpp:37-39).  Stateless; gs_slam_encode_cones calls it per cone.  Pinned against the reference's
 * own cone.cpp (oracle/_ref/libref_cone.so, tests/test_cone.py). */
int  gs_cone_encode(const double cone_xy[2], const double pose_xytheta[3], int32_t reference_quirks, float *azimuth_deg, float *distance);
/* ---- odometry intake and pose output (row f-4), host side -------------------------
 * gs_wgs84_to_cartesian / gs_wgs84_from_cartesian <- wgs84::toCartesian / fromCartesian (src/WGS84toCartesian.hpp:39-113,
 *      119-146): ellipsoidal polyconic projection about the reference point and its step-search inverse; arrays are
 *      {latitude, longitude} in degrees and {x, y} in metres.
 * gs_slam_set_gps_reference       <- m_gpsReference (command line of the microservice)
 * gs_slam_next_wgs84 / _heading   <- Slam::nextSplitPose (src/slam.cpp:154-185; heading wrapped with the float PI)
 * gs_slam_next_geolocation        <- Slam::nextPose (src/slam.cpp:187-209)
 * gs_slam_next_yaw_rate           <- Slam::nextYawRate (src/slam.cpp:211-219)
 * gs_slam_get_odometry            -> m_odometryData (x, y, heading) and m_yawRate: the pose gs_slam_perform is fed
 * gs_slam_encode_pose             <- Slam::sendPose (src/slam.cpp:679-695): {longitude, latitude, heading} as float32;
 *      cfg.reference_quirks keeps the reference's swapped latitude / longitude fields. */
int  gs_wgs84_to_cartesian(const double ref_latlon_deg[2], const double pos_latlon_deg[2], double out_xy[2]);
int  gs_wgs84_from_cartesian(const double ref_latlon_deg[2], const double xy[2], double out_latlon_deg[2]);
int  gs_slam_set_gps_reference(gs_slam *s, double latitude_deg, double longitude_deg);
int  gs_slam_next_wgs84(gs_slam *s, double latitude_deg, double longitude_deg);
int  gs_slam_next_heading(gs_slam *s, double north_heading);
int  gs_slam_next_geolocation(gs_slam *s, double latitude_deg, double longitude_deg, double heading);
int  gs_slam_next_yaw_rate(gs_slam *s, double angular_velocity_z);
/* m_yawReceivedTime / m_lastTimeStamp (src/slam.cpp:216; :73,102,129): sample times (microseconds) of the last yaw-rate
 * message and the last cone message; performSLAM's dt = |difference| / 1e6 (src/slam.cpp:309) */
int  gs_slam_set_sample_times(gs_slam *s, int64_t yaw_received_us, int64_t last_cone_us);
int  gs_slam_get_odometry(gs_slam *s, double out_xy_heading_yawrate[4]);
int  gs_slam_encode_pose(gs_slam *s, float out_lon_lat_heading[3]);

/* ---- the microservice shell (row f-3), transport-independent ---------------------------------------------------------
 * Mirrors main() of the reference (src/opendlv-logic-cfsd18-sensation-slam.cpp:49-119) around the Slam mirror: the same
 * command-line keys and the "at least 10 arguments" rule (:52), the seven data triggers behind their senderStamp filters
 * (:71-108), the gathering window and the keyframe gate (src/slam.cpp:221-257, 286-295), and the messages the localizer
 * publishes (sendPose + sendCones, :404-410, 656-695).  Messages cross this boundary decoded; csrc/gs_shell_cluon.cpp binds
 * it to cluon's OD4Session (Envelope decode / od4.send).  Type ids are the message set's: 19 GeodeticWgs84Reading
 * {v0 latitude, v1 longitude}, 1051 GeodeticHeadingReading {v0 northHeading}, 1116 Geolocation {v0 latitude, v1 longitude,
 * v2 heading}, 1031 AngularVelocityReading {v0 angularVelocityZ}, 1133 ObjectDirection {object_id, v0 azimuth, v1 zenith},
 * 1134 ObjectDistance {object_id, v0 distance}, 1131 ObjectType {object_id, v0 type}. */
typedef struct gs_shell gs_shell;
typedef struct gs_shell_msg {
    int32_t  data_type;
    uint32_t sender_stamp;
    int64_t  sample_time_us;
    uint32_t object_id;
    uint32_t reserved;
    double   v[3];
} gs_shell_msg;
/* argv as main() receives it; fewer than 10 arguments or a missing key -> GS_ERR_INVALID with the usage text in
 * gs_last_error (the reference prints it and returns 1).  device as in gs_config (-2: host-only, for tests of the dispatch). */
int  gs_shell_create(int32_t argc, const char *const *argv, int32_t device, gs_shell **out);
int  gs_shell_destroy(gs_shell *sh);
/* one incoming message; now_us = the caller's clock (starts the gathering window of a frame).  1 taken, 0 ignored. */
int  gs_shell_on_message(gs_shell *sh, const gs_shell_msg *m, int64_t now_us);
/* runs the frame whose gathering window (--gatheringTimeMs) has passed: extract, keyframe gate (--timeBetweenKeyframes, ms),
 * performSLAM, outputs.  1 performSLAM ran, 0 nothing due / not a keyframe. */
int  gs_shell_poll(gs_shell *sh, int64_t now_us);
int  gs_shell_pending_output(gs_shell *sh);
int  gs_shell_take_output(gs_shell *sh, int32_t capacity, gs_shell_msg *out);
int  gs_shell_counters(gs_shell *sh, int64_t out_run_gated[2]);
int  gs_shell_cid(gs_shell *sh);
gs_slam *gs_shell_slam(gs_shell *sh);

#ifdef __cplusplus
}
#endif
#endif /* GRAPHSLAM_H */
