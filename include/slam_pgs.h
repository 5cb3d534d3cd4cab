/* slam_pgs.h — C ABI of the MI355X batched pose-graph SLAM solver (part of libslam_hip.so).
 *
 * Drop-in boundary for the reference's `PoseGraph : Filter` with `implementation: gtsam`
 * (ekf_ws/src/localization_pkg/src/pose_graph.cpp, class declaration filter.h:232-322): the graph-building calls of
 * every timestep and `solvePoseGraph()` (gtsam::LevenbergMarquardtOptimizer, default parameters), for a batch of B
 * independent graphs.  By default they are Monte-Carlo instances that share the command sequence (BetweenFactors), the start
 * pose and the simulator's map and differ in their measurements and in the secondary filter's estimates; the pgs_*_each entry
 * points give every graph its own start pose, map and commands ("heterogeneous batches" below).  Same conventions as
 * slam_batch.h: plain pointers and sizes, int status codes (slam_status_code), text in slam_last_error(), one caller thread per
 * handle, kernels on one stream.
 *
 * Covered beyond the solve: `gtsam::Marginals marginals(graph, result); marginals.marginalCovariance(i)` (pose_graph.cpp:289-294) as
 * pgs_marginals / pgs_get_marginals, for every pose and landmark (the reference's printout of them is not reproduced).
 * Beyond the reference: a robust loss on the landmark factors (pgs_set_robust) and absolute position / heading fixes as unary pose factors
 * (pgs_fix, "absolute fixes" below).
 *
 * Not covered: `implementation: sesync | custom` (the reference itself throws for both, pose_graph.cpp:34-38),
 * unknown landmark ids (the reference throws, pose_graph.cpp:137), `update_landmarks_after_adding` (false in
 * params.yaml:63 and forced false when solving every iteration, pose_graph.cpp:45-48), per-instance timestep counts (a handle
 * is in lockstep: one `timestep` for all of its graphs) and per-instance noise configs, a secondary EKF fused into the device-side
 * simulator (feed pgs_update_each_dev from a slam_batch.h handle instead), a pgs_nav_* controller (slam_nav_run issues the
 * commands; its cmds_out go to pgs_update_each), slam_multi_*, checkpoint files.
 */
#ifndef SLAM_PGS_H
#define SLAM_PGS_H

#include <stdint.h>

#include "slam_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pgs_handle pgs_handle;

/* per-instance status bits (pgs_get_stats) */
enum pgs_instance_flags {
    PGS_INST_OK = 0,
    PGS_INST_POSE_CAP = 1,        /* more timesteps than N_max: the surplus updates were dropped                 */
    PGS_INST_LANDMARK_CAP = 2,    /* more distinct landmark ids than L_max: the surplus landmarks were dropped   */
    PGS_INST_MEAS_CAP = 4,        /* more detections in one message than k_per_pose: the surplus were dropped    */
    PGS_INST_NOT_CONVERGED = 8,   /* LM hit maxIterations (100) or the trial cap                                 */
    PGS_INST_NONFINITE = 16
};

/* Replaces `std::make_unique<PoseGraph>()` + readParams (localization_node.cpp:45-47, pose_graph.cpp:12-66): noise
 * models Diagonal::Sigmas(V00, V00, V11) for the BetweenFactors and Sigmas(W11, W00) for the BearingRangeFactors
 * (pose_graph.cpp:52-54) from the EFFECTIVE V / W of Filter::readCommonParams (filter.h:105-121, incl. its quirk).
 * N_max = pose capacity (num_iterations), L_max <= 255 landmarks, k_per_pose = detections stored per timestep. */
int pgs_create(const slam_config* cfg, int batch, int N_max, int L_max, int k_per_pose, int device, pgs_handle** out);
int pgs_destroy(pgs_handle* h);
int pgs_set_stream(pgs_handle* h, void* hip_stream);
int pgs_set_instance_offset(pgs_handle* h, int64_t first_global_instance);
int pgs_set_seed(pgs_handle* h, uint64_t seed);
int pgs_set_map(pgs_handle* h, const double* map_xy, int L);      /* simulator only (pgs_run_sim); one map for every instance */

/* PoseGraph::init (pose_graph.cpp:68-95): first pose node + PriorFactor with sigmas (1.3, 1.3, 1.2). */
int pgs_init(pgs_handle* h, float x_0, float y_0, float yaw_0);

/* One iterate() of localization_node.cpp:108-140 as seen by the pose graph:
 *   updateNaiveVehPoseEstimate(sec_pose)   (pose_graph.cpp:97-119; sec_pose [batch][3] = the secondary filter's
 *                                           x, y, yaw per instance; NULL keeps the previous estimate)
 *   update(cmd, meas)                      (pose_graph.cpp:199-256 without the solve/stop logic of :201-214,258-266,
 *                                           which belongs to the host mirror)
 * meas [batch][k_stride][3] float32 {id, range, bearing}, meas_count [batch].  HOST pointers. */
int pgs_update(pgs_handle* h, const float cmd[2], const float* meas, const int32_t* meas_count, int k_stride,
               const double* sec_pose);
/* Same with DEVICE pointers (e.g. the EKF engine's measurement dump and pose buffers). */
int pgs_update_dev(pgs_handle* h, const float cmd[2], const float* d_meas, const int32_t* d_meas_count, int k_stride,
                   const double* d_sec_pose);
/* T iterations with everything on the device: measurement generator get_cmd (sim_node.py:209-250) with the
 * instance's noise stream, NaiveFilter::update as the secondary filter (filter.h:342-348, params.yaml:60), then the
 * two calls above.  cmds [T][2] float32 host array. */
int pgs_run_sim(pgs_handle* h, const float* cmds, int T);

/* ---- heterogeneous batches -------------------------------------------------------------------------------------------------
 * Per-instance forms of the calls above, named and laid out like slam_batch.h's slam_*_each (arrays of `batch` rows, HOST pointers
 * unless marked _dev), so that one handle can hold several robots, trajectories or maps, and can follow a slam_batch.h handle whose
 * instances drive their own commands (slam_nav_run).  Every entry point above keeps its behaviour, and per-instance rows that are all
 * equal give the same bits as the shared call.  pgs_solve, pgs_adopt_result, pgs_marginals*, pgs_get_* and pgs_error_stats work on such
 * graphs unchanged, in every solve schedule.
 * Mixing: shared and _each calls may be mixed and take effect in call order.  The handle stays in lockstep (one timestep).  The first
 *   per-instance command moves the handle's BetweenFactor measurements from one row [N_max][2] to one row per instance ([batch][N_max][2]
 *   float32: 8 * batch * N_max bytes, 16 MB at batch 2048 with N_max = 1000, kept until pgs_destroy); the ticks the handle already has
 *   stay in every instance's graph, and a shared call afterwards writes its command into every instance's row.
 * Errors: SLAM_ERR_STATE before pgs_init / pgs_init_each, and for the simulator calls without a map; SLAM_ERR_ARG for NULL or non-finite
 *   host inputs, L[b] out of range, T <= 0.  A call that returns an error has changed nothing. */
/* PoseGraph::init with one start pose per instance: pose0 [batch][3] {x, y, yaw} (float, as pgs_init's arguments) = the first pose
 * node, cur_veh_pose_estimate and the mean of the PriorFactor; truth0 [batch][3] = the simulator's true start pose per instance, NULL =
 * the instance's pose0 row widened to double (what pgs_init does with its arguments).  Resets what pgs_init resets. */
int pgs_init_each(pgs_handle* h, const float* pose0, const double* truth0);
/* Simulator only: one true map per instance, maps [batch][L_stride][2], L [batch] landmarks (ids 0 .. L[b]-1; 1 <= L[b] <= L_stride <=
 * 255).  Replaces the shared map; a later pgs_set_map returns to the shared map. */
int pgs_set_maps(pgs_handle* h, const double* maps, const int32_t* L, int L_stride);
/* One iterate() with one BetweenFactor measurement per instance, cmds [batch][2] {fwd, ang}; otherwise as pgs_update / pgs_update_dev
 * (pgs_update_each_dev: d_cmds is a device pointer too, read in the order of the handle's stream - e.g. the controller's commands of a
 * slam_batch.h handle next to its measurement dump and poses). */
int pgs_update_each(pgs_handle* h, const float* cmds, const float* meas, const int32_t* meas_count, int k_stride,
                    const double* sec_pose);
int pgs_update_each_dev(pgs_handle* h, const float* d_cmds, const float* d_meas, const int32_t* d_meas_count, int k_stride,
                        const double* d_sec_pose);
/* T simulator iterations, cmds [T][batch][2] (the layout of slam_run_sim_each): one copy and one transposing launch, no per-tick host work. */
int pgs_run_sim_each(pgs_handle* h, const float* cmds, int T);

/* PoseGraph::solvePoseGraph (pose_graph.cpp:269-300) for every instance: LM from initial_estimate to `result`.
 * The trials of a batch run in lockstep; once few instances are still active each runs the next lambdas of GTSAM's retry
 * sequence (lambda, 10 lambda, ...) at once in spare slots and the sequential accept / lambda logic is replayed over them, so
 * the result, pgs_get_stats' iteration and trial counts are those of the sequential loop.  The slots multiply the LM work
 * space: SLAM_PGS_LANES slots per instance (default 4, 1 = off; reduced at pgs_create if they would take more than half of
 * the free device memory).  Trial cap: with SLAM_PGS_MAX_TRIALS = K (default 400) every graph consumes at most K lambda trials in
 * every schedule (lockstep with or without lanes, streaming, the lockstep tail after streaming); a graph that reaches K unconverged
 * ends flagged PGS_INST_NOT_CONVERGED with the values of its last accepted trial, so results and counts do not depend on the schedule.
 * Launch shape (results do not depend on it beyond the tolerance of the SYRK's summation order): the kernels of a trial run over
 * the compacted list of running slots (SLAM_PGS_LIST=0: full-size grids); with at most 128 running slots, or a batch that fills
 * the device twice, the block-tridiagonal chain and the Schur-complement SYRK are ONE launch with Y kept in LDS, replicated on
 * 2 - 4 CUs per instance (SLAM_PGS_FUSED=0: always two launches; 2 | 3 | 4: that many workgroups per instance).  The fused
 * kernel needs 2 M + 1 <= 448, M <= 176 mapped landmarks and k_per_pose <= 32; other graphs take the two-launch path. */
int pgs_solve(pgs_handle* h);
/* The solve splits the batch into `groups` contiguous ranges that run their LM loops on separate HIP streams (the
 * latency-bound phases of one group overlap the bandwidth-bound phases of another); results do not depend on it.
 * 0 = automatic: 2 from 128 instances on, 1 below (SLAM_PGS_GROUPS sets the default).  Whatever is asked for, a solve runs at most 16
 * groups and at most one per instance, a profiled solve (pgs_set_profiling) one; the ticks of pgs_run_sim_every_iteration[_each] run one
 * while the setting is 0.  Group g of G owns the instances [g per, min(batch, (g + 1) per)), per = ceil(batch / G). */
int pgs_set_groups(pgs_handle* h, int groups);
/* Streaming solve (round 6): the handle holds `batch` graphs but at most `slots` of them are IN FLIGHT (0 = lockstep, all of them from
 * the first trial on; SLAM_PGS_SLOTS sets the default).  The others wait; when a graph converges the device-side decide step hands
 * its running slot to the next waiting graph, so every LM trial runs a full list of slots instead of a list that decays to the
 * batch's slowest instances, and the host - which no longer decides anything per trial - enqueues trials ahead
 * (SLAM_PGS_STREAM_DEPTH, default 3) and reads the counters of the trial that far back.  Once nothing waits and at most
 * SLAM_PGS_LANES_SWITCH graphs are left the lockstep loop with its lambda lanes finishes them.  Results, iteration and trial counts
 * do not depend on `slots`: a graph's LM sequence depends on nothing but the graph (the reference solves ONE graph per call,
 * pose_graph.cpp:269-300; the batch and its schedule are this library's). */
int pgs_set_slots(pgs_handle* h, int slots);
/* The last solve's schedule: slots[i] = running slots of trial i of solve group `group` (at most cap entries written), *n = trials of
 * that group, *groups = solve groups of the solve.  Mean occupancy = sum(slots) / (trials x slots per group). */
int pgs_last_solve_timeline(pgs_handle* h, int group, int32_t* slots, int cap, int32_t* n, int32_t* groups);
/* `this->initial_estimate = this->result` (pose_graph.cpp:263, solve_graph_every_iteration). */
int pgs_adopt_result(pgs_handle* h);
/* The reference's DEFAULT mode, solve_graph_every_iteration: true (params.yaml:64; pose_graph.cpp:258-264), with the simulator on the
 * device: T x { one tick of pgs_run_sim, pgs_solve, pgs_adopt_result }.  counts [batch][2] (may be NULL) = the LM iterations and
 * lambda trials of every instance summed over the T ticks. */
int pgs_run_sim_every_iteration(pgs_handle* h, const float* cmds, int T, int32_t* counts);
/* The same with one command per instance and tick, cmds [T][batch][2]. */
int pgs_run_sim_every_iteration_each(pgs_handle* h, const float* cmds, int T, int32_t* counts);
/* Phase table of the last such call when SLAM_PGS_ITER_PROF=1 was set (a stream synchronisation after every phase; timing runs leave it
 * unset): out = {host-clock ms in simulator + append, in solve, in adopt, LM trials launched, algorithmic FLOP of the call's consumed
 * trials summed over the batch: Schur-complement SYRK, dense Cholesky + substitutions (n^3/3 + 2 n^2 at n = 2 M)}; the last three are
 * always filled. */
int pgs_last_iter_phases(pgs_handle* h, double out[6]);

/* PoseGraphState payload (pose_graph.cpp:302-387, PoseGraphState.msg): which = 0 initial_estimate, 1 result.
 * poses [timestep+1][3] (x, y, yaw), landmarks [M][2], ids [M]; any pointer may be NULL. */
int pgs_get_graph(pgs_handle* h, int instance, int which, double* poses, double* landmarks, int32_t* timestep,
                  int32_t* M, int32_t* ids);
/* msg_measurement_connections (pose_graph.cpp:176-177): pairs (timestep, landmark index; -1 for a first detection).
 * conn [cap][2]; *n = number of pairs (may exceed cap). */
int pgs_get_connections(pgs_handle* h, int instance, int32_t* conn, int cap, int32_t* n);
/* Per instance [batch]: LM iterations, lambda trials, status bits; initial / final objective, final lambda.  The objective is sum rho:
 * 0.5 |e|^2 of every prior and between factor, and of every landmark factor rho(|e|) of the loss set (pgs_set_robust; 0.5 |e|^2 without). */
int pgs_get_stats(pgs_handle* h, int32_t* iterations, int32_t* trials, int32_t* flags, double* err_init,
                  double* err_final, double* lambda);
/* compute_average_error as the pose-graph plot calls it (plotting_node.py:203-213,432-434) against the simulator's
 * true poses (pgs_run_sim), per instance [batch]; which = 0 initial graph, 1 result. */
int pgs_error_stats(pgs_handle* h, int which, double* per_instance_avg_err);
/* Work of the LAST pgs_solve summed over instances and their trials: algorithmic FLOP of the Schur-complement SYRK
 * S_ext = D - Y^T Y (2 FLOP per stored lower-triangle element and per k where its row of Y^T can be non-zero, i.e. from
 * the first detection of the row's landmark; independent of the kernel's tiling) and the number of LM trials launched. */
int pgs_last_solve_work(pgs_handle* h, double* syrk_flop, int32_t* trials_launched);
/* Per-kernel timing of pgs_solve with HIP events on the handle's stream (off by default).  ms[6] = total milliseconds
 * of the LAST solve spent in {linearize, chain, syrk, chol, backsolve, evaluate}, summed over its trials. */
int pgs_set_profiling(pgs_handle* h, int on);
int pgs_last_solve_kernel_ms(pgs_handle* h, double ms[6]);
/* The last solve run with profiling on, split by how the Schur complement was formed: out = {algorithmic SYRK FLOP of the trials
 * that ran the separate SYRK kernels, FLOP of the trials that ran the fused chain + SYRK kernel, ms spent in those SYRK
 * launches, ms spent in those fused launches, FLOP of the trials of the SEGMENTED elimination (round 5: the pose chain cut at every
 * SLAM_PGS_SEG-th pose, default 32; segments' interiors side by side, then the separators - the reference's solve,
 * pose_graph.cpp:273-300, in another exact elimination order), ms in its SYRK launches, 1 if the solve ran that order (0: a
 * segment of some instance sees more than 63 landmarks, or SLAM_PGS_SEG=0: the sequential chain of rounds 1-4), the segment length}. */
int pgs_last_solve_paths_v2(pgs_handle* h, double* out, int n /* entries of out, <= 8 */);
/* The first four entries only (the ABI of rounds 1-4; ADVICE r05: a caller with `double out[4]` must stay valid). */
int pgs_last_solve_paths(pgs_handle* h, double out[4]);

/* gtsam::Marginals(graph, values).marginalCovariance(key) for every pose and landmark of every instance (pose_graph.cpp:289-294), at the
 * values `which` (0 = initial_estimate, 1 = result; 1 needs a pgs_solve since pgs_init): with J the whitened Jacobian of all factors at
 * those values (no damping) and H = J^T J, the 3x3 diagonal block of H^-1 of every pose and the 2x2 block of every landmark.
 * Pose blocks are in the tangent coordinates of the Pose2 chart the solver uses (GTSAM's Pose2 retract: translation in the pose's OWN
 * frame, then yaw).  With R = [cos yaw, -sin yaw; sin yaw, cos yaw] of that pose, the world-frame x / y covariance is
 * R * pose_cov[0:2, 0:2] * R^T.  Landmark blocks are in world coordinates.  Every block is exactly symmetric.
 * Singular graphs: an instance whose H is not positive definite - a landmark that was created but has no stored factor (its detections
 * fell to PGS_INST_MEAS_CAP; GTSAM throws IndeterminantLinearSystemException there), or a non-positive / non-finite pivot anywhere -
 * gets status 1 and NaN in all of its blocks; no other instance is affected and pgs_get_stats' flags are not touched.
 * The call is synchronous.  Its results belong to the values they were computed at: pgs_init, pgs_update*, pgs_run_sim*, pgs_solve and
 * pgs_adopt_result invalidate them.  The outputs are allocated by the first call; the factorisation runs in the LM work space the
 * handle already has (results, pgs_get_graph and pgs_get_stats of earlier and later solves are bit for bit what they are without the
 * call).  SLAM_PGS_MARG_CHUNK = n runs the batch in launches of n instances (results do not depend on it). */
int pgs_marginals(pgs_handle* h, int which);
/* One instance's blocks: pose_cov [timestep+1][9], lm_cov [M][4] row-major, *status 0 ok / 1 singular; any pointer may be NULL.
 * SLAM_ERR_STATE before a valid pgs_marginals. */
int pgs_get_marginals(pgs_handle* h, int instance, double* pose_cov, double* lm_cov, int32_t* status);
/* The device buffers ([batch][N_max][9], [batch][L_max][4], [batch]) for a consumer on the GPU; valid until the next pgs_marginals. */
int pgs_marginals_dev(pgs_handle* h, const double** d_pose_cov, const double** d_lm_cov, const int32_t** d_status);
/* Algorithmic FLOP of the last pgs_marginals summed over instances and its HIP-event milliseconds.  Model per instance, N poses,
 * n = 2 M: 3N n^2 (triangular product, counted dense) + 12 * 3N n (chain recurrence + Gram) + 2 n^3 / 3 (R^-1 and its Gram)
 * + 3N n^2 + n^3 / 3 (the lambda = 0 factorisation: Schur complement and Cholesky). */
int pgs_last_marginals_work(pgs_handle* h, double* flop, double* ms);

/* ---- robust loss on the landmark factors ------------------------------------------------------------------------------------
 * The graph's defence against bad detections (a wrong id, a range spike): GTSAM's noiseModel::Robust on every BearingRangeFactor, solved
 * by iteratively reweighted least squares inside the same Levenberg-Marquardt loop.  With e the whitened residual of a factor and
 * r = |e|:
 *   PGS_LOSS_NONE (default)      rho = 0.5 r^2                                   w = 1
 *   PGS_LOSS_HUBER, k            rho = 0.5 r^2 (r <= k), k (r - 0.5 k) (r > k)   w = 1 (r <= k), k / r (r > k)
 *   PGS_LOSS_GEMAN_MCCLURE, k    rho = 0.5 k^2 r^2 / (k^2 + r^2)                 w = (k^2 / (k^2 + r^2))^2
 * A factor is linearised as sqrt(w) e, sqrt(w) J with w at the linearisation point (frozen over the lambda trials that share the
 * linearisation); its nonlinear cost is rho(r).  Prior and between factors stay Gaussian.  pgs_get_stats' objective is sum rho; the LM
 * accept test compares it with the weighted linearised cost.  With PGS_LOSS_NONE every result is bit for bit what it is without these calls.
 * kind unknown, or k NaN, <= 0 or +inf for a loss: SLAM_ERR_ARG (checked before the handle).  The setting may change between solves and
 * takes effect at the next pgs_solve, pgs_marginals or pgs_factor_weights, in every solve schedule and in
 * pgs_run_sim_every_iteration[_each]; pgs_marginals then linearises the weighted graph (weights at the values it is called for).  Changing
 * it invalidates the marginals and the factor weights.  One setting per handle; a loss costs 8 bytes of device memory per factor slot
 * and lambda lane, allocated by the first call that solves with it. */
enum pgs_loss_kind { PGS_LOSS_NONE = 0, PGS_LOSS_HUBER = 1, PGS_LOSS_GEMAN_MCCLURE = 2 };
int pgs_set_robust(pgs_handle* h, int kind, double k);
int pgs_get_robust(const pgs_handle* h, int* kind, double* k);
/* The weight w of every stored BearingRangeFactor at the values `which` (0 = initial_estimate, 1 = result; 1 needs a pgs_solve): which
 * detections the solve did not believe.  Device array [batch][N_max][k_per_pose] in slot order (detection s stored at pose t: [t][s], the
 * order of pgs_get_connections); slots at or beyond a pose's count hold NaN; with PGS_LOSS_NONE every stored factor gets 1.0.
 * Synchronous; changes nothing else (results and statistics are bit for bit what they are without the call); invalidated by the calls
 * that invalidate the marginals.  Its output buffer is allocated by the first call. */
int pgs_factor_weights(pgs_handle* h, int which);
/* One instance's weights: w [min(cap, *n)] of *n = (timestep + 1) * k_per_pose entries.  SLAM_ERR_STATE before a valid pgs_factor_weights. */
int pgs_get_factor_weights(pgs_handle* h, int instance, double* w, int cap, int32_t* n);
/* The device buffer for a consumer on the GPU; valid until the next pgs_factor_weights. */
int pgs_factor_weights_dev(pgs_handle* h, const double** d_w);
/* TEST HOOK, not part of the solver interface: the loss function compiled for the HOST (the same source as the kernels, no device
 * needed): rho, w and sqrt(w) at residual norm r.  Argument errors as pgs_set_robust. */
int pgs_robust_loss_host(int kind, double k, double r, double* rho, double* w, double* sw);

/* ---- absolute fixes: unary pose factors ---------------------------------------------------------------------------------------
 * A GPS position, a compass heading, a pose from motion capture: the graph-side counterpart of slam_fix (slam_batch.h).  A stretch
 * with no landmark in view is odometry integrated open loop; a fix is the factor that pulls it back.  A fix of instance b is the EKF's
 * row {z_x, z_y, z_yaw, sigma_pos, sigma_yaw} (5 doubles) plus kinds (SLAM_FIX_POS | SLAM_FIX_YAW); the rows slam_fix_sense* emits go in
 * unchanged.  It attaches to the graph's NEWEST pose (pose `timestep`) as two independent factors, in the tangent coordinates of the
 * solver's Pose2 chart; with wp = 1 / sigma_pos, wy = 1 / sigma_yaw and (s, c) = sin, cos of the pose's yaw:
 *   position   e = ((x - z_x) wp, (y - z_y) wp)          J = wp [[c, -s, 0], [s, c, 0]]
 *   heading    e = remainder(yaw - z_yaw, 2 pi) wy        J = [0, 0, wy]
 * Validation per part: PGS_FIX_ABSENT its kinds bit is clear; PGS_FIX_INVALID a z of the part or its sigma is not finite, or the sigma is
 * <= 0 (unlike the EKF, sigma = 0 is invalid here: it would be an infinite weight); PGS_FIX_STORED otherwise.
 * verdict [batch] = position | heading << 4.  A part a call carries STORED replaces that part at that pose; a part it does not carry stays.
 * Every solve schedule, pgs_marginals, pgs_run_sim_every_iteration[_each] (fixes already in the graph) and the objective of pgs_get_stats
 * honour the fixes.  Cost: 40 + 4 bytes per instance and pose capacity, allocated by the first call that attaches a fix; a handle that never
 * sees one allocates nothing and runs the kernels built without fixes, bit for bit the results of before.  pgs_init[_each] removes every fix.
 * Fix loss: each part may carry a robust loss of its own (the kinds and the function of pgs_set_robust; position: r = |e|, heading: r = |e|),
 * the graph's answer to a GPS jump that the EKF answers with a gate.  One setting per handle.  pgs_set_fix_robust and attaching a fix
 * invalidate the marginals, the factor weights and the fix weights.
 * Errors: SLAM_ERR_ARG first (NULL arrays, an unknown loss kind or a k that is NaN, <= 0 or +inf for a loss, a bad sensor row, fix_every < 1,
 * T <= 0); SLAM_ERR_STATE before pgs_init*, for the sense / run calls without a map, and when the handle's last update was dropped for pose
 * capacity (nothing is stored then).  A call that returns an error has changed nothing.
 * Not covered: full 2x2 position covariances and lever arms, per-instance loss parameters, fixes as a SOURCE inside
 * pgs_run_sim_every_iteration* (fixes already attached are honoured there), a chi-square gate (a graph has no sequential innovation; the loss
 * is its defence), slam_multi_*, checkpoint files, the UKF. */
enum pgs_fix_verdict { PGS_FIX_ABSENT = 0, PGS_FIX_STORED = 1, PGS_FIX_INVALID = 4 };
/* fix [batch][5], kinds [batch], verdict [batch] (may be NULL): HOST pointers; synchronous. */
int pgs_fix(pgs_handle* h, const double* fix, const int32_t* kinds, int32_t* verdict);
/* DEVICE pointers, read in the order of the handle's stream (e.g. slam_fix_sense_dev's outputs next to pgs_update_each_dev); never synchronises. */
int pgs_fix_dev(pgs_handle* h, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict);
int pgs_set_fix_robust(pgs_handle* h, int kind, double k);
int pgs_get_fix_robust(const pgs_handle* h, int* kind, double* k);
/* One instance's stored fixes: fix [min(cap, *n)][5], kinds [min(cap, *n)] of *n = timestep + 1 poses (kinds 0: none at that pose, its row
 * is zero; of a pose with one part the other part's entries are zero).  Any pointer may be NULL. */
int pgs_get_fixes(pgs_handle* h, int instance, double* fix, int32_t* kinds, int cap, int32_t* n);
/* The weight w of both parts of every fix at the values `which` (0 = initial_estimate, 1 = result; 1 needs a pgs_solve): which fixes the
 * solve did not believe.  Device array [batch][N_max][2] (position, heading); NaN where the part is not stored; 1.0 without a fix loss.
 * Synchronous; changes nothing else; invalidated by the calls that invalidate the marginals.  Its buffer is allocated by the first call. */
int pgs_fix_weights(pgs_handle* h, int which);
/* One instance's weights: w [min(cap, *n)][2] of *n = timestep + 1 poses.  SLAM_ERR_STATE before a valid pgs_fix_weights. */
int pgs_get_fix_weights(pgs_handle* h, int instance, double* w, int cap, int32_t* n);
int pgs_fix_weights_dev(pgs_handle* h, const double** d_w);
/* The simulated source, for the runs and the tools: slam_fix_sense's (slam_batch.h: the row format slam_fix_sensor, the draws and their
 * RNG pair indices) on the pose graph's simulator - a fix of the TRUE pose pgs_run_sim left, with the handle's seed, the global instance id
 * and the RNG step the next pgs_run_sim tick would use.  rows [batch], NULL: all-zero rows (nothing is emitted).  The truth and the RNG step
 * are read, never advanced: a following pgs_run_sim gives the bytes it gives without the call.  jumped [batch] may be NULL. */
int pgs_set_fix_sensor_each(pgs_handle* h, const slam_fix_sensor* rows);
int pgs_fix_sense(pgs_handle* h, double* fix, int32_t* kinds, int32_t* jumped);
int pgs_fix_sense_dev(pgs_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped);
/* T simulator iterations with a fix of the source after every tick t (0-based within the call) with (t + 1) % fix_every == 0: the loop of
 * pgs_run_sim[_each] over the ticks in between, pgs_fix_sense and pgs_fix, byte for byte, without the rows' trip to the host.
 * each = 0: cmds [T][2]; 1: cmds [T][batch][2]. */
int pgs_run_sim_fix(pgs_handle* h, const float* cmds, int T, int each, int fix_every);
/* TEST HOOK, not part of the solver interface: one fix factor compiled for the HOST from the kernels' source (csrc/pgs_fix.h; no device
 * needed).  e [3] and J [3][3] row-major (rows 0, 1: position, row 2: heading; rows of a part that is not STORED are zero) WITHOUT the loss;
 * rho [2], w [2] of the two parts under the loss (NaN where the part is not STORED); *verdict as pgs_fix's. */
int pgs_fix_factor_host(const double pose[3], const double row[5], int32_t kinds, int loss_kind, double loss_k, double e[3], double J[9],
                        double rho[2], double w[2], int32_t* verdict);

int pgs_sync(pgs_handle* h);
int pgs_timestep(const pgs_handle* h);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_PGS_H */
