/* slam_batch.h — C ABI of the MI355X batched EKF/UKF-SLAM predict–update engine (libslam_hip.so).
 *
 * This is the drop-in boundary for ONE path of kevin-robb/live_ekf_slam: `Filter::update()` of the EKF / UKF
 * subclasses plus the simulator's range-bearing generator.  Every entry point below names the reference
 * interface it replaces (paths relative to the reference repo root).  Plain pointers and sizes only; no
 * C++/torch types.  All functions return SLAM_OK (0) or a negative slam_status_code; slam_last_error() gives text.
 *
 * Threading: one caller thread per handle (the reference is single-threaded: localization_node.cpp:197).
 * Kernels are enqueued on one HIP stream per handle (slam_set_stream); slam_get_ and slam_sync synchronise.
 *
 * The batch: B independent filter instances.  By default they share the landmark map, the start pose and the command sequence and
 * differ only in their noise streams (Monte-Carlo seeds); the slam_*_each entry points give every instance its own start pose, map and
 * commands (several robots or scenarios in one batch, see "heterogeneous batches" below).  Instance b of this handle has GLOBAL index
 * instance_offset + b (slam_set_instance_offset), which keys its counter-based RNG stream, so results do not
 * depend on how a batch is sharded over GPUs.
 */
#ifndef SLAM_BATCH_H
#define SLAM_BATCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* FilterChoice (ekf_ws/src/localization_pkg/include/localization_pkg/filter.h:44-51) */
enum slam_filter_kind { SLAM_EKF_SLAM = 1, SLAM_UKF_LOC = 2, SLAM_UKF_SLAM = 3 };

/* storage type of x and P in HBM (arithmetic is always fp64, as in the reference's Eigen MatrixXd) */
enum slam_dtype { SLAM_F64 = 0, SLAM_F32 = 1 };

enum slam_status_code {
    SLAM_OK = 0,
    SLAM_ERR_ARG = -1,          /* bad argument / bad handle                                                  */
    SLAM_ERR_HIP = -2,          /* a HIP runtime call failed (text in slam_last_error)                          */
    SLAM_ERR_UNSUPPORTED = -3,  /* configuration not supported by this build (e.g. L_max above the kernel limit) */
    SLAM_ERR_STATE = -4,        /* call order violated (step before init, sim step before set_map, ...)        */
    SLAM_ERR_IO = -5            /* config file unreadable / malformed                                          */
};

/* per-instance status bits returned by slam_status(); an instance with any FAIL bit set is frozen, mirroring the
 * reference where the corresponding condition throws and kills the node (filter.h:5 eigen_assert -> exception). */
enum slam_instance_flags {
    SLAM_INST_OK = 0,
    SLAM_INST_NONFINITE = 1,     /* x or P became non-finite.  Checked after EVERY step of an instance that is not frozen, a step with an
                                    empty message included: the bit is set iff some stored entry of x or P (after the rounding of fp32
                                    storage) is not finite.  Sticky: no later step clears it.  The state is undefined from then on - its
                                    values need not equal the CPU checker's - but the instance keeps stepping: M, ids and the timestep
                                    follow the messages as for any other instance (a frozen instance, SLAM_INST_INDEX_OOR, does not step) */
    SLAM_INST_S_SINGULAR = 2,    /* zero pivot while inverting the 2x2 innovation covariance (ekf.cpp:135).  Sticky as well; the step
                                    goes on with the non-finite S^-1 (as the reference does), which SLAM_INST_NONFINITE then reports     */
    SLAM_INST_INDEX_OOR = 4,     /* landmark index outside x_t (ekf.cpp:115 under the duplicate/unknown-id quirk): a message repeats a
                                    NEW id that it has itself just inserted (a repeat of an id that found no room is skipped again, a
                                    repeat of a mapped id is a second update - as the reference's loop does, detection by detection) */
    SLAM_INST_CAPACITY = 8,      /* a new landmark did not fit L_max (the reference grows without limit, ekf.cpp:144-146).  NOT raised by
                                    long messages (it was, until round 5): every handle walks a message of ANY length like ekf.cpp:73 /
                                    ukf.cpp:249-287, from every entry point - the instances whose message exceeds what the LDS size class
                                    holds (EKF 20 / 50 / 100 / 200, UKF 20 / 50 detections) take that timestep through the HBM-streamed
                                    kernel (slam_step knows the counts; slam_step_dev / slam_update_dev take the caller's k_stride as the
                                    bound, so a stride within the class's capacity keeps the launch on the fast kernel alone; the
                                    simulator when the map is larger than the capacity) - bit-identical, slower for those instances */
    SLAM_INST_SQRT_FAILED = 16,  /* UKF: eigen-iteration did not converge; stale sqtP reused (ukf.cpp:207-211)  */
    SLAM_INST_WATCHDOG = 32      /* EKF: a polling loop of the step kernel's intra-workgroup protocol exceeded its budget (~0.1 s);
                                    the instance is frozen with an undefined state instead of hanging the GPU.  A defect if it ever
                                    shows (round 3's random soak raised it once: tests/test_ring_protocol_model.py)   */
};

/* Flat mirror of the YAML keys the hot path reads (ekf_ws/src/base_pkg/config/params.yaml; key names kept).
 * Filter side: Filter::readCommonParams (filter.h:105-121).  Simulator side: get_cmd (sim_node.py:209-250). */
typedef struct slam_config {
    /* process_noise.mean.{v_d,v_th} (float in filter.h:84-85), process_noise.cov.{V_00,V_11} */
    float v_d, v_th;
    double V_00, V_11;
    /* sensing_noise.mean.{w_r,w_b} (float, filter.h:88-89), sensing_noise.cov.{W_00,W_11} */
    float w_r, w_b;
    double W_00, W_11;
    /* constraints.measurements */
    int landmark_id_is_known;
    float min_landmark_separation;
    /* constraints.commands / constraints.vision — used by the measurement generator only */
    double d_max, th_max;
    double range_max, fov_min, fov_max;
    /* init_pose (params.yaml:19-22) — the simulator's start pose = the filter's init pose */
    double init_x, init_y, init_yaw;
    /* Quirk switches.  Default 1 = behave exactly like the reference.
     * replicate_vw_quirk: filter.h:116-117 store W_00,W_11 into V and leave W = I2.                       */
    int replicate_vw_quirk;
    /* UKF only: resolve unqualified cos/sin on a float argument to the float overload (1) or to double (0);
     * see SURVEY.md Appendix B precision note. */
    int ukf_float_trig;
    int reserved[2];   /* (the test oracle's batch runner keeps two private switches here; the library ignores them) */
    /* Further quirk switches (SURVEY.md Appendix D asks for one per quirk).  0 = what this build takes the reference to
     * do (default); 1 = the alternative reading, so that a maintainer with the reference binary can localise a discrepancy.
     * ekf_abs_is_int (D-6, ekf.cpp:91-92): the unqualified `abs` of the unknown-id association resolves to ::abs(int) - the difference is
     *     truncated to an int first, so the box test passes for |dx| < 1 and |dy| < 1 instead of < min_landmark_separation;
     * ekf_landmark_from_x_pred (D-2, ekf.cpp:115-116): the landmark position of an update is read from x_pred (which earlier updates of
     *     the same step have moved) instead of x_t;
     * ukf_accumulate_zest1 (D-8, ukf.cpp:310-314): z_est(1), the predicted bearing, IS accumulated as the weighted mean of the sigma
     *     points' bearings (the reference leaves it 0: S, C and the innovation then use the raw wrapped bearings);
     * ukf_sensing_yaw_from_sigma (D-9, ukf.cpp:139): sensingModel takes the yaw from its sigma-point argument (rows 2, 3 of X_pred)
     *     instead of this->x_t. */
    int ekf_abs_is_int;
    int ekf_landmark_from_x_pred;
    int ukf_accumulate_zest1;
    int ukf_sensing_yaw_from_sigma;
} slam_config;

typedef struct slam_handle slam_handle;

/* ---- configuration ------------------------------------------------------------------------------------- */
/* Fill *cfg with the values committed in the reference's params.yaml (lines 25-52). */
int slam_config_default(slam_config* cfg);
/* Minimal `key: value` reader for a params.yaml-shaped file; replaces YAML::LoadFile + readCommonParams
 * (localization_node.cpp:29-30, filter.h:105-121).  Unknown keys are ignored, missing keys keep defaults. */
int slam_config_load(slam_config* cfg, const char* yaml_path);

/* ---- lifetime ------------------------------------------------------------------------------------------ */
/* Replaces the filter factory `std::make_unique<EKF|UKF>()` + `filter->readParams(config)`
 * (localization_node.cpp:33-47).  batch = number of instances on THIS device, L_max = landmark capacity
 * (EKF_SLAM: <= 1000 in fp64 [LDS size classes 20 / 50 / 100 / 200; beyond 200 the HBM-streamed class: the same EKF::update with
 * the covariance streamed through HBM in every phase, one launch per timestep, bit-identical but slow - the state of the reference
 * grows without a limit, ekf.cpp:144-146]; fp32 storage: LDS size classes 20 / 50, the streamed class beyond; UKF_SLAM: <= 200 [LDS size classes 20 / 50, beyond 50 its HBM-streamed class]; UKF_LOC: ignored, the
 * state holds no landmarks - its map may have any size and a message any length [beyond 50 detections - 20 while the map has <= 20
 * landmarks - the instance takes the HBM-streamed step kernel]).  The reference grows the state without limit (ekf.cpp:144-146); here the limit of the
 * fast classes is what one workgroup keeps in the 160 KB of LDS of a CU, and of the streamed class 2 x n x n doubles per instance in HBM.
 * dtype SLAM_F32 (fp32 storage of x and P, fp64 arithmetic) is available for EKF_SLAM.
 * UKF results depend on the capacity CLASS: the eigen-decomposition of nearestSPD / sqrt (ukf.cpp:106-123,208) is a cyclic
 * Jacobi iteration whose pair schedule is this build's choice (the reference calls Eigen) - the LDS classes pad the state size to a multiple
 * of four and walk the schedule over quadruples, the HBM-streamed class (L_max > 50) runs the circle method over the indices - so the same
 * measurement stream gives factors that differ in the last bits between an L_max = 50 and an L_max = 51 handle (each bit-identical to the
 * oracle configured with the same L_max, each within 1e-12 of LAPACK's eigh: tests/test_oracle_ukf.py, tests/test_jacobi_schedule.py). */
int slam_create(const slam_config* cfg, int filter_kind, int batch, int L_max, int dtype, int device,
                slam_handle** out);
int slam_destroy(slam_handle* h);
/* Use an existing HIP stream (hipStream_t passed as void*) instead of the handle's own. */
int slam_set_stream(slam_handle* h, void* hip_stream);
int slam_set_instance_offset(slam_handle* h, int64_t first_global_instance);
int slam_set_seed(slam_handle* h, uint64_t seed);
/* Change the simulated sensor limits at run time (constraints.vision.*; sim_node.py:238-243). */
int slam_set_vision(slam_handle* h, double range_max, double fov_min, double fov_max);

/* ---- Filter::init (ekf.cpp:29-34, ukf.cpp:31-45; called from initCallback localization_node.cpp:90-106) -- */
/* Same start pose for every instance (all seeds share the scenario).  Also resets truth pose, timestep,
 * M, status and the error accumulators. */
int slam_init(slam_handle* h, float x_0, float y_0, float yaw_0);

/* True landmark map [L][2] (x,y), id = row index.  Needed by slam_step_sim (sim_node.py:231-236) and by
 * UKF_LOC (`filter->map`, localization_node.cpp:152-156). Host pointer. */
int slam_set_map(slam_handle* h, const double* map_xy, int L);

/* ---- Filter::update (ekf.cpp:37-179, ukf.cpp:161-195; called from iterate localization_node.cpp:131) ------ */
/* One timestep for all instances.  cmd = {fwd, ang} (Command.msg:3-5), shared by the batch.
 * meas: [batch][k_stride][3] float32 {id, range, bearing} (Float32MultiArray layout of sim_node.py:245-249,
 * padded to k_stride detections per instance); meas_count: [batch].  HOST pointers: the message is copied before the call
 * returns (mirroring `lm_meas = lmMeasMsg->data`, ekf.cpp:64), so the caller may reuse its buffers at once.  EKF: like
 * slam_step_sim, consecutive calls are queued (up to slam_set_lazy_steps timesteps, messages of at most 4 detections per
 * instance) and run as one multi-step launch; every other entry point runs what is queued first.
 * QUEUED MEANS NOT ENQUEUED: until the queue runs (it is full, another slam_* entry point is called, or slam_sync), nothing of
 * a queued step is on the handle's stream, so an event recorded or a stream synchronised right after the call sees no work
 * of that step, and a HIP error of a queued step is reported by the call that runs the queue (the queued timesteps are
 * kept, not dropped, when that launch fails).  slam_set_lazy_steps(h, 0) restores one launch per call. */
int slam_step(slam_handle* h, const float cmd[2], const float* meas, const int32_t* meas_count, int k_stride);
/* Same, with DEVICE pointers (no host copy).  The buffers are read in the order of the handle's stream: they may be
 * overwritten by work enqueued on that stream after the call returns.  By default every call enqueues its step on the stream
 * at once (caller-owned buffers on a caller-owned stream: events and stream synchronisation around the call see the step).
 * Queueing is OPT-IN for this entry point: after slam_set_lazy_steps(h, n > 1) (or with SLAM_LAZY_STEPS set) the message is
 * copied device-to-device into a queue of n entries, which run as one multi-step launch; any other entry point runs the queue
 * first, with the caveat stated at slam_step. */
int slam_step_dev(slam_handle* h, const float cmd[2], const float* d_meas, const int32_t* d_meas_count,
                  int k_stride);
/* One timestep where the device-side generator (a port of get_cmd, sim_node.py:209-250) advances each
 * instance's true pose with its own noise stream and produces its measurements, then the filter consumes
 * them in the same kernel.  Also accumulates the position error of plotting_node.py:209-212. */
int slam_step_sim(slam_handle* h, const float cmd[2]);
/* EKF: consecutive slam_step_sim / slam_step calls are queued on the host and run as one multi-step launch of up to n
 * timesteps (default 32, environment variable SLAM_LAZY_STEPS; 0 = one launch per call); every other entry point runs what is
 * queued first, so the results seen through the API do not change (a multi-step launch gives the same bits as single steps),
 * only the speed — and the moment the work reaches the stream (see slam_step).  Calling it also switches the queue of
 * slam_step_dev on (n > 1) or off. */
int slam_set_lazy_steps(slam_handle* h, int n);
/* Timesteps the per-tick entry points have accepted but not yet enqueued on the handle's stream (0 = everything the caller
 * asked for is on the stream: an event recorded now covers it). */
int slam_queued_steps(const slam_handle* h);
/* T consecutive slam_step_sim calls; cmds = [T][2] float32 host array (precomputed trajectory,
 * sim_node.py:142-152). */
int slam_run_sim(slam_handle* h, const float* cmds, int T);
/* Timesteps one kernel launch of slam_run_sim carries (EKF): 0 = the whole call (default; also the environment variable
 * SLAM_RUN_CHUNK at slam_create), 1 = one launch per timestep.  Results do not depend on it. */
int slam_set_run_chunk(slam_handle* h, int steps_per_launch);
/* UKF only: the two public halves of UKF::update, predictionStage(cmd) and updateStage(meas) (filter.h:187-188,
 * ukf.cpp:197-291).  x_t / P_t change when the update stage finishes, exactly as in the reference; the pair gives
 * bit-identical results to slam_step_dev.  d_meas / d_meas_count are DEVICE pointers (k_stride 0 = empty message). */
int slam_predict(slam_handle* h, const float cmd[2]);
int slam_update_dev(slam_handle* h, const float* d_meas, const int32_t* d_meas_count, int k_stride);

/* ---- heterogeneous batches: per-instance start poses, maps and commands ------------------------------------------------------------
 * The entry points above share one command, one start pose and one map over the batch.  These take one per instance (host pointers
 * unless marked _dev), so that one handle can hold several robots, trajectories or maps.  Every entry point above keeps its behaviour,
 * and per-instance rows that are all equal give the same bits as the shared call.
 * Queue: the _each calls run the EKF step queue (slam_set_lazy_steps) first and are not queued themselves, so shared and per-instance
 *   calls may be mixed and run in call order.
 * slam_track_instance: the shadow gets the tracked instance's row of every per-instance input.
 * Checkpoints: maps and commands are inputs, not state; slam_save_state / slam_load_state keep their format, and after a load the caller
 *   sets the maps (slam_set_maps) again as for slam_set_map.
 * The pose graph has the same forms (slam_pgs.h: pgs_init_each, pgs_set_maps, pgs_update_each[_dev], pgs_run_sim_each).
 * Per-instance noise parameters: slam_set_noise_each, below.
 * Not covered: slam_multi_*, a per-instance known map for UKF_LOC. */
/* Filter::init with one start pose per instance: pose0 [batch][3] {x, y, yaw} (float, as slam_init's arguments); truth0 [batch][3] =
 * the simulator's true start pose per instance, NULL = the config's init pose for all.  Resets what slam_init resets. */
int slam_init_each(slam_handle* h, const float* pose0, const double* truth0);
/* SIM mode: one true map per instance, maps [batch][L_stride][2], L [batch] landmarks (ids 0 .. L[b]-1; 1 <= L[b] <= L_stride).
 * Replaces the shared map; a later slam_set_map returns to the shared map.  Where the size class of a launch depends on the map (long
 * messages, slam_step_sim on a map larger than the class holds), the largest L[b] decides.  EKF and UKF_SLAM; UKF_LOC:
 * SLAM_ERR_UNSUPPORTED. */
int slam_set_maps(slam_handle* h, const double* maps, const int32_t* L, int L_stride);
/* One timestep with one command per instance, cmds [batch][2] {fwd, ang}; otherwise as slam_step / slam_step_dev (slam_step_each_dev:
 * d_cmds is a device pointer too, read in the order of the handle's stream). */
int slam_step_each(slam_handle* h, const float* cmds, const float* meas, const int32_t* meas_count, int k_stride);
int slam_step_each_dev(slam_handle* h, const float* d_cmds, const float* d_meas, const int32_t* d_meas_count, int k_stride);
/* T SIM timesteps, cmds [T][batch][2]; EKF multi-step launches and slam_set_run_chunk apply as for slam_run_sim. */
int slam_run_sim_each(slam_handle* h, const float* cmds, int T);
/* UKF only: predictionStage with cmds [batch][2]; the slam_update_dev that follows uses them.  EKF: SLAM_ERR_UNSUPPORTED. */
int slam_predict_each(slam_handle* h, const float* cmds);

/* ---- per-instance noise parameters: tuning sweeps in one batch ---------------------------------------------------------------------
 * One row per instance of what slam_config says about noise, for the filter and - independently - for the simulator, so that ONE handle
 * runs a sweep of settings (one launch per tick instead of one per setting).
 * Filter fields: v_d .. w_b and V_00 .. W_11 are the YAML keys as the FILTER reads them; the handle's replicate_vw_quirk maps them to
 *   the effective V / W exactly as for slam_config (quirk 1: V = diag(W_00, W_11), W = I2; V_00, V_11 are then not read).
 * Simulator fields: sim_V_00 .. sim_W_11 are the half-widths of get_cmd's uniform draws (sim_node.py:216-217,247-248), which slam_config
 *   takes from the same keys V_00 .. W_11.  EXT mode (slam_step*, slam_predict* / slam_update_dev) reads only the filter fields.
 * Kinds: EKF_SLAM in both storage types and every size class (the LDS classes, the HBM-streamed class, the long-message pair of
 *   launches), UKF_SLAM (LDS classes, streamed class, Cholesky square-root mode) and UKF_LOC; SIM and EXT mode; every entry point that
 *   ends in a step launch: slam_step*, slam_step_sim, slam_run_sim, the _each forms, slam_predict* / slam_update_dev, slam_nav_run,
 *   slam_monitor_run.  Instance b reads rows[b]; results do not depend on who shares the batch (an instance with row r gives the bits
 *   of a one-instance handle created from a slam_config with r's values and slam_set_instance_offset(b)).
 * Call order: the call runs the EKF step queue first, like the _each entry points: timesteps accepted before it keep the old values,
 *   later ones take the new.  It may be repeated at any time; rows = NULL returns to the handle's slam_config.  A pending UKF prediction
 *   stage (slam_predict*): SLAM_ERR_STATE.
 * Rows are inputs, not state, like the maps: slam_save_state / slam_load_state keep their format and the caller sets the rows again
 *   after a load; slam_init* does not clear them.  slam_track_instance: the shadow gets the tracked instance's row, and again when the
 *   rows change.
 * Errors: SLAM_ERR_ARG for a NULL handle and for a non-finite field (slam_last_error names the instance and the field).  No other value
 *   check: the reference has none.
 * Not covered: slam_multi_*; the pose graph (slam_pgs.h); per-instance vision limits (slam_set_vision); per-instance d_max / th_max;
 *   per-instance quirk switches; a device-side reduction of the monitor records per group of instances - a caller groups the series = 1
 *   output of slam_monitor_run or slam_consistency's per-instance values on the host. */
typedef struct slam_noise {
    float  v_d, v_th, w_r, w_b;                      /* filter: noise means, as slam_config */
    double V_00, V_11, W_00, W_11;                   /* filter: the YAML keys as the filter reads them (see above) */
    double sim_V_00, sim_V_11, sim_W_00, sim_W_11;   /* simulator: half-widths of get_cmd's uniform draws */
} slam_noise;
/* The row that reproduces the shared behaviour: filter and simulator fields both from cfg (rows all equal to it give the bits of a
 * handle without rows). */
int slam_noise_from_config(const slam_config* cfg, slam_noise* out);
/* rows: [batch], host; NULL = back to the handle's slam_config. */
int slam_set_noise_each(slam_handle* h, const slam_noise* rows);

/* ---- state export: getStateVector / publishState payload (ekf.cpp:181-220, ukf.cpp:47-104) ---------------- */
/* Sizes: x needs n_max doubles, P needs n_max*n_max doubles, ids needs L_max ints, where
 * n_max = 3+2*L_max (EKF) or 4+2*L_max (UKF).  On return *M landmarks are valid, n = 3|4 + 2*M, and P holds the
 * n x n matrix ROW-MAJOR with leading dimension n (EKFState.msg:12-13 order).  Any pointer may be NULL. */
int slam_get_state(slam_handle* h, int instance, double* x, double* P, int32_t* M, int32_t* ids,
                   int32_t* timestep);
/* UKF only — UKFState.X (ukf.cpp:92-101, UKFState.msg): the sigma points of the last prediction stage, COLUMN-major
 * rows x cols = n x (2n+1) with n = 4 + 2*M at the start of that step; X needs n_max*(2*n_max+1) doubles (may be NULL). */
int slam_get_sigma_points(slam_handle* h, int instance, double* X, int32_t* rows, int32_t* cols);
/* publishState EVERY tick at batch speed (the reference's loop is update -> publishState, localization_node.cpp:131-139).
 * Every getter runs the queued timesteps of the whole batch first, so reading one instance's state after every step call
 * would force one launch per tick.  After slam_track_instance(h, b) the library runs instance b ALSO in a one-instance shadow
 * filter - same config, seed, map and global instance id, therefore the same bits (results do not depend on how a batch is
 * partitioned) - stepped at once at every slam_step / slam_step_sim / slam_step_dev / slam_run_sim call on its own stream, and
 * slam_get_state(h, b, ...) answers from the shadow while the batch's steps stay queued.  The instance's current state is
 * copied into the shadow, so tracking may start at any time; instance = -1 switches it off.  EKF handles only (the UKF kinds
 * launch every step at the call; nothing is queued there).  (slam_step_dev: the shadow's
 * step waits for what is already enqueued on the handle's stream, since it reads the caller's device buffers.) */
int slam_track_instance(slam_handle* h, int instance);
/* Vehicle pose estimate (x, y, yaw) of every instance: [batch][3] (EKFState x_v,y_v,yaw_v). */
int slam_get_poses(slam_handle* h, double* poses);
int slam_get_landmark_counts(slam_handle* h, int32_t* M);            /* [batch] */
int slam_get_truth(slam_handle* h, double* truth_poses);             /* [batch][3], sim_node.py x_v */
/* Measurements the generator produced in the last slam_step_sim: meas [batch][k_stride][3], count [batch].  The generator only
 * keeps a copy of its messages once somebody has asked: the FIRST call (or one with a larger k_stride) switches the dump on and
 * returns count = 0 for every instance; call it once before the steps whose messages are wanted. */
int slam_get_last_meas(slam_handle* h, float* meas, int32_t* meas_count, int k_stride);
/* compute_average_error (plotting_node.py:195-218): mean over steps so far of the Euclidean position error of
 * the estimate at timestep t against the true pose of step t, per instance: [batch]. */
int slam_error_stats(slam_handle* h, double* per_instance_avg_err);
int slam_status(slam_handle* h, int32_t* per_instance_flags);       /* [batch] slam_instance_flags */

/* ---- consistency: is the covariance believable? (Bar-Shalom's NEES test over a Monte-Carlo batch) -------------------------------------
 * The reference has no counterpart (its plotter reports the position error only).  For every instance of an SLAM_EKF_SLAM handle, at
 * the handle's current state and computed on the GPU (fp64 arithmetic, whatever the storage type), with n = 3 + 2 M,
 * S = (P_t + P_t^T) / 2 and e = (x - x_true, y - y_true, remainder(yaw - yaw_true, 2 pi), and for landmark slot j:
 * (x_t[3+2j], x_t[4+2j]) - map[ids[j]]):
 *   nees_full [batch]  e^T S^-1 e (normalised estimation error squared; chi-square with n degrees of freedom for a consistent filter)
 *   nees_pose [batch]  the same with the leading 3 x 3 block of S and the first three components of e (marginal of the vehicle pose)
 *   map_rms   [batch]  sqrt(mean over the M landmark slots of the squared Euclidean landmark error); 0 when M = 0
 *   dof       [batch]  n
 *   flags     [batch]  slam_consistency_flags
 * Any output pointer may be NULL.  Truth: the vehicle pose is the simulator's (slam_get_truth; its yaw is not wrapped), the landmark
 * truth is row ids[j] of the true map (slam_set_map, or the instance's own map of slam_set_maps), ids[j] being the id stored with slot j
 * at insertion.  That is the true landmark's index only with landmark_id_is_known = 1: with unknown ids the reference numbers its
 * landmarks in order of insertion (ekf.cpp:84), so such a handle reports nees_pose and dof only (NO_TRUTH for every instance with M > 0).
 * Meaningful only while the handle is stepped by the simulator (slam_step_sim, slam_run_sim and their _each forms): with host-fed
 * measurements the handle's truth does not move, and the call does not try to detect that.
 * The call runs the queued timesteps first, computes on the handle's stream, returns when the results are on the host, and CHANGES
 * NOTHING: state, truth, error sums, counters and every later timestep are bit-identical to a run without it.  The value of an
 * instance does not depend on the batch it sits in, on a second call or on the chunking below.
 * L_max <= 50: the packed triangle of S is factored in LDS.  Beyond (up to 1000 landmarks): in a device workspace the handle owns,
 * (n + 1)(n + 2) / 2 doubles per instance, at most SLAM_CONSISTENCY_WS_BYTES (environment variable read at the call, default 256 MiB;
 * one instance at least) - the batch is then processed in chunks of as many instances as the workspace holds; slow by design.
 * Errors: SLAM_ERR_STATE before slam_init or without a true map, SLAM_ERR_UNSUPPORTED for the UKF kinds.
 * Not covered: the UKF kinds (their state carries (cos yaw, sin yaw), so P is rank-deficient along the unit circle by construction and
 *   indefinite in most steps of the benchmark scenario: a NEES there needs a definition first), slam_multi_* gathers, the pose graph
 *   (slam_pgs.h has pgs_marginals), a time series (the run monitor below records the pose part at every tick of a run and calls this
 *   evaluation at a stride), log-determinants or other information measures, guessing a landmark association for unknown ids. */
enum slam_consistency_flags {
    SLAM_CONSISTENCY_OK = 0,
    SLAM_CONSISTENCY_FULL_NOT_PD = 1,      /* a Cholesky pivot of S is <= 0 or not finite (exactly that test, no floor): nees_full = NaN, the rest
                                              is still reported.  Without a landmark truth (NO_TRUTH) only the 3 x 3 block is factored */
    SLAM_CONSISTENCY_POSE_NOT_PD = 2,      /* the same for one of the first three pivots: nees_pose = NaN as well */
    SLAM_CONSISTENCY_NO_TRUTH = 4,         /* an ids[j] outside the instance's map, or unknown-id mode with M > 0: nees_full = map_rms = NaN */
    SLAM_CONSISTENCY_INSTANCE_FAILED = 8   /* slam_status carries SLAM_INST_NONFINITE or SLAM_INST_WATCHDOG (the state is undefined), or e holds
                                              a non-finite value: everything NaN but dof, no other bit.  The other status bits leave a valid
                                              frozen or truncated state, whose numbers are reported like any other */
};
int slam_consistency(slam_handle* h, double* nees_full, double* nees_pose, double* map_rms, int32_t* dof, int32_t* flags);
/* bytes the model says the last slam_consistency had to read (sum over instances of the factored rows of P, n x ld x element size,
 * plus x, ids, the truth and the map rows) and its device time in ms (HIP events around its launches). */
int slam_last_consistency_work(slam_handle* h, double* bytes, double* ms);

/* ---- run monitor: the error and the pose NEES of the batch at EVERY tick of a run (the curves of a Monte-Carlo study) -------------------
 * slam_error_stats is one mean per instance over the whole run and slam_consistency one snapshot that factors the full matrix.  The monitor
 * evaluates, between the one-step launches of a run and on the handle's stream, for every instance at its current state (fp64 arithmetic,
 * whatever the storage type; defined once in csrc/monitor_kernel.h, restated in tests/monitor_reference.py):
 *   err_pos   [batch]  sqrt(wx wx + wy wy), wx = (double)(float)x - x_true, wy likewise: the position error of the estimate in the float32
 *                      wire format of the state message (EKFState.msg:5-6) - the summand of the handle's error sum (plotting_node.py:209-212),
 *                      so the mean of an instance's series over a run from slam_init is its slam_error_stats
 *   err_yaw   [batch]  remainder(yaw - yaw_true, 2 pi); EKF: yaw = x_t(2), UKF kinds: yaw = remainder(atan2(x_t(3), x_t(2)), 2 pi) (ukf.cpp:71)
 *   nees_pose [batch]  SLAM_EKF_SLAM, both storage types: slam_consistency's nees_pose - e^T S^-1 e with S = (P_t + P_t^T) / 2 of the leading
 *                      3 x 3 block and e = (x - x_true, y - y_true, err_yaw) in fp64, formed and factored by the same operations in the same
 *                      order (pivot test: > 0 and finite, no floor).  UKF kinds: NaN
 *   flags     [batch]  slam_consistency_flags restricted to SLAM_CONSISTENCY_POSE_NOT_PD (nees_pose = NaN) and
 *                      SLAM_CONSISTENCY_INSTANCE_FAILED (slam_status carries SLAM_INST_NONFINITE or SLAM_INST_WATCHDOG, or a component of
 *                      e is not finite: all three values NaN, no other bit).  The landmark part of the state is not looked at, so an
 *                      instance that slam_consistency fails for a non-finite LANDMARK error is a counted instance here
 * and reduces a tick to a RECORD of 16 doubles (counts are stored as doubles; sums and maxima run over the counted instances, a maximum
 * over none is 0):
 *   0 n_ok (not INSTANCE_FAILED)   1 n_failed            2 n_nees (finite nees_pose)   3 n_pose_not_pd
 *   4 sum err_pos                  5 sum err_pos^2       6 max err_pos                 7 sum err_yaw^2
 *   8 max |err_yaw|                9 sum nees_pose      10 #{nees_pose < nees_lo}     11 #{nees_pose > nees_hi}
 *  12 sum M (landmark count clamped to [0, L_max]) over the n_ok instances
 *  13 n_full  14 sum nees_full  15 sum dof: over the instances whose nees_full is finite, on the ticks with a full evaluation (else 0)
 * A per-instance value does not depend on the batch the instance sits in.  A record DOES depend on which instances share the batch: its
 * sums are formed in a fixed order that depends on the batch size alone (256 consecutive instances per workgroup by a fixed tree, then the
 * workgroups in ascending order; no atomics on values), so a record has the same bits on every run and under every chunking below, but the
 * record of a batch is not the sum of the records of its shards to the last bit.
 * Truth and meaning are those of slam_consistency: the simulator's pose, meaningful while the simulator steps the handle.
 * Errors: SLAM_ERR_ARG: nees_lo / nees_hi not finite or lo > hi, full_every < 0, unknown source, T < 0, cmds NULL for SHARED and EACH (these
 *   are checked first, before the handle is looked at), NULL handle.  SLAM_ERR_UNSUPPORTED: full_every != 0 on a UKF handle.
 *   SLAM_ERR_STATE: before slam_init; without a map; slam_monitor_run also: NAV without a path, while slam_track_instance is on, while a
 *   slam_predict is pending.
 * Not covered: a pose NEES for the UKF kinds (the reason given at slam_consistency: their P is rank-deficient by construction); per-instance
 *   nees_full series (call slam_consistency); quantiles or histograms across the batch; monitoring inside multi-step launches (the
 *   monitored run is a once-per-step run by construction: one launch per timestep, DESIGN.md 4.8 has its price); slam_multi_*; the pose
 *   graph; monitor state in checkpoint files (there is none: every call stands alone). */
typedef struct slam_monitor_config {
    double nees_lo, nees_hi;   /* the band of record entries 10 and 11 */
    int full_every;            /* N > 0: slam_consistency's evaluation also runs on every N-th tick (entries 13 - 15); 0: never */
} slam_monitor_config;
/* nees_lo = 0.21579528262389785, nees_hi = 9.348403604496148 (the chi-square quantiles at 0.025 and 0.975 for 3 degrees of freedom),
 * full_every = 0 */
int slam_monitor_config_default(slam_monitor_config* cfg);
/* One evaluation at the current state: runs the queued timesteps, computes on the handle's stream, returns when the results are on the
 * host and CHANGES NOTHING, as slam_consistency.  cfg NULL: the defaults.  rec [16]; err_pos, err_yaw, nees_pose, flags [batch]; any
 * output may be NULL.  full_every != 0: the full evaluation runs too (into the buffers of slam_consistency, chunked by its workspace rule). */
int slam_monitor_now(slam_handle* h, const slam_monitor_config* cfg, double rec[16], double* err_pos, double* err_yaw, double* nees_pose,
                     int32_t* flags);
/* T monitored ticks.  One tick = {NAV only: the controller launch; one SIM timestep, one launch; the monitor}, all on the handle's stream.
 * source SHARED: cmds [T][2] as slam_run_sim; EACH: cmds [T][batch][2] as slam_run_sim_each; NAV: cmds NULL, the commands come from the
 * controller of slam_nav_run (a path must be set).  State, truth, error sums, timestep, RNG and (NAV) the controller state advance exactly
 * as in the unmonitored run of the same commands (slam_run_sim, slam_run_sim_each, slam_nav_run): the same bits.
 * recs [T][16]; err_pos, err_yaw, nees_pose [T][batch]; any may be NULL.  full_every = N > 0: on the ticks t with (t + 1) % N == 0, t counted
 * from this call's first tick, slam_consistency's evaluation runs as well and the record gets entries 13 - 15.
 * Runs the EKF step queue first and is not queued itself.  Long runs are processed in chunks of ticks, each ending synchronised with its
 * records and series copied out: at most 4096 ticks, and at most as many as keep the per-instance series (and the commands of EACH) of a
 * chunk on the device within SLAM_MONITOR_LOG_BYTES (environment variable read at the call, default 256 MiB; one tick at least). */
enum slam_monitor_source { SLAM_MONITOR_SHARED = 0, SLAM_MONITOR_EACH = 1, SLAM_MONITOR_NAV = 2 };
int slam_monitor_run(slam_handle* h, const slam_monitor_config* cfg, int source, const float* cmds, int T, double* recs, double* err_pos,
                     double* err_yaw, double* nees_pose);
/* Device time of the last slam_monitor_run in ms, by HIP events on the handle's stream: everything (one event pair per chunk of ticks), and
 * what the monitor adds alone (its two launches and, on the ticks of a full evaluation, that one's), which needs an event pair per tick:
 * the switch is slam_nav_set_timing(h, 1); without it *monitor_ms = -1. */
int slam_last_monitor_work(slam_handle* h, double* monitor_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the monitor's per-instance function compiled for the HOST (the same source as the kernel, no
 * device needed).  One instance: x = x_t[0 .. 2] (SLAM_EKF_SLAM) or x_t[0 .. 3] (UKF kinds), P3 = the leading 3 x 3 block of P_t row-major as
 * stored (not read for the UKF kinds), truth [3], status = slam_instance_flags.  Any output may be NULL. */
int slam_monitor_instance_host(int filter_kind, const double* x, const double* P3, const double truth[3], int32_t status, double* err_pos,
                               double* err_yaw, double* nees_pose, int32_t* flags);

/* ---- innovation (NIS) statistics: judging a filter WITHOUT the truth (csrc/innovation_kernel.h) ------------------------------------------
 * slam_consistency and the monitor compare the estimate with the simulator's truth, which a handle fed recorded measurements does not
 * have.  The innovation test needs none: for each landmark update with innovation nu = z - h(x_pred) and innovation covariance
 * S = H P_pred H^T + W, NIS = nu^T S^-1 nu is chi-square with 2 degrees of freedom if the filter is consistent.  nu and S exist only inside
 * the step kernel and only for an instant; slam_innovation computes them BEFORE the step, from the pre-step state and the message the step
 * will be given, on the block of P that EKF::update confines itself to for this message (pose + the message's mapped landmarks, at most
 * 35 x 35): the same scalar operations on the same operands, so every value is what the step computes, bit for bit.
 * Per detection slot l, in message order, six doubles: (nis, nu_r, nu_b, S00, S01, S11); slots that are insertions, capacity skips or beyond
 *   the count hold NaN.  nis = nu_r (Si00 nu_r + Si01 nu_b) + nu_b (Si10 nu_r + Si11 nu_b), Si the PartialPivLU inverse of ekf.cpp:135.
 *   S01 = (S(0,1) + S(1,0)) / 2: the filter keeps P symmetric only to rounding, the step inverts S as it is, and nu^T S^-1 nu depends on S
 *   through its symmetric part (to second order in the asymmetry), so the reported values reproduce nis to rounding.  A nu or S that is not
 *   finite makes the slot's nis NaN without a flag.
 * Per instance: nis_sum (the finite nis in ascending l; 0 over none), n_upd (update slots), n_new (insertion slots, counting those skipped
 *   for capacity), post [12] = x_pred[0 .. 2] and the leading 3 x 3 block of P_pred, row-major, after the whole message and before the
 *   storage rounding: what the step will leave in x_t and P_t (rounded to float for SLAM_F32), flags (slam_innovation_flags).
 * Record, 16 doubles (counts as doubles): 0 instances evaluated, 1 INSTANCE_FROZEN, 2 TOO_LONG, 3 WOULD_FREEZE, 4 instances with S_SINGULAR,
 *   5 updates with a finite nis, 6 insertions, 7 sum nis, 8 max nis (0 over none), 9 #{nis < nis_lo}, 10 #{nis > nis_hi}, 11 sum nu_r,
 *   12 sum nu_b, 13 sum nu_r^2, 14 sum nu_b^2 (11 - 14 over the updates of entry 5), 15 reserved, 0.  Sums run in a fixed order that depends
 *   on the batch size alone (per instance in message order, 256 consecutive instances per workgroup by a fixed tree, workgroups ascending).
 * Honours slam_set_noise_each rows, slam_set_maps, the quirk switch ekf_landmark_from_x_pred, both storage types and every capacity class.
 * Errors: SLAM_ERR_ARG (checked first, before the handle is looked at): a band that is not finite or not ordered, NULL cmds, NULL meas or
 *   meas_count where they are read, k_stride <= 0, T < 0, an unknown source; NULL handle.  SLAM_ERR_UNSUPPORTED: the UKF kinds (their S
 *   depends on all sigma points: no block closes), landmark_id_is_known = 0 (that association reads every landmark of x_pred after every
 *   update).  SLAM_ERR_STATE: before slam_init; slam_innovation_run also: without a map for the simulator sources, NAV without a path, while
 *   slam_track_instance is on, while a prediction is pending.
 * Not covered: the UKF kinds; unknown ids; innovation autocorrelation / whiteness; slam_multi_*; the pose graph; evaluation inside
 *   multi-step launches (slam_innovation_run steps once per tick).  These calls reject nothing: innovation gating is slam_gate, below. */
#define SLAM_INNOV_MAX_DET 64   /* detections of one message beyond which the instance is TOO_LONG */
#define SLAM_INNOV_MAX_LM 16    /* distinct mapped landmarks of one message beyond which the instance is TOO_LONG */
enum slam_innovation_flags {
    SLAM_INNOVATION_OK = 0,
    SLAM_INNOVATION_INSTANCE_FROZEN = 1,   /* slam_status carries SLAM_INST_INDEX_OOR: the step skips the instance.  All values NaN, counts 0 */
    SLAM_INNOVATION_WOULD_FREEZE = 2,      /* the message repeats an id it inserts: the step raises SLAM_INST_INDEX_OOR and rolls back.  All NaN */
    SLAM_INNOVATION_S_SINGULAR = 4,        /* the 2 x 2 inverse failed on some slot: its nis is NaN and excluded; the replay goes on as the step does */
    SLAM_INNOVATION_TOO_LONG = 8           /* more than SLAM_INNOV_MAX_DET detections or SLAM_INNOV_MAX_LM distinct mapped landmarks.  All NaN */
};
typedef struct slam_innovation_config {
    double nis_lo, nis_hi;   /* the band of record entries 9 and 10 */
} slam_innovation_config;
/* -2 ln 0.975 and -2 ln 0.025: the 0.025 and 0.975 quantiles of chi-square with 2 degrees of freedom (0.0506356 and 7.3777589) */
int slam_innovation_config_default(slam_innovation_config* cfg);
/* What the next slam_step (cmd_each = 0: cmds [2]) or slam_step_each (cmd_each != 0: cmds [batch][2]) with these arguments will compute.
 * cfg NULL: the defaults.  Host pointers; rec [16], nis_sum / n_upd / n_new / flags [batch], det [batch][SLAM_INNOV_MAX_DET][6],
 * post [batch][12]; any output may be NULL.  Runs the queued timesteps first, computes on the handle's stream, returns with the results on
 * the host and CHANGES NOTHING: a checkpoint before and after is byte-identical. */
int slam_innovation(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* meas,
                    const int32_t* meas_count, int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                    double* det, double* post);
/* The same for slam_step_dev / slam_step_each_dev: d_meas, d_count and (cmd_each != 0) cmds are DEVICE pointers, read in stream order. */
int slam_innovation_dev(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                        const int32_t* d_count, int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                        double* det, double* post);
/* T ticks of {NAV: the controller launch; the innovation launches; the one-step launch}.  Sources SHARED (cmds [T][2]), EACH
 * (cmds [T][batch][2]) and NAV (cmds not read): the simulator generates the messages, as in slam_monitor_run, and the innovation kernel
 * regenerates each before the step does (the generator is counter based).  LOG: host-fed, cmds [T][2], meas [T][batch][k_stride][3],
 * meas_count [T][batch]; meas, meas_count and k_stride are not read by the other sources.  State, truth, error sums, timestep, RNG and
 * controller state advance bit for bit as in the plain run of the same inputs (slam_run_sim, slam_run_sim_each, slam_nav_run, a slam_step
 * loop).  recs [T][16], nis_sum / n_upd / flags [T][batch]: tick t describes the step from t to t + 1; any may be NULL.  Long runs are
 * processed in chunks of ticks exactly as slam_monitor_run does it (at most 4096 ticks, SLAM_MONITOR_LOG_BYTES, the LOG source's message
 * rows counted in); chunking changes no bit. */
enum slam_innovation_source { SLAM_INNOVATION_SHARED = 0, SLAM_INNOVATION_EACH = 1, SLAM_INNOVATION_NAV = 2, SLAM_INNOVATION_LOG = 3 };
int slam_innovation_run(slam_handle* h, const slam_innovation_config* cfg, int source, const float* cmds, const float* meas,
                        const int32_t* meas_count, int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* flags);
/* Device time of the last slam_innovation_run in ms, as slam_last_monitor_work: everything, and the innovation launches alone, which
 * needs slam_nav_set_timing(h, 1); without it *innovation_ms = -1. */
int slam_last_innovation_work(slam_handle* h, double* innovation_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the per-instance function compiled for the HOST (the same source as the kernel, no device
 * needed).  One instance: x [3 + 2 M], P row-major n x n with n = 3 + 2 M, ids [M], 0 <= M <= L_max, status = slam_instance_flags, cmd [2],
 * meas [k][3] with k >= 0 (NULL for k = 0), noise: the filter fields of one slam_noise row with V_00 .. W_11 taken as the EFFECTIVE values
 * (no replicate_vw_quirk mapping), lm_from_pred = the quirk switch, f32_storage != 0: x and P are rounded to float before they are read, as
 * the handle stores them.  Outputs as slam_innovation for one instance (det [SLAM_INNOV_MAX_DET][6], post [12]); any may be NULL. */
int slam_innovation_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                  const float* meas, int k, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                  const slam_innovation_config* cfg, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new,
                                  int32_t* flags, double* det, double* post);

/* ---- innovation gating: the chi-square gate on every detection (csrc/gate_kernel.h) -------------------------------------------------------
 * slam_innovation tells which detections the filter should not believe; the step still takes every one of them in, and one wrong
 * association or range spike bends the pose and every correlated landmark.  slam_gate runs the same replay and REJECTS an update slot iff
 * its nis is finite and nis > gate: the slot's update is not applied in the replay, and the message comes back with the rejected
 * detections taken out, in message order.  The step kernels are untouched: the unmodified step consumes the filtered message and computes
 * exactly what the gated replay computed (an update slot is a found id; the insertion, skip and freeze decisions look only at ids that
 * were not found, so removing an update slot changes no other slot's plan).  A gated step equals, byte for byte, a plain step on the
 * filtered message.
 * A slot whose nis is not finite (S_SINGULAR, a non-finite nu or S) is NEVER rejected: it goes through as the step has it.  A slot whose
 * nis equals the gate is accepted.  Instances flagged INSTANCE_FROZEN, WOULD_FREEZE or TOO_LONG pass their message through unchanged:
 * n_rej = 0, every verdict 0.
 * Outputs as slam_innovation, with these differences: a rejected slot still reports its six det values; nis_sum, post and the record's
 *   entries 5 and 7 - 14 run over the ACCEPTED updates (post is the state after them, which is what the step on the filtered message
 *   leaves); n_upd counts the update slots of the incoming message, rejected or not; record entry 15 = rejected detections.
 *   n_rej [batch]; verdict [batch][SLAM_INNOV_MAX_DET] int32 (slam_gate_verdict).
 *   Output message, with count_in = min(max(count, 0), k_stride): the kept detections in message order, count_out = their number, the
 *   triplets count_out .. count_in - 1 written as 0.0f, nothing written from count_in up.  A passed-through instance: count_out = count as
 *   given, and its first count_in triplets copied when the output is not the input.
 * Honours slam_set_noise_each rows, slam_set_maps, the quirk switch ekf_landmark_from_x_pred, both storage types and every capacity class.
 * Errors and scope as slam_innovation (argument checks first, before the handle is looked at; SLAM_ERR_UNSUPPORTED for the UKF kinds and
 *   for landmark_id_is_known = 0); also SLAM_ERR_ARG for a gate that is NaN or <= 0 (+inf is allowed: nothing is rejected) and for outputs
 *   that overlap the inputs other than in place; slam_step_gated* and slam_gate_run: SLAM_ERR_STATE while slam_track_instance is on or a
 *   prediction is pending.
 * Not covered: the simulator sources (their step generates its own message inside the step kernel; slam_gate_run_sim, "simulator source
 *   with a sensor fault model" below, puts the simulator in front of the gated step instead); slam_multi_*; the pose graph;
 *   multi-step launches (a gated step is one launch per tick); rejecting on anything but the individual NIS - there is no joint
 *   compatibility test here (id-less detections get one in slam_associate_joint, below), and a detection of an unmapped id is inserted
 *   ungated (detections without ids: slam_associate, below). */
enum slam_gate_verdict {
    SLAM_GATE_NOT_UPDATE = 0,   /* insertion, capacity skip, beyond the count, or any slot of a passed-through instance */
    SLAM_GATE_ACCEPTED = 1,
    SLAM_GATE_REJECTED = 2
};
typedef struct slam_gate_config {
    double gate;             /* reject iff nis is finite and nis > gate; > 0, may be +inf */
    double nis_lo, nis_hi;   /* the band of record entries 9 and 10, as slam_innovation_config */
} slam_gate_config;
/* gate = -2 ln 0.001 = 13.815510557964274, the 0.999 quantile of chi-square with 2 degrees of freedom; the band of
 * slam_innovation_config_default */
int slam_gate_config_default(slam_gate_config* cfg);
/* Gates the message the next slam_step (cmd_each = 0: cmds [2]) or slam_step_each (cmd_each != 0: cmds [batch][2]) would be given and
 * CHANGES NOTHING in the handle: a checkpoint before and after is byte-identical.  Host pointers; arguments and outputs as slam_innovation,
 * then meas_out [batch][k_stride][3], count_out [batch], n_rej [batch], verdict [batch][SLAM_INNOV_MAX_DET]; any output may be NULL.
 * meas_out / count_out may be meas / meas_count themselves, both or neither (one alone is SLAM_ERR_ARG).  The message is staged on the
 * device, so here meas_out comes back whole: the slots the gate does not write hold the input's values. */
int slam_gate(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* meas_count,
              int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post,
              float* meas_out, int32_t* count_out, int32_t* n_rej, int32_t* verdict);
/* The same with d_meas, d_count, (cmd_each != 0) cmds, d_meas_out and d_count_out as DEVICE pointers, read and written in stream order;
 * d_meas_out and d_count_out are required.  In place (d_meas_out == d_meas and d_count_out == d_count) is allowed; any other overlap of an
 * output with an input or with the other output is SLAM_ERR_ARG.  The other outputs are host pointers and may be NULL. */
int slam_gate_dev(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                  int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post,
                  float* d_meas_out, int32_t* d_count_out, int32_t* n_rej, int32_t* verdict);
/* One gated timestep: the gate launches into a buffer the handle owns, then the ordinary one-step launch on the filtered message, all on
 * the handle's stream; the caller's message is not written.  Run the EKF step queue first and are not queued themselves.  rec [16] and
 * n_rej [batch] (host) are optional: with both NULL the call does not synchronise.  slam_step_gated / _each take host messages (and host
 * cmds [batch][2]), the _dev forms device messages (slam_step_gated_each_dev: device cmds), as the slam_step family. */
int slam_step_gated(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* meas, const int32_t* meas_count, int k_stride,
                    double rec[16], int32_t* n_rej);
int slam_step_gated_dev(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* d_meas, const int32_t* d_count,
                        int k_stride, double rec[16], int32_t* n_rej);
int slam_step_gated_each(slam_handle* h, const slam_gate_config* cfg, const float* cmds, const float* meas, const int32_t* meas_count,
                         int k_stride, double rec[16], int32_t* n_rej);
int slam_step_gated_each_dev(slam_handle* h, const slam_gate_config* cfg, const float* d_cmds, const float* d_meas, const int32_t* d_count,
                             int k_stride, double rec[16], int32_t* n_rej);
/* T host-fed gated ticks of {the gate launches; the one-step launch on the filtered message}, in the layout of slam_innovation_run's LOG
 * source: cmds [T][2] (cmd_each != 0: [T][batch][2]), meas [T][batch][k_stride][3], meas_count [T][batch].  The state advances bit for bit
 * as T calls of slam_step_gated (slam_step_gated_each) would leave it.  recs [T][16], nis_sum / n_upd / n_rej / flags [T][batch]; any may
 * be NULL.  Chunks of ticks by the rule of slam_innovation_run (at most 4096 ticks, SLAM_MONITOR_LOG_BYTES); chunking changes no bit. */
int slam_gate_run(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* meas_count,
                  int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags);
/* Device time of the last slam_gate_run in ms, as slam_last_innovation_work: everything, and the gate launches alone, which needs
 * slam_nav_set_timing(h, 1); without it *gate_ms = -1. */
int slam_last_gate_work(slam_handle* h, double* gate_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the gate's per-instance function compiled for the HOST (the same source as the kernel, no
 * device needed).  Arguments as slam_innovation_instance_host, except: meas holds min(max(count, 0), k_stride) triplets, count is the
 * count as given and k_stride > 0 the capacity of the message row.  Extra outputs meas_out [k_stride][3] (may be meas), count_out, n_rej,
 * verdict [SLAM_INNOV_MAX_DET]; any output may be NULL. */
int slam_gate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                            const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                            const slam_gate_config* cfg, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                            double* det, double* post, float* meas_out, int32_t* count_out, int32_t* n_rej, int32_t* verdict);

/* ---- association of detections WITHOUT ids: nearest neighbour in Mahalanobis distance (csrc/assoc_kernel.h) ------------------------------
 * slam_innovation, slam_gate and the known-id step assume every detection carries a landmark id.  A range-bearing sensor without fiducials
 * gives (r, b) and nothing else; for it landmark_id_is_known = 0 offers the reference's rule (ekf.cpp:82-98), a box test on positions that
 * ignores the covariance and runs inside the step's slow path.  slam_associate labels the message instead, from the PRE-step state, on a
 * handle with landmark_id_is_known = 1: the unmodified known-id step then consumes the labelled message on its fast path, and
 * slam_innovation or slam_gate can be put in between.  The id column of the incoming message is NOT READ.
 * Cost: for detection l and mapped slot j < M, d2[l][j] is, bit for bit, the nis slam_innovation reports in slot 0 for the one-detection
 *   message [(ids[j], r_l, b_l)] at the same state, command and noise row; NaN where the 2 x 2 inverse failed or nu or S is not finite.  The
 *   quirk switch ekf_landmark_from_x_pred cannot matter: no update precedes a cost.
 * Decisions per instance, count_in = min(max(count, 0), k_stride): per detection the best finite cost (ties: lowest j) and the second best.
 *   INVALID: M > 0 and no finite cost.  NEW candidate: M == 0 or best > gate_new.  MATCH candidate: best <= gate_match.  AMBIGUOUS: the rest.
 *   A landmark is seen at most once per message: among the MATCH candidates of one slot the smallest (d2, l) wins, the others are CONFLICT
 *   and dropped.  NEW candidates in message order get rank 0, 1, ... and the id base + rank, base = 0 for M == 0, else 1 + max(ids[0 .. M));
 *   a candidate is NO_ROOM when M + rank >= L_max or when its id is not below 2^24 (a message carries ids as floats).
 * Output message: the MATCHED and NEW detections in message order as ((float)id, r, b), r and b copied bit for bit; count_out = their
 *   number; the triplets count_out .. count_in - 1 written as 0.0f; nothing written from count_in up.  In place is allowed under the
 *   gate's overlap rules.  Instances that cannot be associated emit an EMPTY message (count_out = 0, every verdict 0, the first count_in
 *   triplets zeroed), so that an unlabelled id never reaches the step: status SLAM_INST_INDEX_OOR (flag SLAM_INNOVATION_INSTANCE_FROZEN)
 *   and more than SLAM_INNOV_MAX_DET detections (flag SLAM_INNOVATION_TOO_LONG).  There is no limit on distinct landmarks.
 * Outputs, any may be NULL: verdict [batch][SLAM_INNOV_MAX_DET] int32 (slam_assoc_verdict); slot [batch][SLAM_INNOV_MAX_DET] int32, the
 *   best j or -1; det [batch][SLAM_INNOV_MAX_DET][4] doubles (d2_best, d2_second, nu_r, nu_b of the best), NaN where undefined; n_match,
 *   n_new, n_drop (ambiguous + conflict + no room + invalid), flags [batch]; meas_out, count_out as the gate's.
 * Record, 16 doubles: 0 instances evaluated, 1 FROZEN, 2 TOO_LONG, 3 detections in, 4 matched, 5 new, 6 ambiguous, 7 sum of d2_best over the
 *   matched, 8 max of d2_best over the matched (0 over none), 9 conflict, 10 no room, 11 invalid, 12 - 15 reserved, 0; summed in the fixed
 *   order of the innovation record.
 * Honours slam_set_noise_each rows, both storage types and every capacity class (L_max <= 1000).
 * Errors: SLAM_ERR_ARG (checked first, before the handle is looked at): gate_match or gate_new NaN, gate_match <= 0, gate_match > gate_new
 *   (gate_new = +inf is allowed: localisation against the map that exists, only M == 0 inserts); NULL cmds, meas or meas_count,
 *   k_stride <= 0, T < 0, outputs that overlap the inputs other than in place; NULL handle.  SLAM_ERR_UNSUPPORTED: the UKF kinds, and
 *   handles with landmark_id_is_known = 0 (those associate inside their step).  SLAM_ERR_STATE: before slam_init; slam_step_associated*
 *   and slam_associate_run also while slam_track_instance is on or a prediction is pending.
 * Not covered: joint compatibility (JCBB) - that is slam_associate_joint, below; reassigning conflict losers; the ln det S term of the full likelihood; the simulator sources (slam_associate_run_sim, below, puts the simulator in front instead);
 *   slam_multi_*; the pose graph; a fused associate-plus-gate call - chain slam_associate_dev and slam_step_gated_dev on device buffers. */
enum slam_assoc_verdict {
    SLAM_ASSOC_NONE = 0,        /* beyond the count, or any slot of an instance that emits an empty message */
    SLAM_ASSOC_MATCHED = 1,
    SLAM_ASSOC_NEW = 2,
    SLAM_ASSOC_AMBIGUOUS = 3,   /* gate_match < best <= gate_new: dropped */
    SLAM_ASSOC_CONFLICT = 4,    /* lost its landmark to a detection with a smaller (d2, l): dropped */
    SLAM_ASSOC_NO_ROOM = 5,     /* a new landmark the map or the id range has no room for: dropped */
    SLAM_ASSOC_INVALID = 6,     /* no finite cost: dropped */
    SLAM_ASSOC_JOINT_UNPAIRED = 7   /* slam_associate_joint only: had candidates, left out by the best hypothesis: dropped */
};
typedef struct slam_assoc_config {
    double gate_match;   /* a detection matches its nearest landmark iff d2_best <= gate_match; > 0 */
    double gate_new;     /* it is a new landmark iff d2_best > gate_new; >= gate_match, may be +inf */
} slam_assoc_config;
/* gate_match = -2 ln 0.01 = 9.210340371976182 and gate_new = -2 ln 1e-6 = 27.631021115928547: the 0.99 and 1 - 1e-6 quantiles of chi-square
 * with 2 degrees of freedom */
int slam_assoc_config_default(slam_assoc_config* cfg);
/* Associates the message the next slam_step (cmd_each = 0: cmds [2]) or slam_step_each (cmd_each != 0: cmds [batch][2]) would be given
 * and CHANGES NOTHING in the handle: a checkpoint before and after is byte-identical.  Host pointers; cfg NULL: the defaults.  meas_out /
 * count_out may be meas / meas_count themselves, both or neither.  The message is staged on the device, so meas_out comes back whole:
 * the slots the kernel does not write hold the input's values. */
int slam_associate(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* meas_count,
                   int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, int32_t* verdict,
                   int32_t* slot, double* det, float* meas_out, int32_t* count_out);
/* The same with d_meas, d_count, (cmd_each != 0) cmds, d_meas_out and d_count_out as DEVICE pointers, read and written in stream order;
 * d_meas_out and d_count_out are required.  In place is allowed; any other overlap is SLAM_ERR_ARG.  The other outputs are host pointers. */
int slam_associate_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                       const int32_t* d_count, int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                       int32_t* verdict, int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out);
/* One associated timestep: the association launches into a buffer the handle owns, then the ordinary one-step launch on the labelled
 * message, all on the handle's stream; the caller's message is not written.  cmd_each as above (slam_step_associated_dev with
 * cmd_each != 0: cmds is a device pointer).  rec [16] and n_drop [batch] (host) are optional: with both NULL the call does not synchronise. */
int slam_step_associated(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas,
                         const int32_t* meas_count, int k_stride, double rec[16], int32_t* n_drop);
int slam_step_associated_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop);
/* T host-fed associated ticks in the layout of slam_gate_run: cmds [T][2] (cmd_each != 0: [T][batch][2]), meas [T][batch][k_stride][3],
 * meas_count [T][batch].  The state advances bit for bit as T calls of slam_step_associated would leave it.  recs [T][16], n_match / n_new /
 * n_drop / flags [T][batch]; any may be NULL.  Chunks of ticks by the rule of slam_innovation_run; chunking changes no bit. */
int slam_associate_run(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas,
                       const int32_t* meas_count, int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                       int32_t* flags);
/* What the association launches of the last slam_associate, slam_associate_dev or slam_associate_run had to move, and the device time of
 * the last slam_associate_run.  bytes [2]: the model in bytes - per instance (3 n + 10 M) elements of P (rows 0 - 2 whole, per landmark
 * P[ii .. ii + 1][0 .. 2] and the 2 x 2 diagonal block), x, ids and the message in and out - and the same with the reads of P counted in
 * 128-byte lines (the strided column reads touch one line per row).  assoc_ms: the association launches alone, which needs
 * slam_nav_set_timing(h, 1), else -1; total_ms: the whole run; both -1 before any slam_associate_run.  Any output may be NULL. */
int slam_last_associate_work(slam_handle* h, double* bytes, double* assoc_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: associate_instance() compiled for the HOST (the same source as the kernel, no device
 * needed).  Arguments as slam_gate_instance_host (lm_from_pred is accepted and cannot matter).  Outputs, any may be NULL: rec [16], n_match,
 * n_new, n_drop, flags, cost [count_in][M] the full matrix, verdict and slot [SLAM_INNOV_MAX_DET], det [SLAM_INNOV_MAX_DET][4],
 * meas_out [k_stride][3] (may be meas), count_out. */
int slam_associate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                 const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                 const slam_assoc_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                                 double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out);

/* ---- joint-compatibility association of detections WITHOUT ids: JCBB (csrc/joint_kernel.h) ------------------------------------------------
 * slam_associate judges every detection alone.  When the pose is uncertain relative to the landmark spacing (a stretch without detections,
 * then a cluster of landmarks) every detection sits inside the individual gate of several landmarks, and nearest neighbour drops them as
 * AMBIGUOUS or CONFLICT or matches a consistently shifted set: it cannot see that the errors of all detections are tied together through
 * the pose.  slam_associate_joint judges the hypothesis as a whole (Neira and Tardos, joint compatibility branch and bound): among the
 * hypotheses whose STACKED innovation passes a chi-square test with 2 m degrees of freedom, it takes the one that pairs the most
 * detections.  Same pattern and same rules as slam_associate: a side kernel labels the message from the PRE-step state, the unmodified
 * known-id step consumes it, slam_innovation, slam_gate and the map calls chain behind it unchanged; message in and out, in place and
 * overlap rules, cmd_each, the empty message of frozen and TOO_LONG instances, NEW ranks and ids, NO_ROOM: all as there.
 * Costs: d2[l][j], nu and the per-landmark S of slam_associate, bit for bit.
 * Candidates of detection l: the slots with finite d2 <= gate_match, ascending by (d2, j); the first SLAM_JOINT_MAX_CAND are kept.  A
 *   detection without a candidate is INVALID (M > 0 and no finite cost), NEW (M == 0 or best > gate_new) or AMBIGUOUS, as there.
 * Hypotheses: every detection with candidates is paired with one of them or left unpaired; a landmark is used at most once; at most
 *   SLAM_JOINT_MAX_PAIR = SLAM_INNOV_MAX_LM pairings, so a jointly labelled message is never TOO_LONG for slam_innovation / slam_gate
 *   because of its matches.
 * Joint distance of m pairings: nu stacked; S (2 m x 2 m) with the cost phase's S_j on the diagonal and H_a P_pred[block a, block b] H_b^T
 *   off it, from the predicted state before any update (P as the handle stores it); a Cholesky factor grown by two rows per pairing (pivot
 *   test: > 0 and finite; a failed pivot makes the pairing incompatible, flag SLAM_JOINT_S_SINGULAR); d2_m = d2_{m-1} + (y^2 + y^2) with
 *   y = L^-1 nu, so the distance never decreases along a branch.  Compatible iff d2_m <= gate_joint[m - 1].  The evaluation order is fixed in
 *   csrc/joint_kernel.h.
 * Search: depth first over the detections with candidates in message order, candidates in ascending (d2, j), then the unpaired branch.
 *   Best: most pairings, then smallest joint distance, then first found.  A branch is cut when pairs + min(remaining, 16 - pairs) is
 *   below the best's pairings, or equals them while its distance is >= the best's.  A node is one attempted pairing; after max_nodes
 *   nodes the search stops with the best so far - the branch at hand, its remaining detections unpaired, competes - and the flag
 *   SLAM_JOINT_BUDGET.  The first dive is sequential-compatibility nearest neighbour.
 * Verdicts: slam_assoc_verdict, and SLAM_ASSOC_JOINT_UNPAIRED: the detection had candidates, the best hypothesis leaves it out, it is
 *   dropped and never inserted as new.
 * Outputs as slam_associate (slot: the paired slot when MATCHED, else the individual best; det: d2 and nu of the paired slot when MATCHED),
 *   then d2_joint [batch] (the best hypothesis' distance, 0 without pairings), nodes [batch], ncand [batch][SLAM_INNOV_MAX_DET] candidates
 *   kept; n_drop = ambiguous + unpaired + no room + invalid; flags: SLAM_INNOVATION_INSTANCE_FROZEN, SLAM_INNOVATION_TOO_LONG and
 *   slam_joint_flags.
 * Record, 16 doubles: 0 instances evaluated, 1 FROZEN, 2 TOO_LONG, 3 detections in, 4 matched, 5 new, 6 ambiguous, 7 sum of d2_joint, 8 max
 *   of d2_joint, 9 unpaired, 10 no room, 11 invalid, 12 sum of nodes, 13 instances with SLAM_JOINT_BUDGET, 14 instances with
 *   SLAM_JOINT_S_SINGULAR, 15 matched detections whose slot is not their individual best; summed in the fixed order of the innovation record.
 * Errors: as slam_associate (SLAM_ERR_ARG is checked first, before the handle is looked at; SLAM_ERR_UNSUPPORTED for the UKF kinds and for
 *   landmark_id_is_known = 0; SLAM_ERR_STATE before slam_init, and for the steps and the run while slam_track_instance is on or a
 *   prediction is pending); also SLAM_ERR_ARG for a gate_joint entry that is NaN, <= 0 or below its predecessor (+inf is allowed) and for
 *   max_nodes outside 1 .. 65536.
 * Not covered: the UKF kinds; the simulator sources (slam_associate_joint_run_sim, below, puts the simulator in front instead);
 *   slam_multi_*; the pose graph; joint association inside slam_manage_run /
 *   slam_manage_merge_run; the ln det S term of the full likelihood; more than 16 pairings per message. */
#define SLAM_JOINT_MAX_CAND 4    /* candidates kept per detection */
#define SLAM_JOINT_MAX_PAIR 16   /* pairings of one hypothesis */
enum slam_joint_flags {
    SLAM_JOINT_BUDGET = 16,       /* the search stopped at max_nodes */
    SLAM_JOINT_S_SINGULAR = 32,   /* a pivot of the joint Cholesky factor failed on some node: that pairing was incompatible */
    SLAM_JOINT_LM_TABLE = 64      /* more than 64 distinct candidate landmarks: the candidates beyond them were never paired */
};
typedef struct slam_joint_config {
    double gate_match;       /* the individual match gate, as slam_assoc_config */
    double gate_new;         /* the new-landmark gate, as slam_assoc_config */
    double gate_joint[16];   /* the joint gates, entry m - 1 for m pairings: > 0, non-decreasing, may be +inf */
    int32_t max_nodes;       /* the node budget of the search, 1 .. 65536 */
} slam_joint_config;
/* gate_match and gate_new of slam_assoc_config_default; gate_joint[m - 1] = the 0.99 quantile of chi-square with 2 m degrees of freedom
 * (entry 0 = gate_match); max_nodes = 2048 */
int slam_joint_config_default(slam_joint_config* cfg);
/* As slam_associate: CHANGES NOTHING in the handle.  d2_joint, nodes [batch] and ncand [batch][SLAM_INNOV_MAX_DET] may be NULL. */
int slam_associate_joint(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas,
                         const int32_t* meas_count, int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                         int32_t* flags, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out, double* d2_joint,
                         int32_t* nodes, int32_t* ncand);
/* As slam_associate_dev: d_meas, d_count, (cmd_each != 0) cmds, d_meas_out and d_count_out are DEVICE pointers. */
int slam_associate_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                             int32_t* flags, int32_t* verdict, int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out,
                             double* d2_joint, int32_t* nodes, int32_t* ncand);
/* One jointly associated timestep, as slam_step_associated*: with rec and n_drop NULL the call does not synchronise. */
int slam_step_associated_joint(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas,
                               const int32_t* meas_count, int k_stride, double rec[16], int32_t* n_drop);
int slam_step_associated_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                                   const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop);
/* T host-fed jointly associated ticks in the layout of slam_associate_run; the state advances bit for bit as T calls of
 * slam_step_associated_joint would leave it.  recs [T][16], n_match / n_new / n_drop / flags / nodes [T][batch], d2_joint [T][batch]; any may
 * be NULL.  Chunking changes no bit. */
int slam_associate_joint_run(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas,
                             const int32_t* meas_count, int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                             int32_t* flags, double* d2_joint, int32_t* nodes);
/* As slam_last_associate_work, for the last slam_associate_joint, slam_associate_joint_dev or slam_associate_joint_run: the association's
 * model plus, per node, the 2 x 2 landmark - landmark blocks of P read on demand (one per pairing already on the branch: 4 elements, one
 * 128-byte line each).  joint_ms: the joint launches alone, which needs slam_nav_set_timing(h, 1), else -1. */
int slam_last_joint_work(slam_handle* h, double* bytes, double* joint_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: joint_instance() compiled for the HOST.  Arguments and outputs as
 * slam_associate_instance_host, then d2_joint, nodes, ncand [SLAM_INNOV_MAX_DET]; any output may be NULL. */
int slam_associate_joint_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                       const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                       const slam_joint_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                                       int32_t* flags, double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out,
                                       int32_t* count_out, double* d2_joint, int32_t* nodes, int32_t* ncand);

/* ---- map management: landmarks leave the map again (csrc/map_kernel.h) ------------------------------------------------------------------
 * With slam_associate every detection farther than gate_new from the map becomes a landmark, and without the calls below nothing ever
 * leaves the map: with clutter (a false return, a moving object seen twice) the state grows until slam_associate answers
 * SLAM_ASSOC_NO_ROOM and SLAM_INST_CAPACITY sticks.  EKF handles only.
 * Removal: slam_remove_landmarks takes remove [batch][L_max] int32, nonzero = drop this slot; entries at or above M[b] are ignored.  In
 *   covariance form this is exact marginalisation: with the kept slots k0 < k1 < ... in their old order, x', ids' and P' are the
 *   sub-vector and sub-matrix on the state indices {0, 1, 2} u {3 + 2 k, 4 + 2 k}, bit for bit (NaNs included), stored at the leading
 *   dimension of the smaller state with zero pad columns; M' = M - removed; ids[M' .. L_max) and the track counters of those slots are
 *   zeroed.  Status flags, timestep, truth and err_sum are not touched, and the status is not consulted: frozen or non-finite instances
 *   move their bits like any other.  An instance with nothing to remove is not written at all.  The step kernels are unchanged: what is
 *   left is an ordinary state of fewer landmarks.  A removed id that shows up again in a known-id message is inserted as NEW by the step,
 *   and slam_associate's base = 1 + max id may hand a removed top id out again: an id names a landmark only while it is in the map.
 * Record, 16 doubles: 0 instances touched, 1 landmarks removed, 2 elements of P moved (n'^2 per touched instance), 3 - 15 reserved, 0;
 *   summed in the fixed order of the innovation record.
 * Track evidence: seen and expected, [batch][L_max] int32 each, per-handle state OUTSIDE the checkpoint format, allocated by the first
 *   call that needs them and zero after slam_init*, slam_load_state and slam_map_track_reset.  slam_map_tally, called after the step that
 *   consumed the labelled message, adds for every slot j < M of the post-step state
 *     seen_now = some triplet l < count has (int32)id == ids[j]          (an id that is NaN or outside int32 matches nothing)
 *     in_view  = !(r > range_max * range_shrink) && beta > fov_min + fov_margin && beta < fov_max - fov_margin
 *     seen[j] += seen_now;  expected[j] += seen_now || in_view
 *   with r and beta of the estimated landmark from the estimated pose (the stored x, widened for fp32 storage), computed as the simulator
 *   computes them for the true ones; range_max and fov_* are the handle's vision parameters (slam_set_vision).  An instance is skipped
 *   whole when it is frozen (SLAM_INST_INDEX_OOR), failed (SLAM_INST_NONFINITE, SLAM_INST_WATCHDOG) or its assoc_flags entry is not 0.
 * Prune rule: slam_map_prune removes slot j iff expected[j] >= min_expected && (double)seen[j] < min_ratio * (double)expected[j], decided
 *   and compacted on the device in one launch; the counters of the kept slots move with them.
 * Honours both storage types and every capacity class (L_max <= 1000).
 * Errors: SLAM_ERR_ARG (checked first, before the handle is looked at): a NULL mask, message or count, k_stride <= 0, T < 0, a map config
 *   with a NaN, range_shrink outside (0, 1], fov_margin < 0, min_expected < 1, min_ratio outside [0, 1] or prune_every < 1, the errors of
 *   the association's arguments; NULL handle.  SLAM_ERR_UNSUPPORTED: the UKF kinds (their sqtP, Vt and ages would have to follow), and
 *   for slam_step_managed* and slam_manage_run what slam_step_associated refuses.  SLAM_ERR_STATE: before slam_init, while
 *   slam_track_instance is on, while a prediction is pending.  Every call runs the queued timesteps first.
 * Not covered: merging duplicate landmarks (these calls do not merge: see "landmark merging" below, slam_map_merge); the UKF;
 *   slam_multi_*; the simulator sources (slam_manage_run_sim and slam_manage_merge_run_sim, below, put the simulator in front instead);
 *   the pose graph; counters in checkpoints. */
typedef struct slam_map_config {
    double range_shrink;    /* a landmark is expected within range_max * range_shrink; in (0, 1] */
    double fov_margin;      /* ... and at least this far inside the field of view, rad; >= 0 */
    int32_t min_expected;   /* a slot is judged once it was expected this often; >= 1 */
    double min_ratio;       /* ... and goes when seen / expected is below this; in [0, 1] */
    int32_t prune_every;    /* slam_manage_run prunes after every prune_every-th tick; >= 1 */
} slam_map_config;
/* range_shrink 0.9, fov_margin 0.1, min_expected 10, min_ratio 0.3, prune_every 10 */
int slam_map_config_default(slam_map_config* cfg);
/* remove: host pointer.  n_removed [batch] and rec [16] (host) are optional: with both NULL the call does not synchronise. */
int slam_remove_landmarks(slam_handle* h, const int32_t* remove, int32_t* n_removed, double rec[16]);
/* The same with the mask as a DEVICE pointer, read in stream order; n_removed and rec are host pointers. */
int slam_remove_landmarks_dev(slam_handle* h, const int32_t* d_remove, int32_t* n_removed, double rec[16]);
/* The tally of one labelled message (host pointers; cfg NULL: the defaults); assoc_flags [batch] may be NULL.  Does not synchronise. */
int slam_map_tally(slam_handle* h, const slam_map_config* cfg, const float* meas, const int32_t* meas_count, int k_stride,
                   const int32_t* assoc_flags);
/* The same with d_meas, d_count and d_assoc_flags as DEVICE pointers, read in stream order. */
int slam_map_tally_dev(slam_handle* h, const slam_map_config* cfg, const float* d_meas, const int32_t* d_count, int k_stride,
                       const int32_t* d_assoc_flags);
/* The prune rule on the counters as they are, then the removal, without a host round trip.  rec [16], n_removed [batch]: as above. */
int slam_map_prune(slam_handle* h, const slam_map_config* cfg, double rec[16], int32_t* n_removed);
/* The counters, [batch][L_max] each (zeros before the first tally); either may be NULL. */
int slam_map_get_track(slam_handle* h, int32_t* seen, int32_t* expected);
int slam_map_track_reset(slam_handle* h);
/* One managed timestep: the launches of slam_step_associated*, then the tally on the labelled message the handle owns, with the
 * association's flags, all on the handle's stream.  Arguments as slam_step_associated*; with rec and n_drop NULL nothing synchronises. */
int slam_step_managed(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                      const float* meas, const int32_t* meas_count, int k_stride, double rec[16], int32_t* n_drop);
int slam_step_managed_dev(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                          const float* d_meas, const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop);
/* T host-fed managed ticks in the layout of slam_associate_run; a prune follows tick t when (t + 1) % prune_every == 0, t counted within
 * the run.  The state and the counters advance bit for bit as the loop of slam_step_managed and slam_map_prune would leave them.  recs
 * [T][16], n_match / n_new / n_drop / flags [T][batch] as slam_associate_run; n_removed [T][batch], 0 on the ticks without a prune; any may
 * be NULL.  Chunks of ticks by the rule of slam_innovation_run; chunking changes no bit. */
int slam_manage_run(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                    const float* meas, const int32_t* meas_count, int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new,
                    int32_t* n_drop, int32_t* n_removed, int32_t* flags);
/* What the removals of the last slam_remove_landmarks*, slam_map_prune or slam_manage_run (all its prunes) had to move, and the device
 * times of the last slam_manage_run.  bytes: the model - per touched instance n'^2 elements of P read and written and its pads written,
 * x, ids and the counters; per instance M, its mask row below M (a prune: its two counter rows) and n_removed: an instance with nothing
 * to remove adds those few words and no P.  prune_ms: the prune launches alone, which needs slam_nav_set_timing(h, 1), else -1;
 * total_ms: the whole run; both -1 before any slam_manage_run.  Synchronises.  Any output may be NULL. */
int slam_last_map_work(slam_handle* h, double* bytes, double* prune_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the tally, the decision and the compaction of ONE instance compiled for the HOST from
 * csrc/map_kernel.h (the source the kernels compile, no device needed), in this order: the tally of (meas, count, k_stride) when meas is
 * not NULL (skipped by status and assoc_flag as on the device); then the removal of the slots of `remove` [M] (nonzero = drop) or, with
 * remove NULL and prune != 0, of the slots the prune rule picks.  x [3 + 2 M], P [n][n] packed, ids [L_max], seen / expected [L_max]
 * (may both be NULL without a tally or prune) are updated IN PLACE: P' is packed [n'][n'] at the front of P.  f32_storage: x and P are
 * rounded to float first, as the handle stores them.  mask_out [L_max] (the decision, may be NULL), M_out. */
int slam_map_instance_host(double* x, double* P, int32_t* ids, int M, int L_max, int32_t status, const float* meas, int count, int k_stride,
                           int32_t assoc_flag, double range_max, double fov_min, double fov_max, int f32_storage, const slam_map_config* cfg,
                           int32_t* seen, int32_t* expected, const int32_t* remove, int prune, int32_t* mask_out, int32_t* M_out);

/* ---- landmark merging: duplicate landmarks are found and fused (csrc/merge_kernel.h) -----------------------------------------------------
 * A detection farther than gate_new from every mapped landmark is inserted as a new one.  After the pose has drifted, or on one outlier
 * return, a landmark that is already mapped is inserted a second time; from then on the two copies split the detections, each looks
 * rarely seen to the prune rule, the state is larger than it should be and both copies keep their own error.  The prune rule can only
 * delete a copy.  The calls below fuse the two: an EKF update with the pseudo-measurement l_i - l_j = 0 (noise sigma^2 I), then the
 * exact marginalisation of slot j by the compaction of slam_remove_landmarks.  EKF handles only, both storage types, L_max <= 1000.
 * With ii = 3 + 2 i, jj = 3 + 2 j, i < j, from the stored state (widened to double for fp32 storage):
 * Cost:     delta = (x[ii] - x[jj], x[ii+1] - x[jj+1]);
 *           S[a][b] = (P[ii+a][ii+b] - P[ii+a][jj+b]) - (P[jj+a][ii+b] - P[jj+a][jj+b]) + [a == b] sigma^2 (both off-diagonal blocks of
 *           P are read: P is symmetric only to rounding); Si = the 2 x 2 LU inverse the step uses;
 *           d2 = delta0 (Si00 delta0 + Si01 delta1) + delta1 (Si10 delta0 + Si11 delta1), unfused; NaN where Si failed or delta or S is
 *           not finite.  The cost belongs to the unordered pair.
 * Decision: nn(j) = the slot with the smallest finite d2 <= gate_merge against j, ties to the lowest slot, -1 if none.  (i, j) is a
 *           duplicate iff nn(i) == j && nn(j) == i: a slot is in at most one pair, and no traversal order matters.  Instances that are
 *           non-finite, frozen or stopped by the watchdog, or with M < 2, have no pairs.
 * Fusion:   the pairs of an instance in ascending i, each on the state the previous one left: with c_r = (P[r][ii] - P[r][jj],
 *           P[r][ii+1] - P[r][jj+1]) and g_c = (P[ii][c] - P[jj][c], P[ii+1][c] - P[jj+1][c]), S and Si as above from the current state
 *           (Si failed or S not finite: the pair is skipped and counted SINGULAR), K_r = c_r Si, x[r] += K_r (-delta) (yaw wrapped as
 *           in the step), P[r][c] -= K_r g_c, stored rounded to the storage type.  Then slot j of every fused pair is removed: the kept
 *           slot is i, the kept id ids[i]; with track counters expected' = max(expected[i], expected[j]),
 *           seen[i] = min(seen[i] + seen[j], expected'), expected[i] = expected'.  Flags, timestep, truth and err_sum are untouched; an
 *           instance without a fused pair is not written.  Exact copies (S = 0 with sigma = 0) are SINGULAR; sigma > 0 fuses them.
 * Record, 16 doubles, entry 8 a maximum and every other a sum, in the fixed order of the innovation record: 0 instances touched,
 *   1 pairs fused, 2 slots with a candidate (nn >= 0) that was not mutual - for slam_merge_landmarks: entries that were ignored -,
 *   3 pairs skipped SINGULAR, 4 elements of P updated (n^2 per fused pair), 7 the sum and 8 the largest d2 of the fused pairs, each taken
 *   from the state the pair was fused on (0 without one); the rest reserved, 0.
 * Errors: SLAM_ERR_ARG (checked first, with a text, before the handle is looked at): a NULL partner array, T < 0, a merge config with
 *   gate_merge not finite or <= 0, sigma not finite or < 0, merge_every < 1, the errors of slam_manage_run's arguments; NULL handle.
 *   SLAM_ERR_UNSUPPORTED and SLAM_ERR_STATE: as slam_map_prune; slam_manage_merge_run: as slam_manage_run.
 * Not covered: the UKF; slam_multi_*; joint (multi-pair) updates; merging inside multi-step launches; counters in checkpoints. */
typedef struct slam_merge_config {
    double gate_merge;      /* a pair is a candidate when its d2 is at most this; finite and > 0 */
    double sigma;           /* standard deviation of the pseudo-measurement l_i - l_j = 0, m; finite and >= 0 */
    int32_t merge_every;    /* slam_manage_merge_run merges after every merge_every-th tick; >= 1 */
} slam_merge_config;
/* gate_merge = -2 ln 0.05, the 0.95 quantile of chi-square with 2 degrees of freedom; sigma 0: the copies are the same point; merge_every 10 */
int slam_merge_config_default(slam_merge_config* cfg);
/* The decision alone, no state change.  partner [batch][L_max] int32 (host): the slot's mutual partner, -1 if none (and at or above M);
 * d2 [batch][L_max] (host, may be NULL): the d2 of the slot's best candidate, mutual or not, NaN if it has none.  Synchronises. */
int slam_map_duplicates(slam_handle* h, const slam_merge_config* cfg, int32_t* partner, double* d2);
/* The same with DEVICE pointers, written in stream order (d_d2 may be NULL); does not synchronise. */
int slam_map_duplicates_dev(slam_handle* h, const slam_merge_config* cfg, int32_t* d_partner, double* d_d2);
/* Fuses the pairs the caller gives: partner [batch][L_max] (host).  The entry of slot s is honoured iff s < M, 0 <= partner[s] < M,
 * partner[s] != s and partner[partner[s]] == s; every other entry that is not -1 is ignored and counted (record entry 2), and an instance
 * that is non-finite, frozen or stopped by the watchdog honours none.  gate_merge is not consulted.  n_merged [batch] and rec [16] (host)
 * are optional: with both NULL the call does not synchronise. */
int slam_merge_landmarks(slam_handle* h, const slam_merge_config* cfg, const int32_t* partner, int32_t* n_merged, double rec[16]);
/* The same with the partner array as a DEVICE pointer, read in stream order. */
int slam_merge_landmarks_dev(slam_handle* h, const slam_merge_config* cfg, const int32_t* d_partner, int32_t* n_merged, double rec[16]);
/* Find, fuse and compact in one call, without a host round trip.  rec, n_merged: as above. */
int slam_map_merge(slam_handle* h, const slam_merge_config* cfg, double rec[16], int32_t* n_merged);
/* slam_manage_run's ticks, and after tick t with (t + 1) % merge_every == 0 a slam_map_merge, before that tick's prune.  The state and the
 * counters advance bit for bit as the loop of slam_step_managed, slam_map_merge and slam_map_prune would leave them.  Outputs as
 * slam_manage_run, and n_merged [T][batch], 0 on the ticks without a merge; any may be NULL.  Chunks of ticks by the rule of
 * slam_innovation_run; chunking changes no bit. */
int slam_manage_merge_run(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const slam_merge_config* merge_cfg,
                          const float* cmds, int cmd_each, const float* meas, const int32_t* meas_count, int k_stride, int T, double* recs,
                          int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* n_merged, int32_t* flags);
/* What the last slam_map_duplicates*, slam_merge_landmarks*, slam_map_merge or slam_manage_merge_run (all its merges) had to move, and
 * the device times of the last slam_manage_merge_run.  bytes: the model, summed in integers on the device outside the timed part - per
 * eligible instance of a find P and x read once; per attempted pair the gathers (8 n elements); per fused pair P and x read and written
 * once; the partner row; the compaction as slam_last_map_work counts it.  merge_ms: the merge launches alone, which needs
 * slam_nav_set_timing(h, 1), else -1; total_ms: the whole run; both -1 before any slam_manage_merge_run.  Synchronises. */
int slam_last_merge_work(slam_handle* h, double* bytes, double* merge_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the find, the fusion and the compaction of ONE instance compiled for the HOST from
 * csrc/merge_kernel.h (the source the kernels compile, no device needed).  x [3 + 2 M], P [n][n] packed, ids [L_max], seen / expected
 * [L_max] (both or neither) are updated IN PLACE: P' is packed [n'][n'] at the front of P.  f32_storage: x and P are rounded to float
 * first, as the handle stores them.  The find always runs: partner_out [L_max] and d2_out [L_max] (may be NULL).  fuse != 0: the pairs
 * of partner_in [L_max] - or, with partner_in NULL, the pairs found - are fused and their slots removed.  rec [16] (may be NULL): the
 * instance's contribution to the record; M_out. */
int slam_merge_instance_host(double* x, double* P, int32_t* ids, int M, int L_max, int32_t status, int f32_storage, const slam_merge_config* cfg,
                             int32_t* seen, int32_t* expected, const int32_t* partner_in, int fuse, int32_t* partner_out, double* d2_out,
                             double rec[16], int32_t* M_out);

/* ---- simulator source with a sensor fault model for the robust runs (csrc/sense_kernel.h) -------------------------------------------------
 * slam_gate_run, slam_associate_run, slam_associate_joint_run, slam_manage_run and slam_manage_merge_run are host-fed: their messages come
 * from a log, the handle's truth does not move, and a recorded log fixes the trajectory.  The calls below put the simulator in front of
 * them on the device: a side kernel writes the message the unmodified known-id step (or a gate, an association, a managed step in front of
 * it) is then given, with dropouts, range spikes, clutter, a shuffled order and erased ids drawn per instance from the handle's counter
 * based generator; a second side kernel commits the simulator's bookkeeping after the step, so slam_get_truth, slam_error_stats,
 * slam_monitor_now and the pose part of slam_consistency see such a run.  The step kernels are untouched.  EKF_SLAM with
 * landmark_id_is_known = 1, both storage types; honours slam_set_maps, slam_set_noise_each, per-instance commands.
 * Model, instance b (global id g = instance offset + b) at RNG step s, the step slam_step_sim would use:
 *   0. clean message: exactly slam_step_sim's - pair 0 for the motion, pair 1 + v for the v-th visible landmark in ascending id - from the
 *      instance's simulator noise, map and the vision limits.  The true pose advances into a STAGED row.  c_vis visible, the first
 *      c = min(c_vis, SLAM_SENSE_MAX_DET) are kept; more sets SLAM_SENSE_TOO_LONG.  An instance whose status carries SLAM_INST_INDEX_OOR
 *      is skipped: count 0, nothing staged, SLAM_SENSE_INSTANCE_FROZEN.
 *   1. fault draws, pair indices the clean generator never uses, F = 0x40000000: (a_v, b_v) = pair F + v, (m_v, k_v) = pair F + 64 + v for
 *      v < c; (ur_j, ub_j) = pair F + 128 + j, (e_j, kc_j) = pair F + 136 + j for clutter slot j < n_clutter.
 *   2. dropout: detection v is missed iff a_v < p_miss.
 *   3. range spike: a detection that was not missed is spiked iff b_v < p_spike; then
 *      r_out = (float)((double)r_f32 + (spike_lo + (spike_hi - spike_lo) * m_v)), r_f32 the clean float of the message.
 *   4. clutter: slot j is present iff e_j < p_clutter; r = (float)(clutter_r_min + (range_max - clutter_r_min) * ur_j),
 *      beta = (float)(fov_min + (fov_max - fov_min) * ub_j), id = (float)(L_b + j) with L_b the instance's map size: never an id of the
 *      true map - a known-id pipeline inserts it as a phantom, an id-less one never reads it.
 *   5. order: shuffle = 0: survivors in ascending v, then present clutter in ascending j; shuffle = 1: all of them ascending by
 *      (key, position in the shuffle = 0 order), keys k_v / kc_j.
 *   6. erase_ids = 1: the id column is the quiet NaN 0x7FC00000.
 *   7. output: n_out detections; the first min(n_out, k_stride) are written, the rest of the row up to k_stride as 0.0f; count = n_out
 *      (the consumers clamp as they always do).  origin [batch][k_stride] int32: the true map row, -1 for clutter and beyond the message;
 *      fault [batch][k_stride] int32: 1 spiked, else 0.
 *   Every expression is evaluated as parenthesised, in fp64, unfused.  The default row (all zero) gives slam_step_sim's message bit for bit.
 * Record, 16 doubles, every entry a sum in the fixed order of the innovation record: 0 instances sensed, 1 FROZEN, 2 TOO_LONG, 3 clean
 *   detections kept, 4 missed, 5 spiked, 6 clutter present, 7 sum of n_out, 8 sum of max(n_out - k_stride, 0), 9 sum of the spike amounts (per
 *   instance in ascending v), 10 instances committed, 11 sum of the position errors added at the commit, 12 - 15 reserved, 0.  Entries 10 and
 *   11 are the commit's: 0 in the record of slam_sense.
 * Commit, per instance, after the step: if timestep == (the timestep at the sense) + 1 the staged true pose becomes the truth and
 *   ekf_position_error of the STORED estimate (widened) against it is added to the error sum - the value the simulator step adds, in both
 *   storage types.  Otherwise nothing: an instance that froze in this step keeps its pre-step truth and error sum, as in slam_step_sim.
 * Protocol: slam_sense[_dev]; the caller's step - slam_step[_each]_dev, slam_step_gated*_dev, slam_step_associated*_dev,
 *   slam_step_managed_dev - on the message; slam_sense_commit, before any slam_map_prune or slam_map_merge of the tick (a merge can move
 *   the pose; the simulator's error is taken after the step).  The commit leaves the handle's RNG step at s + 1 however many step calls
 *   ran in between; an instance that advanced by more or less than one timestep is not committed.  While a sense is pending,
 *   SLAM_ERR_STATE for a second sense, slam_step_sim, slam_run_sim*, slam_nav_run, slam_monitor_run, slam_innovation_run with a simulator
 *   source, the *_run_sim calls and slam_save_state; slam_init* and slam_load_state clear it.
 * Rows are inputs, not state, like the noise rows: checkpoints keep their format, slam_init* does not clear them.
 * Errors: SLAM_ERR_ARG (checked first, before the handle is looked at): NULL cmds or outputs, k_stride <= 0, T < 0, an unknown source or
 *   SLAM_INNOVATION_LOG, the errors of the LOG sibling's configs; NULL handle; a sensor row with a probability outside [0, 1] or not
 *   finite, spike_lo > spike_hi or not finite, n_clutter outside 0 .. SLAM_SENSE_MAX_CLUTTER, clutter_r_min negative, not finite or above
 *   the handle's range_max (slam_last_error names the instance and the field).  SLAM_ERR_UNSUPPORTED: the UKF kinds and
 *   landmark_id_is_known = 0, state untouched.  SLAM_ERR_STATE: before slam_init, without a map, for NAV without a path, while
 *   slam_track_instance is on, while a prediction or a sense is pending; slam_sense_commit with nothing pending.
 * Not covered: the UKF kinds; the pose graph; slam_multi_*; a simulator source inside multi-step launches; wrong-id (swapped fiducial)
 *   faults; bursty or correlated faults; more than SLAM_SENSE_MAX_DET clean detections per message; the landmark part of slam_consistency
 *   on id-less runs (its truth lookup goes by the filter's own ids). */
#define SLAM_SENSE_MAX_DET 64      /* clean detections of one message (= SLAM_INNOV_MAX_DET) */
#define SLAM_SENSE_MAX_CLUTTER 8   /* clutter slots of one message */
enum slam_sense_flags {
    SLAM_SENSE_INSTANCE_FROZEN = 1,   /* status SLAM_INST_INDEX_OOR: nothing sensed, nothing staged */
    SLAM_SENSE_TOO_LONG = 2           /* more than SLAM_SENSE_MAX_DET landmarks in view: the surplus (highest ids) is not in the message */
};
typedef struct slam_sensor {
    double p_miss;          /* a clean detection is dropped with this probability */
    double p_spike;         /* a surviving detection gets a range spike with this probability */
    double spike_lo, spike_hi;   /* the spike is uniform in [spike_lo, spike_hi), m, added to the range */
    double p_clutter;       /* each of the n_clutter slots holds a false detection with this probability */
    double clutter_r_min;   /* clutter ranges are uniform in [clutter_r_min, range_max); 0 <= clutter_r_min <= range_max */
    int32_t n_clutter;      /* 0 .. SLAM_SENSE_MAX_CLUTTER */
    int32_t shuffle;        /* nonzero: the message order is random instead of ascending id */
    int32_t erase_ids;      /* nonzero: the id column is NaN */
} slam_sensor;
/* the all-off row: every field 0 */
int slam_sensor_default(slam_sensor* row);
/* rows: [batch], host; NULL = the all-off row for every instance.  Runs the step queue first, like slam_set_noise_each. */
int slam_set_sensor_each(slam_handle* h, const slam_sensor* rows);
/* One tick of the model for the command the step will be given (cmd_each = 0: cmds [2]; else cmds [batch][2]), into the caller's HOST
 * buffers: meas [batch][k_stride][3], meas_count [batch]; optional origin, fault [batch][k_stride], truth_next [batch][3] (the staged true
 * pose; a frozen instance: its pose as it is) and rec [16].  The truth is staged and a sense is pending.  Synchronises. */
int slam_sense(slam_handle* h, const float* cmds, int cmd_each, float* meas, int32_t* meas_count, int k_stride, int32_t* origin, int32_t* fault,
               double* truth_next, double rec[16]);
/* The same into DEVICE buffers, written in the order of the handle's stream (cmd_each != 0: cmds is a device pointer too); d_origin and
 * d_fault may be NULL.  Does not synchronise. */
int slam_sense_dev(slam_handle* h, const float* cmds, int cmd_each, float* d_meas, int32_t* d_count, int k_stride, int32_t* d_origin,
                   int32_t* d_fault);
/* After the caller's step: the commit of every instance, and the tick's record with entries 10 and 11 (rec may be NULL: the call does not
 * synchronise then). */
int slam_sense_commit(slam_handle* h, double rec[16]);
/* Optional HOST arrays of a *_run_sim call, any may be NULL: meas [T][batch][k_stride][3] and count [T][batch], the message as emitted,
 * before the run's own filtering; origin, fault [T][batch][k_stride]; truth [T][batch][3] after the tick's commit; err_pos [T][batch], the
 * value the commit added, NaN where not committed; cmds [T][batch][2], what the step was given (which matters for NAV);
 * recs [T][16], the sense records. */
typedef struct slam_sense_log {
    float* meas; int32_t* count; int32_t* origin; int32_t* fault; double* truth; double* err_pos; float* cmds; double* recs;
} slam_sense_log;
/* The five host-fed runs with the simulator as their source: the configs and outputs of the LOG sibling, source = SLAM_INNOVATION_SHARED
 * (cmds [T][2]), _EACH (cmds [T][batch][2]) or _NAV (cmds not read; slam_nav_set_path* first); SLAM_INNOVATION_LOG is SLAM_ERR_ARG.  A tick
 * is {NAV: the controller launch; the sense launch; the sibling's own launches and its one-step launch on that message; the commit
 * launch; the sibling's prune or merge}.  The filter state, the records and every series are, bit for bit, what the LOG sibling gives on
 * log->meas, log->count and log->cmds.  The rows of the log count in the chunk budget of slam_innovation_run; chunking changes no bit. */
int slam_gate_run_sim(slam_handle* h, const slam_gate_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                      double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags, const slam_sense_log* log);
int slam_associate_run_sim(slam_handle* h, const slam_assoc_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                           int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, const slam_sense_log* log);
int slam_associate_joint_run_sim(slam_handle* h, const slam_joint_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                                 int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint, int32_t* nodes,
                                 const slam_sense_log* log);
int slam_manage_run_sim(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, int source, const float* cmds,
                        int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* flags,
                        const slam_sense_log* log);
int slam_manage_merge_run_sim(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg,
                              const slam_merge_config* merge_cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                              int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* n_merged, int32_t* flags,
                              const slam_sense_log* log);
/* TEST HOOK, not part of the filter interface: the model of ONE instance compiled for the HOST from csrc/sense_kernel.h (the source the
 * kernel compiles, no device needed).  instance: the global id; truth [3]: the true pose before the tick; status: slam_instance_flags;
 * map_xy [L][2]; d_max, th_max: the config's command limits; sim_noise [4]: the half-widths sim_V_00, sim_V_11, sim_W_00, sim_W_11;
 * row NULL: the all-off row.  Outputs, any but meas and count may be NULL: meas [k_stride][3], count, origin and fault [k_stride],
 * truth_next [3], flags (slam_sense_flags), rec [16]. */
int slam_sense_instance_host(uint64_t seed, int64_t instance, uint32_t step, const double truth[3], const float cmd[2], int32_t status,
                             const double* map_xy, int L, double d_max, double th_max, double range_max, double fov_min, double fov_max,
                             const double sim_noise[4], const slam_sensor* row, int k_stride, float* meas, int32_t* count, int32_t* origin,
                             int32_t* fault, double truth_next[3], int32_t* flags, double rec[16]);

/* ---- absolute position and heading fixes: GPS, compass, motion capture (csrc/fix_kernel.h) ---------------------------------------------------
 * Every other measurement of the batch is a range-bearing detection of a landmark; a stretch with no landmark in view is dead reckoning
 * whose error grows without bound.  A fix is a direct measurement of the pose: of (x, y), of the yaw, or of both.  EKF_SLAM, both storage
 * types, every size class; no step, gate, association, map, merge or sense kernel changes.
 * A fix of instance b is one row fix [batch][5] of doubles {z_x, z_y, z_yaw, sigma_pos, sigma_yaw} and one int32 kinds [batch]: bit 0
 * (SLAM_FIX_POS) the position part is present, bit 1 (SLAM_FIX_YAW) the heading part; other bits are ignored.  The parts are applied
 * sequentially, position first, then heading, each on the state the previous one left (stored values, widened for fp32 storage):
 *   position: nu = (z_x - x[0], z_y - x[1]); S = P[0:2][0:2] + sigma_pos^2 I; Si = the PartialPivLU inverse the step uses;
 *             nis = nu^T Si nu; accepted: K = P[:, 0:2] Si, x += K nu (yaw wrapped as in the step), P -= K P[0:2, :]
 *   heading:  nu = the wrapped z_yaw - x[2]; S = P[2][2] + sigma_yaw^2; nis = nu^2 / S; accepted: k = P[:, 2] / S, x += k nu (yaw
 *             wrapped), P -= k P[2, :]
 *   (the exact operation order is csrc/fix_kernel.h's; results are stored rounded to the storage type).
 * Verdict of a part (slam_fix_verdict), in this order: 0 absent; INVALID: a z or the sigma of the part is not finite, or sigma < 0;
 *   SINGULAR: the inverse failed or S is not finite (heading: S not finite or <= 0), or nis is not finite; REJECTED: nis > the part's
 *   gate (a nis equal to the gate is accepted); APPLIED.  Only APPLIED writes.  verdict [batch] int32 = position | heading << 4;
 *   nis [batch][2]: the part's nis where it is APPLIED or REJECTED, NaN otherwise.
 * An instance whose status carries SLAM_INST_NONFINITE, SLAM_INST_INDEX_OOR or SLAM_INST_WATCHDOG is not written and reports verdict 0; an
 *   instance without an APPLIED part is not written at all.  M, ids, flags, timestep, truth, the error sum and the track counters are
 *   never touched.  An instance with both parts applied has its P read and written ONCE (csrc/fix_kernel.h has the argument why that
 *   equals the two sequential updates in bits).
 * Record, 16 doubles, every entry a sum in the fixed order of the sense record: 0 instances written; 1 - 5 position parts present /
 *   applied / rejected / singular / invalid; 6 - 10 the same for heading; 11, 12 the sums of the nis of the applied position and heading
 *   parts; 13 instances skipped by their status (they add to no other entry); 14, 15 reserved, 0.
 * Sense protocol: a fix belongs after slam_sense_commit, as a merge does (it moves the pose; the simulator's error is taken after the
 *   step).  While a sense waits for its commit every call of this section is SLAM_ERR_STATE.
 * Errors: SLAM_ERR_ARG (checked first, with a text, before the handle is looked at): a NULL fix or kinds array, a config with a gate that
 *   is NaN or <= 0 (+inf is allowed: nothing is rejected) or fix_every < 1, T < 0, an unknown source or SLAM_INNOVATION_LOG, NULL cmds for
 *   SHARED and EACH, NULL outputs of slam_fix_sense*; NULL handle; a sensor row with a negative or non-finite half-width or sigma, a
 *   probability outside [0, 1], jump_lo > jump_hi or not finite, kinds outside 0 .. 3 (slam_last_error names the instance and the field).
 *   SLAM_ERR_UNSUPPORTED: the UKF kinds (their P is rank-deficient in the (cos, sin) yaw pair), state untouched.  SLAM_ERR_STATE: before
 *   slam_init, while slam_track_instance is on, while a prediction or a sense is pending; slam_fix_sense* and slam_fix_run without a true
 *   map; SLAM_INNOVATION_NAV without a path.  The step queue is run first.
 * Not covered: the UKF kinds; the pose graph, whose counterpart is a unary pose factor (slam_pgs.h: pgs_fix, fed by slam_fix_sense_dev's rows unchanged); slam_multi_*; fixes inside the five *_run_sim
 *   runs and inside multi-step launches (a caller composes them from the _dev calls); full 2 x 2 position covariances; lever arms;
 *   checkpoints of the sensor rows (inputs, like noise rows). */
enum slam_fix_kinds { SLAM_FIX_POS = 1, SLAM_FIX_YAW = 2 };
enum slam_fix_verdict { SLAM_FIX_ABSENT = 0, SLAM_FIX_APPLIED = 1, SLAM_FIX_REJECTED = 2, SLAM_FIX_SINGULAR = 3, SLAM_FIX_INVALID = 4 };
typedef struct slam_fix_config {
    double gate_pos;        /* a position part is rejected when its nis exceeds this; > 0, +inf: never */
    double gate_yaw;        /* the same for a heading part */
    int32_t fix_every;      /* slam_fix_run fixes after every fix_every-th tick; >= 1 */
} slam_fix_config;
/* gate_pos = -2 ln 0.001 and gate_yaw = 10.827566170662733, the 0.999 quantiles of chi-square with 2 and 1 degrees of freedom; fix_every 10 */
int slam_fix_config_default(slam_fix_config* cfg);
/* One fix of every instance from HOST arrays fix [batch][5], kinds [batch].  verdict [batch], nis [batch][2], rec [16] (host) may each be
 * NULL; the call synchronises only when one of them is wanted.  cfg NULL: the defaults. */
int slam_fix(slam_handle* h, const slam_fix_config* cfg, const double* fix, const int32_t* kinds, int32_t* verdict, double* nis, double rec[16]);
/* The same from DEVICE arrays, read in the order of the handle's stream; d_verdict [batch], d_nis [batch][2] and d_rec [16] are device
 * pointers and may each be NULL.  Never synchronises. */
int slam_fix_dev(slam_handle* h, const slam_fix_config* cfg, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict, double* d_nis,
                 double* d_rec);
/* A simulated source of fixes of the handle's TRUE pose, for runs and tools.  Draws of instance g at RNG step s - the step the next
 * simulator step would use - from the handle's counter based generator, at pair indices neither the clean generator nor the fault model
 * (F = 0x40000000) uses, G = 0x50000000:
 *   (u0, u1) = pair G      z_x = (t_x + (2 a) u0) - a, z_y = (t_y + (2 a) u1) - a, a = pos_halfwidth
 *   (v0, v1) = pair G + 1  z_yaw = the wrapped (t_yaw + (2 h) v0) - h, h = yaw_halfwidth; the position part is missed iff v1 < p_miss_pos
 *   (j0, j1) = pair G + 2  a position part that was not missed jumps iff j0 < p_jump, by m = jump_lo + (jump_hi - jump_lo) * j1
 *   (d0, d1) = pair G + 3  in the direction phi = (2 pi d0) - pi: z_x += m cos phi, z_y += m sin phi; the heading part is missed iff
 *                          d1 < p_miss_yaw
 * kinds_out = kinds & 3 without the missed parts; the z of a part that is not emitted is 0; sigma_pos and sigma_yaw are copied.  fp64, as
 * parenthesised.  The all-zero row emits nothing.  The status is not consulted; the truth and the RNG step are read, never advanced. */
typedef struct slam_fix_sensor {
    double pos_halfwidth;   /* position noise, uniform in [-a, a) per axis, m */
    double yaw_halfwidth;   /* heading noise, uniform, rad */
    double sigma_pos;       /* what the emitted row claims, copied */
    double sigma_yaw;
    double p_miss_pos;      /* the position part is missing with this probability */
    double p_miss_yaw;
    double p_jump;          /* an emitted position jumps (multipath) with this probability */
    double jump_lo, jump_hi;   /* the jump is uniform in [jump_lo, jump_hi), m, in a uniform direction */
    int32_t kinds;          /* the parts the source emits: slam_fix_kinds, 0 .. 3 */
} slam_fix_sensor;
/* the all-zero row */
int slam_fix_sensor_default(slam_fix_sensor* row);
/* rows: [batch], host; NULL = the all-zero row for every instance.  Runs the step queue first, like slam_set_sensor_each. */
int slam_set_fix_sensor_each(slam_handle* h, const slam_fix_sensor* rows);
/* One emission into HOST arrays fix [batch][5], kinds [batch] and (may be NULL) jumped [batch].  Synchronises. */
int slam_fix_sense(slam_handle* h, double* fix, int32_t* kinds, int32_t* jumped);
/* The same into DEVICE arrays in the order of the handle's stream; d_jumped may be NULL.  Does not synchronise. */
int slam_fix_sense_dev(slam_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped);
/* T ticks.  A tick is {the command by source - SLAM_INNOVATION_SHARED (cmds [T][2]), _EACH (cmds [T][batch][2]) or _NAV (cmds not read,
 * the controller launch) -; one simulator timestep, as slam_nav_run launches it}; after tick t with (t + 1) % fix_every == 0 also {the
 * slam_fix_sense_dev launch, the slam_fix_dev launch}.  The state advances bit for bit as the loop of the single calls would leave it.
 * Optional HOST series: recs [T][16], verdict [T][batch], nis [T][batch][2], and through fix_log (may be NULL, as may its members) the
 * emitted rows fix [T][batch][5] and kinds [T][batch]; ticks without a fix give zeros, and NaN for nis.  Chunks of ticks by the rule of
 * slam_monitor_run; chunking changes no bit. */
typedef struct slam_fix_log {
    double* fix; int32_t* kinds;
} slam_fix_log;
int slam_fix_run(slam_handle* h, const slam_fix_config* cfg, int source, const float* cmds, int T, double* recs, int32_t* verdict, double* nis,
                 const slam_fix_log* fix_log);
/* What the last slam_fix*, or all the fixes of the last slam_fix_run, had to move, and the device times of the last slam_fix_run.  bytes:
 * the model, summed in integers on the device outside the timed part - per evaluated part the gather of 4 n + 2 (position) or 2 n + 1
 * (heading) elements; per instance WRITTEN, whatever its parts, P and x read and written once; the fix row, kinds, M, status, verdict and
 * nis.  fix_ms: the fix-sense and fix launches alone, which needs slam_nav_set_timing(h, 1), else -1; total_ms: the whole run; both -1
 * before any slam_fix_run.  Synchronises. */
int slam_last_fix_work(slam_handle* h, double* bytes, double* fix_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the fix of ONE instance compiled for the HOST from csrc/fix_kernel.h (the source the
 * kernel compiles, no device needed), as two sequential passes.  x [3 + 2 M], P [n][n] packed, both in place; row [5]; outputs verdict,
 * nis [2], rec [16] may be NULL. */
int slam_fix_instance_host(double* x, double* P, int M, int L_max, int32_t status, int f32_storage, const slam_fix_config* cfg, const double row[5],
                           int32_t kinds, int32_t* verdict, double nis[2], double rec[16]);
/* TEST HOOK: the simulated source of ONE instance on the host.  instance: the global id; truth [3]; row NULL: the all-zero row. */
int slam_fix_sense_instance_host(uint64_t seed, int64_t instance, uint32_t step, const double truth[3], const slam_fix_sensor* row, double fix[5],
                                 int32_t* kinds, int32_t* jumped);

/* ---- map score: the estimated map against the true map WITHOUT ids (csrc/score_kernel.h) ---------------------------------------------------
 * slam_consistency and the monitor's full evaluation look the landmark truth up through ids[j]; with landmark_id_is_known = 0 they report
 * NO_TRUTH.  This call matches every estimated landmark of every instance of an SLAM_EKF_SLAM handle to the true map by position instead
 * and reports what every SLAM paper reports: matched, duplicate and spurious landmarks, the map error, and the per-landmark and joint NEES
 * under that matching.  Known or unknown ids, both storage types, every capacity up to 1000 landmarks, the shared map or the maps of
 * slam_set_maps.  Computed on the GPU in fp64 arithmetic (unfused), whatever the storage type.
 * Definitions, per instance; M is clamped to [0, L_max], Lb is the size of the instance's true map:
 *   d2(j, r)   for slot j < M and true row r < Lb: dx = x[3+2j] - map[2r], dy = x[4+2j] - map[2r+1], d2 = dx dx + dy dy
 *   row[j]     the r of least d2, ties to the lowest r; a d2 that is not finite never wins.  If no d2 is finite or the least exceeds
 *              match_radius^2 (formed once on the host; d2 equal to it is inside): row[j] = -1 and the slot is SPURIOUS
 *   role[j]    slam_score_role: among the slots that claim one true row the one of least d2 is MATCHED (ties to the lowest j), the others
 *              are DUPLICATE; slots >= M are NONE with row = -1 and NaN values
 *   lm_err[j]  sqrt(d2) of a MATCHED or DUPLICATE slot, NaN otherwise
 *   lm_nees[j] of a MATCHED or DUPLICATE slot: the factorisation of slam_consistency on the slot's symmetrised 2 x 2 block with e = (dx, dy)
 *              appended - a = P[i][i], b = (P[i+1][i] + P[i][i+1]) / 2, c = P[i+1][i+1], i = 3 + 2 j; s0 = sqrt(a), y0 = dx / s0, l = b / s0,
 *              d = c - l l, y1 = (dy - y0 l) / sqrt(d), lm_nees = y0 y0 + y1 y1.  The pivot test is slam_consistency's (a and d > 0 and
 *              finite, no floor); a failed test gives NaN and LM_NOT_PD.  NaN otherwise
 *   n_matched, n_duplicate, n_spurious   the counts of the roles (their sum is M)
 *   map_rms    sqrt((sum of d2 over the MATCHED slots, ascending j, one addition per slot) / n_matched), 0 over none
 *   max_err    the largest lm_err over the MATCHED slots, 0 over none
 *   nees_matched, dof_matched   with full = 1: e^T S^-1 e and 3 + 2 n_matched, e = (x - x_true, y - y_true, remainder(yaw - yaw_true, 2 pi),
 *              then (dx, dy) of the MATCHED slots in ascending j) and S the principal submatrix of (P + P^T) / 2 on those rows: DUPLICATE
 *              and SPURIOUS slots are marginalised out by dropping their rows.  The factorisation, its pivot test, its size classes, its
 *              workspace and SLAM_CONSISTENCY_WS_BYTES are slam_consistency's; a failed pivot gives NaN and MATCHED_NOT_PD.  With known ids
 *              and every slot MATCHED to the row of its id, nees_matched, map_rms and dof_matched have the bits of slam_consistency's
 *              nees_full, map_rms and dof.  With full = 0: NaN and dof_matched = 0
 *   flags      slam_score_flags
 * A landmark coordinate that is not finite does not fail the instance: its slot is SPURIOUS.
 * rec [16] (counts as doubles; a fixed summation order that depends on the batch size alone): 0 instances scored (not INSTANCE_FAILED),
 *   1 failed, then over the scored ones 2 sum of M, 3 MATCHED, 4 DUPLICATE, 5 SPURIOUS slots, 6 sum of d2 over MATCHED, 7 largest lm_err over
 *   MATCHED, 8 the finite lm_nees of MATCHED slots, 9 their sum, 10 how many are < lm_lo, 11 how many are > lm_hi, 12 the finite
 *   nees_matched, 13 their sum, 14 the sum of dof_matched over those, 15 instances with at least one DUPLICATE or SPURIOUS slot.
 * Any output pointer may be NULL; the per-instance outputs are [batch], the per-slot ones [batch][L_max].  Like slam_consistency the call
 * runs the queued timesteps first, computes on the handle's stream, returns when the results are on the host, and CHANGES NOTHING: a
 * checkpoint written before and after is byte-identical.  The values of an instance do not depend on the batch it sits in, on a second
 * call or on the chunking of the workspace class.  Meaningful for the pose part only while the simulator steps the handle.
 * Errors: SLAM_ERR_ARG (checked first, before the handle is looked at): match_radius NaN or <= 0 (+inf is allowed: nothing is SPURIOUS
 *   for its distance), a band that is not finite or not ordered; NULL handle.  SLAM_ERR_UNSUPPORTED: the UKF kinds.  SLAM_ERR_STATE: before
 *   slam_init; without a true map.
 * Not covered: optimal (Hungarian) assignment or Mahalanobis matching (the matching is greedy per true row, in Euclidean distance); which
 *   true rows were ever in view (the caller holds the origin logs of the simulator source; Lb - n_matched is what the call can say); the
 *   UKF kinds, slam_multi_* and the pose graph; a *_run form or a stride inside the monitor (the call changes nothing, so a caller scores
 *   between the chunks of any run); checkpoint state (there is none). */
typedef struct slam_score_config {
    double match_radius;   /* > 0, may be +inf (default): a slot farther than this from every true row is SPURIOUS */
    double lm_lo, lm_hi;   /* band of record entries 10 / 11; default: the chi-square(2) quantiles slam_innovation_config_default uses */
    int full;              /* 0: matching and per-landmark values only (default); 1: also nees_matched (a factorisation per instance) */
} slam_score_config;
enum slam_score_role { SLAM_SCORE_NONE = 0, SLAM_SCORE_MATCHED = 1, SLAM_SCORE_DUPLICATE = 2, SLAM_SCORE_SPURIOUS = 3 };
enum slam_score_flags {
    SLAM_SCORE_OK = 0,
    SLAM_SCORE_MATCHED_NOT_PD = 1,     /* full = 1: a Cholesky pivot of the selected submatrix is <= 0 or not finite: nees_matched = NaN, the rest
                                          is still reported */
    SLAM_SCORE_LM_NOT_PD = 4,          /* the same for the 2 x 2 block of a MATCHED or DUPLICATE slot: that slot's lm_nees = NaN */
    SLAM_SCORE_INSTANCE_FAILED = 8     /* as SLAM_CONSISTENCY_INSTANCE_FAILED: slam_status carries SLAM_INST_NONFINITE or SLAM_INST_WATCHDOG, or a
                                          component of the pose error is not finite: every value NaN, counts and dof_matched 0, row = -1,
                                          role NONE, no other bit */
};
int slam_score_config_default(slam_score_config* cfg);
int slam_map_score(slam_handle* h, const slam_score_config* cfg /* NULL: defaults */, double rec[16], int32_t* n_matched, int32_t* n_duplicate,
                   int32_t* n_spurious, double* map_rms, double* max_err, double* nees_matched, int32_t* dof_matched, int32_t* flags, int32_t* row,
                   int32_t* role, double* lm_err, double* lm_nees);
/* bytes the model says the last slam_map_score had to move (summed in integers on the device, outside the timed part: x, the 2 x 2 diagonal
 * blocks of the slots with a row, the map once, M, status and truth, the outputs; with full = 1 also the selected elements of P and the
 * list they are selected by - nothing else of P is read with full = 0) and its device time in ms (HIP events around its launches). */
int slam_last_score_work(slam_handle* h, double* bytes, double* ms);
/* TEST HOOK, not part of the filter interface: the scoring of ONE instance compiled for the HOST from csrc/score_kernel.h (the source the
 * kernel compiles, no device needed).  x [3 + 2 M], P [n][n] row-major, 0 <= M <= L_max, truth [3], map [L][2], L >= 1; the outputs are the
 * per-instance ones except nees_matched / dof_matched (single values) and the per-slot ones ([L_max] each); any may be NULL. */
int slam_map_score_instance_host(const double* x, const double* P, int M, int L_max, int32_t status, const double truth[3], const double* map, int L,
                                 int f32_storage, const slam_score_config* cfg, int32_t* n_matched, int32_t* n_duplicate, int32_t* n_spurious,
                                 double* map_rms, double* max_err, int32_t* flags, int32_t* row, int32_t* role, double* lm_err, double* lm_nees);

/* ---- closed loop: commands from each instance's own estimate (goal_pursuit_node.py:23-50, pure_pursuit.py:17-161) ---------------------
 * The entry points above run open loop: every command is fixed before the run.  The reference's default launch (sim_base.launch,
 * precompute_trajectory false) closes the loop instead: goal_pursuit_node computes each Command from the state the filter has just published.
 * slam_nav_run does that on the device for every instance: one tick = {controller kernel, one SIM timestep with per-instance commands},
 * both on the handle's stream, no host round trip.
 * The controller is a restatement of PurePursuit.get_next_cmd / pare_path / choose_lookahead_pt / cmd_loose / cmd_tight (method SLAM_NAV_PP)
 * and direct_nav (SLAM_NAV_DIRECT), defined once in csrc/nav_kernel.h and mirrored in live_ekf_slam_amd/navigation.py:
 *   estimate in   the wire values of the state message, x_v, y_v, yaw_v rounded to float32 (EKFState.msg:5-7; UKF: yaw_v =
 *                 remainder(atan2(x_t(3), x_t(2)), 2 pi), ukf.cpp:71) - slam_nav_estimates returns exactly these
 *   command out   float32 (Command.msg) after the clamps to [0, d_max] and [-th_max, th_max] of the handle's slam_config
 *   state         per instance: head (index of the first waypoint still queued: the queue is always a suffix of the path, since pare_path
 *                 deletes up to the FIRST queued waypoint within 0.15 m, which need not be the head - a path that passes near itself is
 *                 cut short as in the reference), integ, err_prev, finish_tick (the first tick whose command was issued with an empty
 *                 queue, counted from the last reset; -1 until then)
 *   arithmetic    fp64; powers are multiplication chains (x^4 = (x x)(x x), x^12 = x^8 x^4, the cube x x x), distances sqrt, atan2 the
 *                 library's deterministic one, the heading error IEEE remainder(., 2 pi); no fused multiply-add
 * Guards the reference lacks: consecutive equal waypoints are refused with SLAM_ERR_ARG when a path is set (the reference divides by zero
 * there); an instance whose estimate is not finite, or which is frozen (SLAM_INST_INDEX_OOR), gets the command (0, 0) and keeps its
 * controller state.
 * Setting a path resets the controller state; slam_init and slam_init_each reset it too and keep the path.
 * Kinds: EKF_SLAM in both storage types, UKF_SLAM, UKF_LOC; works with slam_set_maps.
 * Errors: SLAM_ERR_STATE before slam_init, before a path is set, without a map, or while slam_track_instance is on; SLAM_ERR_ARG for a bad
 * config (dt <= 0, a lookahead distance that is not positive and finite, more than 64 lookahead radii, unknown method or control), a bad
 * path (no points, more than 1024, a non-finite coordinate, consecutive equal waypoints) or T < 0.
 * Not covered: planning the path (A*, the occupancy map, the local planner, click goals) - the caller brings the waypoints; the zero
 *   "kick-off" command the reference's simulator publishes first (issue slam_step_sim with (0, 0) before slam_nav_run for it); controller
 *   state in slam_save_state files; slam_multi_*; a controller on the pose graph's own estimate (a pose graph FOLLOWS such a run: cmds_out,
 *   the measurement dump and slam_get_poses of every tick go to pgs_update_each, slam_pgs.h). */
enum slam_nav_method { SLAM_NAV_PP = 0, SLAM_NAV_DIRECT = 1 };     /* path_planning.nav_method "pp" | "direct" ("simple" = direct) */
enum slam_nav_control { SLAM_NAV_LOOSE = 0, SLAM_NAV_TIGHT = 1 };  /* the launch file's tight_control (goal_pursuit_node.py:158-161) */
typedef struct slam_nav_config {
    double dt, lookahead_dist_init, lookahead_dist_max;            /* params.yaml:14,83-84 */
    int method, control;
} slam_nav_config;
/* dt 0.05, lookahead 0.2 .. 2 m, "pp" (params.yaml:14,81-84), loose control (sim_base.launch) */
int slam_nav_config_default(slam_nav_config* cfg);
/* Reads dt, nav_method, lookahead_dist_init, lookahead_dist_max from a params.yaml-shaped file, as slam_config_load: missing keys keep
 * what *cfg holds (control is an argument of the launch file, not a key).  SLAM_ERR_IO: unreadable file, unknown nav_method. */
int slam_nav_config_load(slam_nav_config* cfg, const char* yaml_path);
/* One path for every instance: pts [P][2] (x, y), host pointer, 1 <= P <= 1024. */
int slam_nav_set_path(slam_handle* h, const slam_nav_config* cfg, const double* pts, int P);
/* One path per instance: pts [batch][P_stride][2], P [batch] waypoints each (1 <= P[b] <= P_stride <= 1024). */
int slam_nav_set_paths(slam_handle* h, const slam_nav_config* cfg, const double* pts, const int32_t* P, int P_stride);
/* T ticks of {controller, one SIM timestep}.  Runs the EKF step queue first and is not queued itself; advances truth, error sums,
 * timestep and RNG exactly as T calls of slam_run_sim_each(h, cmds, 1) with the same commands would.  cmds_out: host [T][batch][2], the
 * commands issued (NULL: not wanted).  SLAM_ERR_STATE also while a slam_predict is pending.  Returns when the ticks are done.  Long runs
 * are processed in chunks of ticks by the rule of slam_monitor_run, each ending synchronised with its rows of cmds_out copied out: at most
 * 4096 ticks, and - when cmds_out is given - at most as many as keep the command log of a chunk (8 bytes per instance and tick) within
 * SLAM_MONITOR_LOG_BYTES (default 256 MiB; one tick at least).  Chunking changes no bit. */
int slam_nav_run(slam_handle* h, int T, float* cmds_out);
/* Controller state, [batch] each, any pointer may be NULL: remaining = waypoints still queued. */
int slam_nav_state(slam_handle* h, int32_t* remaining, int32_t* finish_tick, double* integ, double* err_prev);
/* The estimates the next controller tick would read: est [batch][3] float32 (x_v, y_v, yaw_v), the state message's wire values. */
int slam_nav_estimates(slam_handle* h, float* est);
/* Device time of the last slam_nav_run in ms, by HIP events on the handle's stream: everything (one event pair per chunk of ticks, always),
 * and the controller kernels alone.  The latter needs an event pair around every controller launch, which is off by default:
 * slam_nav_set_timing(h, 1) switches it on for the following runs (0: off again); without it *controller_ms = -1. */
int slam_nav_set_timing(slam_handle* h, int per_tick);
int slam_last_nav_work(slam_handle* h, double* controller_ms, double* total_ms);
/* TEST HOOK, not part of the filter interface: the controller's tick function compiled for the HOST (the same source as the kernel, no
 * device needed), so that the restatement and the argument checks can be tested where there is no GPU.  One instance, one tick.
 * d_max / th_max: the clamps; est: wire values; frozen != 0: the instance is frozen; tick: ticks since the reset.  head, finish_tick,
 * integ, err_prev are read and updated in place; cmd receives (fwd, ang).  SLAM_ERR_ARG as for slam_nav_set_path. */
int slam_nav_tick_host(const slam_nav_config* cfg, double d_max, double th_max, const double* pts, int P, const float est[3], int frozen,
                       int tick, int32_t* head, int32_t* finish_tick, double* integ, double* err_prev, float cmd[2]);

/* ---- scenario generators (host side; sim_node.py:63-206) ------------------------------------------------------ */
/* generate_landmarks + generate_full_trajectory of the reference simulator for one scenario seed (the reference seeds
 * CPython's Mersenne Twister; the same generator is implemented in include/slam_scenario.hpp, so a seed gives the reference's
 * map and command sequence bit for bit).  map_type: "random" | "grid" | "demo" | "igvc1" (the two fixed maps are read from
 * fixed_maps_json = live_ekf_slam_amd/data/fixed_maps.json; num_landmarks is ignored for them and for "grid").
 * Out: map_xy [*num_landmarks_out][2] (may be NULL to query the count; capacity in landmarks), cmds [num_iterations][2] float32
 * (fwd, ang) = the Command messages of sim_node.py:142-152.  Runs on the host; no GPU needed. */
int slam_scenario_make(const char* map_type, const char* fixed_maps_json, uint64_t seed, int num_landmarks, int num_iterations,
                       double* map_xy, int map_capacity, int32_t* num_landmarks_out, float* cmds);

/* ---- checkpoint / resume --------------------------------------------------------------------------------- */
/* The reference keeps the filter only in memory (a killed node loses the run).  slam_save_state writes everything a handle
 * needs to continue - x, P, landmark counts and ids, status, timestep, the simulator's true pose, the error accumulators,
 * the RNG step / seed / instance offset (UKF: also the square root of the last prediction stage and the warm-start
 * eigenvectors) - to one binary file (raw slabs, 64 MB at a time through the host); slam_load_state restores it into a handle
 * created with the same kind, batch, L_max and dtype (the map, the config and the sensor limits are the caller's to set
 * again).  A run continued from a loaded state is bit-identical to the uninterrupted one. */
int slam_save_state(slam_handle* h, const char* path);
int slam_load_state(slam_handle* h, const char* path);

/* ---- misc ------------------------------------------------------------------------------------------------ */
int slam_sync(slam_handle* h);
int slam_batch(const slam_handle* h);
int slam_state_dim_max(const slam_handle* h);
/* Algorithmic HBM bytes of the last step summed over instances: sum_b 2*(n_b^2+n_b)*sizeof(storage)
 * (SURVEY.md §8d).  Computed on the device from the per-instance M; synchronises. */
int slam_algorithmic_bytes(slam_handle* h, double* bytes);
/* Workload statistics: instance-steps by the number of detections in their message (out[k] for k = 0..6, out[7] for
 * k >= 7), accumulated by the EKF / UKF step kernels since slam_create or the last reset (ekf.cpp:65 `num_landmarks`).  The cost
 * of EKF::update grows with k (one rank-2 downdate of P per detection, ekf.cpp:140), so a throughput figure is only
 * meaningful together with this histogram.  Synchronises. */
int slam_k_histogram(slam_handle* h, uint64_t out[8], int reset);
/* UKF handles: out[0] = Jacobi sweeps that rotated at least one pair, out[1] = eigen-decompositions (instance-steps), summed
 * by the square-root kernel since slam_create or the last reset: out[0] / out[1] is the mean number of sweeps the
 * `nearestSPD` + `.sqrt()` of ukf.cpp:106-123,208 took, which sets the arithmetic of a UKF step.  Synchronises. */
int slam_ukf_sweep_stats(slam_handle* h, uint64_t out[2], int reset);
/* UKF matrix square root of every step (UKF_SLAM and UKF_LOC handles).
 * SLAM_UKF_SQRT_EIGEN (default): nearestSPD + `.sqrt()` of ukf.cpp:106-123,208, a symmetric eigen-decomposition, bit-identical to the
 *   reference.
 * SLAM_UKF_SQRT_CHOLESKY: an opt-in mode that is NOT bit-identical to the reference and pays off only where P is positive
 *   definite, which the reference's signed process noise (ukf.cpp:183-186) rarely leaves: on the reference configuration most steps
 *   fall back and the mode is SLOWER than the default.  Each step forms
 *   Y = 0.5 (P + P^T) * float((2M+4)/(1-W_0)) exactly as nearestSPD does, factors Y = L L^T with a lower-triangular L and takes the
 *   columns of L as the sigma-point offsets, X_i = x +- L(:, i-1).  L L^T = Y gives sigma points with the same first two moments as the
 *   symmetric root.  sqtP (slam_get_sigma_points) then holds L^T row-major, zeros below its diagonal.  If a pivot
 *   d_k = Y_kk - sum_j L_kj^2 is <= 1e-8 (the floor of nearestSPD's cwiseMax) or not finite, that instance takes the eigen path for
 *   that step, starting Jacobi cold: every Cholesky step discards the warm-start eigenvectors.  Such a fallback is counted, not
 *   flagged (the step succeeded).  Everything after the square root is unchanged.  The mode persists until set again and is not
 *   part of a state file.  A handle that has taken Cholesky steps is no longer bit-identical to the reference after switching back
 *   (its warm start was reset).
 * Returns SLAM_ERR_ARG for EKF handles or an unknown mode, SLAM_ERR_UNSUPPORTED for the Cholesky mode on the HBM-streamed size class
 * (UKF_SLAM with L_max > 50), which has no Cholesky kernel. */
enum slam_ukf_sqrt_mode { SLAM_UKF_SQRT_EIGEN = 0, SLAM_UKF_SQRT_CHOLESKY = 1 };
int slam_ukf_set_sqrt_mode(slam_handle* h, int mode);
/* UKF handles: out[0] = Cholesky factorisations that succeeded, out[1] = instance-steps that fell back to the eigen path, since
 * slam_create or the last reset (also zeroed by slam_reset_counters_async).  SLAM_ERR_ARG for EKF handles.  Synchronises. */
int slam_ukf_sqrt_stats(slam_handle* h, uint64_t out[2], int reset);
/* EKF handles: what the step kernels moved through global memory, counted ON THE DEVICE (one accumulation per pass and
 * workgroup, summed per launch like the k histogram) since slam_create or the last reset: out[0] = bytes the passes of the
 * P stream read + wrote (`P -= K (H P)`, ekf.cpp:140, applied for a group of deferred updates at once), out[1] = every other
 * global byte (thin row / column gathers, the vehicle rows / columns the prediction changes, x / ids / scalars at launch
 * start and end), out[2] = passes, out[3] = rank-2 updates those passes applied.  bench.py's roofline.traffic is
 * out[0] + out[1] of the timed launches; profiles/r03* hold the rocprofv3 PMC cross-check.  Synchronises. */
int slam_traffic_counters(slam_handle* h, uint64_t out[4], int reset);
/* Zero the counters of slam_k_histogram and slam_traffic_counters in stream order (no host synchronisation): for measurements that
 * must not leave the device idle between their warm-up and their timed launches (bench.py). */
int slam_reset_counters_async(slam_handle* h);
/* The step-kernel instantiation this handle launches (multi_step != 0: the multi-step launch of slam_run_sim / the queues,
 * else the one-step launch): name as rocprofv3 prints it (e.g. "ekf_step_kernel<103,4,4,4,double,1,true>"), and
 * out = {static LDS bytes per workgroup, VGPRs, threads per workgroup, workgroups one CU holds at once, CUs of the device}.
 * Needs a HIP device (the runtime is asked, nothing is hard-coded). */
int slam_kernel_info(slam_handle* h, int multi_step, char* name, int name_cap, int32_t out[5]);
/* Diagnostics: flag 32 = every workgroup of the EKF multi-step kernel stamps the wall clock and its detection count per
 * timestep (read back by the profiling tools / bench.py's per-k table), flag 4 = per-phase cycle counters; 0 = off (default;
 * the environment variable SLAM_DEBUG_FLAGS sets the initial value).
 * TEST-ONLY flags, accepted here and never from the environment variable: 128 = the pass leader of the EKF multi-step kernel loses
 * its `applied` update, so the control wavefront starves and the watchdog must flag the instance (SLAM_INST_WATCHDOG); 1024 = the
 * control wavefront's look at its ring slot always answers "full", so every update of the decoupled loop finishes its thin work
 * before it waits for the slot and is published (the order an update takes when the ring is full) - whether the ring is full
 * depends on timing, and a test must not.  Results are the same bits with and without 1024. */
int slam_set_debug_flags(slam_handle* h, int flags);
/* Build introspection: 1 if the library holds the EKF step-kernel tuning variant `variant` (code PIPE*1000 + W*100 + KG*10 +
 * UNR, selected per handle by the environment variable SLAM_WAVES_PER_FILTER) for landmark capacity L_max and storage
 * dtype; 0 = the default, always present.  Release builds hold the defaults only; asking a handle for a variant the build
 * lacks makes its steps fail with SLAM_ERR_HIP. */
int slam_variant_available(int L_max, int dtype, int variant);
/* Diagnostics: evaluate the device's elementary functions on host arrays a[n], b[n]; out[8*n] =
 * {sin a, cos a, atan2(a,b), remainder(a,2pi), sqrt|a|, a/b, (double)(float)a, u53 noise} per element.
 * Used by the parity tests to prove the device math is bit-identical to the host's. */
int slam_math_probe(const double* a, const double* b, double* out, int n, int device);
/* Diagnostics: ONE of the functions the kernels share with the CPU oracle (slam_math.h, slam_rng.h) or the UKF kernels' own
 * wrappers, evaluated on the device for every item of the host arrays a..d[n]; results in out[n][out_per_item] (out_per_item >= the
 * op's result count; further entries of an item keep their values).  Arrays an op does not read may be NULL.
 *   op  reads                          writes per item
 *   0   a                              sin, cos                      (det_sincos)
 *   1   a = y, b = x                   det_atan2(y, x)
 *   2   a                              rem2pi(a), wrap2pi(a)         (the short-cut, the device library's remainder(a, 2 pi))
 *   3   a, b                           sqrt(a), a / b, (double)(float)a
 *   4   a, b, c, d = S row-major       Si[0..3], ok (1 / 0)          (inv2x2_lu)
 *   5   a, b = as_int (0 / not 0)      assoc_abs(a, as_int)
 *   6   a, b = float_trig (0 / not 0)  sin, cos of tsincos((float)a, float_trig)   (the UKF kernels' unqualified sin / cos)
 *   7   a = cos, b = sin               yaw_of(cos, sin)              (the UKF kernels' (float) remainder(atan2(sin, cos), 2 pi))
 *   8   a..d = counters, packed        u0, u1 of noise_pair(seed, inst, t, p)
 * Packing of op 8, every value an integer below 2^48 and so exact in a double: a = seed mod 2^48, b = inst mod 2^48,
 * c = (seed >> 48) + 65536 * t, d = (inst >> 48) + 65536 * p.
 * Used by tests/test_math_edges_gpu.py, which compares every result with the host's bit for bit. */
int slam_math_probe2(int op, const double* a, const double* b, const double* c, const double* d, double* out, int out_per_item, int n, int device);
const char* slam_last_error(void);
const char* slam_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SLAM_BATCH_H */
