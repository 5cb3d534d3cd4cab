// pgs_handle.h — the pose-graph handle of the C ABI (include/slam_pgs.h), shared by the translation units that implement it: pgs_capi.cpp
// (graph building, the solve, marginals, the landmark factors' loss) and pgs_capi_fix.cpp (absolute fixes).  Not installed, not part of the ABI.
#pragma once
#include "../../include/slam_pgs.h"

#include <hip/hip_runtime.h>

#include <vector>

#include "capi_internal.h"
#include "host/pgs_schedule.h"
#include "pgs_kernel.h"

struct pgs_handle {
    slam_config cfg;
    int B, N_max, L_max, KP, LD, device;
    int timestep = 0;                          // p.N = timestep + 1 at every launch: written by pgs_init[_each] and advance() only, each with p.N
    bool inited = false;
    bool solved = false;                       // a pgs_solve has run since pgs_init: `result` exists
    hipStream_t stream = nullptr;
    bool own_stream = false;
    uint64_t seed = 2025;
    int64_t inst0 = 0;
    slam::PgsParams p;
    // The device arrays behind p's pointer fields, each with the address of the field it backs (bind_arrays writes it).  slot_bytes > 0:
    // a per-slot array the clones (lambda lanes) get a copy of when a solve begins (clone_instances / clone_listed), bytes per slot.
    struct Array { DevBuf<char> buf; void** field; size_t slot_bytes; };
    std::vector<Array> arrays;                 // sized by pgs_create
    std::vector<Array> seg_arrays;             // sized for segments of seg_alloc poses (segT joins on first use): replaced as a whole by resize_segments
    DevBuf<double> map;                        // p.map
    DevBuf<float> dcmds;                       // p.cmds while the handle has seen shared calls only: one row [N_max][2]
    // Heterogeneous batches (pgs_*_each).  dcmds_each: one row of BetweenFactor measurements per instance, [B][N_max][2] floats = 8 B N_max
    // bytes (16 MB at batch 2048 with N_max = 1000; 0.1 % of that handle's LM work space), allocated by the first per-instance command and
    // kept for the handle's lifetime; p.cmds then points at it (ensure_cmds_each).  Not per slot: the lambda lanes read their instance's row.
    DevBuf<float> dcmds_each;
    DevBuf<float> dcmd_stage;                  // host commands on their way into the rows ([T][B][2] or [T][2])
    DevBuf<double> dmaps; DevBuf<int32_t> dLs; // pgs_set_maps: p.map_each [B][map_stride][2], p.L_each [B]
    DevBuf<float> dpose_each; DevBuf<double> dtruth_each;   // pgs_init_each's staging, [B][3] each
    DevBuf<float> dmeas; DevBuf<int32_t> dcount; DevBuf<double> dsec;   // pgs_update's staging
    DevBuf<double> dout;
    // The tuning values (host/pgs_schedule.h), read from the environment by pgs_create.  Of these, `lanes` may shrink there (the lanes multiply
    // the LM work space), and `groups` / `slots` follow pgs_set_groups / pgs_set_slots.
    //  * solve groups: the batch is split into contiguous ranges whose LM loops run on their own streams, so the latency-bound phases of one
    //    group overlap the bandwidth-bound phases of another;
    //  * streaming (pgs_kernel.h "streaming"): at most `slots` graphs of the batch are in flight (0 = lockstep: all of them), split over the
    //    solve groups; trials are enqueued `stream_depth` ahead of the host's reading of their counters.
    slam_host::PgsTuning tune;
    std::vector<hipStream_t> gstreams;
    std::vector<hipEvent_t> gevents;
    PinnedDefaultBuf<int32_t> h_active;        // pinned host: per-group active counts
    DevBuf<int32_t> d_cnt;                     // device [kPgsMaxGroups][2][8]: the counter blocks, ping-pong by trial parity
    DevBuf<int32_t> d_wait;                    // device [kPgsMaxGroups]: the groups' wait cursors
    PinnedDefaultBuf<int32_t> h_ring;          // pinned host [kPgsMaxGroups][kPgsRing][8]
    std::vector<hipEvent_t> ring_events;       // [kPgsMaxGroups][kPgsRing]
    std::vector<std::vector<int32_t>> timeline;   // per group: slots that ran in every trial of the last solve
    DevBuf<int32_t> d_tick;                    // [B][2] LM iterations / trials summed over the ticks of pgs_run_sim_every_iteration
    DevBuf<double> d_tick_flop;                // [B][2] algorithmic FLOP (SYRK | Cholesky) of the same
    double iter_ms[4] = {0, 0, 0, 0};
    double host_launch_ms = 0.0, host_wait_ms = 0.0;   // tune.host_prof: host clock spent enqueuing trials / waiting for their counters (stderr, every-iteration runs)
    long long iter_trials = 0;
    double path_ms[3] = {0.0, 0.0, 0.0};      // profiled solve: ms in the separate SYRK launches / in the fused chain + SYRK launches / in the segmented path's SYRK launches
    bool seg_ok = false;                      // this solve runs the segmented elimination (decided in pgs_solve from the plan)
    // Round 6: the segment length is chosen PER SOLVE from {tune.seg_len, tune.seg_len / 2, ... >= 8}: the longest whose every segment sees at most
    // kPgsSegMaxLm landmarks (a wide sensor on a dense map overflowed 32-pose segments and the whole solve fell back to the sequential chain,
    // 2.3 x slower).  seg_cur: where the next solve's search starts (only goes down while the graph grows; pgs_init resets it); seg_alloc: the
    // length the segment-count-dependent arrays are sized for (re-made on demand, resize_segments); seg_used: the last solve's.
    int seg_cur = 32, seg_alloc = 32, seg_used = 0;
    bool fused_ok = false;                    // this solve's graphs fit the fused kernel (decided in pgs_solve from max M)
    bool syrk_inst_ok = false;                // ... and the instance-resident SYRK (its kPgsSyrkInstTiles tiles hold every lower triangle)
    int cus = 256;                            // compute units of the device
    int last_trials = 0;
    bool profiling = false;                  // per-kernel hipEvent timing of pgs_solve (pgs_set_profiling)
    std::vector<hipEvent_t> events;
    std::vector<int> trial_fused;             // profiled solve: the fused choice (0 | 2 | 3 | 4) of every trial
    double kernel_ms[slam::kPgsTrialKernels] = {0, 0, 0, 0, 0, 0};
    // marginal covariances (pgs_marginals): the outputs, and the per-instance flags / lambda = 0 the trial kernels read in place of the
    // solve's own (nothing pgs_get_stats returns is touched).  Allocated by the first call.  mg_valid: they belong to the current values.
    DevBuf<double> mg_pose, mg_lm, mg_flop, mg_lambda;   // [B][N_max][9], [B][L_max][4], [B], [B]
    DevBuf<int32_t> mg_status, mg_state;                 // [B], [3][B]: state | lin_ok | solve_ok
    hipEvent_t mg_ev[2] = {nullptr, nullptr};
    bool mg_valid = false;
    double mg_ms = 0.0;
    // robust loss of the bearing-range factors (pgs_set_robust): the setting as the caller left it; apply_robust copies it into p - with lin0
    // behind it - when the next solve / marginals / factor weights begin.  fw: the factor weights' own output, [B][N_max][KP], first use.
    int loss_kind = slam::kPgsLossNone;
    double loss_k = 0.0;
    DevBuf<double> rb_lin0;                    // p.lin0, [slots][N_max * KP]: allocated by the first such call with a loss set
    DevBuf<double> fw;
    bool fw_valid = false;
    // Absolute fixes (pgs_capi_fix.cpp; pgs_fix.h).  fix_row / fix_kind: p.fix_row [B][N_max][5] and p.fix_kind [B][N_max], inputs of an instance
    // like cmds and prior (one row per instance, the lambda lanes read their instance's) - allocated and zeroed by the first call that attaches
    // a fix, cleared by pgs_init[_each]; a handle that never sees a fix has none and launches the kernels built without them.  The fix loss as
    // the caller left it (apply_robust copies it into p).  fxw: pgs_fix_weights' output [B][N_max][2].  fix_sensor: the simulated source's rows.
    // The staging of the host forms: dfix [B][5], dfix_kinds / dfix_verdict / dfix_jumped [B].  tick_dropped: the handle's last update was
    // refused for pose capacity (a fix then has no pose of its own to go to).
    DevBuf<double> fix_row; DevBuf<int32_t> fix_kind;
    int fix_loss_kind = slam::kPgsLossNone;
    double fix_loss_k = 0.0;
    DevBuf<double> fxw;
    bool fxw_valid = false;
    DevBuf<slam_fix_sensor> fix_sensor;
    bool fix_sensor_set = false;
    DevBuf<double> dfix; DevBuf<int32_t> dfix_kinds, dfix_verdict, dfix_jumped;
    bool tick_dropped = false;

    // what was computed from the graph and its values - the marginals, the factor weights, the fix weights - no longer belongs to them
    void invalidate_derived() { mg_valid = false; fw_valid = false; fxw_valid = false; }
};

namespace pgs_capi {

inline int check(pgs_handle* h) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

// The handle's loss settings into the parameter block the kernels get (pgs_capi.cpp).  A loss - on the landmark factors, or on the fixes of a
// handle that has fixes - needs lin0: allocated there once; on failure the handle, parameter block included, is what it was.
int apply_robust(pgs_handle* h);
bool robust_args_ok(int kind, double k);

}  // namespace pgs_capi
