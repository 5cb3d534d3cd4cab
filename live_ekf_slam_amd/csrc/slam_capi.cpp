// slam_capi.cpp — C ABI (include/slam_batch.h) over the HIP kernels.  Host-side only: owns device memory,
// the stream, the step counter and the config; every compute entry point enqueues one fused kernel.
// There is NO CPU fallback: without a HIP device every compute call fails with SLAM_ERR_HIP.
#include "../../include/slam_batch.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "capi_internal.h"
#include "consistency_kernel.h"
#include "host/config_parse.h"
#include "host/noise_pack.h"
#include "host/tick_chunks.h"
#include "ekf_kernel.h"
#include "gate_kernel.h"
#include "innovation_kernel.h"
#include "monitor_kernel.h"
#include "nav_kernel.h"
#include "slam_math.h"
#include "ukf_kernel.h"

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// fn(begin, end) over [0, n) on a few host threads (packing 65 536 per-instance messages is ~1 ms on one core)
template <class F>
void host_parallel(size_t n, F fn) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = n < 8192 ? 1 : (hw >= 8 ? 4 : (hw >= 2 ? 2 : 1));
    if (nt == 1) { fn((size_t)0, n); return; }
    std::vector<std::thread> th;
    const size_t per = (n + nt - 1) / nt;
    for (size_t i = 1; i < nt; ++i) th.emplace_back(fn, i * per, (i + 1) * per < n ? (i + 1) * per : n);
    fn((size_t)0, per < n ? per : n);
    for (auto& t : th) t.join();
}

// EKF: consecutive calls of the per-tick entry points (slam_step_sim, slam_step, slam_step_dev) are queued on the host and run as
// ONE multi-step launch when the queue is full or anything else touches the handle (every other entry point runs it first).  The
// kernels are asynchronous anyway, and a multi-step launch gives the same bits as single steps, so only the speed changes (one
// launch per call re-reads x, ids and the thin rows / columns of P and cannot keep update groups open across timesteps).  Steps
// run in call order, so the queue holds the steps of one source at a time (queue_takes) and one function runs it (flush_lazy).
struct StepQueue {
    enum Source { kNone, kSim, kHost, kDev } src = kNone;
    std::vector<float> cmds;                      // [steps][2]
    int ks = 0;                                   // detections per instance of this fill (host and device messages)
    int steps() const { return (int)(cmds.size() / 2); }
    // host messages (slam_step): each call packs its message into one of two pinned fills; the flush copies the fill on the copy
    // stream, so packing the next fill overlaps the launch of the last one
    struct HostFill {
        PinnedBuf<float> hmeas; PinnedBuf<int32_t> hcount; PinnedBuf<float> hcmds;   // pinned: [lazy_max][B][ks][3], [lazy_max][B], [lazy_max][2]
        DevBuf<float> dmeas; DevBuf<int32_t> dcount;                                 // device
        hipEvent_t copied = nullptr, used = nullptr;
        bool in_use = false;
    } host[2];
    int host_cur = 0;
    int host_ks = 2;                              // stride of the next host fill: the largest message seen so far
    // device messages (slam_step_dev): copied device-to-device at the call on the compute stream (so the caller may overwrite its
    // buffers in stream order, as with an immediate launch); one buffer suffices, since copies and launches share the stream
    DevBuf<float> dmeas; DevBuf<int32_t> dcount;  // [lazy_max][B][ks][3], [lazy_max][B]
};

// Device times of the last per-tick run of one kind (run_chunked): part_ms is the sum over the launch group each tick marks, -1 while
// slam_nav_set_timing is off; total_ms is the sum over the chunks, -1 until such a run has run on the handle.
struct RunTimes { double part_ms = -1.0, total_ms = -1.0; };

}  // namespace

struct slam_handle {
    slam_config cfg;
    int kind, B, L_max, dtype, device;
    int n_max, ld_max, pstride, xstride;
    int waves_per_filter = 0;
    int dbg = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool inited = false;
    uint64_t seed = 2025;
    int64_t inst0 = 0;
    uint32_t step = 0;
    double range_max, fov_min, fov_max;
    // device buffers
    // device buffers (released with the handle)
    DevBuf<char> dP, dP2;                      // dP = current P_t; dP2 = second buffer (EKF: layout changes, UKF: ping-pong)
    DevBuf<char> dx; int esz = 8;              // x_t; element size of P / x storage
    DevBuf<double> dscratch;                   // fp32 storage: fp64 slab for P between detection groups
    DevBuf<int32_t> dM, dids, dflags, dts; DevBuf<double> dtruth, derr;
    DevBuf<double> dmap; int L = 0;
    DevBuf<float> dmeas; DevBuf<int32_t> dcount; int k_stride = 0;   // last-measurement dump (slam_get_last_meas); k_stride: what both hold
    // slam_step (host measurements): two pinned staging buffers + two device buffers, filled on a copy stream while the
    // previous step's kernel runs; no stream synchronisation per step
    struct Stage {
        PinnedBuf<float> hmeas; PinnedBuf<int32_t> hcount;     // pinned host
        DevBuf<float> dmeas; DevBuf<int32_t> dcount;           // device
        hipEvent_t copied = nullptr, used = nullptr;
        bool in_use = false;
    } stage[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t shadow_ev = nullptr;
    uint32_t stage_next = 0;
    DevBuf<unsigned long long> dkhist;                         // [8] instance-steps by detection count
    StepQueue q;                                               // EKF: the queued steps of slam_step_sim, slam_step and slam_step_dev
    int eager_init = 2;                                        // first idle-GPU launch size (SLAM_EAGER_FLUSH, 0 = off)
    int eager_target = 2;                                      // queued steps an idle GPU is given at once (doubles per such launch)
    bool lazy_explicit = false;                                // slam_set_lazy_steps / SLAM_LAZY_STEPS asked for queueing: slam_step_dev queues only then
    int lazy_max = 32;                                         // 0 / 1 = off (SLAM_LAZY_STEPS, slam_set_lazy_steps); per launch a workgroup pays
                                                               // ~25 us of start / drain: 16 -> 61 M, 32 -> 66 M, 64 -> 70 M steps/s (one launch: 73 M)
    // slam_track_instance: instance `tracked` also runs in a one-instance SHADOW filter (same config, seed, map and GLOBAL
    // instance id, hence the same bits: results do not depend on how a batch is partitioned), stepped at once at every step
    // call on its own stream, so that slam_get_state(h, tracked) - the publishState of every tick, localization_node.cpp:139 -
    // does not have to run the batch's queued timesteps first.
    slam_handle* shadow = nullptr; int tracked = -1;
    std::vector<double> hmap;                  // host copy of the map (the shadow needs it)
    DevBuf<double> dscalar;
    DevBuf<unsigned long long> dprof;
    DevBuf<double> dsq; DevBuf<int32_t> dnsq;         // UKF: matrix square root scratch + its dimension
    DevBuf<double> dxprev;                            // UKF: x_t the last sigma points were drawn around
    DevBuf<double> dvt; DevBuf<int32_t> dvage;        // UKF: V^T of the last eigen-decomposition + warm-start age
    DevBuf<double> dbigws;                            // UKF beyond the LDS size classes: [B][2 * pstride] scratch (ukf_big_kernel.hip)
    DevBuf<uint4> drot;                               // UKF (n <= 44): pass table of the fast sqrt kernel (launch_ukf_quad_table)
    DevBuf<uint8_t> dchol; bool chol = false;         // UKF: SLAM_UKF_SQRT_CHOLESKY is on; [B] "the Cholesky factor succeeded" (ukf_chol_kernel)
    hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr}; hipEvent_t aux_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // UKF run_sim: the other parts of the batch
    int ukf_parts = 2;                                                               // streams the UKF batch is split over (SLAM_UKF_PARTS, 1..4)
    int ukf_split_min = 1024;                                                        // batch size from which it is used
    bool predicted = false; float pred_cmd[2] = {0.f, 0.f};   // UKF: slam_predict done, slam_update_dev pending
    DevBuf<float> dmapf;                              // UKF_LOC: the known map as float32 [id, x, y] triplets
    DevBuf<float> dcmds;                              // command sequence of a multi-step launch (slam_run_sim)
    int run_chunk = 0;                                // timesteps per launch in slam_run_sim (0 = all of them)
    int base = 3;                                     // state offset of the first landmark: 3 (EKF) or 4 (UKF)
    bool dump_meas = false;
    // per-instance inputs (the slam_*_each entry points).  slam_set_maps: one true map per instance, [B][map_stride][2] and [B] landmark
    // counts; while maps_each is set, L above is the largest count (the size-class and LDS decisions use it) and the kernels read these
    // instead of dmap.  Host copies for the shadow of slam_track_instance.
    DevBuf<double> dmaps; DevBuf<int32_t> dLs; int map_stride = 0; bool maps_each = false;
    std::vector<double> hmaps; std::vector<int32_t> hLs;
    DevBuf<float> dcmd_each;                          // per-instance commands of the launches of one call: [T][B][2]
    // slam_set_noise_each: [B] packed rows the step kernels read (noise_each: they are set) and the caller's rows for the shadow
    DevBuf<slam::NoiseRow> dnoise; bool noise_each = false;
    std::vector<slam_noise> hnoise;
    bool pred_each = false;                           // UKF: slam_predict_each done, the pending update stage reads dcmd_each
    DevBuf<float> dpose_each; DevBuf<double> dstart_each;   // slam_init_each: EKF [B][3] start poses; [B][4] UKF x_t heads + [B][3] true poses
    // slam_consistency: [3][B] nees_full, nees_pose, map_rms and [2][B] dof, flags on the device; the packed triangles of one chunk of
    // instances (L_max > 50 only, grown on demand); what the last call had to read and its device time
    DevBuf<double> dcons, dcons_ws; DevBuf<int32_t> dconsi;
    double cons_bytes = 0.0, cons_ms = -1.0;
    // slam_nav_*: the path (shared [P][2], or [B][stride][2] with [B] lengths), the controller state of every instance, the command log
    // of one chunk of ticks, ticks since the state was reset and the device times of the last slam_nav_run
    struct Nav {
        bool set = false, each = false;
        slam_nav_config cfg;
        int P = 0, stride = 0;
        DevBuf<double> dpath; DevBuf<int32_t> dP;
        DevBuf<int32_t> dhead, dfinish; DevBuf<double> dinteg, derrp;
        DevBuf<float> dlog;
        int tick = 0;
        bool time_ticks = false;   // slam_nav_set_timing: every per-tick run brackets one launch group of each tick with an event pair
        RunTimes times;
    } nav;
    // the events of a per-tick run (run_chunked): one pair per chunk and, while time_ticks is on, one per tick of a chunk.  One pool serves
    // every kind of run: a run returns synchronised, so two never overlap on a handle.
    std::vector<hipEvent_t> run_ev;
    // slam_monitor_*: the per-workgroup partial records of one evaluation, the records and the per-instance series of one chunk of ticks
    // ([series][ticks][B] doubles, [B] flags of slam_monitor_now) and the device times of the last slam_monitor_run
    struct Mon {
        DevBuf<double> dpart, drec, dlog; DevBuf<int32_t> dflags;
        RunTimes times;
    } mon;
    // slam_innovation_*: the staged message and per-instance commands of a host-fed evaluation (one chunk of ticks for the LOG source), the
    // per-instance outputs ([B] nis_sum, [B][12] post, [B][16] contributions, the partial records, the records and the nis_sum series of a
    // chunk; [B][64][6] detection slots when asked for; [3][ticks][B] n_upd, flags, n_new) and the device times of the last run
    struct Inn {
        DevBuf<float> dmeas, dcmd; DevBuf<int32_t> dcount;
        DevBuf<double> dval, ddet, dpart, drec, dlog; DevBuf<int32_t> dint;
        RunTimes times;
    } inn;
    // slam_gate_*: the filtered message of a gated step or of one tick of slam_gate_run ([B][k_stride][3] and [B] counts), [ticks][B] n_rej
    // and [B][64] verdicts, the device times of the last slam_gate_run.  Everything else is staged in `inn`.
    struct Gate {
        DevBuf<float> dmeas; DevBuf<int32_t> dcount, drej, dverdict;
        RunTimes times;
    } gate;
};

namespace {

// The fields of a step launch that say where its input comes from, either filter kind: `sim` = the device-side generator, else messages of
// stride k_stride at meas / count; long_cap > 0: messages may exceed the size class (long_message_cap).  The generator's measurements are
// dumped while slam_get_last_meas asked for them.
template <class Params>
void set_step_input(const slam_handle* h, Params& p, int sim, int long_cap, const float* meas, const int32_t* count, int k_stride) {
    p.sim = sim;
    p.long_mode = long_cap > 0 ? 1 : 0; p.long_cap = long_cap;
    p.meas_in = meas; p.meas_count_in = count; p.k_stride_in = k_stride;
    if (sim && h->dump_meas) { p.meas_out = h->dmeas; p.meas_count_out = h->dcount; p.k_stride_out = h->k_stride; }
}

// Every EKF step launch: T = 0 is one timestep with `cmd`; T > 0 is a multi-step launch over the device commands d_cmds, whose first
// command is `cmd`, with the messages of timestep t at meas + t * B * k_stride * 3 / count + t * B.
// The maps of slam_set_maps, if set, and per-instance commands d_cmd_each (device, [T][B][2]; NULL = the shared ones).
template <class Params>
void set_each_inputs(const slam_handle* h, Params& p, const float* d_cmd_each) {
    if (h->maps_each) { p.map_each = h->dmaps; p.L_each = h->dLs; p.map_stride = h->map_stride; }
    p.cmd_each = d_cmd_each;
    p.noise_each = h->noise_each ? h->dnoise.get() : nullptr;
}

void fill_ekf_params(slam_handle* h, slam::EkfStepParams& p, const float cmd[2], int sim, int long_cap, const float* meas, const int32_t* count,
                     int k_stride, const float* d_cmds, int T, const float* d_cmd_each = nullptr) {
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.P_out = h->dP2; p.x = h->dx; p.scratch = h->dscratch; p.M = h->dM; p.ids = h->dids; p.flags = h->dflags; p.timestep = h->dts;
    p.truth = h->dtruth; p.err_sum = h->derr; p.map = h->dmap; p.L = h->L;
    p.fwd = cmd[0]; p.ang = cmd[1];
    const slam_config& c = h->cfg;
    p.v_d = c.v_d; p.v_th = c.v_th; p.w_r = c.w_r; p.w_b = c.w_b;
    if (c.replicate_vw_quirk) {  // filter.h:116-117: W_00/W_11 land in V, W stays I2
        p.V00 = c.W_00; p.V11 = c.W_11; p.W00 = 1.0; p.W11 = 1.0;
    } else {
        p.V00 = c.V_00; p.V11 = c.V_11; p.W00 = c.W_00; p.W11 = c.W_11;
    }
    p.id_known = c.landmark_id_is_known;
    p.min_sep = c.min_landmark_separation;
    p.abs_is_int = c.ekf_abs_is_int ? 1 : 0; p.lm_from_pred = c.ekf_landmark_from_x_pred ? 1 : 0;
    p.sV00 = c.V_00; p.sV11 = c.V_11; p.sW00 = c.W_00; p.sW11 = c.W_11;
    p.d_max = c.d_max; p.th_max = c.th_max;
    p.range_max = h->range_max; p.fov_min = h->fov_min; p.fov_max = h->fov_max;
    p.seed = h->seed; p.inst0 = h->inst0; p.step = h->step;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.dbg = h->dbg;
    p.prof = (h->dbg & (4 | 32)) ? h->dprof : nullptr;
    p.khist = h->dkhist;
    set_step_input(h, p, sim, long_cap, meas, count, k_stride);
    p.cmds = d_cmds; p.T = T;
    set_each_inputs(h, p, d_cmd_each);
}

// d_cmd_each: [B][2] per-instance commands of this timestep (device), NULL = cmd
void fill_ukf_params(slam_handle* h, slam::UkfStepParams& p, const float cmd[2], const float* d_cmd_each = nullptr) {
    memset(&p, 0, sizeof(p));
    p.P = (const double*)h->dP.get(); p.P_out = (double*)h->dP2.get(); p.x = (double*)h->dx.get(); p.sqtP = h->dsq; p.n_sq = h->dnsq; p.x_prev = h->dxprev; p.Vt_store = h->dvt; p.v_age = h->dvage;
    p.M = h->dM; p.ids = h->dids; p.flags = h->dflags; p.timestep = h->dts;
    p.truth = h->dtruth; p.err_sum = h->derr; p.map = h->dmap; p.L = h->L;
    p.fwd = cmd[0]; p.ang = cmd[1];
    const slam_config& c = h->cfg;
    p.v_d = c.v_d; p.v_th = c.v_th; p.w_r = c.w_r; p.w_b = c.w_b;
    if (c.replicate_vw_quirk) { p.V00 = c.W_00; p.V11 = c.W_11; p.W00 = 1.0; p.W11 = 1.0; }
    else { p.V00 = c.V_00; p.V11 = c.V_11; p.W00 = c.W_00; p.W11 = c.W_11; }
    p.float_trig = c.ukf_float_trig;
    p.acc_zest1 = c.ukf_accumulate_zest1 ? 1 : 0; p.yaw_sigma = c.ukf_sensing_yaw_from_sigma ? 1 : 0;
    p.sV00 = c.V_00; p.sV11 = c.V_11; p.sW00 = c.W_00; p.sW11 = c.W_11;
    p.d_max = c.d_max; p.th_max = c.th_max;
    p.range_max = h->range_max; p.fov_min = h->fov_min; p.fov_max = h->fov_max;
    p.seed = h->seed; p.inst0 = h->inst0; p.step = h->step;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.b_off = 0; p.b_cnt = h->B;
    p.loc = h->kind == SLAM_UKF_LOC; p.mapf = h->dmapf;
    p.quad_tab = h->drot;
    p.khist = h->dkhist;
    p.big_ws = h->dbigws;
    p.prof = (h->dbg & 4) ? h->dprof : nullptr;
    p.chol_ok = h->chol ? h->dchol : nullptr;
    set_each_inputs(h, p, d_cmd_each);
}

// ekf.cpp:65,73 and ukf.cpp:249-287 walk a message of any length.  The LDS size classes hold as many detections of one message as the class
// holds landmarks (every message without repeated ids about a map the state can hold fits); a launch whose messages MAY be longer - external
// measurements: the caller's bound k_stride is (slam_step passes the largest count it saw); SIM mode: the map is - runs the long-message path
// of launch_ekf_step / launch_ukf_step: the instances concerned go through the HBM-streamed kernels, which read a message where it lies
// (same state layout, same arithmetic: both are bit-identical to the oracle; about a pass over P per detection slower).  Returns the class
// capacity if that path is needed, 0 if not (the streamed classes have no limit in the first place).  fp32-storage EKF handles too: the
// streamed kernel reads and writes floats there and runs the timestep in the handle's fp64 slab.
int long_message_cap(slam_handle* h, int sim, int k_stride, int* cap_out) {
    *cap_out = 0;
    int cap;
    if (h->kind == SLAM_EKF_SLAM) {
        if (h->L_max > (h->esz == 4 ? slam::kEkfLdsMaxLandmarksF32 : slam::kEkfLdsMaxLandmarks)) return SLAM_OK;   // a streamed class: no limit
        cap = slam::ekf_class_message_capacity(h->L_max);
    } else {
        if (h->kind == SLAM_UKF_SLAM && h->L_max > slam::kUkfLdsMaxLandmarks) return SLAM_OK;
        cap = slam::ukf_class_message_capacity(h->L_max, h->kind == SLAM_UKF_LOC, h->L);
    }
    if (!(sim ? h->L > cap : k_stride > cap)) return SLAM_OK;
    if (h->kind != SLAM_EKF_SLAM)   // scratch of the streamed step kernel (P_pred), on first use
        HIP_TRY(h->dbigws.reserve((size_t)h->B * 2 * h->pstride));
    *cap_out = cap;
    return SLAM_OK;
}

// one UKF timestep of instances [b_off, b_off + b_cnt) on `stream`
int launch_ukf_pair(slam_handle* h, const float cmd[2], int sim, int long_cap, const float* meas, const int32_t* count, int k_stride,
                    int b_off, int b_cnt, hipStream_t stream, const float* d_cmd_each = nullptr) {
    slam::UkfStepParams p;
    fill_ukf_params(h, p, cmd, d_cmd_each);
    set_step_input(h, p, sim, long_cap, meas, count, k_stride);
    p.b_off = b_off; p.b_cnt = b_cnt;
    HIP_TRY(slam::launch_ukf_sqrt(p, stream));   // nearestSPD + sqrt (ukf.cpp:106-123,208)
    HIP_TRY(slam::launch_ukf_step(p, stream));   // predictionStage + updateStage (ukf.cpp:197-372)
    return SLAM_OK;
}

// one timestep, either filter kind; `sim` = device-side measurement generator; d_cmd_each: [B][2] per-instance commands (device) or NULL
int launch_step(slam_handle* h, const float cmd[2], int sim, const float* d_meas, const int32_t* d_count, int k_stride,
                const float* d_cmd_each = nullptr) {
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
    int long_cap = 0;
    if (const int rc = long_message_cap(h, sim, k_stride, &long_cap)) return rc;
    if (h->kind == SLAM_EKF_SLAM) {
        slam::EkfStepParams p;
        fill_ekf_params(h, p, cmd, sim, long_cap, d_meas, d_count, k_stride, nullptr, 0, d_cmd_each);
        HIP_TRY(slam::launch_ekf_step(p, h->waves_per_filter, h->esz == 4, h->stream));
    } else {
        TRY(launch_ukf_pair(h, cmd, sim, long_cap, d_meas, d_count, k_stride, 0, h->B, h->stream, d_cmd_each));
        std::swap(h->dP, h->dP2);   // UKF: the kernel wrote the next P_t into the other buffer (the EKF kernel updates dP in place)
    }
    h->step += 1;
    return SLAM_OK;
}

// h->k_stride is set only once both buffers hold that stride
int ensure_meas_buffers(slam_handle* h, int k_stride) {
    if (h->k_stride >= k_stride) return SLAM_OK;
    HIP_TRY(h->dmeas.reserve((size_t)3 * k_stride * h->B)); HIP_TRY(h->dcount.reserve((size_t)h->B));
    HIP_TRY(hipMemsetAsync(h->dcount, 0, sizeof(int32_t) * (size_t)h->B, h->stream));   // no detections recorded at the new stride yet
    h->k_stride = k_stride;
    return SLAM_OK;
}

// Room for n elements in a buffer of the handle that launches in flight may still use: they finish before it is replaced.  A buffer that
// has its size costs a comparison.
template <class T>
int grow(slam_handle* h, DevBuf<T>& buf, size_t n) {
    if (buf.cap() >= n) return SLAM_OK;
    if (buf) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(buf.reserve(n));
    return SLAM_OK;
}

// slam_set_map or slam_set_maps has given the simulator a true map
bool has_map(const slam_handle* h) { return h->dmap || h->maps_each; }

// per-instance commands [T][B][2] of one call from the host into dcmd_each, in stream order (the launches of earlier calls that read the
// buffer come first; it grows only once they are done).  A pending prediction stage reads the buffer, so nothing may replace it then.
int upload_cmds_each(slam_handle* h, const float* cmds, int T) {
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
    const size_t n = 2 * (size_t)T * h->B;
    if (n == 0) return SLAM_OK;
    TRY(grow(h, h->dcmd_each, n));
    HIP_TRY(hipMemcpyAsync(h->dcmd_each, cmds, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

constexpr float kNoCmd[2] = {0.f, 0.f};   // the shared command of a launch whose commands are per instance (not read)

// slam_init / slam_init_each / setting a path: head = 0, integ = err_prev = 0, finish_tick = -1 for every instance, in stream order
int nav_reset(slam_handle* h) {
    if (!h->nav.set) return SLAM_OK;
    const size_t B = (size_t)h->B;
    HIP_TRY(hipMemsetAsync(h->nav.dhead, 0, sizeof(int32_t) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.dfinish, 0xff, sizeof(int32_t) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.dinteg, 0, sizeof(double) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.derrp, 0, sizeof(double) * B, h->stream));
    h->nav.tick = 0;
    return SLAM_OK;
}

// The launch parameters of launch_consistency at the handle's current state, with its output buffers and workspace reserved; *chunk_out:
// instances per launch of the workspace class.
int consistency_params(slam_handle* h, slam::ConsistencyParams* out, int* chunk_out) {
    const size_t B = (size_t)h->B;
    HIP_TRY(h->dcons.reserve(3 * B));
    HIP_TRY(h->dconsi.reserve(2 * B));
    // beyond the LDS classes the packed triangles live in a workspace of at most SLAM_CONSISTENCY_WS_BYTES (default 256 MiB; one
    // instance at least), and the batch is processed in chunks of as many instances as it holds
    const size_t per = slam::consistency_ws_per_instance(h->L_max);
    int chunk = h->B;
    if (per) {
        const char* env = getenv("SLAM_CONSISTENCY_WS_BYTES");
        const double budget = env ? atof(env) : 256.0 * 1024 * 1024;
        const double fit = budget / (8.0 * (double)per);
        chunk = fit >= (double)h->B ? h->B : (fit >= 1.0 ? (int)fit : 1);
        HIP_TRY(h->dcons_ws.reserve(per * (size_t)chunk));
    }
    slam::ConsistencyParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.ids = h->dids; p.status = h->dflags; p.truth = h->dtruth;
    p.map = h->dmap; p.L = h->L;
    if (h->maps_each) { p.map_each = h->dmaps; p.L_each = h->dLs; p.map_stride = h->map_stride; }
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.id_known = h->cfg.landmark_id_is_known ? 1 : 0;
    p.nees_full = h->dcons; p.nees_pose = h->dcons + B; p.map_rms = h->dcons + 2 * B; p.dof = h->dconsi; p.flags = h->dconsi + B;
    p.ws = h->dcons_ws; p.ws_stride = per;
    *out = p; *chunk_out = chunk;
    return SLAM_OK;
}

}  // namespace

static int run_sim_now(slam_handle* h, const float* cmds, int T, const float* d_cmd_each = nullptr);
static int flush_lazy(slam_handle* h);
static int step_host_now(slam_handle* h, const float cmd[2], const float* d_cmd_each, const float* meas, const int32_t* count, int k_stride, int kmax);
// Whether the EKF step queue can take one more step from `src` as it stands: it is empty, or it holds steps of the same source with a
// compatible stride (host messages: at most the stride of the fill, device messages: the same stride) and has room.  If it cannot, the
// caller runs the queue first, so that steps run in call order.
static bool queue_takes(const slam_handle* h, StepQueue::Source src, int ks) {
    const StepQueue& q = h->q;
    if (q.steps() == 0) return true;
    const bool stride_ok = src == StepQueue::kHost ? ks <= q.ks : ks == q.ks;
    return q.src == src && stride_ok && q.steps() < h->lazy_max;
}
// The queue exists to give the GPU long multi-step launches while the caller keeps calling once per tick; when the GPU has
// nothing to do, waiting for the queue to fill only delays the work (a run of K calls paid one whole queue of packing with
// the GPU idle before the first launch).  So a queued step is launched at once if the compute stream is idle.
// Launching every single queued step would waste the multi-step kernel (2.4 vs 1.5 ms per step), so the idle-GPU launch
// needs `eager_target` queued steps, and the target doubles with every such launch (2, 4, 8, ... up to the queue length):
// the pipeline fills geometrically instead of after one whole queue.  SLAM_EAGER_FLUSH=0 switches it off.  Only slam_step
// does this (its caller spends ~1 ms per call delivering a message); slam_step_sim calls cost microseconds, so its queue is
// full long before the first launch would have finished.
static bool eager_flush(slam_handle* h, int queued) {
    if (h->eager_target <= 0 || queued < h->eager_target) return false;
    const hipError_t e = hipStreamQuery(h->stream);
    (void)hipGetLastError();   // hipErrorNotReady is an answer, not an error
    if (e != hipSuccess) return false;
    h->eager_target = 2 * queued < h->lazy_max ? 2 * queued : h->lazy_max;
    return true;
}
static constexpr int kExtQ = 4;   // detections per instance a queued slam_step message can hold

extern "C" {

int slam_internal_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

const char* slam_last_error(void) { return g_err; }
const char* slam_version(void) { return "live_ekf_slam_amd 0.1 (gfx950)"; }

int slam_config_default(slam_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->v_d = 0.0f; c->v_th = 0.0f; c->V_00 = 0.01; c->V_11 = 0.001;      // params.yaml:39-45
    c->w_r = 0.0f; c->w_b = 0.0f; c->W_00 = 0.01; c->W_11 = 0.01;        // params.yaml:46-52
    c->landmark_id_is_known = 1; c->min_landmark_separation = 0.1f;        // params.yaml:35-36
    c->d_max = 0.1; c->th_max = 0.0546;                                    // params.yaml:27-28
    c->range_max = 3.0; c->fov_min = -1.57; c->fov_max = 1.57;             // params.yaml:30-32
    c->init_x = 0.0; c->init_y = 0.0; c->init_yaw = 0.0;                   // params.yaml:19-22
    c->replicate_vw_quirk = 1;
    c->ukf_float_trig = 1;
    return SLAM_OK;
}

// The reference reads one YAML file with nested maps; the keys the hot path needs are unique leaf names
// except min_landmark_separation (constraints.measurements vs map), disambiguated by section tracking.  The reader
// itself is host/config_parse.h (host-only, also compiled under ASan + UBSan by `make -C oracle asan`).
int slam_config_load(slam_config* c, const char* path) {
    if (!c || !path) return fail(SLAM_ERR_ARG, "NULL argument");
    std::string err;
    const int rc = slam_host::config_parse_file(c, path, &err);
    if (rc) return fail(SLAM_ERR_IO, "%s", err.c_str());
    return SLAM_OK;
}

int slam_create(const slam_config* cfg, int kind, int batch, int L_max, int dtype, int device, slam_handle** out) {
    if (!cfg || !out) return fail(SLAM_ERR_ARG, "NULL argument");
    if (batch <= 0 || L_max <= 0) return fail(SLAM_ERR_ARG, "batch and L_max must be positive");
    if (kind != SLAM_EKF_SLAM && kind != SLAM_UKF_SLAM && kind != SLAM_UKF_LOC)
        return fail(SLAM_ERR_ARG, "unknown filter kind %d", kind);
    // The four quirk switches took over fields that were `reserved` until round 4: a caller compiled against that header may
    // have left anything there, and any non-zero value would silently switch a reference quirk off.  Only 0 and 1 are configurations.
    for (const int q : {cfg->ekf_abs_is_int, cfg->ekf_landmark_from_x_pred, cfg->ukf_accumulate_zest1, cfg->ukf_sensing_yaw_from_sigma})
        if (q != 0 && q != 1) return fail(SLAM_ERR_ARG, "slam_config quirk switch = %d: the switches (ekf_abs_is_int, ekf_landmark_from_x_pred, ukf_accumulate_zest1, "
                                          "ukf_sensing_yaw_from_sigma) are 0 or 1 - zero-initialise the struct (slam_config_default)", q);
    if (kind == SLAM_UKF_LOC) L_max = 1;   // localisation only: the state never holds landmarks
    if (dtype != SLAM_F64 && !(dtype == SLAM_F32 && kind == SLAM_EKF_SLAM))
        return fail(SLAM_ERR_UNSUPPORTED, "fp32 state storage is implemented for EKF_SLAM only");
    if (L_max > (kind != SLAM_EKF_SLAM ? slam::kUkfMaxLandmarks : slam::kEkfMaxLandmarks))
        return fail(SLAM_ERR_UNSUPPORTED, "L_max %d exceeds the limit of this filter kind (EKF %d, UKF %d): the EKF beyond %d landmarks (fp32 storage: beyond %d) and the UKF beyond 50 run the HBM-streamed size classes, whose working set is 2 x n x n doubles per instance in HBM", L_max, slam::kEkfMaxLandmarks, slam::kUkfMaxLandmarks, slam::kEkfLdsMaxLandmarks, slam::kEkfLdsMaxLandmarksF32);
    HIP_TRY(hipSetDevice(device));
    slam_handle* h = new slam_handle();
    h->cfg = *cfg; h->kind = kind; h->B = batch; h->L_max = L_max; h->dtype = dtype; h->device = device;
    h->esz = dtype == SLAM_F32 ? 4 : 8;
    h->base = (kind == SLAM_EKF_SLAM) ? 3 : 4;
    h->n_max = h->base + 2 * L_max;
    // per-filter slab: n_max rows of the padded leading dimension (EKF: slam::ekf_ld, rows start on 16-byte boundaries;
    // the UKF packs n x n with n even), 256/512-byte aligned
    h->ld_max = kind == SLAM_EKF_SLAM ? slam::ekf_ld(h->n_max, h->esz) : h->n_max;
    h->pstride = round_up(h->n_max * h->ld_max + 4, 64);
    h->xstride = round_up(h->n_max + 1, 2);
    h->range_max = cfg->range_max; h->fov_min = cfg->fov_min; h->fov_max = cfg->fov_max;
    const char* env = getenv("SLAM_WAVES_PER_FILTER");
    if (env) h->waves_per_filter = atoi(env);
    env = getenv("SLAM_DEBUG_FLAGS");   // 4 / 32: phase and per-step timers.  The ablation bits (1, 2, 16: WRONG results) are
    if (env) h->dbg = atoi(env);        // compiled out of the release kernels (-DSLAM_ABLATE builds only)
#ifndef SLAM_ABLATE
    h->dbg &= (4 | 32);   // (the fault-injection bit 128 is reachable through slam_set_debug_flags only: no environment variable can plant it)
#endif
    env = getenv("SLAM_UKF_SPLIT_MIN");   // batch size from which UKF run_sim splits the batch over two streams
    if (env) h->ukf_split_min = atoi(env);
    env = getenv("SLAM_UKF_PARTS");   // streams the UKF batch is split over in run_sim (2..4)
    if (env) h->ukf_parts = atoi(env);
    env = getenv("SLAM_LAZY_STEPS");   // slam_step_sim calls queued per multi-step launch (0 = one launch per call)
    if (env) { h->lazy_max = atoi(env); h->lazy_explicit = true; }
    env = getenv("SLAM_EAGER_FLUSH");   // queued steps from which an idle GPU is given work before the queue is full (0 = never)
    if (env) h->eager_init = h->eager_target = atoi(env);
    env = getenv("SLAM_RUN_CHUNK");   // timesteps per launch of slam_run_sim (1 = one launch per step)
    if (env) h->run_chunk = atoi(env);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return fail(SLAM_ERR_HIP, "hipStreamCreate -> %s", hipGetErrorString(e)); }
    h->own_stream = true;
    const size_t B = (size_t)batch;
    hipError_t errs[] = {
        h->dP.reserve((size_t)h->esz * B * h->pstride),
        h->dP2.reserve((size_t)h->esz * B * h->pstride),
        h->dx.reserve((size_t)h->esz * B * h->xstride),
        h->dM.reserve(B),
        h->dids.reserve(B * L_max),
        h->dflags.reserve(B),
        h->dts.reserve(B),
        h->dtruth.reserve(B * 3),
        h->derr.reserve(B),
        h->dscalar.reserve(4),
        (h->dbg & (4 | 32)) ? h->dprof.reserve(slam::kEkfProfSlots * B) : hipSuccess,
        h->dkhist.reserve(16),
        kind != SLAM_EKF_SLAM ? h->dsq.reserve(B * h->pstride) : hipSuccess,
        h->esz == 4 ? h->dscratch.reserve(B * h->pstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->dnsq.reserve(B) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->dxprev.reserve(B * h->xstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->dvt.reserve(B * h->pstride) : hipSuccess,
        (kind == SLAM_UKF_SLAM && L_max > slam::kUkfLdsMaxLandmarks) ? h->dbigws.reserve(B * 2 * h->pstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->dvage.reserve(B) : hipSuccess,
        (kind != SLAM_EKF_SLAM && h->n_max <= 44) ? h->drot.reserve(slam::kUkfQuadTabEntries) : hipSuccess,
    };
    for (hipError_t ee : errs)
        if (ee != hipSuccess) {
            slam_destroy(h);
            return fail(SLAM_ERR_HIP, "allocating device memory -> %s", hipGetErrorString(ee));
        }
    // every buffer a getter can read before slam_init is zeroed (M = 0, flags = 0, timestep = 0, ...)
    hipError_t zs[] = {
        hipMemsetAsync(h->dP, 0, (size_t)h->esz * B * h->pstride, h->stream),
        hipMemsetAsync(h->dP2, 0, (size_t)h->esz * B * h->pstride, h->stream),
        hipMemsetAsync(h->dx, 0, (size_t)h->esz * B * h->xstride, h->stream),
        hipMemsetAsync(h->dids, 0, sizeof(int32_t) * B * L_max, h->stream),
        hipMemsetAsync(h->dM, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dflags, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dts, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dtruth, 0, sizeof(double) * B * 3, h->stream),
        hipMemsetAsync(h->derr, 0, sizeof(double) * B, h->stream),
        hipMemsetAsync(h->dkhist, 0, sizeof(unsigned long long) * 16, h->stream),
        h->dnsq ? hipMemsetAsync(h->dnsq, 0, sizeof(int32_t) * B, h->stream) : hipSuccess,
        h->dprof ? hipMemsetAsync(h->dprof, 0, sizeof(unsigned long long) * slam::kEkfProfSlots * B, h->stream) : hipSuccess,
        h->drot ? slam::launch_ukf_quad_table(h->drot, h->stream) : hipSuccess,
    };
    for (hipError_t ee : zs)
        if (ee != hipSuccess) {
            slam_destroy(h);
            return fail(SLAM_ERR_HIP, "hipMemsetAsync -> %s", hipGetErrorString(ee));
        }
    *out = h;
    return SLAM_OK;
}

int slam_destroy(slam_handle* h) {
    if (!h) return SLAM_OK;
    if (h->shadow) { slam_destroy(h->shadow); h->shadow = nullptr; }
    flush_lazy(h);
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (auto& st : h->aux_stream) if (st) { hipStreamSynchronize(st); hipStreamDestroy(st); }
    for (auto& ev : h->aux_ev) if (ev) hipEventDestroy(ev);
    for (auto& ev : h->run_ev) if (ev) hipEventDestroy(ev);
    if (h->copy_stream) { hipStreamSynchronize(h->copy_stream); hipStreamDestroy(h->copy_stream); }
    if (h->shadow_ev) hipEventDestroy(h->shadow_ev);
    for (auto& f : h->q.host)
        if (f.copied) { hipEventDestroy(f.copied); hipEventDestroy(f.used); }
    for (auto& s : h->stage)
        if (s.copied) { hipEventDestroy(s.copied); hipEventDestroy(s.used); }
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;   // the device and pinned buffers
    return SLAM_OK;
}

int slam_set_stream(slam_handle* h, void* s) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    return SLAM_OK;
}
int slam_set_instance_offset(slam_handle* h, int64_t v) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->inst0 = v;
    return h->shadow ? slam_set_instance_offset(h->shadow, v + h->tracked) : SLAM_OK;
}
int slam_set_seed(slam_handle* h, uint64_t s) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->seed = s;
    return h->shadow ? slam_set_seed(h->shadow, s) : SLAM_OK;
}
int slam_set_vision(slam_handle* h, double range_max, double fov_min, double fov_max) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->range_max = range_max; h->fov_min = fov_min; h->fov_max = fov_max;
    return h->shadow ? slam_set_vision(h->shadow, range_max, fov_min, fov_max) : SLAM_OK;
}

int slam_init(slam_handle* h, float x0, float y0, float yaw0) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->kind == SLAM_EKF_SLAM) {
        slam::EkfInitParams p;
        memset(&p, 0, sizeof(p));   // (the per-instance pointers stay NULL: the shared start pose)
        p.P = h->dP; p.x = h->dx; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride; p.f32_storage = h->esz == 4;
        p.x0 = x0; p.y0 = y0; p.yaw0 = yaw0;
        // the simulator starts from the un-rounded YAML pose (sim_node.py:361); the filter gets float args
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        HIP_TRY(slam::launch_ekf_init(p, h->stream));
    } else {
        slam::UkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = (double*)h->dP.get(); p.x = (double*)h->dx.get(); p.n_sq = h->dnsq; p.v_age = h->dvage; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride;
        double s, c;   // x_t << x_0, y_0, cos(yaw_0), sin(yaw_0) with a float argument (ukf.cpp:33)
        slam::det_sincos((double)yaw0, &s, &c);
        p.x0 = x0; p.y0 = y0;
        p.c0 = h->cfg.ukf_float_trig ? (double)(float)c : c;
        p.s0 = h->cfg.ukf_float_trig ? (double)(float)s : s;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        HIP_TRY(slam::launch_ukf_init(p, h->stream));
    }
    h->step = 0;
    h->inited = true;
    TRY(nav_reset(h));
    if (h->shadow) return slam_init(h->shadow, x0, y0, yaw0);
    return SLAM_OK;
}

int slam_set_map(slam_handle* h, const double* map_xy, int L) {
    if (!h || !map_xy || L <= 0) return fail(SLAM_ERR_ARG, "bad map");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->dmap) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(h->dmap.reserve(2 * (size_t)L));
    HIP_TRY(hipMemcpyAsync(h->dmap, map_xy, sizeof(double) * 2 * (size_t)L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->kind == SLAM_UKF_LOC) {   // trueMapCallback: filter->map = [id, x, y] float32 (localization_node.cpp:152-156)
        std::vector<float> trip((size_t)3 * L);
        for (int i = 0; i < L; ++i) { trip[3 * i] = (float)i; trip[3 * i + 1] = (float)map_xy[2 * i]; trip[3 * i + 2] = (float)map_xy[2 * i + 1]; }
        HIP_TRY(h->dmapf.reserve(trip.size()));
        HIP_TRY(hipMemcpy(h->dmapf, trip.data(), sizeof(float) * trip.size(), hipMemcpyHostToDevice));
    }
    h->L = L;
    h->maps_each = false;   // (after slam_set_maps: back to the shared map)
    h->hmap.assign(map_xy, map_xy + 2 * (size_t)L);
    if (h->shadow) { const int rs = slam_set_map(h->shadow, map_xy, L); if (rs) return rs; }
    return SLAM_OK;
}

int slam_step_dev(slam_handle* h, const float cmd[2], const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || !cmd || !d_meas || !d_count || k_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    if (h->shadow) {   // the tracked instance's slice of the message, ordered after what the caller enqueued on the handle's stream
        if (!h->shadow_ev) HIP_TRY(hipEventCreateWithFlags(&h->shadow_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->shadow_ev, h->stream));
        HIP_TRY(hipStreamWaitEvent(h->shadow->stream, h->shadow_ev, 0));
        const int rs = slam_step_dev(h->shadow, cmd, d_meas + (size_t)h->tracked * k_stride * 3, d_count + h->tracked, k_stride);
        if (rs) return rs;
        // ... and the other way round: the shadow reads the CALLER's buffers on its own stream, and the header promises that they
        // may be overwritten by work enqueued on the handle's stream after this call returns
        HIP_TRY(hipEventRecord(h->shadow_ev, h->shadow->stream));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->shadow_ev, 0));
    }
    // Device buffers on the caller's stream: queueing is OPT-IN here (slam_set_lazy_steps / SLAM_LAZY_STEPS), because a queued
    // call enqueues only its device-to-device copy on the stream, not the step itself
    if (h->kind == SLAM_EKF_SLAM && h->lazy_explicit && h->lazy_max > 1 && h->run_chunk != 1 && !h->dump_meas &&
        k_stride <= slam::ekf_class_message_capacity(h->L_max)) {   // (messages that may be longer: one launch pair per step, launch_step)
        StepQueue& q = h->q;
        if (!queue_takes(h, StepQueue::kDev, k_stride)) TRY(flush_lazy(h));   // earlier steps first
        const size_t B = (size_t)h->B;
        const size_t steps = (size_t)h->lazy_max;
        if (q.dmeas.cap() < 3 * (size_t)k_stride * B * steps || q.dcount.cap() < B * steps) {
            if (q.dmeas) HIP_TRY(hipStreamSynchronize(h->stream));
            HIP_TRY(q.dmeas.reserve(3 * (size_t)k_stride * B * steps)); HIP_TRY(q.dcount.reserve(B * steps));
        }
        const size_t n = (size_t)q.steps();
        HIP_TRY(hipMemcpyAsync(q.dmeas + n * B * k_stride * 3, d_meas, sizeof(float) * 3 * (size_t)k_stride * B, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(q.dcount + n * B, d_count, sizeof(int32_t) * B, hipMemcpyDeviceToDevice, h->stream));
        q.src = StepQueue::kDev; q.ks = k_stride;
        q.cmds.push_back(cmd[0]); q.cmds.push_back(cmd[1]);
        return q.steps() >= h->lazy_max ? flush_lazy(h) : SLAM_OK;
    }
    TRY(flush_lazy(h));
    if (h->kind == SLAM_UKF_LOC && !h->dmapf) return fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    return launch_step(h, cmd, 0, d_meas, d_count, k_stride);
}

int slam_step(slam_handle* h, const float cmd[2], const float* meas, const int32_t* count, int k_stride) {
    if (!h || !cmd || !meas || !count || k_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    if (h->shadow) {   // the tracked instance's slice of the message runs in the shadow at once
        const int rs = slam_step(h->shadow, cmd, meas + (size_t)h->tracked * k_stride * 3, count + h->tracked, k_stride);
        if (rs) return rs;
    }
    const size_t B = (size_t)h->B;
    int kmax = 0;   // the longest message, clamped to k_stride
    for (size_t b = 0; b < B; ++b) kmax = count[b] > kmax ? count[b] : kmax;   // 65 536 ints: ~20 us
    kmax = kmax < k_stride ? kmax : k_stride;
    if (h->kind == SLAM_EKF_SLAM && h->lazy_max > 1 && h->run_chunk != 1 && kmax <= kExtQ) {
        StepQueue& q = h->q;
        // a fill of the queue has ONE stride (detections per instance): the largest message this handle has seen so far, at
        // least 2 (a high-water mark: a stride per fill taken from its first message ended fills early whenever a larger
        // message followed, 46 instead of 65 M steps/s); a message above the mark ends the fill and raises it
        if (!queue_takes(h, StepQueue::kHost, kmax)) TRY(flush_lazy(h));
        if (kmax > q.host_ks) q.host_ks = kmax;
        StepQueue::HostFill& f = q.host[q.host_cur];
        if (q.steps() == 0) {
            if (f.in_use) { HIP_TRY(hipEventSynchronize(f.used)); f.in_use = false; }   // the launch that read this fill is done
            // capacity: the full stride kExtQ at once while that stays below 128 MB per fill (re-pinning 100 MB of host memory
            // costs ~40 ms each time the stride grows: 0.5 ms per step over a 300-step run); above that, the stride actually seen
            const size_t full = (size_t)3 * kExtQ * B * h->lazy_max;
            const size_t need = sizeof(float) * full <= ((size_t)128 << 20) ? full : (size_t)3 * q.host_ks * B * h->lazy_max;   // floats
            HIP_TRY(f.hmeas.reserve(need)); HIP_TRY(f.hcount.reserve(B * h->lazy_max)); HIP_TRY(f.hcmds.reserve(2 * (size_t)h->lazy_max));
            HIP_TRY(f.dmeas.reserve(need)); HIP_TRY(f.dcount.reserve(B * h->lazy_max));
            if (!f.copied) {
                HIP_TRY(hipEventCreateWithFlags(&f.copied, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&f.used, hipEventDisableTiming));
            }
            q.src = StepQueue::kHost; q.ks = q.host_ks;
        }
        const int ks = q.ks;
        const size_t n = (size_t)q.steps();
        float* dst = f.hmeas + n * B * ks * 3;
        int32_t* dcnt = f.hcount + n * B;
        const int kc = k_stride < ks ? k_stride : ks;   // detections per instance that are packed
        // The count is clamped to what is packed, like the immediate path clamps to k_stride, so the kernel never
        // reads a slot this call did not fill.  The copy itself has a compile-time size (kc detections, all within the caller's
        // k_stride): a per-instance variable-length memcpy made the call six times slower (1.28 vs 0.2 ms at batch 65 536).
        auto pack = [&](auto kc_tag) {
            constexpr int KC = decltype(kc_tag)::value;
            host_parallel(B, [&](size_t b0, size_t b1) {
                for (size_t b = b0; b < b1; ++b) {
                    const int cb = count[b];
                    dcnt[b] = cb < 0 ? 0 : (cb < KC ? cb : KC);
                    memcpy(dst + b * ks * 3, meas + b * (size_t)k_stride * 3, sizeof(float) * 3 * KC);
                }
            });
        };
        switch (kc) {
            case 1: pack(std::integral_constant<int, 1>{}); break;
            case 2: pack(std::integral_constant<int, 2>{}); break;
            case 3: pack(std::integral_constant<int, 3>{}); break;
            default: pack(std::integral_constant<int, 4>{}); break;   // kc <= ks <= kExtQ = 4
        }
        q.cmds.push_back(cmd[0]); q.cmds.push_back(cmd[1]);
        return (q.steps() >= h->lazy_max || eager_flush(h, q.steps())) ? flush_lazy(h) : SLAM_OK;
    }
    TRY(flush_lazy(h));
    return step_host_now(h, cmd, nullptr, meas, count, k_stride, kmax);
}

}  // extern "C"

// One timestep on host messages, launched at the call (after what is queued).  d_cmd_each: [B][2] per-instance commands already on the
// handle's stream (device), NULL = cmd.  kmax: the longest message of the call, clamped to k_stride.
static int step_host_now(slam_handle* h, const float cmd[2], const float* d_cmd_each, const float* meas, const int32_t* count, int k_stride, int kmax) {
    const size_t B = (size_t)h->B;
    if (h->kind == SLAM_UKF_LOC && !h->dmapf) return fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    // The caller's buffers may be reused right after return (ekf.cpp:64 copies the message), so the message is packed
    // into one of two PINNED staging buffers (only max_b count[b] detections per instance travel), copied on a separate
    // stream while the previous step's kernel is still running, and the kernel waits for the copy by event.  The host
    // blocks only when it gets two steps ahead of the GPU.
    slam_handle::Stage& s = h->stage[h->stage_next & 1];
    h->stage_next += 1;
    if (kmax < 1) kmax = 1;
    if (!h->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    if (!s.copied) {
        HIP_TRY(hipEventCreateWithFlags(&s.copied, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&s.used, hipEventDisableTiming));
    }
    HIP_TRY(s.hcount.reserve(B)); HIP_TRY(s.dcount.reserve(B));
    if (s.in_use) HIP_TRY(hipEventSynchronize(s.used));   // the kernel of two steps ago has consumed this buffer
    const size_t need = (size_t)3 * kmax * B;
    const size_t cap = (size_t)3 * (kmax < 8 && k_stride >= 8 ? 8 : kmax) * B;   // (grown to at least 8 detections at once)
    if (s.hmeas.cap() < need) HIP_TRY(s.hmeas.reserve(cap));
    if (s.dmeas.cap() < need) HIP_TRY(s.dmeas.reserve(cap));
    memcpy(s.hcount, count, sizeof(int32_t) * B);
    if (kmax == k_stride) {
        memcpy(s.hmeas, meas, sizeof(float) * need);
    } else {
        for (size_t b = 0; b < B; ++b)
            memcpy(s.hmeas + (size_t)3 * kmax * b, meas + (size_t)3 * k_stride * b, sizeof(float) * 3 * kmax);
    }
    HIP_TRY(hipMemcpyAsync(s.dcount, s.hcount, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(hipMemcpyAsync(s.dmeas, s.hmeas, sizeof(float) * need, hipMemcpyHostToDevice, h->copy_stream));
    HIP_TRY(hipEventRecord(s.copied, h->copy_stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, s.copied, 0));
    // (kmax = the longest message of this call: beyond the size class's capacity the instances concerned take the streamed kernel, launch_step)
    int rc = launch_step(h, cmd, 0, s.dmeas, s.dcount, kmax, d_cmd_each);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(s.used, h->stream));
    s.in_use = true;
    return SLAM_OK;
}

extern "C" {

int slam_step_sim(slam_handle* h, const float cmd[2]) {
    if (!h || !cmd) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    if (h->shadow) { const int rs = slam_step_sim(h->shadow, cmd); if (rs) return rs; }
    if (h->kind == SLAM_EKF_SLAM && h->lazy_max > 1 && !h->dump_meas && h->run_chunk != 1) {
        StepQueue& q = h->q;
        if (!queue_takes(h, StepQueue::kSim, 0)) TRY(flush_lazy(h));   // measurement-driven steps queued before this one run first
        q.src = StepQueue::kSim; q.ks = 0;
        q.cmds.push_back(cmd[0]); q.cmds.push_back(cmd[1]);
        return q.steps() >= h->lazy_max ? flush_lazy(h) : SLAM_OK;
    }
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return launch_step(h, cmd, 1, nullptr, nullptr, 0);
}

int slam_queued_steps(const slam_handle* h) {
    if (!h) return 0;
    return h->q.steps();
}

int slam_set_lazy_steps(slam_handle* h, int n) {
    if (!h || n < 0) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    h->lazy_max = n;
    h->lazy_explicit = true;
    return SLAM_OK;
}

int slam_run_sim(slam_handle* h, const float* cmds, int T) {
    if (!h || !cmds || T < 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    if (h->shadow) { const int rs = slam_run_sim(h->shadow, cmds, T); if (rs) return rs; }
    TRY(flush_lazy(h));
    return run_sim_now(h, cmds, T);
}

}  // extern "C"

// d_cmd_each: the commands are per instance, [T][B][2] on the device (cmds is not read)
static int run_sim_now(slam_handle* h, const float* cmds, int T, const float* d_cmd_each) {
    if (T == 0) return SLAM_OK;
    const size_t each_step = 2 * (size_t)h->B;   // floats of d_cmd_each per timestep
    auto cmd_at = [&](size_t t) { return d_cmd_each ? kNoCmd : cmds + 2 * t; };
    auto each_at = [&](size_t t) { return d_cmd_each ? d_cmd_each + t * each_step : nullptr; };
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
    if (h->kind != SLAM_EKF_SLAM && !h->dump_meas && h->B >= h->ukf_split_min) {
        // UKF: two launches per timestep (LDS-bound eigen-sqrt, then the latency-heavier sigma-point kernel).  The two
        // halves of the batch run on two streams and drift apart, so one half's sqrt overlaps the other's step kernel.
        HIP_TRY(hipSetDevice(h->device));
        const int NP = h->ukf_parts < 2 ? 2 : (h->ukf_parts > 4 ? 4 : h->ukf_parts);
        for (int a = 0; a < NP - 1; ++a)
            if (!h->aux_stream[a]) {
                HIP_TRY(hipStreamCreateWithFlags(&h->aux_stream[a], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&h->aux_ev[a + 1], hipEventDisableTiming));
            }
        if (!h->aux_ev[0]) HIP_TRY(hipEventCreateWithFlags(&h->aux_ev[0], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->aux_ev[0], h->stream));
        for (int a = 0; a < NP - 1; ++a) HIP_TRY(hipStreamWaitEvent(h->aux_stream[a], h->aux_ev[0], 0));
        const int per = (h->B + NP - 1) / NP;
        int long_cap = 0;
        if (const int rc = long_message_cap(h, 1, 0, &long_cap)) return rc;
        for (int t = 0; t < T; ++t) {
            for (int part = 0; part < NP; ++part) {
                const int b_off = part * per;
                const int b_cnt = h->B - b_off < per ? h->B - b_off : per;
                if (b_cnt <= 0) continue;
                TRY(launch_ukf_pair(h, cmd_at(t), 1, long_cap, nullptr, nullptr, 0, b_off, b_cnt, part ? h->aux_stream[part - 1] : h->stream, each_at(t)));
            }
            std::swap(h->dP, h->dP2);
            h->step += 1;
        }
        for (int a = 0; a < NP - 1; ++a) {
            HIP_TRY(hipEventRecord(h->aux_ev[a + 1], h->aux_stream[a]));
            HIP_TRY(hipStreamWaitEvent(h->stream, h->aux_ev[a + 1], 0));
        }
        return SLAM_OK;
    }
    if (h->kind != SLAM_EKF_SLAM || h->dump_meas || h->run_chunk == 1) {
        // one launch (pair) per timestep
        HIP_TRY(hipSetDevice(h->device));
        for (int t = 0; t < T; ++t) {
            int rc = launch_step(h, cmd_at(t), 1, nullptr, nullptr, 0, each_at(t));
            if (rc) return rc;
        }
        return SLAM_OK;
    }
    // EKF: every workgroup carries its instance through a whole chunk of timesteps, keeping x_t, the landmark ids,
    // the true pose and the thin rows/cols of P on chip; only the P stream touches HBM each step.
    HIP_TRY(hipSetDevice(h->device));
    if (!d_cmd_each) {
        TRY(grow(h, h->dcmds, 2 * (size_t)T));
        HIP_TRY(hipMemcpyAsync(h->dcmds, cmds, sizeof(float) * 2 * (size_t)T, hipMemcpyHostToDevice, h->stream));
    }
    const int chunk = h->run_chunk > 0 ? h->run_chunk : T;
    int long_cap = 0;   // a map with more landmarks than a message of this size class holds: the streamed kernel, a launch per timestep
    if (const int rc = long_message_cap(h, 1, 0, &long_cap)) return rc;
    for (int t0 = 0; t0 < T; t0 += chunk) {
        const int tc = T - t0 < chunk ? T - t0 : chunk;
        slam::EkfStepParams p;
        if (d_cmd_each) fill_ekf_params(h, p, kNoCmd, 1, long_cap, nullptr, nullptr, 0, nullptr, tc, each_at(t0));
        else fill_ekf_params(h, p, cmds + 2 * (size_t)t0, 1, long_cap, nullptr, nullptr, 0, h->dcmds + 2 * (size_t)t0, tc);
        HIP_TRY(slam::launch_ekf_step(p, h->waves_per_filter, h->esz == 4, h->stream));
        h->step += (uint32_t)tc;
    }
    return SLAM_OK;
}

// Runs what the step queue holds: messages as one multi-step launch, generator steps through run_sim_now.  The queue is emptied only
// once the launch is enqueued: a failed flush keeps the queued timesteps (and fails again on the next call) instead of dropping them
// silently.
static int flush_lazy(slam_handle* h) {
    StepQueue& q = h->q;
    const int T = q.steps();
    if (T == 0) return SLAM_OK;
    StepQueue::HostFill& f = q.host[q.host_cur];
    if (q.src == StepQueue::kSim) {
        TRY(run_sim_now(h, q.cmds.data(), T));   // chunking (run_chunk) and messages longer than the size class apply here too
    } else {
        const size_t B = (size_t)h->B;
        HIP_TRY(hipSetDevice(h->device));
        const float* cmds = q.cmds.data();
        const float* meas = q.dmeas; const int32_t* count = q.dcount;
        if (q.src == StepQueue::kHost) {
            if (!h->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
            HIP_TRY(hipMemcpyAsync(f.dcount, f.hcount, sizeof(int32_t) * B * T, hipMemcpyHostToDevice, h->copy_stream));
            HIP_TRY(hipMemcpyAsync(f.dmeas, f.hmeas, sizeof(float) * 3 * q.ks * B * T, hipMemcpyHostToDevice, h->copy_stream));
            HIP_TRY(hipEventRecord(f.copied, h->copy_stream));
            memcpy(f.hcmds, cmds, sizeof(float) * 2 * (size_t)T);
            cmds = f.hcmds; meas = f.dmeas; count = f.dcount;
        }
        TRY(grow(h, h->dcmds, 2 * (size_t)T));
        // device messages: a pageable source, so the copy is staged by the runtime before the call returns and q.cmds may be reused at once
        HIP_TRY(hipMemcpyAsync(h->dcmds, cmds, sizeof(float) * 2 * (size_t)T, hipMemcpyHostToDevice, h->stream));
        if (q.src == StepQueue::kHost) HIP_TRY(hipStreamWaitEvent(h->stream, f.copied, 0));
        slam::EkfStepParams p;
        fill_ekf_params(h, p, cmds, 0, 0, meas, count, q.ks, h->dcmds, T);
        HIP_TRY(slam::launch_ekf_step(p, h->waves_per_filter, h->esz == 4, h->stream));
        h->step += (uint32_t)T;
    }
    const StepQueue::Source src = q.src;
    q.src = StepQueue::kNone;
    q.cmds.clear();
    if (src == StepQueue::kHost) {   // the next fill packs into the other buffers while this one is copied and read
        HIP_TRY(hipEventRecord(f.used, h->stream));
        f.in_use = true;
        q.host_cur ^= 1;
    }
    return SLAM_OK;
}

extern "C" {

// UKF::predictionStage / UKF::updateStage (filter.h:187-188, ukf.cpp:197-291) as two calls.  predictionStage only
// writes members that updateStage consumes (sqtP, X, X_pred, x_pred, P_pred); x_t / P_t change when updateStage
// finishes (ukf.cpp:289-290).  So the split is: predict = nearestSPD + sqrt (the kernel that dominates the step) with
// the command remembered; update = the fused sigma-point / update / insertion kernel with that command.  The pair is
// bit-identical to slam_step_dev.
int slam_predict(slam_handle* h, const float cmd[2]) {
    if (!h || !cmd) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate prediction stage: EKF::update does both (ekf.cpp:37-179); use slam_step");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->predicted) return fail(SLAM_ERR_STATE, "slam_predict called twice without slam_update_dev");
    HIP_TRY(hipSetDevice(h->device));
    slam::UkfStepParams p;
    fill_ukf_params(h, p, cmd);
    HIP_TRY(slam::launch_ukf_sqrt(p, h->stream));
    h->pred_cmd[0] = cmd[0]; h->pred_cmd[1] = cmd[1];
    h->pred_each = false;
    h->predicted = true;
    return SLAM_OK;
}
int slam_update_dev(slam_handle* h, const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || k_stride < 0 || (k_stride > 0 && (!d_meas || !d_count))) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate update stage (ekf.cpp:37-179); use slam_step");
    if (!h->predicted) return fail(SLAM_ERR_STATE, "slam_update_dev needs a preceding slam_predict");
    HIP_TRY(hipSetDevice(h->device));
    if (k_stride == 0) {   // empty message for every instance
        int rc = ensure_meas_buffers(h, 1);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(h->dcount, 0, sizeof(int32_t) * (size_t)h->B, h->stream));
        d_meas = h->dmeas; d_count = h->dcount; k_stride = 1;
    }
    int long_cap = 0;
    if (const int rc = long_message_cap(h, 0, k_stride, &long_cap)) return rc;
    slam::UkfStepParams p;
    fill_ukf_params(h, p, h->pred_cmd, h->pred_each ? h->dcmd_each.get() : nullptr);
    p.sim = 0;
    p.long_mode = long_cap > 0 ? 1 : 0; p.long_cap = long_cap;
    p.meas_in = d_meas; p.meas_count_in = d_count; p.k_stride_in = k_stride;
    HIP_TRY(slam::launch_ukf_step(p, h->stream));
    std::swap(h->dP, h->dP2);
    h->step += 1;
    h->predicted = false;
    h->pred_each = false;
    return SLAM_OK;
}

// UKFState.X (ukf.cpp:92-101): the sigma points of the last predictionStage, column-major n x (2n+1):
// X = [x, x + offset i, x - offset i] with offset i = row i of sqtP (ukf.cpp:214-219) around the x_t that step started from.
int slam_get_sigma_points(slam_handle* h, int inst, double* X, int32_t* rows, int32_t* cols) {
    if (!h || inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "bad instance");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "sigma points exist for the UKF kinds only");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, h->dnsq + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    n = n < 0 ? 0 : (n > h->n_max ? h->n_max : n);
    if (rows) *rows = n;
    if (cols) *cols = n > 0 ? 2 * n + 1 : 0;
    if (!X || n <= 0) return SLAM_OK;
    std::vector<double> x(n), S((size_t)n * n);
    HIP_TRY(hipMemcpy(x.data(), h->dxprev + (size_t)inst * h->xstride, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(S.data(), h->dsq + (size_t)inst * h->pstride, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
    // offset i = row i of sqtP, as ukf_step_kernel reads it: the symmetric eigen root (both halves written from one value) or, in
    // SLAM_UKF_SQRT_CHOLESKY mode, L^T row-major, whose row i is column i of L
    for (int r = 0; r < n; ++r) X[r] = x[r];
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < n; ++r) {
            X[(size_t)(1 + i) * n + r] = x[r] + S[(size_t)i * n + r];
            X[(size_t)(1 + n + i) * n + r] = x[r] - S[(size_t)i * n + r];
        }
    return SLAM_OK;
}

// device -> host copy of `count` stored elements, widened to double when the storage type is fp32
static int fetch_elems(slam_handle* h, double* dst, const void* dbase, size_t elem_offset, size_t count) {
    if (h->esz == 8) {
        HIP_TRY(hipMemcpy(dst, (const char*)dbase + elem_offset * 8, count * 8, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp(count);
        HIP_TRY(hipMemcpy(tmp.data(), (const char*)dbase + elem_offset * 4, count * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < count; ++i) dst[i] = (double)tmp[i];
    }
    return SLAM_OK;
}

int slam_get_state(slam_handle* h, int inst, double* x, double* P, int32_t* M, int32_t* ids, int32_t* ts) {
    if (!h || inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "bad instance");
    if (h->shadow && inst == h->tracked) return slam_get_state(h->shadow, 0, x, P, M, ids, ts);   // the batch's queue stays queued
    TRY(flush_lazy(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int32_t m = 0;
    HIP_TRY(hipMemcpy(&m, h->dM + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    m = m < 0 ? 0 : (m > h->L_max ? h->L_max : m);   // never index past the caller's n_max-sized buffers
    const int n = h->base + 2 * m;
    if (M) *M = m;
    int rc;
    if (x && (rc = fetch_elems(h, x, h->dx, (size_t)inst * h->xstride, n))) return rc;
    if (P) {   // rows of the device matrix are ld elements apart (pad columns beyond n); the caller gets packed n x n
        const int ld = h->kind == SLAM_EKF_SLAM ? slam::ekf_ld(n, h->esz) : n;
        std::vector<double> tmp((size_t)n * ld);
        if ((rc = fetch_elems(h, tmp.data(), h->dP, (size_t)inst * h->pstride, (size_t)n * ld))) return rc;
        for (int r = 0; r < n; ++r) memcpy(P + (size_t)r * n, tmp.data() + (size_t)r * ld, sizeof(double) * n);
    }
    if (ids && m > 0) HIP_TRY(hipMemcpy(ids, h->dids + (size_t)inst * h->L_max, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    if (ts) HIP_TRY(hipMemcpy(ts, h->dts + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_get_poses(slam_handle* h, double* poses) {
    if (!h || !poses) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->esz == 8) {
        HIP_TRY(hipMemcpy2D(poses, sizeof(double) * 3, h->dx, sizeof(double) * h->xstride, sizeof(double) * 3, h->B, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp((size_t)3 * h->B);
        HIP_TRY(hipMemcpy2D(tmp.data(), sizeof(float) * 3, h->dx, sizeof(float) * h->xstride, sizeof(float) * 3, h->B, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) poses[i] = (double)tmp[i];
    }
    return SLAM_OK;
}

static int copy_out(slam_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h || !dst) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SLAM_OK;
}
int slam_get_landmark_counts(slam_handle* h, int32_t* M) { return copy_out(h, M, h ? h->dM : nullptr, h ? sizeof(int32_t) * (size_t)h->B : 0); }
int slam_get_truth(slam_handle* h, double* t) { return copy_out(h, t, h ? h->dtruth : nullptr, h ? sizeof(double) * 3 * (size_t)h->B : 0); }
int slam_status(slam_handle* h, int32_t* f) { return copy_out(h, f, h ? h->dflags : nullptr, h ? sizeof(int32_t) * (size_t)h->B : 0); }

int slam_get_last_meas(slam_handle* h, float* meas, int32_t* count, int k_stride) {
    if (!h || !meas || !count || k_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (!h->dump_meas || h->k_stride < k_stride) {
        // enable the dump for subsequent slam_step_sim calls; nothing recorded yet for past steps
        int rc = ensure_meas_buffers(h, k_stride);
        if (rc) return rc;
        if (!h->dump_meas) {
            h->dump_meas = true;
            memset(count, 0, sizeof(int32_t) * (size_t)h->B);
            return SLAM_OK;
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy2D(meas, sizeof(float) * 3 * k_stride, h->dmeas, sizeof(float) * 3 * h->k_stride,
                        sizeof(float) * 3 * k_stride, h->B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, h->dcount, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_error_stats(slam_handle* h, double* avg) {
    if (!h || !avg) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    std::vector<int32_t> ts(h->B);
    int rc = copy_out(h, avg, h->derr, sizeof(double) * (size_t)h->B);
    if (rc) return rc;
    rc = copy_out(h, ts.data(), h->dts, sizeof(int32_t) * (size_t)h->B);
    if (rc) return rc;
    for (int i = 0; i < h->B; ++i) avg[i] = ts[i] > 0 ? avg[i] / ts[i] : 0.0;  // sum(errors) / num_iters
    return SLAM_OK;
}

extern "C" int slam_internal_error_stats_dev(slam_handle* h, double* d_out, long long pad) {
    if (!h || !d_out || pad < h->B) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(slam::launch_avg_error(h->derr, h->dts, h->B, (int)pad, d_out, h->stream));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    return SLAM_OK;
}

// ---- checkpoint / resume (the reference keeps the filter only in memory) ------------------------------
namespace {
struct CkptHeader {
    char magic[8];            // "SLAMCKP1"
    int32_t kind, B, L_max, dtype, n_max, pstride, xstride, esz;
    uint32_t step;
    int32_t inited, reserved0;
    uint64_t seed;
    int64_t inst0;
};
struct CkptItem { void* dev; size_t bytes; };

std::vector<CkptItem> ckpt_items(slam_handle* h) {
    const size_t B = (size_t)h->B, e = (size_t)h->esz;
    std::vector<CkptItem> it = {
        {h->dP, e * B * h->pstride}, {h->dx, e * B * h->xstride}, {h->dM, sizeof(int32_t) * B}, {h->dids, sizeof(int32_t) * B * h->L_max},
        {h->dflags, sizeof(int32_t) * B}, {h->dts, sizeof(int32_t) * B}, {h->dtruth, sizeof(double) * B * 3}, {h->derr, sizeof(double) * B},
    };
    if (h->kind != SLAM_EKF_SLAM) {   // UKF: the square root of the last prediction stage and the warm-start eigenvectors
        it.push_back({h->dsq, sizeof(double) * B * h->pstride}); it.push_back({h->dnsq, sizeof(int32_t) * B});
        it.push_back({h->dxprev, sizeof(double) * B * h->xstride}); it.push_back({h->dvt, sizeof(double) * B * h->pstride});
        it.push_back({h->dvage, sizeof(int32_t) * B});
    }
    return it;
}
}  // namespace

int slam_save_state(slam_handle* h, const char* path) {
    if (!h || !path) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    FILE* f = fopen(path, "wb");
    if (!f) return fail(SLAM_ERR_IO, "cannot write %s", path);
    CkptHeader hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, "SLAMCKP1", 8);
    hd.kind = h->kind; hd.B = h->B; hd.L_max = h->L_max; hd.dtype = h->dtype; hd.n_max = h->n_max; hd.pstride = h->pstride; hd.xstride = h->xstride;
    hd.esz = h->esz; hd.step = h->step; hd.inited = h->inited ? 1 : 0; hd.seed = h->seed; hd.inst0 = h->inst0;
    bool ok = fwrite(&hd, sizeof(hd), 1, f) == 1;
    std::vector<char> buf((size_t)64 << 20);
    for (const CkptItem& it : ckpt_items(h))
        for (size_t off = 0; ok && off < it.bytes; off += buf.size()) {
            const size_t nb = it.bytes - off < buf.size() ? it.bytes - off : buf.size();
            if (hipMemcpy(buf.data(), (const char*)it.dev + off, nb, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return fail(SLAM_ERR_HIP, "copying the state to the host failed"); }
            ok = fwrite(buf.data(), 1, nb, f) == nb;
        }
    ok = (fclose(f) == 0) && ok;
    return ok ? SLAM_OK : fail(SLAM_ERR_IO, "short write to %s", path);
}

int slam_load_state(slam_handle* h, const char* path) {
    if (!h || !path) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    FILE* f = fopen(path, "rb");
    if (!f) return fail(SLAM_ERR_IO, "cannot open %s", path);
    CkptHeader hd;
    if (fread(&hd, sizeof(hd), 1, f) != 1 || memcmp(hd.magic, "SLAMCKP1", 8) != 0) { fclose(f); return fail(SLAM_ERR_IO, "%s is not a state file of this library", path); }
    if (hd.kind != h->kind || hd.B != h->B || hd.L_max != h->L_max || hd.dtype != h->dtype || hd.pstride != h->pstride || hd.xstride != h->xstride || hd.esz != h->esz) {
        fclose(f);
        return fail(SLAM_ERR_ARG, "%s holds kind %d, batch %d, L_max %d, dtype %d; the handle is kind %d, batch %d, L_max %d, dtype %d", path, hd.kind, hd.B, hd.L_max,
                    hd.dtype, h->kind, h->B, h->L_max, h->dtype);
    }
    if (hd.n_max != h->n_max) { fclose(f); return fail(SLAM_ERR_ARG, "%s was written for a state capacity of %d, the handle has %d", path, hd.n_max, h->n_max); }
    // The step kernels trust the per-instance counters (n = 3 + 2 M sizes every loop over LDS and the instance's slab), so a
    // corrupted or hand-made file must be refused BEFORE anything reaches the device: landmark counts, the size of the UKF's
    // stored square root and the timesteps are checked on the host first.
    {
        const std::vector<CkptItem> items = ckpt_items(h);
        std::vector<size_t> off(items.size() + 1, sizeof(hd));
        for (size_t i = 0; i < items.size(); ++i) off[i + 1] = off[i] + items[i].bytes;
        std::vector<int32_t> col((size_t)h->B);
        auto column = [&](size_t item, const char* what, int lo, int hi) -> int {
            if (fseek(f, (long)off[item], SEEK_SET) != 0 || fread(col.data(), sizeof(int32_t), col.size(), f) != col.size()) return fail(SLAM_ERR_IO, "%s is truncated", path);
            for (size_t b = 0; b < col.size(); ++b)
                if (col[b] < lo || col[b] > hi) return fail(SLAM_ERR_ARG, "%s: %s of instance %zu is %d, outside [%d, %d]", path, what, b, col[b], lo, hi);
            return SLAM_OK;
        };
        int rc = column(2, "the landmark count", 0, h->L_max);
        if (!rc) rc = column(5, "the timestep", 0, INT32_MAX);
        if (!rc && h->kind != SLAM_EKF_SLAM) rc = column(9, "the size of the stored square root", 0, h->n_max);
        // -1 is the cold-start marker (ukf_init_kernel, and both sqrt kernels after SLAM_INST_SQRT_FAILED); the kernels count the
        // age up to kUkfWarmMaxAge = 100 and start cold from there, so nothing a run can produce lies outside [-1, 100].
        if (!rc && h->kind != SLAM_EKF_SLAM) rc = column(12, "the age of the warm-start eigenvectors", -1, 100);
        if (rc) { fclose(f); return rc; }
        if (fseek(f, (long)sizeof(hd), SEEK_SET) != 0) { fclose(f); return fail(SLAM_ERR_IO, "cannot rewind %s", path); }
    }
    std::vector<char> buf((size_t)64 << 20);
    for (const CkptItem& it : ckpt_items(h))
        for (size_t off = 0; off < it.bytes; off += buf.size()) {
            const size_t nb = it.bytes - off < buf.size() ? it.bytes - off : buf.size();
            if (fread(buf.data(), 1, nb, f) != nb) { fclose(f); return fail(SLAM_ERR_IO, "%s is truncated", path); }
            if (hipMemcpy((char*)it.dev + off, buf.data(), nb, hipMemcpyHostToDevice) != hipSuccess) { fclose(f); return fail(SLAM_ERR_HIP, "copying the state to the device failed"); }
        }
    fclose(f);
    h->step = hd.step; h->inited = hd.inited != 0; h->seed = hd.seed; h->inst0 = hd.inst0;
    h->predicted = false;
    if (h->shadow) {   // the tracked instance restarts from the loaded state
        const int tr = h->tracked;
        const int rc = slam_track_instance(h, tr);
        if (rc) return rc;
    }
    return SLAM_OK;
}

int slam_track_instance(slam_handle* h, int inst) {
    if (!h || inst >= h->B) return fail(SLAM_ERR_ARG, "bad instance");
    TRY(flush_lazy(h));
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    if (h->shadow) { slam_destroy(h->shadow); h->shadow = nullptr; h->tracked = -1; }
    if (inst < 0) return SLAM_OK;
    if (h->kind != SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "EKF handles only: the UKF launches every step at the call, there is no queue a getter would have to run");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    slam_handle* s = nullptr;
    int rc = slam_create(&h->cfg, h->kind, 1, h->L_max, h->dtype, h->device, &s);
    if (rc) return rc;
    s->lazy_max = 0;                     // every step of the shadow is launched at the call
    s->seed = h->seed; s->inst0 = h->inst0 + inst;
    s->range_max = h->range_max; s->fov_min = h->fov_min; s->fov_max = h->fov_max;
    s->waves_per_filter = h->waves_per_filter;
    if (!h->hmap.empty()) rc = slam_set_map(s, h->hmap.data(), (int)(h->hmap.size() / 2));
    if (!rc && h->maps_each)   // the instance's own map (set after the shared one, which it replaces)
        rc = slam_set_maps(s, h->hmaps.data() + (size_t)inst * h->map_stride * 2, h->hLs.data() + inst, h->map_stride);
    if (!rc && h->noise_each) rc = slam_set_noise_each(s, h->hnoise.data() + inst);   // the instance's noise row
    if (!rc && h->inited) {
        // the instance's state as it is now: same slab layout (pstride / xstride depend on L_max and dtype only)
        const size_t b = (size_t)inst, e = (size_t)h->esz;
        hipError_t errs[] = {
            hipMemcpy(s->dP, (const char*)h->dP + b * h->pstride * e, (size_t)h->pstride * e, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dx, (const char*)h->dx + b * h->xstride * e, (size_t)h->xstride * e, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dM, h->dM + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dids, h->dids + b * h->L_max, sizeof(int32_t) * h->L_max, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dflags, h->dflags + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dts, h->dts + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dtruth, h->dtruth + 3 * b, sizeof(double) * 3, hipMemcpyDeviceToDevice),
            hipMemcpy(s->derr, h->derr + b, sizeof(double), hipMemcpyDeviceToDevice),
            h->dsq ? hipMemcpy(s->dsq, h->dsq + b * h->pstride, sizeof(double) * h->pstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->dnsq ? hipMemcpy(s->dnsq, h->dnsq + b, sizeof(int32_t), hipMemcpyDeviceToDevice) : hipSuccess,
            h->dxprev ? hipMemcpy(s->dxprev, h->dxprev + b * h->xstride, sizeof(double) * h->xstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->dvt ? hipMemcpy(s->dvt, h->dvt + b * h->pstride, sizeof(double) * h->pstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->dvage ? hipMemcpy(s->dvage, h->dvage + b, sizeof(int32_t), hipMemcpyDeviceToDevice) : hipSuccess,
        };
        for (hipError_t ee : errs)
            if (ee != hipSuccess) { slam_destroy(s); return fail(SLAM_ERR_HIP, "copying the tracked instance -> %s", hipGetErrorString(ee)); }
        s->step = h->step; s->inited = true;
    }
    if (rc) { slam_destroy(s); return rc; }
    h->shadow = s; h->tracked = inst;
    return SLAM_OK;
}

int slam_sync(slam_handle* h) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->eager_target = h->eager_init;   // the pipeline is drained: the next burst of calls fills it from small launches again
    return SLAM_OK;
}
int slam_batch(const slam_handle* h) { return h ? h->B : 0; }
int slam_state_dim_max(const slam_handle* h) { return h ? h->n_max : 0; }

int slam_set_run_chunk(slam_handle* h, int steps_per_launch) {
    if (!h || steps_per_launch < 0) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    h->run_chunk = steps_per_launch;
    return SLAM_OK;
}

// Per-timestep stamps of the EKF multi-step kernel (flag 32) / phase cycle counters (flag 4) for subsequent launches; 0 = off.
// The ablation bits are honoured by -DSLAM_ABLATE builds only.
int slam_set_debug_flags(slam_handle* h, int flags) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
#ifndef SLAM_ABLATE
    flags &= (4 | 32 | 128);   // 128: tests only, provokes the watchdog of the EKF step kernel
#endif
    if ((flags & (4 | 32)) && !h->dprof) {
        HIP_TRY(h->dprof.reserve(slam::kEkfProfSlots * (size_t)h->B));
        HIP_TRY(hipMemset(h->dprof, 0, sizeof(unsigned long long) * h->dprof.cap()));
    }
    h->dbg = flags;
    return SLAM_OK;
}

int slam_variant_available(int L_max, int dtype, int variant) { return slam::ekf_variant_available(L_max, dtype == SLAM_F32, variant); }

int slam_k_histogram(slam_handle* h, uint64_t out[8], int reset) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram element size");
    HIP_TRY(hipMemcpy(out, h->dkhist, sizeof(uint64_t) * 8, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist, 0, sizeof(uint64_t) * 8));
    return SLAM_OK;
}

int slam_traffic_counters(slam_handle* h, uint64_t out[4], int reset) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind != SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "the traffic counters are kept by the EKF step kernels");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->dkhist + slam::kEkfTrafficSlot, sizeof(uint64_t) * 4, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + slam::kEkfTrafficSlot, 0, sizeof(uint64_t) * 4));
    return SLAM_OK;
}

// Both counter sets zeroed IN STREAM ORDER, without a host round trip (round 6): a measurement that resets the counters between its
// warm-up and its timed launches no longer leaves the device idle for the reads and resets - profiles/r06a/launch_edges.txt: an idle
// device before a 20-step launch costs it 9 % (clocks).
int slam_reset_counters_async(slam_handle* h) {
    if (!h) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->dkhist, 0, sizeof(unsigned long long) * 16, h->stream));
    return SLAM_OK;
}

int slam_kernel_info(slam_handle* h, int multi_step, char* name, int name_cap, int32_t out[5]) {
    if (!h || (!name && !out)) return fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind != SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "EKF handles only");
    HIP_TRY(hipSetDevice(h->device));
    slam::EkfKernelInfo ki;
    HIP_TRY(slam::ekf_kernel_info(h->L_max, h->B, h->waves_per_filter, h->esz == 4, multi_step ? 1 : 0, &ki));
    if (name && name_cap > 0) { strncpy(name, ki.name, (size_t)name_cap - 1); name[name_cap - 1] = 0; }
    if (out) {
        hipDeviceProp_t pr;
        HIP_TRY(hipGetDeviceProperties(&pr, h->device));
        out[0] = ki.lds_bytes; out[1] = ki.vgprs; out[2] = ki.threads; out[3] = ki.wg_per_cu; out[4] = pr.multiProcessorCount;
    }
    return SLAM_OK;
}

int slam_ukf_sweep_stats(slam_handle* h, uint64_t out[2], int reset) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_STATE, "UKF handles only");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());   // the UKF splits large batches over two streams
    HIP_TRY(hipMemcpy(out, h->dkhist + 8, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + 8, 0, sizeof(uint64_t) * 2));
    return SLAM_OK;
}

int slam_ukf_set_sqrt_mode(slam_handle* h, int mode) {
    if (!h) return fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_ARG, "the square-root mode is a UKF setting");
    if (mode != SLAM_UKF_SQRT_EIGEN && mode != SLAM_UKF_SQRT_CHOLESKY) return fail(SLAM_ERR_ARG, "unknown square-root mode %d", mode);
    if (mode == SLAM_UKF_SQRT_CHOLESKY && h->L_max > slam::kUkfLdsMaxLandmarks)
        return fail(SLAM_ERR_UNSUPPORTED, "the Cholesky square root exists for the LDS size classes only (L_max <= %d), this handle has L_max %d",
                    slam::kUkfLdsMaxLandmarks, h->L_max);
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (mode == SLAM_UKF_SQRT_CHOLESKY) HIP_TRY(h->dchol.reserve((size_t)h->B));
    h->chol = mode == SLAM_UKF_SQRT_CHOLESKY;
    return SLAM_OK;
}

int slam_ukf_sqrt_stats(slam_handle* h, uint64_t out[2], int reset) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_ARG, "UKF handles only");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());   // the UKF splits large batches over two streams
    HIP_TRY(hipMemcpy(out, h->dkhist + slam::kUkfCholSlot, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + slam::kUkfCholSlot, 0, sizeof(uint64_t) * 2));
    return SLAM_OK;
}

int slam_algorithmic_bytes(slam_handle* h, double* bytes) {
    if (!h || !bytes) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->dscalar, 0, sizeof(double), h->stream));
    HIP_TRY(slam::launch_algorithmic_bytes(h->dM, h->B, h->base, h->esz, h->dscalar, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(bytes, h->dscalar, sizeof(double), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// ---- NEES consistency statistics (consistency_kernel.hip) --------------------------------------------------------------------------------
int slam_consistency(slam_handle* h, double* nees_full, double* nees_pose, double* map_rms, int32_t* dof, int32_t* flags) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind != SLAM_EKF_SLAM)
        return fail(SLAM_ERR_UNSUPPORTED, "slam_consistency is defined for EKF_SLAM only: the UKF state carries (cos yaw, sin yaw), so its P is rank-deficient "
                                          "along the unit circle by construction and indefinite in most steps - a NEES there needs a definition first");
    TRY(flush_lazy(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->L <= 0 || !(h->maps_each ? (bool)h->dmaps : (bool)h->dmap))
        return fail(SLAM_ERR_STATE, "no true map to compare the landmarks with: call slam_set_map (or slam_set_maps) first");
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    slam::ConsistencyParams p;
    int chunk = 0;
    TRY(consistency_params(h, &p, &chunk));
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], h->stream);
    if (e == hipSuccess) e = slam::launch_consistency(p, h->esz == 4, chunk, h->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[1], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    float ms = -1.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (e != hipSuccess) { (void)hipGetLastError(); return fail(SLAM_ERR_HIP, "slam_consistency -> %s", hipGetErrorString(e)); }
    std::vector<int32_t> hd(B);
    HIP_TRY(hipMemcpy(hd.data(), h->dconsi, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    // the model: P once (the n rows of ld elements that are factored), x, ids, M, status, truth, the landmarks' map rows, the outputs
    double bytes = 0.0;
    for (size_t b = 0; b < B; ++b) {
        const int n = hd[b], m = (n - 3) / 2;
        const int nf = (!p.id_known && m > 0) ? 3 : n;
        bytes += (double)nf * slam::ekf_ld(n, h->esz) * h->esz + (double)nf * h->esz + 4.0 * (nf > 3 ? m : 0) + 8.0 + 24.0 + 16.0 * (nf > 3 ? m : 0) + 32.0;
    }
    h->cons_bytes = bytes; h->cons_ms = (double)ms;
    if (dof) memcpy(dof, hd.data(), sizeof(int32_t) * B);
    if (nees_full) HIP_TRY(hipMemcpy(nees_full, h->dcons, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (nees_pose) HIP_TRY(hipMemcpy(nees_pose, h->dcons + B, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (map_rms) HIP_TRY(hipMemcpy(map_rms, h->dcons + 2 * B, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, h->dconsi + B, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_last_consistency_work(slam_handle* h, double* bytes, double* ms) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (h->cons_ms < 0.0) return fail(SLAM_ERR_STATE, "slam_consistency has not run on this handle");
    if (bytes) *bytes = h->cons_bytes;
    if (ms) *ms = h->cons_ms;
    return SLAM_OK;
}

// debug only (not declared in slam_batch.h): per-block phase cycles of the LAST launch, summed over blocks
// (SLAM_DEBUG_FLAGS & 4)
int slam_debug_read_prof(slam_handle* h, unsigned long long* out) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->dprof) return fail(SLAM_ERR_STATE, "SLAM_DEBUG_FLAGS has no timer bit (4 / 32) set");
    const size_t S = h->kind == SLAM_EKF_SLAM ? slam::kEkfProfSlots : 16;   // the UKF kernels use 16 slots per block
    std::vector<unsigned long long> buf(S * h->B);
    HIP_TRY(hipMemcpy(buf.data(), h->dprof, sizeof(unsigned long long) * buf.size(), hipMemcpyDeviceToHost));
    const int nslot = h->kind == SLAM_EKF_SLAM ? 64 : 16;   // out[64] for the EKF (slots 16.. = decoupled loop, 40.. = split control), out[16] for the UKF
    for (int i = 0; i < nslot; ++i) out[i] = 0;
    for (int b = 0; b < h->B; ++b)
        for (int i = 0; i < nslot; ++i) out[i] += buf[S * b + i];
    return SLAM_OK;
}

// debug only: the raw [B][16] buffer
int slam_debug_read_prof_raw(slam_handle* h, unsigned long long* out) {
    if (!h || !out) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->dprof) return fail(SLAM_ERR_STATE, "SLAM_DEBUG_FLAGS has no timer bit (4 / 32) set");
    const size_t S = h->kind == SLAM_EKF_SLAM ? slam::kEkfProfSlots : 16;   // out: [B][S]
    HIP_TRY(hipMemcpy(out, h->dprof, sizeof(unsigned long long) * S * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// device math probe for the bit-exactness tests (a, b, out are HOST arrays; out has 8*n doubles)
int slam_math_probe(const double* a, const double* b, double* out, int n, int device) {
    if (!a || !b || !out || n <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> da, db, dout;   // (released on every return)
    HIP_TRY(da.reserve(n)); HIP_TRY(db.reserve(n)); HIP_TRY(dout.reserve(8 * (size_t)n));
    HIP_TRY(hipMemcpy(da, a, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(slam::launch_math_probe(da, db, dout, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// ---- heterogeneous batches: per-instance start poses, maps and commands ---------------------------------------------------------------
int slam_init_each(slam_handle* h, const float* pose0, const double* truth0) {
    if (!h || !pose0) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    if (h->kind == SLAM_EKF_SLAM) {
        HIP_TRY(h->dpose_each.reserve(3 * B));
        if (truth0) HIP_TRY(h->dstart_each.reserve(3 * B));
        HIP_TRY(hipMemcpyAsync(h->dpose_each, pose0, sizeof(float) * 3 * B, hipMemcpyHostToDevice, h->stream));
        if (truth0) HIP_TRY(hipMemcpyAsync(h->dstart_each, truth0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, h->stream));
        slam::EkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = h->dP; p.x = h->dx; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride; p.f32_storage = h->esz == 4;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        p.pose_each = h->dpose_each; p.truth_each = truth0 ? h->dstart_each.get() : nullptr;
        HIP_TRY(slam::launch_ekf_init(p, h->stream));
    } else {
        // x_t << x_0, y_0, cos(yaw_0), sin(yaw_0) with a float argument (ukf.cpp:33), per instance as slam_init computes it
        std::vector<double> st(7 * B);
        for (size_t b = 0; b < B; ++b) {
            double sn, cs;
            slam::det_sincos((double)pose0[3 * b + 2], &sn, &cs);
            st[4 * b] = pose0[3 * b]; st[4 * b + 1] = pose0[3 * b + 1];
            st[4 * b + 2] = h->cfg.ukf_float_trig ? (double)(float)cs : cs;
            st[4 * b + 3] = h->cfg.ukf_float_trig ? (double)(float)sn : sn;
        }
        if (truth0) memcpy(st.data() + 4 * B, truth0, sizeof(double) * 3 * B);
        HIP_TRY(h->dstart_each.reserve(7 * B));
        HIP_TRY(hipMemcpyAsync(h->dstart_each, st.data(), sizeof(double) * (truth0 ? 7 : 4) * B, hipMemcpyHostToDevice, h->stream));
        slam::UkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = (double*)h->dP.get(); p.x = (double*)h->dx.get(); p.n_sq = h->dnsq; p.v_age = h->dvage; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        p.x_each = h->dstart_each; p.truth_each = truth0 ? h->dstart_each + 4 * B : nullptr;
        HIP_TRY(slam::launch_ukf_init(p, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // (the host vector of the UKF is staged; the buffers are free for the next call)
    h->step = 0;
    h->inited = true;
    TRY(nav_reset(h));
    if (h->shadow) return slam_init_each(h->shadow, pose0 + 3 * (size_t)h->tracked, truth0 ? truth0 + 3 * (size_t)h->tracked : nullptr);
    return SLAM_OK;
}

int slam_set_maps(slam_handle* h, const double* maps, const int32_t* L, int L_stride) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind == SLAM_UKF_LOC) return fail(SLAM_ERR_UNSUPPORTED, "UKF_LOC localises against one known map: slam_set_map");
    if (!maps || !L || L_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    const size_t B = (size_t)h->B;
    int Lmax = 0;
    for (size_t b = 0; b < B; ++b) {
        if (L[b] <= 0 || L[b] > L_stride) return fail(SLAM_ERR_ARG, "instance %zu: %d landmarks, outside [1, L_stride = %d]", b, L[b], L_stride);
        Lmax = L[b] > Lmax ? L[b] : Lmax;
    }
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    const size_t nm = 2 * (size_t)L_stride * B;
    if (h->dmaps.cap() < nm || h->dLs.cap() < B) {   // both new blocks first: a failure leaves the handle with the maps it had
        DevBuf<double> m; DevBuf<int32_t> l;
        HIP_TRY(m.reserve(nm)); HIP_TRY(l.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));     // the launches that read the old ones are done
        h->dmaps = std::move(m); h->dLs = std::move(l);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(hipMemcpyAsync(h->dmaps, maps, sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->dLs, L, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->maps_each = true; h->map_stride = L_stride; h->L = Lmax;
    if (h->kind == SLAM_EKF_SLAM) {   // the shadow of slam_track_instance (EKF handles only) takes its slice
        h->hmaps.assign(maps, maps + nm);
        h->hLs.assign(L, L + B);
    }
    if (h->shadow) return slam_set_maps(h->shadow, maps + (size_t)h->tracked * L_stride * 2, L + h->tracked, L_stride);
    return SLAM_OK;
}

int slam_noise_from_config(const slam_config* cfg, slam_noise* out) {
    if (!cfg || !out) return fail(SLAM_ERR_ARG, "NULL argument");
    slam_host::noise_from_config(*cfg, out);
    return SLAM_OK;
}

int slam_set_noise_each(slam_handle* h, const slam_noise* rows) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    const size_t B = (size_t)h->B;
    std::vector<slam::NoiseRow> packed(rows ? B : 0);
    if (rows) {
        size_t bad = 0; const char* field = nullptr;
        if (slam_host::noise_pack(rows, B, h->cfg.replicate_vw_quirk, packed.data(), &bad, &field))
            return fail(SLAM_ERR_ARG, "instance %zu: noise field %s is not finite", bad, field);
    }
    TRY(flush_lazy(h));   // the timesteps accepted so far keep the values they were accepted with
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    HIP_TRY(hipSetDevice(h->device));
    // the shadow of slam_track_instance first (its row, or back to its config): if that fails, the batch keeps the rows it had
    if (h->shadow) TRY(slam_set_noise_each(h->shadow, rows ? rows + h->tracked : nullptr));
    if (!rows) {
        h->noise_each = false; h->hnoise.clear();   // (the launches in flight keep reading dnoise: it stays allocated)
        return SLAM_OK;
    }
    if (h->dnoise.cap() < B) {   // the new block first: a failure leaves the handle with the rows it had
        DevBuf<slam::NoiseRow> d;
        HIP_TRY(d.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->dnoise = std::move(d);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old rows are done
    }
    for (int i = 0; i < 3; ++i)
        if (h->aux_stream[i]) HIP_TRY(hipStreamSynchronize(h->aux_stream[i]));
    HIP_TRY(hipMemcpyAsync(h->dnoise, packed.data(), sizeof(slam::NoiseRow) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->noise_each = true;
    h->hnoise.assign(rows, rows + B);
    return SLAM_OK;
}

int slam_step_each(slam_handle* h, const float* cmds, const float* meas, const int32_t* count, int k_stride) {
    if (!h || !cmds || !meas || !count || k_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    if (h->shadow) {
        const int t = h->tracked;
        const int rs = slam_step_each(h->shadow, cmds + 2 * (size_t)t, meas + (size_t)t * k_stride * 3, count + t, k_stride);
        if (rs) return rs;
    }
    TRY(flush_lazy(h));   // not queued itself: what is queued runs first
    const size_t B = (size_t)h->B;
    int kmax = 0;
    for (size_t b = 0; b < B; ++b) kmax = count[b] > kmax ? count[b] : kmax;
    kmax = kmax < k_stride ? kmax : k_stride;
    TRY(upload_cmds_each(h, cmds, 1));
    return step_host_now(h, kNoCmd, h->dcmd_each, meas, count, k_stride, kmax);
}

int slam_step_each_dev(slam_handle* h, const float* d_cmds, const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || !d_cmds || !d_meas || !d_count || k_stride <= 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    if (h->shadow) {   // as slam_step_dev: the shadow's step is ordered after the caller's work on the handle's stream, and the other way round
        if (!h->shadow_ev) HIP_TRY(hipEventCreateWithFlags(&h->shadow_ev, hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->shadow_ev, h->stream));
        HIP_TRY(hipStreamWaitEvent(h->shadow->stream, h->shadow_ev, 0));
        const int t = h->tracked;
        const int rs = slam_step_each_dev(h->shadow, d_cmds + 2 * (size_t)t, d_meas + (size_t)t * k_stride * 3, d_count + t, k_stride);
        if (rs) return rs;
        HIP_TRY(hipEventRecord(h->shadow_ev, h->shadow->stream));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->shadow_ev, 0));
    }
    TRY(flush_lazy(h));
    if (h->kind == SLAM_UKF_LOC && !h->dmapf) return fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    return launch_step(h, kNoCmd, 0, d_meas, d_count, k_stride, d_cmds);
}

int slam_run_sim_each(slam_handle* h, const float* cmds, int T) {
    if (!h || !cmds || T < 0) return fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    if (h->shadow && T > 0) {   // the tracked instance's column of the commands
        std::vector<float> mine(2 * (size_t)T);
        for (size_t t = 0; t < (size_t)T; ++t) {
            mine[2 * t] = cmds[(t * h->B + h->tracked) * 2];
            mine[2 * t + 1] = cmds[(t * h->B + h->tracked) * 2 + 1];
        }
        const int rs = slam_run_sim_each(h->shadow, mine.data(), T);
        if (rs) return rs;
    }
    TRY(flush_lazy(h));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    TRY(upload_cmds_each(h, cmds, T));
    return run_sim_now(h, nullptr, T, h->dcmd_each);
}

int slam_predict_each(slam_handle* h, const float* cmds) {
    if (!h || !cmds) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate prediction stage: EKF::update does both (ekf.cpp:37-179); use slam_step_each");
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->predicted) return fail(SLAM_ERR_STATE, "slam_predict called twice without slam_update_dev");
    HIP_TRY(hipSetDevice(h->device));
    TRY(upload_cmds_each(h, cmds, 1));   // read by the update stage; nothing replaces it until then
    slam::UkfStepParams p;
    fill_ukf_params(h, p, kNoCmd, h->dcmd_each);
    HIP_TRY(slam::launch_ukf_sqrt(p, h->stream));
    h->pred_each = true;
    h->predicted = true;
    return SLAM_OK;
}

// ---- closed loop: pure-pursuit commands from each instance's estimate (nav_kernel.hip) ----------------------------------------------------
int slam_nav_config_default(slam_nav_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->dt = 0.05;                                                  // params.yaml:14
    c->lookahead_dist_init = 0.2; c->lookahead_dist_max = 2.0;     // params.yaml:83-84
    c->method = SLAM_NAV_PP; c->control = SLAM_NAV_LOOSE;          // params.yaml:81; sim_base.launch tight_control false
    return SLAM_OK;
}

int slam_nav_config_load(slam_nav_config* c, const char* path) {
    if (!c || !path) return fail(SLAM_ERR_ARG, "NULL argument");
    FILE* f = fopen(path, "r");
    if (!f) return fail(SLAM_ERR_IO, "cannot open %s", path);
    char line[1024];
    double v;
    int rc = SLAM_OK;
    while (rc == SLAM_OK && fgets(line, sizeof(line), f)) {
        const size_t len = strlen(line);
        if (len == sizeof(line) - 1 && line[len - 1] != '\n') {   // over-long line: dropped whole, as config_parse_file does
            int ch;
            while ((ch = fgetc(f)) != EOF && ch != '\n') {}
            continue;
        }
        const bool top = line[0] != ' ' && line[0] != '\t';        // dt is a top-level key; the others are unique leaf names
        if (top && slam_host::parse_scalar(line, "dt", &v)) { if (isfinite(v)) c->dt = v; else rc = fail(SLAM_ERR_IO, "value of dt is not finite"); }
        else if (slam_host::parse_scalar(line, "lookahead_dist_init", &v)) { if (isfinite(v)) c->lookahead_dist_init = v; else rc = fail(SLAM_ERR_IO, "value of lookahead_dist_init is not finite"); }
        else if (slam_host::parse_scalar(line, "lookahead_dist_max", &v)) { if (isfinite(v)) c->lookahead_dist_max = v; else rc = fail(SLAM_ERR_IO, "value of lookahead_dist_max is not finite"); }
        else {
            const char* q = line;
            while (*q == ' ' || *q == '\t') ++q;
            if (strncmp(q, "nav_method:", 11) == 0) {
                char word[32] = "";
                sscanf(q + 11, " %*[\"']%31[A-Za-z_]", word);
                if (!word[0]) sscanf(q + 11, " %31[A-Za-z_]", word);
                if (strcmp(word, "pp") == 0) c->method = SLAM_NAV_PP;
                else if (strcmp(word, "direct") == 0 || strcmp(word, "simple") == 0) c->method = SLAM_NAV_DIRECT;
                else rc = fail(SLAM_ERR_IO, "nav_method \"%s\" is none of pp, direct, simple (goal_pursuit_node.py:45-53)", word);
            }
        }
    }
    fclose(f);
    return rc;
}

}  // extern "C"

namespace {

int nav_check_config(const slam_nav_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "nav config is NULL");
    if (!(c->dt > 0.0) || !isfinite(c->dt)) return fail(SLAM_ERR_ARG, "nav config: dt = %g must be positive and finite", c->dt);
    if (!(c->lookahead_dist_init > 0.0) || !isfinite(c->lookahead_dist_init) || !(c->lookahead_dist_max > 0.0) || !isfinite(c->lookahead_dist_max))
        return fail(SLAM_ERR_ARG, "nav config: lookahead distances %g .. %g must be positive and finite", c->lookahead_dist_init, c->lookahead_dist_max);
    int radii = 0;
    for (double d = c->lookahead_dist_init; d <= c->lookahead_dist_max; d *= 1.25)
        if (++radii > slam::kNavMaxRadii) return fail(SLAM_ERR_ARG, "nav config: more than %d lookahead radii between %g and %g", slam::kNavMaxRadii, c->lookahead_dist_init, c->lookahead_dist_max);
    if (c->method != SLAM_NAV_PP && c->method != SLAM_NAV_DIRECT) return fail(SLAM_ERR_ARG, "nav config: unknown method %d", c->method);
    if (c->control != SLAM_NAV_LOOSE && c->control != SLAM_NAV_TIGHT) return fail(SLAM_ERR_ARG, "nav config: unknown control %d", c->control);
    return SLAM_OK;
}

// one path of P points: finite, 1 <= P <= cap, no two consecutive waypoints equal (choose_lookahead_pt would divide by a = 0)
int nav_check_path(const double* pts, int P, long long inst) {
    if (P < 1 || P > slam::kNavMaxWaypoints) return fail(SLAM_ERR_ARG, "path of %d waypoints (instance %lld): 1 .. %d are supported", P, inst, slam::kNavMaxWaypoints);
    for (int i = 0; i < P; ++i) {
        if (!isfinite(pts[2 * i]) || !isfinite(pts[2 * i + 1])) return fail(SLAM_ERR_ARG, "waypoint %d (instance %lld) is not finite", i, inst);
        if (i > 0 && pts[2 * i] == pts[2 * i - 2] && pts[2 * i + 1] == pts[2 * i - 1])
            return fail(SLAM_ERR_ARG, "waypoints %d and %d (instance %lld) are equal: the reference divides by zero there (pure_pursuit.py:124)", i - 1, i, inst);
    }
    return SLAM_OK;
}

slam::NavConsts nav_consts(const slam_nav_config& c, double d_max, double th_max) {
    slam::NavConsts k;
    k.dt = c.dt; k.la_init = c.lookahead_dist_init; k.la_max = c.lookahead_dist_max; k.d_max = d_max; k.th_max = th_max;
    k.method = c.method; k.control = c.control;
    return k;
}

// the path is on the device: controller state buffers, reset
int nav_install(slam_handle* h, const slam_nav_config* cfg, bool each, int P, int stride) {
    const size_t B = (size_t)h->B;
    HIP_TRY(h->nav.dhead.reserve(B)); HIP_TRY(h->nav.dfinish.reserve(B)); HIP_TRY(h->nav.dinteg.reserve(B)); HIP_TRY(h->nav.derrp.reserve(B));
    h->nav.cfg = *cfg; h->nav.each = each; h->nav.P = P; h->nav.stride = stride; h->nav.set = true;
    TRY(nav_reset(h));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the caller's arrays are free again
    return SLAM_OK;
}

// ---- per-tick runs (slam_nav_run, slam_monitor_run, slam_innovation_run, slam_gate_run): what they share -------------------------------------

// The one place a NavParams is filled from the handle (everything but tick and cmd_log); the commands go to the first row of dcmd_each.
int nav_params(slam_handle* h, slam::NavParams* out) {
    TRY(grow(h, h->dcmd_each, 2 * (size_t)h->B));
    slam::NavParams p;
    memset(&p, 0, sizeof(p));
    p.x = h->dx; p.flags = h->dflags; p.path = h->nav.dpath;
    p.P_each = h->nav.each ? h->nav.dP.get() : nullptr; p.P = h->nav.P; p.path_stride = h->nav.stride;
    p.B = h->B; p.xstride = h->xstride; p.ukf = h->kind != SLAM_EKF_SLAM;
    p.c = nav_consts(h->nav.cfg, h->cfg.d_max, h->cfg.th_max);
    p.head = h->nav.dhead; p.finish_tick = h->nav.dfinish; p.integ = h->nav.dinteg; p.err_prev = h->nav.derrp;
    p.cmd_out = h->dcmd_each;
    *out = p;
    return SLAM_OK;
}

// the next controller tick on the handle's stream
int nav_launch(slam_handle* h, slam::NavParams& p) {
    p.tick = h->nav.tick;
    HIP_TRY(slam::launch_nav_tick(p, h->esz == 4, h->stream));
    h->nav.tick += 1;
    return SLAM_OK;
}

int innovation_supported(const slam_handle* h);

// What a per-tick run `who` checks once its own arguments are in order: the handle, then its state, then the queued timesteps run.
// ekf_known_ids: the run evaluates innovations (innovation_supported).
int run_enter(slam_handle* h, const char* who, bool need_map, bool need_path, bool ekf_known_ids) {
    if (!h) return fail(SLAM_ERR_ARG, "%s: NULL handle", who);
    if (ekf_known_ids) TRY(innovation_supported(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "%s: slam_init has not been called", who);
    if (need_map && !has_map(h)) return fail(SLAM_ERR_STATE, "%s runs the simulator: slam_set_map (or slam_set_maps) has not been called", who);
    if (need_path && !h->nav.set) return fail(SLAM_ERR_STATE, "%s: no path: call slam_nav_set_path or slam_nav_set_paths first", who);
    if (h->shadow) return fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    // (checked before the first launch: a controller tick would overwrite the commands the pending update stage reads)
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
    return flush_lazy(h);
}

// T ticks in chunks of `chunk`.  Per chunk: before(t0, tc) enqueues the uploads of ticks [t0, t0 + tc); tick(t0, t, mark) enqueues the
// launches of tick t0 + t and passes the one launch group whose time is wanted through mark(launch); then the stream is synchronised and
// after(t0, tc) copies the rows of the chunk out.  The device time of every chunk is summed into times.total_ms and, while `timed`, that of
// every marked group into times.part_ms: an event pair per chunk and per tick of a chunk, from the handle's pool.
template <class Before, class Tick, class After>
int run_chunked(slam_handle* h, int T, int chunk, bool timed, RunTimes& times, Before before, Tick tick, After after) {
    while (h->run_ev.size() < 2 + (timed ? 2 * (size_t)chunk : 0)) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        h->run_ev.push_back(e);
    }
    hipEvent_t* const ev = h->run_ev.data();
    times.part_ms = timed ? 0.0 : -1.0; times.total_ms = 0.0;
    for (int t0 = 0; t0 < T; t0 += chunk) {
        const int tc = T - t0 < chunk ? T - t0 : chunk;
        TRY(before(t0, tc));
        HIP_TRY(hipEventRecord(ev[0], h->stream));
        for (int t = 0; t < tc; ++t)
            TRY(tick(t0, t, [&](auto launch) -> int {
                if (timed) HIP_TRY(hipEventRecord(ev[2 + 2 * t], h->stream));
                TRY(launch());
                if (timed) HIP_TRY(hipEventRecord(ev[3 + 2 * t], h->stream));
                return SLAM_OK;
            }));
        HIP_TRY(hipEventRecord(ev[1], h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        times.total_ms += (double)ms;
        for (int t = 0; timed && t < tc; ++t) {
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 + 2 * t], ev[3 + 2 * t]));
            times.part_ms += (double)ms;
        }
        TRY(after(t0, tc));
    }
    return SLAM_OK;
}

// slam_last_*_work; t: the times of that kind of run, NULL with a NULL handle
int last_work(const RunTimes* t, const char* run, double* part_ms, double* total_ms) {
    if (!t) return fail(SLAM_ERR_ARG, "NULL handle");
    if (t->total_ms < 0.0) return fail(SLAM_ERR_STATE, "%s has not run on this handle", run);
    if (part_ms) *part_ms = t->part_ms;
    if (total_ms) *total_ms = t->total_ms;
    return SLAM_OK;
}

// Where the command of a tick comes from: kShared: row t0 + t of the host array cmds [T][2]; kEach: cmds is [T][B][2] on the host, and the
// rows of a chunk are uploaded to dcmd_each before its ticks; kNav: the controller computes them, one launch per tick.
struct TickCmds {
    enum Source { kShared, kEach, kNav } src;
    const float* cmds;
    slam::NavParams np;

    int init(slam_handle* h, Source s, const float* host_cmds) {
        src = s; cmds = host_cmds;
        memset(&np, 0, sizeof(np));
        return src == kNav ? nav_params(h, &np) : SLAM_OK;
    }
    double bytes_per_tick(const slam_handle* h) const { return src == kEach ? 4.0 * 2.0 * (double)h->B : 0.0; }   // on the device
    int upload(slam_handle* h, int t0, int tc) const { return src == kEach ? upload_cmds_each(h, cmds + (size_t)t0 * 2 * h->B, tc) : SLAM_OK; }
    // tick t of the chunk at t0: the shared command and the device row of per-instance commands (NULL: shared) of its step launch
    int select(slam_handle* h, int t0, int t, const float** cmd, const float** d_each) {
        *cmd = kNoCmd; *d_each = h->dcmd_each;
        if (src == kNav) return nav_launch(h, np);
        if (src == kEach) *d_each = h->dcmd_each + (size_t)t * 2 * h->B;
        else { *cmd = cmds + 2 * (size_t)(t0 + t); *d_each = nullptr; }
        return SLAM_OK;
    }
};

}  // namespace

extern "C" {

int slam_nav_set_path(slam_handle* h, const slam_nav_config* cfg, const double* pts, int P) {
    if (!h || !pts) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(nav_check_config(cfg));
    TRY(nav_check_path(pts, P, -1));
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old path are done
    h->nav.set = false;
    HIP_TRY(h->nav.dpath.reserve(2 * (size_t)P));
    HIP_TRY(hipMemcpyAsync(h->nav.dpath, pts, sizeof(double) * 2 * (size_t)P, hipMemcpyHostToDevice, h->stream));
    return nav_install(h, cfg, false, P, 0);
}

int slam_nav_set_paths(slam_handle* h, const slam_nav_config* cfg, const double* pts, const int32_t* P, int P_stride) {
    if (!h || !pts || !P) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(nav_check_config(cfg));
    if (P_stride < 1 || P_stride > slam::kNavMaxWaypoints) return fail(SLAM_ERR_ARG, "P_stride = %d: 1 .. %d are supported", P_stride, slam::kNavMaxWaypoints);
    const size_t B = (size_t)h->B;
    for (size_t b = 0; b < B; ++b) {
        if (P[b] > P_stride) return fail(SLAM_ERR_ARG, "instance %zu: %d waypoints exceed P_stride = %d", b, P[b], P_stride);
        TRY(nav_check_path(pts + b * (size_t)P_stride * 2, P[b], (long long)b));
    }
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->nav.set = false;
    HIP_TRY(h->nav.dpath.reserve(2 * (size_t)P_stride * B)); HIP_TRY(h->nav.dP.reserve(B));
    HIP_TRY(hipMemcpyAsync(h->nav.dpath, pts, sizeof(double) * 2 * (size_t)P_stride * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->nav.dP, P, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    return nav_install(h, cfg, true, 0, P_stride);
}

int slam_nav_run(slam_handle* h, int T, float* cmds_out) {
    if (T < 0) return fail(SLAM_ERR_ARG, "T = %d is negative", T);
    TRY(run_enter(h, "slam_nav_run", true, true, false));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t row = 2 * (size_t)h->B;
    // what a tick holds on the device: its row of the command log
    const int chunk = slam_host::ticks_per_chunk(T, cmds_out ? 4.0 * (double)row : 0.0, slam_host::tick_log_budget());
    if (cmds_out) TRY(grow(h, h->nav.dlog, (size_t)chunk * row));
    slam::NavParams p;
    TRY(nav_params(h, &p));
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->nav.times, [](int, int) { return SLAM_OK; },
        [&](int, int t, auto mark) -> int {
            p.cmd_log = cmds_out ? h->nav.dlog + (size_t)t * row : nullptr;
            TRY(mark([&] { return nav_launch(h, p); }));
            return launch_step(h, kNoCmd, 1, nullptr, nullptr, 0, h->dcmd_each);
        },
        [&](int t0, int tc) -> int {
            if (cmds_out) HIP_TRY(hipMemcpy(cmds_out + (size_t)t0 * row, h->nav.dlog, sizeof(float) * (size_t)tc * row, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
}

int slam_nav_state(slam_handle* h, int32_t* remaining, int32_t* finish_tick, double* integ, double* err_prev) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (!h->nav.set) return fail(SLAM_ERR_STATE, "no path: call slam_nav_set_path or slam_nav_set_paths first");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = (size_t)h->B;
    if (remaining) {
        std::vector<int32_t> Pb(B, h->nav.P);
        HIP_TRY(hipMemcpy(remaining, h->nav.dhead, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
        if (h->nav.each) HIP_TRY(hipMemcpy(Pb.data(), h->nav.dP, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
        for (size_t b = 0; b < B; ++b) remaining[b] = Pb[b] - remaining[b];
    }
    if (finish_tick) HIP_TRY(hipMemcpy(finish_tick, h->nav.dfinish, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (integ) HIP_TRY(hipMemcpy(integ, h->nav.dinteg, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (err_prev) HIP_TRY(hipMemcpy(err_prev, h->nav.derrp, sizeof(double) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_nav_estimates(slam_handle* h, float* est) {
    if (!h || !est) return fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = (size_t)h->B;
    const int w = h->kind == SLAM_EKF_SLAM ? 3 : 4;
    if (h->esz == 4) {   // EKF, fp32 storage: the stored floats are the wire values
        HIP_TRY(hipMemcpy2D(est, sizeof(float) * 3, h->dx, sizeof(float) * h->xstride, sizeof(float) * 3, B, hipMemcpyDeviceToHost));
        return SLAM_OK;
    }
    std::vector<double> head((size_t)w * B);
    HIP_TRY(hipMemcpy2D(head.data(), sizeof(double) * w, h->dx, sizeof(double) * h->xstride, sizeof(double) * w, B, hipMemcpyDeviceToHost));
    for (size_t b = 0; b < B; ++b) {
        const double* x = head.data() + (size_t)w * b;
        est[3 * b] = (float)x[0]; est[3 * b + 1] = (float)x[1];
        est[3 * b + 2] = (float)(w == 3 ? x[2] : remainder(slam::det_atan2(x[3], x[2]), slam::kTwoPi));   // ukf.cpp:71
    }
    return SLAM_OK;
}

int slam_nav_set_timing(slam_handle* h, int per_tick) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    h->nav.time_ticks = per_tick != 0;
    return SLAM_OK;
}

int slam_last_nav_work(slam_handle* h, double* controller_ms, double* total_ms) {
    return last_work(h ? &h->nav.times : nullptr, "slam_nav_run", controller_ms, total_ms);
}

int slam_nav_tick_host(const slam_nav_config* cfg, double d_max, double th_max, const double* pts, int P, const float est[3], int frozen,
                       int tick, int32_t* head, int32_t* finish_tick, double* integ, double* err_prev, float cmd[2]) {
    if (!pts || !est || !head || !finish_tick || !integ || !err_prev || !cmd) return fail(SLAM_ERR_ARG, "NULL argument");
    TRY(nav_check_config(cfg));
    TRY(nav_check_path(pts, P, -1));
    if (*head < 0 || *head > P) return fail(SLAM_ERR_ARG, "head = %d outside [0, P = %d]", *head, P);
    slam::NavState s;
    s.head = *head; s.finish_tick = *finish_tick; s.integ = *integ; s.err_prev = *err_prev;
    slam::nav_tick(nav_consts(*cfg, d_max, th_max), slam::NavPathView{pts}, P, (double)est[0], (double)est[1], (double)est[2], frozen != 0, tick, s, cmd);
    *head = s.head; *finish_tick = s.finish_tick; *integ = s.integ; *err_prev = s.err_prev;
    return SLAM_OK;
}

}  // extern "C"

// ---- run monitor: per-tick error and pose-NEES records (monitor_kernel.hip) ----------------------------------------------------------------
namespace {

// *out = *cfg (NULL: the defaults), checked
int monitor_config(const slam_monitor_config* cfg, slam_monitor_config* out) {
    if (cfg) *out = *cfg; else slam_monitor_config_default(out);
    if (!isfinite(out->nees_lo) || !isfinite(out->nees_hi) || out->nees_lo > out->nees_hi)
        return fail(SLAM_ERR_ARG, "monitor config: the band nees_lo = %g .. nees_hi = %g must be finite and ordered", out->nees_lo, out->nees_hi);
    if (out->full_every < 0) return fail(SLAM_ERR_ARG, "monitor config: full_every = %d is negative", out->full_every);
    return SLAM_OK;
}

int monitor_full_supported(const slam_handle* h, const slam_monitor_config& c) {
    if (c.full_every != 0 && h->kind != SLAM_EKF_SLAM)
        return fail(SLAM_ERR_UNSUPPORTED, "monitor config: full_every = %d needs EKF_SLAM (slam_consistency is not defined for the UKF kinds); full_every = 0 runs", c.full_every);
    return SLAM_OK;
}

slam::MonitorParams monitor_params(slam_handle* h, const slam_monitor_config& c) {
    slam::MonitorParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.status = h->dflags; p.truth = h->dtruth;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.ukf = h->kind != SLAM_EKF_SLAM;
    p.nees_lo = c.nees_lo; p.nees_hi = c.nees_hi;
    p.partials = h->mon.dpart;
    return p;
}

// one evaluation on the handle's stream; full: launch_consistency first, into the handle's buffers, its results into entries 13 - 15
int monitor_launch(slam_handle* h, slam::MonitorParams& p, bool full) {
    p.nees_full = nullptr; p.dof = nullptr;
    if (full) {
        slam::ConsistencyParams cp;
        int chunk = 0;
        TRY(consistency_params(h, &cp, &chunk));
        HIP_TRY(slam::launch_consistency(cp, h->esz == 4, chunk, h->stream));
        p.nees_full = cp.nees_full; p.dof = cp.dof;
    }
    p.P = h->dP;   // (the UKF step swaps its two buffers)
    HIP_TRY(slam::launch_monitor(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_monitor_config_default(slam_monitor_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->nees_lo = 0.21579528262389785; c->nees_hi = 9.348403604496148;   // chi-square quantiles at 0.025 and 0.975, 3 degrees of freedom
    c->full_every = 0;
    return SLAM_OK;
}

int slam_monitor_now(slam_handle* h, const slam_monitor_config* cfg, double rec[16], double* err_pos, double* err_yaw, double* nees_pose, int32_t* flags) {
    slam_monitor_config c;
    TRY(monitor_config(cfg, &c));
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(monitor_full_supported(h, c));
    TRY(flush_lazy(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return fail(SLAM_ERR_STATE, "no true map, so no simulated truth to compare with: call slam_set_map (or slam_set_maps) first");
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->mon.dpart, (size_t)slam::monitor_blocks(h->B) * slam::kMonRecLen));
    TRY(grow(h, h->mon.drec, slam::kMonRecLen));
    TRY(grow(h, h->mon.dlog, 3 * B));
    TRY(grow(h, h->mon.dflags, B));
    slam::MonitorParams p = monitor_params(h, c);
    p.err_pos = h->mon.dlog; p.err_yaw = h->mon.dlog + B; p.nees_pose = h->mon.dlog + 2 * B; p.flags = h->mon.dflags;
    p.rec = h->mon.drec;
    TRY(monitor_launch(h, p, c.full_every != 0));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (rec) HIP_TRY(hipMemcpy(rec, h->mon.drec, sizeof(double) * slam::kMonRecLen, hipMemcpyDeviceToHost));
    if (err_pos) HIP_TRY(hipMemcpy(err_pos, p.err_pos, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (err_yaw) HIP_TRY(hipMemcpy(err_yaw, p.err_yaw, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (nees_pose) HIP_TRY(hipMemcpy(nees_pose, p.nees_pose, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, h->mon.dflags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_monitor_run(slam_handle* h, const slam_monitor_config* cfg, int source, const float* cmds, int T, double* recs, double* err_pos,
                     double* err_yaw, double* nees_pose) {
    slam_monitor_config c;
    TRY(monitor_config(cfg, &c));
    if (source != SLAM_MONITOR_SHARED && source != SLAM_MONITOR_EACH && source != SLAM_MONITOR_NAV) return fail(SLAM_ERR_ARG, "unknown command source %d", source);
    if (T < 0) return fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (source != SLAM_MONITOR_NAV && !cmds) return fail(SLAM_ERR_ARG, "cmds is NULL: the sources SHARED and EACH read the commands from it");
    if (h) TRY(monitor_full_supported(h, c));
    TRY(run_enter(h, "slam_monitor_run", true, source == SLAM_MONITOR_NAV, false));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    double* const series[3] = {err_pos, err_yaw, nees_pose};
    int ns = 0;
    for (double* s : series) ns += s != nullptr;
    TickCmds tcmd;
    TRY(tcmd.init(h, source == SLAM_MONITOR_EACH ? TickCmds::kEach : source == SLAM_MONITOR_NAV ? TickCmds::kNav : TickCmds::kShared, cmds));
    // what a tick holds on the device: its rows of the series and, for EACH, of the commands
    const int chunk = slam_host::ticks_per_chunk(T, 8.0 * (double)ns * (double)B + tcmd.bytes_per_tick(h), slam_host::tick_log_budget());
    TRY(grow(h, h->mon.dpart, (size_t)slam::monitor_blocks(h->B) * slam::kMonRecLen));
    TRY(grow(h, h->mon.drec, (size_t)chunk * slam::kMonRecLen));
    if (ns) TRY(grow(h, h->mon.dlog, (size_t)ns * chunk * B));
    slam::MonitorParams p = monitor_params(h, c);
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->mon.times, [&](int t0, int tc) { return tcmd.upload(h, t0, tc); },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(launch_step(h, cmd, 1, nullptr, nullptr, 0, d_each));
            double* slot = h->mon.dlog;
            p.err_pos = err_pos ? slot + (size_t)t * B : nullptr; if (err_pos) slot += (size_t)chunk * B;
            p.err_yaw = err_yaw ? slot + (size_t)t * B : nullptr; if (err_yaw) slot += (size_t)chunk * B;
            p.nees_pose = nees_pose ? slot + (size_t)t * B : nullptr;
            p.rec = h->mon.drec + (size_t)t * slam::kMonRecLen;
            return mark([&] { return monitor_launch(h, p, c.full_every > 0 && (t0 + t + 1) % c.full_every == 0); });
        },
        [&](int t0, int tc) -> int {
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kMonRecLen, h->mon.drec, sizeof(double) * (size_t)tc * slam::kMonRecLen, hipMemcpyDeviceToHost));
            const double* slot = h->mon.dlog;
            for (double* s : series)
                if (s) {
                    HIP_TRY(hipMemcpy(s + (size_t)t0 * B, slot, sizeof(double) * (size_t)tc * B, hipMemcpyDeviceToHost));
                    slot += (size_t)chunk * B;
                }
            return SLAM_OK;
        });
}

int slam_last_monitor_work(slam_handle* h, double* monitor_ms, double* total_ms) {
    return last_work(h ? &h->mon.times : nullptr, "slam_monitor_run", monitor_ms, total_ms);
}

int slam_monitor_instance_host(int filter_kind, const double* x, const double* P3, const double truth[3], int32_t status, double* err_pos,
                               double* err_yaw, double* nees_pose, int32_t* flags) {
    if (filter_kind != SLAM_EKF_SLAM && filter_kind != SLAM_UKF_SLAM && filter_kind != SLAM_UKF_LOC) return fail(SLAM_ERR_ARG, "unknown filter kind %d", filter_kind);
    const bool ukf = filter_kind != SLAM_EKF_SLAM;
    if (!x || !truth || (!ukf && !P3)) return fail(SLAM_ERR_ARG, "NULL argument");
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const slam::MonitorValue v = slam::monitor_instance(x, ukf ? zero : P3, truth, status, ukf);
    if (err_pos) *err_pos = v.err_pos;
    if (err_yaw) *err_yaw = v.err_yaw;
    if (nees_pose) *nees_pose = v.nees_pose;
    if (flags) *flags = v.flags;
    return SLAM_OK;
}

}  // extern "C"

// ---- innovation (NIS) statistics of the message the next step will process (innovation_kernel.hip) ----------------------------------------
namespace {

// *out = *cfg (NULL: the defaults), checked
int innovation_config(const slam_innovation_config* cfg, slam_innovation_config* out) {
    if (cfg) *out = *cfg; else slam_innovation_config_default(out);
    if (!isfinite(out->nis_lo) || !isfinite(out->nis_hi) || out->nis_lo > out->nis_hi)
        return fail(SLAM_ERR_ARG, "innovation config: the band nis_lo = %g .. nis_hi = %g must be finite and ordered", out->nis_lo, out->nis_hi);
    return SLAM_OK;
}

int innovation_supported(const slam_handle* h) {
    if (h->kind != SLAM_EKF_SLAM)
        return fail(SLAM_ERR_UNSUPPORTED, "innovation statistics need EKF_SLAM: the innovation covariance of the UKF kinds depends on all sigma points, so no block of P closes");
    if (!h->cfg.landmark_id_is_known)
        return fail(SLAM_ERR_UNSUPPORTED, "innovation statistics need landmark_id_is_known = 1: the association of unknown ids reads every landmark of x_pred after every update");
    return SLAM_OK;
}

// the per-instance buffers of one evaluation; det: the detection slots are wanted
int innovation_reserve(slam_handle* h, bool det) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->inn.dval, (1 + 12 + slam::kInnovRecLen) * B));
    TRY(grow(h, h->inn.dpart, (size_t)slam::innovation_blocks(h->B) * slam::kInnovRecLen));
    if (det) TRY(grow(h, h->inn.ddet, B * slam::kInnovMaxDet * slam::kInnovDetLen));
    return SLAM_OK;
}

// the launch parameters of one evaluation of the step launch_step(h, cmd, sim, d_meas, d_count, k_stride, d_cmd_each) would run now
slam::InnovParams innovation_params(slam_handle* h, const slam_innovation_config& c, const float cmd[2], int sim, const float* d_meas,
                                    const int32_t* d_count, int k_stride, const float* d_cmd_each) {
    slam::InnovParams p;
    memset(&p, 0, sizeof(p));
    fill_ekf_params(h, p.s, cmd, sim, 0, d_meas, d_count, k_stride, nullptr, 0, d_cmd_each);
    const size_t B = (size_t)h->B;
    p.nis_lo = c.nis_lo; p.nis_hi = c.nis_hi;
    p.inst_rec = h->inn.dval + 13 * B;
    p.partials = h->inn.dpart;
    return p;
}

// The outputs of one evaluation (slam_innovation*, slam_gate*): on the device they have fixed places in the handle's buffers.
struct InnovOut { double *rec, *nis_sum, *post, *det; int32_t *n_upd, *flags, *n_new; };

int innovation_outputs(slam_handle* h, bool det, InnovOut* d) {
    const size_t B = (size_t)h->B;
    TRY(innovation_reserve(h, det));
    TRY(grow(h, h->inn.drec, slam::kInnovRecLen));
    TRY(grow(h, h->inn.dint, 3 * B));
    *d = {h->inn.drec, h->inn.dval, h->inn.dval + B, det ? h->inn.ddet.get() : nullptr, h->inn.dint, h->inn.dint + B, h->inn.dint + 2 * B};
    return SLAM_OK;
}

// once the stream has run dry: the outputs the caller wants (non-NULL in `to`) from their device places
int innovation_download(slam_handle* h, const InnovOut& d, const InnovOut& to) {
    const size_t B = (size_t)h->B;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (to.rec) HIP_TRY(hipMemcpy(to.rec, d.rec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (to.nis_sum) HIP_TRY(hipMemcpy(to.nis_sum, d.nis_sum, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (to.post) HIP_TRY(hipMemcpy(to.post, d.post, sizeof(double) * 12 * B, hipMemcpyDeviceToHost));
    if (to.det) HIP_TRY(hipMemcpy(to.det, d.det, sizeof(double) * B * slam::kInnovMaxDet * slam::kInnovDetLen, hipMemcpyDeviceToHost));
    if (to.n_upd) HIP_TRY(hipMemcpy(to.n_upd, d.n_upd, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.flags) HIP_TRY(hipMemcpy(to.flags, d.flags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_new) HIP_TRY(hipMemcpy(to.n_new, d.n_new, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// slam_innovation / slam_innovation_dev once the message and the commands are on the device
int innovation_now(slam_handle* h, const slam_innovation_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                   const int32_t* d_count, int k_stride, const InnovOut& to) {
    InnovOut d;
    TRY(innovation_outputs(h, to.det != nullptr, &d));
    slam::InnovParams p = innovation_params(h, c, cmd, 0, d_meas, d_count, k_stride, d_cmd_each);
    p.nis_sum = d.nis_sum; p.post = d.post; p.n_upd = d.n_upd; p.flags = d.flags; p.n_new = d.n_new; p.det = d.det; p.rec = d.rec;
    HIP_TRY(slam::launch_innovation(p, h->esz == 4, h->stream));
    return innovation_download(h, d, to);
}

// the checks slam_innovation and slam_innovation_dev share; the queued timesteps run first
int innovation_enter(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride,
                     slam_innovation_config* c) {
    TRY(innovation_config(cfg, c));
    if (!cmds) return fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

// n floats from the host into the handle's staging buffer for per-instance commands, in stream order
int innovation_upload_cmds(slam_handle* h, const float* cmds, size_t n) {
    TRY(grow(h, h->inn.dcmd, n));
    HIP_TRY(hipMemcpyAsync(h->inn.dcmd, cmds, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

// the host messages of `ticks` ticks into the handle's staging buffers ([ticks][B][k_stride][3] and [ticks][B]), in stream order
int upload_messages(slam_handle* h, const float* meas, const int32_t* count, int k_stride, size_t ticks) {
    const size_t nc = ticks * h->B, nm = 3 * (size_t)k_stride * nc;
    TRY(grow(h, h->inn.dmeas, nm));
    TRY(grow(h, h->inn.dcount, nc));
    HIP_TRY(hipMemcpyAsync(h->inn.dmeas, meas, sizeof(float) * nm, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->inn.dcount, count, sizeof(int32_t) * nc, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_innovation_config_default(slam_innovation_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->nis_lo = -2.0 * log(0.975); c->nis_hi = -2.0 * log(0.025);   // chi-square quantiles at 0.025 and 0.975, 2 degrees of freedom
    return SLAM_OK;
}

int slam_innovation(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                    int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post) {
    slam_innovation_config c;
    TRY(innovation_enter(h, cfg, cmds, meas, count, k_stride, &c));
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * (size_t)h->B));
    return innovation_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride,
                          {rec, nis_sum, post, det, n_upd, flags, n_new});
}

int slam_innovation_dev(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                        const int32_t* d_count, int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                        double* det, double* post) {
    slam_innovation_config c;
    TRY(innovation_enter(h, cfg, cmds, d_meas, d_count, k_stride, &c));
    return innovation_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride,
                          {rec, nis_sum, post, det, n_upd, flags, n_new});
}

int slam_innovation_run(slam_handle* h, const slam_innovation_config* cfg, int source, const float* cmds, const float* meas, const int32_t* count,
                        int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* flags) {
    slam_innovation_config c;
    TRY(innovation_config(cfg, &c));
    if (source != SLAM_INNOVATION_SHARED && source != SLAM_INNOVATION_EACH && source != SLAM_INNOVATION_NAV && source != SLAM_INNOVATION_LOG)
        return fail(SLAM_ERR_ARG, "unknown source %d", source);
    if (T < 0) return fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (source != SLAM_INNOVATION_NAV && !cmds) return fail(SLAM_ERR_ARG, "cmds is NULL: the sources SHARED, EACH and LOG read the commands from it");
    const bool log = source == SLAM_INNOVATION_LOG;
    if (log && (!meas || !count)) return fail(SLAM_ERR_ARG, "meas or meas_count is NULL: the source LOG reads the messages from them");
    if (log && k_stride <= 0) return fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TRY(run_enter(h, "slam_innovation_run", !log, source == SLAM_INNOVATION_NAV, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B, mrow = 3 * (size_t)k_stride * B;
    TickCmds tcmd;   // (LOG: the commands are shared ones)
    TRY(tcmd.init(h, source == SLAM_INNOVATION_EACH ? TickCmds::kEach : source == SLAM_INNOVATION_NAV ? TickCmds::kNav : TickCmds::kShared, cmds));
    // what a tick holds on the device: its rows of the series, of the commands (EACH) and of the messages (LOG)
    const double per_tick = 8.0 * (nis_sum ? (double)B : 0.0) + 4.0 * (double)B * ((n_upd ? 1 : 0) + (flags ? 1 : 0)) + tcmd.bytes_per_tick(h) +
                            (log ? 4.0 * (double)mrow + 4.0 * (double)B : 0.0);
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, (size_t)chunk * slam::kInnovRecLen));
    if (nis_sum) TRY(grow(h, h->inn.dlog, (size_t)chunk * B));
    TRY(grow(h, h->inn.dint, 2 * (size_t)chunk * B));
    int32_t* const d_upd = h->inn.dint;
    int32_t* const d_flags = h->inn.dint + (size_t)chunk * B;
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->inn.times,
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            return log ? upload_messages(h, meas + (size_t)t0 * mrow, count + (size_t)t0 * B, k_stride, (size_t)tc) : SLAM_OK;
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            const float* const d_meas = log ? h->inn.dmeas + (size_t)t * mrow : nullptr;
            const int32_t* const d_count = log ? h->inn.dcount + (size_t)t * B : nullptr;
            slam::InnovParams p = innovation_params(h, c, cmd, log ? 0 : 1, d_meas, d_count, log ? k_stride : 0, d_each);
            p.nis_sum = nis_sum ? h->inn.dlog + (size_t)t * B : nullptr;
            p.n_upd = n_upd ? d_upd + (size_t)t * B : nullptr;
            p.flags = flags ? d_flags + (size_t)t * B : nullptr;
            p.rec = h->inn.drec + (size_t)t * slam::kInnovRecLen;
            TRY(mark([&]() -> int { HIP_TRY(slam::launch_innovation(p, h->esz == 4, h->stream)); return SLAM_OK; }));
            return launch_step(h, cmd, log ? 0 : 1, d_meas, d_count, log ? k_stride : 0, d_each);
        },
        [&](int t0, int tc) -> int {
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kInnovRecLen, h->inn.drec, sizeof(double) * (size_t)tc * slam::kInnovRecLen, hipMemcpyDeviceToHost));
            if (nis_sum) HIP_TRY(hipMemcpy(nis_sum + (size_t)t0 * B, h->inn.dlog, sizeof(double) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (n_upd) HIP_TRY(hipMemcpy(n_upd + (size_t)t0 * B, d_upd, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (flags) HIP_TRY(hipMemcpy(flags + (size_t)t0 * B, d_flags, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
}

int slam_last_innovation_work(slam_handle* h, double* innovation_ms, double* total_ms) {
    return last_work(h ? &h->inn.times : nullptr, "slam_innovation_run", innovation_ms, total_ms);
}

int slam_innovation_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                  const float* meas, int k, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                  const slam_innovation_config* cfg, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new,
                                  int32_t* flags, double* det, double* post) {
    slam_innovation_config c;
    TRY(innovation_config(cfg, &c));
    if (!x || !P || !cmd || !noise) return fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return fail(SLAM_ERR_ARG, "ids is NULL");
    if (k < 0 || (k > 0 && !meas)) return fail(SLAM_ERR_ARG, "k = %d is negative, or meas is NULL", k);
    if (const char* f = slam_host::noise_bad_field(*noise)) return fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
    const slam::InnovNoise nz = {noise->v_d, noise->v_th, noise->w_r, noise->w_b, noise->V_00, noise->V_11, noise->W_00, noise->W_11};
    const int n = 3 + 2 * M;
    std::vector<slam::InnovWork> ws(1);
    for (int i = 0; i < 3 * (k < slam::kInnovMaxDet ? k : slam::kInnovMaxDet); ++i) ws[0].meas[i] = meas[i];
    const bool f32 = f32_storage != 0;
    const slam::InnovResult v = slam::innovation_instance(
        slam::InnovSeq(), ws[0], [&](int i) { return f32 ? (double)(float)x[i] : x[i]; },
        [&](int r, int cc) { const double e = P[(size_t)r * n + cc]; return f32 ? (double)(float)e : e; }, ids, M, L_max, status, cmd[0], cmd[1], k, nz,
        lm_from_pred != 0, c.nis_lo, c.nis_hi, det);
    if (rec) slam::innovation_record(v, rec);
    if (nis_sum) *nis_sum = v.nis_sum;
    if (n_upd) *n_upd = v.n_upd;
    if (n_new) *n_new = v.n_new;
    if (flags) *flags = v.flags;
    if (post) memcpy(post, v.post, sizeof(v.post));
    return SLAM_OK;
}

}  // extern "C"

// ---- innovation gating: the chi-square gate on the message the next step will process (gate_kernel.hip) -----------------------------------
namespace {

// *out = *cfg (NULL: the defaults), checked
int gate_config(const slam_gate_config* cfg, slam_gate_config* out) {
    if (cfg) *out = *cfg; else slam_gate_config_default(out);
    if (!(out->gate > 0.0)) return fail(SLAM_ERR_ARG, "gate config: gate = %g must be positive (+inf: nothing is rejected)", out->gate);
    if (!isfinite(out->nis_lo) || !isfinite(out->nis_hi) || out->nis_lo > out->nis_hi)
        return fail(SLAM_ERR_ARG, "gate config: the band nis_lo = %g .. nis_hi = %g must be finite and ordered", out->nis_lo, out->nis_hi);
    return SLAM_OK;
}

bool gate_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* const pa = (const char*)a; const char* const pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

// the checks every gate entry point shares, in the order of slam_innovation: arguments, then the handle; the queued timesteps run first
int gate_enter(slam_handle* h, const slam_gate_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride,
               const float* meas_out, const int32_t* count_out, bool need_out, slam_gate_config* c) {
    TRY(gate_config(cfg, c));
    if (!cmds) return fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (need_out && (!meas_out || !count_out)) return fail(SLAM_ERR_ARG, "d_meas_out or d_count_out is NULL");
    if ((meas_out == meas) != (count_out == count))
        return fail(SLAM_ERR_ARG, "in place means both: meas_out == meas and count_out == meas_count, or neither");
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

// the gate launches of one message on the handle's stream; the per-instance outputs may be NULL
int gate_launch(slam_handle* h, const slam_gate_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                const int32_t* d_count, int k_stride, float* d_meas_out, int32_t* d_count_out, double* d_rec, double* d_nis_sum, double* d_post,
                double* d_det, int32_t* d_n_upd, int32_t* d_flags, int32_t* d_n_new, int32_t* d_n_rej, int32_t* d_verdict) {
    const slam_innovation_config band = {c.nis_lo, c.nis_hi};
    slam::GateParams p;
    memset(&p, 0, sizeof(p));
    p.in = innovation_params(h, band, cmd, 0, d_meas, d_count, k_stride, d_cmd_each);
    p.in.nis_sum = d_nis_sum; p.in.post = d_post; p.in.det = d_det; p.in.n_upd = d_n_upd; p.in.flags = d_flags; p.in.n_new = d_n_new;
    p.in.rec = d_rec;
    p.gate = c.gate; p.meas_out = d_meas_out; p.count_out = d_count_out; p.n_rej = d_n_rej; p.verdict = d_verdict;
    HIP_TRY(slam::launch_gate(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

// slam_gate / slam_gate_dev once the message and the commands are on the device; d_meas_out / d_count_out: where the filtered message goes
int gate_now(slam_handle* h, const slam_gate_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
             int k_stride, float* d_meas_out, int32_t* d_count_out, const InnovOut& to, int32_t* n_rej, int32_t* verdict) {
    const size_t B = (size_t)h->B;
    InnovOut d;
    TRY(innovation_outputs(h, to.det != nullptr, &d));
    TRY(grow(h, h->gate.drej, B));
    if (verdict) TRY(grow(h, h->gate.dverdict, B * slam::kInnovMaxDet));
    TRY(gate_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out, d.rec, d.nis_sum, d.post, d.det, d.n_upd, d.flags,
                    d.n_new, h->gate.drej, verdict ? h->gate.dverdict.get() : nullptr));
    TRY(innovation_download(h, d, to));
    if (n_rej) HIP_TRY(hipMemcpy(n_rej, h->gate.drej, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (verdict) HIP_TRY(hipMemcpy(verdict, h->gate.dverdict, sizeof(int32_t) * B * slam::kInnovMaxDet, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// the filtered message of one tick, the records of `ticks` ticks and the per-instance contributions
int gate_reserve_step(slam_handle* h, int k_stride, size_t ticks) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->gate.dmeas, 3 * (size_t)k_stride * B));
    TRY(grow(h, h->gate.dcount, B));
    TRY(grow(h, h->gate.drej, ticks * B));
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, ticks * slam::kInnovRecLen));
    return SLAM_OK;
}

int gate_step_state(const slam_handle* h, const char* who) {
    if (h->shadow) return fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    if (h->predicted) return fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
    return SLAM_OK;
}

// one gated timestep once the message and the commands are on the device
int step_gated_now(slam_handle* h, const slam_gate_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                   const int32_t* d_count, int k_stride, double* rec, int32_t* n_rej) {
    const size_t B = (size_t)h->B;
    TRY(gate_reserve_step(h, k_stride, 1));
    TRY(gate_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, h->gate.dmeas, h->gate.dcount, h->inn.drec, nullptr, nullptr, nullptr, nullptr,
                    nullptr, nullptr, h->gate.drej, nullptr));
    TRY(launch_step(h, cmd, 0, h->gate.dmeas, h->gate.dcount, k_stride, d_cmd_each));
    if (!rec && !n_rej) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (rec) HIP_TRY(hipMemcpy(rec, h->inn.drec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (n_rej) HIP_TRY(hipMemcpy(n_rej, h->gate.drej, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int step_gated_host(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                    int k_stride, double* rec, int32_t* n_rej) {
    slam_gate_config c;
    TRY(gate_enter(h, cfg, cmds, meas, count, k_stride, nullptr, nullptr, false, &c));
    TRY(gate_step_state(h, "a gated step"));
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * (size_t)h->B));
    return step_gated_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, rec, n_rej);
}

int step_gated_dev(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                   int k_stride, double* rec, int32_t* n_rej) {
    slam_gate_config c;
    TRY(gate_enter(h, cfg, cmds, d_meas, d_count, k_stride, nullptr, nullptr, false, &c));
    TRY(gate_step_state(h, "a gated step"));
    return step_gated_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, rec, n_rej);
}

}  // namespace

extern "C" {

int slam_gate_config_default(slam_gate_config* c) {
    if (!c) return fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->gate = -2.0 * log(0.001);   // the 0.999 quantile of chi-square with 2 degrees of freedom
    c->nis_lo = -2.0 * log(0.975); c->nis_hi = -2.0 * log(0.025);
    return SLAM_OK;
}

int slam_gate(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count, int k_stride,
              double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post, float* meas_out,
              int32_t* count_out, int32_t* n_rej, int32_t* verdict) {
    slam_gate_config c;
    TRY(gate_enter(h, cfg, cmds, meas, count, k_stride, meas_out, count_out, false, &c));
    const size_t B = (size_t)h->B, nm = 3 * (size_t)k_stride * B;
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * B));
    TRY(grow(h, h->gate.dmeas, nm));
    TRY(grow(h, h->gate.dcount, B));
    // (slots the kernel does not write keep what the caller gave: the output row starts as the input row)
    HIP_TRY(hipMemcpyAsync(h->gate.dmeas, h->inn.dmeas, sizeof(float) * nm, hipMemcpyDeviceToDevice, h->stream));
    TRY(gate_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, h->gate.dmeas,
                 h->gate.dcount, {rec, nis_sum, post, det, n_upd, flags, n_new}, n_rej, verdict));
    if (meas_out) HIP_TRY(hipMemcpy(meas_out, h->gate.dmeas, sizeof(float) * nm, hipMemcpyDeviceToHost));
    if (count_out) HIP_TRY(hipMemcpy(count_out, h->gate.dcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_gate_dev(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                  int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post,
                  float* d_meas_out, int32_t* d_count_out, int32_t* n_rej, int32_t* verdict) {
    slam_gate_config c;
    TRY(gate_enter(h, cfg, cmds, d_meas, d_count, k_stride, d_meas_out, d_count_out, true, &c));
    const size_t B = (size_t)h->B, bm = sizeof(float) * 3 * (size_t)k_stride * B, bc = sizeof(int32_t) * B;
    if ((d_meas_out != d_meas && gate_overlap(d_meas_out, bm, d_meas, bm)) || (d_count_out != d_count && gate_overlap(d_count_out, bc, d_count, bc)) ||
        gate_overlap(d_meas_out, bm, d_count, bc) || gate_overlap(d_count_out, bc, d_meas, bm) || gate_overlap(d_meas_out, bm, d_count_out, bc))
        return fail(SLAM_ERR_ARG, "the output message overlaps the input (only d_meas_out == d_meas with d_count_out == d_count is allowed) or itself");
    return gate_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, d_meas_out, d_count_out,
                    {rec, nis_sum, post, det, n_upd, flags, n_new}, n_rej, verdict);
}

int slam_step_gated(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* meas, const int32_t* count, int k_stride,
                    double rec[16], int32_t* n_rej) {
    return step_gated_host(h, cfg, cmd, 0, meas, count, k_stride, rec, n_rej);
}

int slam_step_gated_dev(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* d_meas, const int32_t* d_count, int k_stride,
                        double rec[16], int32_t* n_rej) {
    return step_gated_dev(h, cfg, cmd, 0, d_meas, d_count, k_stride, rec, n_rej);
}

int slam_step_gated_each(slam_handle* h, const slam_gate_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride,
                         double rec[16], int32_t* n_rej) {
    return step_gated_host(h, cfg, cmds, 1, meas, count, k_stride, rec, n_rej);
}

int slam_step_gated_each_dev(slam_handle* h, const slam_gate_config* cfg, const float* d_cmds, const float* d_meas, const int32_t* d_count,
                             int k_stride, double rec[16], int32_t* n_rej) {
    return step_gated_dev(h, cfg, d_cmds, 1, d_meas, d_count, k_stride, rec, n_rej);
}

int slam_gate_run(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                  int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags) {
    slam_gate_config c;
    TRY(gate_config(cfg, &c));
    if (T < 0) return fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (!cmds) return fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TRY(run_enter(h, "slam_gate_run", false, false, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B, mrow = 3 * (size_t)k_stride * B;
    TickCmds tcmd;
    TRY(tcmd.init(h, cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds));
    // what a tick holds on the device: its rows of the series, of the commands (cmd_each) and of the messages
    const double per_tick = 8.0 * (nis_sum ? (double)B : 0.0) + 4.0 * (double)B * ((n_upd ? 1 : 0) + (flags ? 1 : 0) + (n_rej ? 1 : 0)) +
                            tcmd.bytes_per_tick(h) + 4.0 * (double)mrow + 4.0 * (double)B;
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(gate_reserve_step(h, k_stride, (size_t)chunk));
    if (nis_sum) TRY(grow(h, h->inn.dlog, (size_t)chunk * B));
    TRY(grow(h, h->inn.dint, 2 * (size_t)chunk * B));
    int32_t* const d_upd = h->inn.dint;
    int32_t* const d_flags = h->inn.dint + (size_t)chunk * B;
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->gate.times,
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            return upload_messages(h, meas + (size_t)t0 * mrow, count + (size_t)t0 * B, k_stride, (size_t)tc);
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(mark([&] {
                return gate_launch(h, c, cmd, d_each, h->inn.dmeas + (size_t)t * mrow, h->inn.dcount + (size_t)t * B, k_stride, h->gate.dmeas,
                                   h->gate.dcount, h->inn.drec + (size_t)t * slam::kInnovRecLen, nis_sum ? h->inn.dlog + (size_t)t * B : nullptr,
                                   nullptr, nullptr, n_upd ? d_upd + (size_t)t * B : nullptr, flags ? d_flags + (size_t)t * B : nullptr, nullptr,
                                   h->gate.drej + (size_t)t * B, nullptr);
            }));
            return launch_step(h, cmd, 0, h->gate.dmeas, h->gate.dcount, k_stride, d_each);
        },
        [&](int t0, int tc) -> int {
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kInnovRecLen, h->inn.drec, sizeof(double) * (size_t)tc * slam::kInnovRecLen, hipMemcpyDeviceToHost));
            if (nis_sum) HIP_TRY(hipMemcpy(nis_sum + (size_t)t0 * B, h->inn.dlog, sizeof(double) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (n_upd) HIP_TRY(hipMemcpy(n_upd + (size_t)t0 * B, d_upd, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (flags) HIP_TRY(hipMemcpy(flags + (size_t)t0 * B, d_flags, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (n_rej) HIP_TRY(hipMemcpy(n_rej + (size_t)t0 * B, h->gate.drej, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
}

int slam_last_gate_work(slam_handle* h, double* gate_ms, double* total_ms) {
    return last_work(h ? &h->gate.times : nullptr, "slam_gate_run", gate_ms, total_ms);
}

int slam_gate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                            const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                            const slam_gate_config* cfg, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                            double* det, double* post, float* meas_out, int32_t* count_out, int32_t* n_rej, int32_t* verdict) {
    slam_gate_config c;
    TRY(gate_config(cfg, &c));
    if (!x || !P || !cmd || !noise) return fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return fail(SLAM_ERR_ARG, "ids is NULL");
    if (k_stride <= 0) return fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (count > 0 && !meas) return fail(SLAM_ERR_ARG, "meas is NULL");
    if (const char* f = slam_host::noise_bad_field(*noise)) return fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
    const slam::InnovNoise nz = {noise->v_d, noise->v_th, noise->w_r, noise->w_b, noise->V_00, noise->V_11, noise->W_00, noise->W_11};
    const int n = 3 + 2 * M;
    std::vector<slam::InnovWork> ws(1);
    const bool f32 = f32_storage != 0;
    int32_t rej = 0;
    const slam::InnovResult v = slam::gate_instance_host(
        ws[0], [&](int i) { return f32 ? (double)(float)x[i] : x[i]; },
        [&](int r, int cc) { const double e = P[(size_t)r * n + cc]; return f32 ? (double)(float)e : e; }, ids, M, L_max, status, cmd[0], cmd[1], meas,
        count, k_stride, nz, lm_from_pred != 0, c.nis_lo, c.nis_hi, c.gate, det, meas_out, count_out, &rej, verdict);
    if (rec) slam::gate_record(v, rej, rec);
    if (nis_sum) *nis_sum = v.nis_sum;
    if (n_upd) *n_upd = v.n_upd;
    if (n_new) *n_new = v.n_new;
    if (flags) *flags = v.flags;
    if (post) memcpy(post, v.post, sizeof(v.post));
    if (n_rej) *n_rej = rej;
    return SLAM_OK;
}

}  // extern "C"
