// capi_step.cpp — C ABI: the timesteps.  How a step launch is parameterised, the EKF step queue and its flush, and every entry point that
// advances the filters by itself (slam_step*, slam_run_sim*, slam_predict* / slam_update_dev).
#include <stdlib.h>
#include <string.h>

#include <thread>
#include <type_traits>
#include <utility>
#include <vector>

#include "slam_handle.h"
#include "ekf_kernel.h"
#include "ukf_kernel.h"

namespace slam_capi {

namespace {

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

// What a step launch of either filter kind takes from the handle in the same way: the state other than P and x, the command, the noise
// (with the V/W quirk) and the simulator's, the limits, vision, seed / instance offset / step, sizes and strides, the histogram.
template <class Params>
void set_common_params(const slam_handle* h, Params& p, const float cmd[2]) {
    p.M = h->dM; p.ids = h->dids; p.flags = h->dflags; p.timestep = h->dts;
    p.truth = h->dtruth; p.err_sum = h->derr; p.map = h->dmap; p.L = h->L;
    p.fwd = cmd[0]; p.ang = cmd[1];
    const slam_config& c = h->cfg;
    p.v_d = c.v_d; p.v_th = c.v_th; p.w_r = c.w_r; p.w_b = c.w_b;
    if (c.replicate_vw_quirk) {  // filter.h:116-117: W_00/W_11 land in V, W stays I2
        p.V00 = c.W_00; p.V11 = c.W_11; p.W00 = 1.0; p.W11 = 1.0;
    } else {
        p.V00 = c.V_00; p.V11 = c.V_11; p.W00 = c.W_00; p.W11 = c.W_11;
    }
    p.sV00 = c.V_00; p.sV11 = c.V_11; p.sW00 = c.W_00; p.sW11 = c.W_11;
    p.d_max = c.d_max; p.th_max = c.th_max;
    p.range_max = h->range_max; p.fov_min = h->fov_min; p.fov_max = h->fov_max;
    p.seed = h->seed; p.inst0 = h->inst0; p.step = h->step;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.khist = h->dkhist;
}

// The maps of slam_set_maps, if set, and per-instance commands d_cmd_each (device, [T][B][2]; NULL = the shared ones).
template <class Params>
void set_each_inputs(const slam_handle* h, Params& p, const float* d_cmd_each) {
    if (h->each.maps_each) { p.map_each = h->each.dmaps; p.L_each = h->each.dLs; p.map_stride = h->each.map_stride; }
    p.cmd_each = d_cmd_each;
    p.noise_each = h->each.noise_each ? h->each.dnoise.get() : nullptr;
}

// the two events of a fill, on first use
int stage_events(slam_handle::Stage& f) {
    if (f.copied) return SLAM_OK;
    HIP_TRY(hipEventCreateWithFlags(&f.copied, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&f.used, hipEventDisableTiming));
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

// Whether the EKF step queue can take one more step from `src` as it stands: it is empty, or it holds steps of the same source with a
// compatible stride (host messages: at most the stride of the fill, device messages: the same stride) and has room.  If it cannot, the
// caller runs the queue first, so that steps run in call order.
bool queue_takes(const slam_handle* h, StepQueue::Source src, int ks) {
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
bool eager_flush(slam_handle* h, int queued) {
    if (h->eager_target <= 0 || queued < h->eager_target) return false;
    const hipError_t e = hipStreamQuery(h->stream);
    (void)hipGetLastError();   // hipErrorNotReady is an answer, not an error
    if (e != hipSuccess) return false;
    h->eager_target = 2 * queued < h->lazy_max ? 2 * queued : h->lazy_max;
    return true;
}
constexpr int kExtQ = 4;   // detections per instance a queued slam_step message can hold

// d_cmd_each: the commands are per instance, [T][B][2] on the device (cmds is not read)
int run_sim_now(slam_handle* h, const float* cmds, int T, const float* d_cmd_each = nullptr) {
    if (T == 0) return SLAM_OK;
    const size_t each_step = 2 * (size_t)h->B;   // floats of d_cmd_each per timestep
    auto cmd_at = [&](size_t t) { return d_cmd_each ? kNoCmd : cmds + 2 * t; };
    auto each_at = [&](size_t t) { return d_cmd_each ? d_cmd_each + t * each_step : nullptr; };
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
    if (h->kind != SLAM_EKF_SLAM && !h->dump_meas && h->B >= h->ukf.split_min) {
        // UKF: two launches per timestep (LDS-bound eigen-sqrt, then the latency-heavier sigma-point kernel).  The two
        // halves of the batch run on two streams and drift apart, so one half's sqrt overlaps the other's step kernel.
        HIP_TRY(hipSetDevice(h->device));
        const int NP = h->ukf.parts < 2 ? 2 : (h->ukf.parts > 4 ? 4 : h->ukf.parts);
        for (int a = 0; a < NP - 1; ++a)
            if (!h->ukf.aux_stream[a]) {
                HIP_TRY(hipStreamCreateWithFlags(&h->ukf.aux_stream[a], hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&h->ukf.aux_ev[a + 1], hipEventDisableTiming));
            }
        if (!h->ukf.aux_ev[0]) HIP_TRY(hipEventCreateWithFlags(&h->ukf.aux_ev[0], hipEventDisableTiming));
        HIP_TRY(hipEventRecord(h->ukf.aux_ev[0], h->stream));
        for (int a = 0; a < NP - 1; ++a) HIP_TRY(hipStreamWaitEvent(h->ukf.aux_stream[a], h->ukf.aux_ev[0], 0));
        const int per = (h->B + NP - 1) / NP;
        int long_cap = 0;
        if (const int rc = long_message_cap(h, 1, 0, &long_cap)) return rc;
        for (int t = 0; t < T; ++t) {
            for (int part = 0; part < NP; ++part) {
                const int b_off = part * per;
                const int b_cnt = h->B - b_off < per ? h->B - b_off : per;
                if (b_cnt <= 0) continue;
                TRY(launch_ukf_pair(h, cmd_at(t), 1, long_cap, nullptr, nullptr, 0, b_off, b_cnt, part ? h->ukf.aux_stream[part - 1] : h->stream, each_at(t)));
            }
            std::swap(h->dP, h->dP2);
            h->step += 1;
        }
        for (int a = 0; a < NP - 1; ++a) {
            HIP_TRY(hipEventRecord(h->ukf.aux_ev[a + 1], h->ukf.aux_stream[a]));
            HIP_TRY(hipStreamWaitEvent(h->stream, h->ukf.aux_ev[a + 1], 0));
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

// One timestep on host messages, launched at the call (after what is queued).  d_cmd_each: [B][2] per-instance commands already on the
// handle's stream (device), NULL = cmd.  kmax: the longest message of the call, clamped to k_stride.
int step_host_now(slam_handle* h, const float cmd[2], const float* d_cmd_each, const float* meas, const int32_t* count, int k_stride, int kmax) {
    const size_t B = (size_t)h->B;
    if (h->kind == SLAM_UKF_LOC && !h->ukf.dmapf) return slam_internal_fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    // The caller's buffers may be reused right after return (ekf.cpp:64 copies the message), so the message is packed
    // into one of two PINNED staging buffers (only max_b count[b] detections per instance travel), copied on a separate
    // stream while the previous step's kernel is still running, and the kernel waits for the copy by event.  The host
    // blocks only when it gets two steps ahead of the GPU.
    slam_handle::Stage& s = h->stage[h->stage_next & 1];
    h->stage_next += 1;
    if (kmax < 1) kmax = 1;
    if (!h->copy_stream) HIP_TRY(hipStreamCreateWithFlags(&h->copy_stream, hipStreamNonBlocking));
    TRY(stage_events(s));
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

}  // namespace

void fill_ekf_params(slam_handle* h, slam::EkfStepParams& p, const float cmd[2], int sim, int long_cap, const float* meas, const int32_t* count,
                     int k_stride, const float* d_cmds, int T, const float* d_cmd_each) {
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.P_out = h->dP2; p.x = h->dx; p.scratch = h->dscratch;
    set_common_params(h, p, cmd);
    const slam_config& c = h->cfg;
    p.id_known = c.landmark_id_is_known;
    p.min_sep = c.min_landmark_separation;
    p.abs_is_int = c.ekf_abs_is_int ? 1 : 0; p.lm_from_pred = c.ekf_landmark_from_x_pred ? 1 : 0;
    p.dbg = h->dbg;
    p.prof = (h->dbg & (4 | 32)) ? h->dprof : nullptr;
    set_step_input(h, p, sim, long_cap, meas, count, k_stride);
    p.cmds = d_cmds; p.T = T;
    set_each_inputs(h, p, d_cmd_each);
}

void fill_ukf_params(slam_handle* h, slam::UkfStepParams& p, const float cmd[2], const float* d_cmd_each) {
    memset(&p, 0, sizeof(p));
    p.P = (const double*)h->dP.get(); p.P_out = (double*)h->dP2.get(); p.x = (double*)h->dx.get(); p.sqtP = h->ukf.dsq; p.n_sq = h->ukf.dnsq; p.x_prev = h->ukf.dxprev; p.Vt_store = h->ukf.dvt; p.v_age = h->ukf.dvage;
    set_common_params(h, p, cmd);
    const slam_config& c = h->cfg;
    p.float_trig = c.ukf_float_trig;
    p.acc_zest1 = c.ukf_accumulate_zest1 ? 1 : 0; p.yaw_sigma = c.ukf_sensing_yaw_from_sigma ? 1 : 0;
    p.b_off = 0; p.b_cnt = h->B;
    p.loc = h->kind == SLAM_UKF_LOC; p.mapf = h->ukf.dmapf;
    p.quad_tab = h->ukf.drot;
    p.big_ws = h->ukf.dbigws;
    p.prof = (h->dbg & 4) ? h->dprof : nullptr;
    p.chol_ok = h->ukf.chol ? h->ukf.dchol : nullptr;
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
        HIP_TRY(h->ukf.dbigws.reserve((size_t)h->B * 2 * h->pstride));
    *cap_out = cap;
    return SLAM_OK;
}

int launch_step(slam_handle* h, const float cmd[2], int sim, const float* d_meas, const int32_t* d_count, int k_stride,
                const float* d_cmd_each) {
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
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

// per-instance commands [T][B][2] of one call from the host into dcmd_each, in stream order (the launches of earlier calls that read the
// buffer come first; it grows only once they are done).  A pending prediction stage reads the buffer, so nothing may replace it then.
int upload_cmds_each(slam_handle* h, const float* cmds, int T) {
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before the next step");
    const size_t n = 2 * (size_t)T * h->B;
    if (n == 0) return SLAM_OK;
    TRY(grow(h, h->each.dcmd_each, n));
    HIP_TRY(hipMemcpyAsync(h->each.dcmd_each, cmds, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

// Runs what the step queue holds: messages as one multi-step launch, generator steps through run_sim_now.  The queue is emptied only
// once the launch is enqueued: a failed flush keeps the queued timesteps (and fails again on the next call) instead of dropping them
// silently.
int flush_lazy(slam_handle* h) {
    StepQueue& q = h->q;
    const int T = q.steps();
    if (T == 0) return SLAM_OK;
    slam_handle::Stage& f = q.host[q.host_cur];
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

}  // namespace slam_capi

using namespace slam_capi;

extern "C" {

int slam_step_dev(slam_handle* h, const float cmd[2], const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || !cmd || !d_meas || !d_count || k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
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
    if (h->kind == SLAM_UKF_LOC && !h->ukf.dmapf) return slam_internal_fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    return launch_step(h, cmd, 0, d_meas, d_count, k_stride);
}

int slam_step(slam_handle* h, const float cmd[2], const float* meas, const int32_t* count, int k_stride) {
    if (!h || !cmd || !meas || !count || k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
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
        slam_handle::Stage& f = q.host[q.host_cur];
        if (q.steps() == 0) {
            if (f.in_use) { HIP_TRY(hipEventSynchronize(f.used)); f.in_use = false; }   // the launch that read this fill is done
            // capacity: the full stride kExtQ at once while that stays below 128 MB per fill (re-pinning 100 MB of host memory
            // costs ~40 ms each time the stride grows: 0.5 ms per step over a 300-step run); above that, the stride actually seen
            const size_t full = (size_t)3 * kExtQ * B * h->lazy_max;
            const size_t need = sizeof(float) * full <= ((size_t)128 << 20) ? full : (size_t)3 * q.host_ks * B * h->lazy_max;   // floats
            HIP_TRY(f.hmeas.reserve(need)); HIP_TRY(f.hcount.reserve(B * h->lazy_max)); HIP_TRY(f.hcmds.reserve(2 * (size_t)h->lazy_max));
            HIP_TRY(f.dmeas.reserve(need)); HIP_TRY(f.dcount.reserve(B * h->lazy_max));
            TRY(stage_events(f));
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

int slam_step_sim(slam_handle* h, const float cmd[2]) {
    if (!h || !cmd) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    TRY(sense_idle(h, "slam_step_sim"));
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
    if (!h || n < 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    h->lazy_max = n;
    h->lazy_explicit = true;
    return SLAM_OK;
}

int slam_run_sim(slam_handle* h, const float* cmds, int T) {
    if (!h || !cmds || T < 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    TRY(sense_idle(h, "slam_run_sim"));
    if (h->shadow) { const int rs = slam_run_sim(h->shadow, cmds, T); if (rs) return rs; }
    TRY(flush_lazy(h));
    return run_sim_now(h, cmds, T);
}

int slam_set_run_chunk(slam_handle* h, int steps_per_launch) {
    if (!h || steps_per_launch < 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    h->run_chunk = steps_per_launch;
    return SLAM_OK;
}

// UKF::predictionStage / UKF::updateStage (filter.h:187-188, ukf.cpp:197-291) as two calls.  predictionStage only
// writes members that updateStage consumes (sqtP, X, X_pred, x_pred, P_pred); x_t / P_t change when updateStage
// finishes (ukf.cpp:289-290).  So the split is: predict = nearestSPD + sqrt (the kernel that dominates the step) with
// the command remembered; update = the fused sigma-point / update / insertion kernel with that command.  The pair is
// bit-identical to slam_step_dev.
int slam_predict(slam_handle* h, const float cmd[2]) {
    if (!h || !cmd) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate prediction stage: EKF::update does both (ekf.cpp:37-179); use slam_step");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "slam_predict called twice without slam_update_dev");
    HIP_TRY(hipSetDevice(h->device));
    slam::UkfStepParams p;
    fill_ukf_params(h, p, cmd);
    HIP_TRY(slam::launch_ukf_sqrt(p, h->stream));
    h->ukf.pred_cmd[0] = cmd[0]; h->ukf.pred_cmd[1] = cmd[1];
    h->ukf.pred_each = false;
    h->ukf.predicted = true;
    return SLAM_OK;
}
int slam_update_dev(slam_handle* h, const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || k_stride < 0 || (k_stride > 0 && (!d_meas || !d_count))) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate update stage (ekf.cpp:37-179); use slam_step");
    if (!h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "slam_update_dev needs a preceding slam_predict");
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
    fill_ukf_params(h, p, h->ukf.pred_cmd, h->ukf.pred_each ? h->each.dcmd_each.get() : nullptr);
    p.sim = 0;
    p.long_mode = long_cap > 0 ? 1 : 0; p.long_cap = long_cap;
    p.meas_in = d_meas; p.meas_count_in = d_count; p.k_stride_in = k_stride;
    HIP_TRY(slam::launch_ukf_step(p, h->stream));
    std::swap(h->dP, h->dP2);
    h->step += 1;
    h->ukf.predicted = false;
    h->ukf.pred_each = false;
    return SLAM_OK;
}

int slam_step_each(slam_handle* h, const float* cmds, const float* meas, const int32_t* count, int k_stride) {
    if (!h || !cmds || !meas || !count || k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
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
    return step_host_now(h, kNoCmd, h->each.dcmd_each, meas, count, k_stride, kmax);
}

int slam_step_each_dev(slam_handle* h, const float* d_cmds, const float* d_meas, const int32_t* d_count, int k_stride) {
    if (!h || !d_cmds || !d_meas || !d_count || k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
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
    if (h->kind == SLAM_UKF_LOC && !h->ukf.dmapf) return slam_internal_fail(SLAM_ERR_STATE, "UKF_LOC needs the known map: call slam_set_map first (localization_node.cpp:113-116)");
    return launch_step(h, kNoCmd, 0, d_meas, d_count, k_stride, d_cmds);
}

int slam_run_sim_each(slam_handle* h, const float* cmds, int T) {
    if (!h || !cmds || T < 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "slam_set_map has not been called");
    TRY(sense_idle(h, "slam_run_sim_each"));
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
    return run_sim_now(h, nullptr, T, h->each.dcmd_each);
}

int slam_predict_each(slam_handle* h, const float* cmds) {
    if (!h || !cmds) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "EKF has no separate prediction stage: EKF::update does both (ekf.cpp:37-179); use slam_step_each");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "slam_predict called twice without slam_update_dev");
    HIP_TRY(hipSetDevice(h->device));
    TRY(upload_cmds_each(h, cmds, 1));   // read by the update stage; nothing replaces it until then
    slam::UkfStepParams p;
    fill_ukf_params(h, p, kNoCmd, h->each.dcmd_each);
    HIP_TRY(slam::launch_ukf_sqrt(p, h->stream));
    h->ukf.pred_each = true;
    h->ukf.predicted = true;
    return SLAM_OK;
}

}  // extern "C"
