// capi_assoc.cpp — C ABI: maximum-likelihood association of detections without ids with the landmarks of the map (assoc_kernel.hip)
#include <math.h>
#include <string.h>

#include <vector>

#include "assoc_kernel.h"
#include "capi_assoc.h"
#include "capi_innovation.h"
#include "capi_run.h"
#include "ekf_kernel.h"
#include "host/noise_pack.h"
#include "host/tick_chunks.h"

using namespace slam_capi;

namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int assoc_config(const slam_assoc_config* cfg, slam_assoc_config* out) {
    if (cfg) *out = *cfg; else slam_assoc_config_default(out);
    if (isnan(out->gate_match) || isnan(out->gate_new) || !(out->gate_match > 0.0) || out->gate_match > out->gate_new)
        return slam_internal_fail(SLAM_ERR_ARG, "assoc config: 0 < gate_match = %g <= gate_new = %g does not hold (gate_new may be +inf)",
                                  out->gate_match, out->gate_new);
    return SLAM_OK;
}

bool assoc_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* const pa = (const char*)a; const char* const pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

// the arguments every entry point of one message shares, checked before the handle is looked at
int assoc_args(const slam_assoc_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride, const float* meas_out,
               const int32_t* count_out, bool need_out, slam_assoc_config* c) {
    TRY(assoc_config(cfg, c));
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (need_out && (!meas_out || !count_out)) return slam_internal_fail(SLAM_ERR_ARG, "d_meas_out or d_count_out is NULL");
    if ((meas_out == meas) != (count_out == count))
        return slam_internal_fail(SLAM_ERR_ARG, "in place means both: meas_out == meas and count_out == meas_count, or neither");
    return SLAM_OK;
}

int assoc_supported(const slam_handle* h) {
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "association needs EKF_SLAM: the innovation covariance of the UKF kinds depends on all sigma points, so no block of P closes");
    if (!h->cfg.landmark_id_is_known)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "association labels messages for the known-id step: a handle with landmark_id_is_known = 0 associates inside its step");
    return SLAM_OK;
}

// the handle, once the arguments are in order; the queued timesteps run first
int assoc_enter(slam_handle* h) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(assoc_supported(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

int assoc_step_state(const slam_handle* h, const char* who) {
    if (h->shadow) return slam_internal_fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
    return SLAM_OK;
}

// the association launches of one message on the handle's stream
int assoc_launch(slam_handle* h, const slam_assoc_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
                 int k_stride, float* d_meas_out, int32_t* d_count_out, double* d_rec, const AssocDev& d) {
    slam::AssocParams p;
    memset(&p, 0, sizeof(p));
    fill_ekf_params(h, p.s, cmd, 0, 0, d_meas, d_count, k_stride, nullptr, 0, d_cmd_each);
    p.gate_match = c.gate_match; p.gate_new = c.gate_new;
    p.meas_out = d_meas_out; p.count_out = d_count_out;
    p.n_match = d.n_match; p.n_new = d.n_new; p.n_drop = d.n_drop; p.flags = d.flags; p.n_lm = d.n_lm; p.verdict = d.verdict; p.slot = d.slot; p.det = d.det;
    p.inst_rec = h->inn.dval + 13 * (size_t)h->B;   // (the places innovation_reserve gives the contributions and the partial records)
    p.partials = h->inn.dpart;
    p.rec = d_rec;
    HIP_TRY(slam::launch_associate(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

// the labelled message of one tick, the records and the counts of `ticks` ticks, the contributions and the traffic sums (zeroed in stream order)
int assoc_reserve(slam_handle* h, int k_stride, size_t ticks) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->assoc.dmeas, 3 * (size_t)k_stride * B));
    TRY(grow(h, h->assoc.dcount, B));
    TRY(grow(h, h->assoc.dint, 5 * ticks * B));
    TRY(grow(h, h->assoc.dwork, 3));
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, ticks * slam::kInnovRecLen));
    HIP_TRY(hipMemsetAsync(h->assoc.dwork, 0, 3 * sizeof(unsigned long long), h->stream));
    return SLAM_OK;
}

}  // namespace slam_capi

namespace {

// the traffic model of `ticks` associations whose counts are in dint ([5][stride] rows, the first ticks * B of each), summed on the stream
int assoc_sum_work(slam_handle* h, size_t ticks, size_t stride) {
    const int32_t* const di = h->assoc.dint;
    HIP_TRY(slam::launch_associate_work(di + 4 * stride, di, di + stride, di + 2 * stride, ticks * (size_t)h->B, h->esz, h->assoc.dwork, h->stream));
    return SLAM_OK;
}

// after a synchronisation: the sums since assoc_reserve
int assoc_read_work(slam_handle* h) {
    unsigned long long wk[3];
    HIP_TRY(hipMemcpy(wk, h->assoc.dwork, sizeof(wk), hipMemcpyDeviceToHost));
    h->assoc.bytes = (double)wk[0] * h->esz + (double)wk[1];
    h->assoc.lines = 128.0 * (double)wk[2] + (double)wk[1];
    return SLAM_OK;
}

struct AssocOut { double* rec; int32_t *n_match, *n_new, *n_drop, *flags, *verdict, *slot; double* det; };

// slam_associate / slam_associate_dev once the message and the commands are on the device
int associate_now(slam_handle* h, const slam_assoc_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
                  int k_stride, float* d_meas_out, int32_t* d_count_out, const AssocOut& to) {
    const size_t B = (size_t)h->B, nd = B * slam::kInnovMaxDet;
    int32_t* const di = h->assoc.dint;
    if (to.verdict) TRY(grow(h, h->assoc.dverdict, nd));
    if (to.slot) TRY(grow(h, h->assoc.dslot, nd));
    if (to.det) TRY(grow(h, h->assoc.ddet, nd * slam::kAssocDetLen));
    const AssocDev d = {di, di + B, di + 2 * B, di + 3 * B, di + 4 * B, to.verdict ? h->assoc.dverdict.get() : nullptr, to.slot ? h->assoc.dslot.get() : nullptr,
                        to.det ? h->assoc.ddet.get() : nullptr};
    TRY(assoc_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out, h->inn.drec, d));
    TRY(assoc_sum_work(h, 1, B));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(assoc_read_work(h));
    if (to.rec) HIP_TRY(hipMemcpy(to.rec, h->inn.drec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (to.n_match) HIP_TRY(hipMemcpy(to.n_match, d.n_match, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_new) HIP_TRY(hipMemcpy(to.n_new, d.n_new, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_drop) HIP_TRY(hipMemcpy(to.n_drop, d.n_drop, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.flags) HIP_TRY(hipMemcpy(to.flags, d.flags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.verdict) HIP_TRY(hipMemcpy(to.verdict, d.verdict, sizeof(int32_t) * nd, hipMemcpyDeviceToHost));
    if (to.slot) HIP_TRY(hipMemcpy(to.slot, d.slot, sizeof(int32_t) * nd, hipMemcpyDeviceToHost));
    if (to.det) HIP_TRY(hipMemcpy(to.det, d.det, sizeof(double) * nd * slam::kAssocDetLen, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// one associated timestep once the message and the commands are on the device
int step_associated_now(slam_handle* h, const slam_assoc_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                        const int32_t* d_count, int k_stride, double* rec, int32_t* n_drop) {
    const size_t B = (size_t)h->B;
    TRY(assoc_reserve(h, k_stride, 1));
    int32_t* const di = h->assoc.dint;
    TRY(assoc_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, h->assoc.dmeas, h->assoc.dcount, h->inn.drec,
                     {nullptr, nullptr, di + 2 * B, nullptr, nullptr, nullptr, nullptr, nullptr}));
    TRY(launch_step(h, cmd, 0, h->assoc.dmeas, h->assoc.dcount, k_stride, d_cmd_each));
    if (!rec && !n_drop) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (rec) HIP_TRY(hipMemcpy(rec, h->inn.drec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (n_drop) HIP_TRY(hipMemcpy(n_drop, di + 2 * B, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_assoc_config_default(slam_assoc_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->gate_match = -2.0 * log(0.01);   // the 0.99 and 1 - 1e-6 quantiles of chi-square with 2 degrees of freedom
    c->gate_new = -2.0 * log(1e-6);
    return SLAM_OK;
}

int slam_associate(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                   int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, int32_t* verdict, int32_t* slot,
                   double* det, float* meas_out, int32_t* count_out) {
    slam_assoc_config c;
    TRY(assoc_args(cfg, cmds, meas, count, k_stride, meas_out, count_out, false, &c));
    TRY(assoc_enter(h));
    const size_t B = (size_t)h->B, nm = 3 * (size_t)k_stride * B;
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * B));
    TRY(assoc_reserve(h, k_stride, 1));
    // (slots the kernel does not write keep what the caller gave: the output row starts as the input row)
    HIP_TRY(hipMemcpyAsync(h->assoc.dmeas, h->inn.dmeas, sizeof(float) * nm, hipMemcpyDeviceToDevice, h->stream));
    TRY(associate_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, h->assoc.dmeas,
                      h->assoc.dcount, {rec, n_match, n_new, n_drop, flags, verdict, slot, det}));
    if (meas_out) HIP_TRY(hipMemcpy(meas_out, h->assoc.dmeas, sizeof(float) * nm, hipMemcpyDeviceToHost));
    if (count_out) HIP_TRY(hipMemcpy(count_out, h->assoc.dcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_associate_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                       int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, int32_t* verdict,
                       int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out) {
    slam_assoc_config c;
    TRY(assoc_args(cfg, cmds, d_meas, d_count, k_stride, d_meas_out, d_count_out, true, &c));
    TRY(assoc_enter(h));
    const size_t B = (size_t)h->B, bm = sizeof(float) * 3 * (size_t)k_stride * B, bc = sizeof(int32_t) * B;
    if ((d_meas_out != d_meas && assoc_overlap(d_meas_out, bm, d_meas, bm)) || (d_count_out != d_count && assoc_overlap(d_count_out, bc, d_count, bc)) ||
        assoc_overlap(d_meas_out, bm, d_count, bc) || assoc_overlap(d_count_out, bc, d_meas, bm) || assoc_overlap(d_meas_out, bm, d_count_out, bc))
        return slam_internal_fail(SLAM_ERR_ARG, "the output message overlaps the input (only d_meas_out == d_meas with d_count_out == d_count is allowed) or itself");
    TRY(assoc_reserve(h, 1, 1));
    return associate_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, d_meas_out, d_count_out,
                         {rec, n_match, n_new, n_drop, flags, verdict, slot, det});
}

int slam_step_associated(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                         int k_stride, double rec[16], int32_t* n_drop) {
    slam_assoc_config c;
    TRY(assoc_args(cfg, cmds, meas, count, k_stride, nullptr, nullptr, false, &c));
    TRY(assoc_enter(h));
    TRY(assoc_step_state(h, "an associated step"));
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * (size_t)h->B));
    return step_associated_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, rec, n_drop);
}

int slam_step_associated_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop) {
    slam_assoc_config c;
    TRY(assoc_args(cfg, cmds, d_meas, d_count, k_stride, nullptr, nullptr, false, &c));
    TRY(assoc_enter(h));
    TRY(assoc_step_state(h, "an associated step"));
    return step_associated_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, rec, n_drop);
}

}  // extern "C"

namespace {

// slam_associate_run and slam_associate_run_sim once their arguments are in order: T associated ticks with the commands of `csrc` on the messages of `msgs`
int associate_run(slam_handle* h, const char* who, const slam_assoc_config& c, TickCmds::Source csrc, const float* cmds, TickMsgs& msgs, int T,
                  double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags) {
    const int k_stride = msgs.k_stride;
    TRY(run_enter(h, who, msgs.sim(), csrc == TickCmds::kNav, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    TickCmds tcmd;
    TRY(tcmd.init(h, csrc, cmds));
    // what a tick holds on the device: its rows of the counts, of the commands (cmd_each) and of the messages
    const double per_tick = 5.0 * 4.0 * (double)B + tcmd.bytes_per_tick(h) + msgs.bytes_per_tick(h, tcmd);
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(assoc_reserve(h, k_stride, (size_t)chunk));
    TRY(msgs.reserve(h, tcmd, chunk));
    const size_t cb = (size_t)chunk * B;
    int32_t* const di = h->assoc.dint;
    const int rc = run_chunked(
        h, T, chunk, h->nav.time_ticks, h->assoc.times,
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            return msgs.upload(h, t0, tc);
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each, *dm;
            const int32_t* dc;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(msgs.produce(h, tcmd, t, cmd, d_each, &dm, &dc));
            const size_t o = (size_t)t * B;
            TRY(mark([&] {
                return assoc_launch(h, c, cmd, d_each, dm, dc, k_stride, h->assoc.dmeas, h->assoc.dcount,
                                    h->inn.drec + (size_t)t * slam::kInnovRecLen,
                                    {di + o, di + cb + o, di + 2 * cb + o, di + 3 * cb + o, di + 4 * cb + o, nullptr, nullptr, nullptr});
            }));
            TRY(launch_step(h, cmd, 0, h->assoc.dmeas, h->assoc.dcount, k_stride, d_each));
            return msgs.commit(h, t);
        },
        [&](int t0, int tc) -> int {
            const size_t nb = sizeof(int32_t) * (size_t)tc * B, o = (size_t)t0 * B;
            TRY(msgs.download(h, tcmd, t0, tc));
            TRY(assoc_sum_work(h, (size_t)tc, cb));   // (after the chunk's events: it is no part of the run's times)
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kInnovRecLen, h->inn.drec, sizeof(double) * (size_t)tc * slam::kInnovRecLen, hipMemcpyDeviceToHost));
            if (n_match) HIP_TRY(hipMemcpy(n_match + o, di, nb, hipMemcpyDeviceToHost));
            if (n_new) HIP_TRY(hipMemcpy(n_new + o, di + cb, nb, hipMemcpyDeviceToHost));
            if (n_drop) HIP_TRY(hipMemcpy(n_drop + o, di + 2 * cb, nb, hipMemcpyDeviceToHost));
            if (flags) HIP_TRY(hipMemcpy(flags + o, di + 3 * cb, nb, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
    TRY(rc);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return assoc_read_work(h);
}

}  // namespace

extern "C" {

int slam_associate_run(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                       int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags) {
    slam_assoc_config c;
    TRY(assoc_config(cfg, &c));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_log(meas, count, k_stride);
    return associate_run(h, "slam_associate_run", c, cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T, recs, n_match, n_new, n_drop, flags);
}

int slam_associate_run_sim(slam_handle* h, const slam_assoc_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                           int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, const slam_sense_log* log) {
    slam_assoc_config c;
    TickCmds::Source csrc;
    TRY(assoc_config(cfg, &c));
    TRY(sim_run_source(source, cmds, &csrc));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_sim(log, k_stride);
    return associate_run(h, "slam_associate_run_sim", c, csrc, cmds, msgs, T, recs, n_match, n_new, n_drop, flags);
}

int slam_last_associate_work(slam_handle* h, double* bytes, double* assoc_ms, double* total_ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->assoc.bytes < 0.0) return slam_internal_fail(SLAM_ERR_STATE, "slam_associate, slam_associate_dev or slam_associate_run has not run on this handle");
    if (bytes) { bytes[0] = h->assoc.bytes; bytes[1] = h->assoc.lines; }
    if (assoc_ms) *assoc_ms = h->assoc.times.part_ms;
    if (total_ms) *total_ms = h->assoc.times.total_ms;
    return SLAM_OK;
}

int slam_associate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                 const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                 const slam_assoc_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                                 double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out) {
    (void)lm_from_pred;   // (no update precedes a cost: x_pred and x_t hold the same landmark positions)
    slam_assoc_config c;
    TRY(assoc_config(cfg, &c));
    if (!x || !P || !cmd || !noise) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (count > 0 && !meas) return slam_internal_fail(SLAM_ERR_ARG, "meas is NULL");
    if (const char* f = slam_host::noise_bad_field(*noise)) return slam_internal_fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
    const slam::InnovNoise nz = {noise->v_d, noise->v_th, noise->w_r, noise->w_b, noise->V_00, noise->V_11, noise->W_00, noise->W_11};
    const int n = 3 + 2 * M;
    std::vector<slam::AssocWork> ws(1);
    const bool f32 = f32_storage != 0;
    const slam::AssocResult v = slam::associate_instance_host(
        ws[0], [&](int i) { return f32 ? (double)(float)x[i] : x[i]; },
        [&](int r, int cc) { const double e = P[(size_t)r * n + cc]; return f32 ? (double)(float)e : e; }, ids, M, L_max, status, cmd[0], cmd[1], meas,
        count, k_stride, nz, c.gate_match, c.gate_new, cost, verdict, slot, det, meas_out, count_out);
    if (rec) slam::assoc_record(v, rec);
    if (n_match) *n_match = v.n_match;
    if (n_new) *n_new = v.n_new;
    if (n_drop) *n_drop = v.n_drop;
    if (flags) *flags = v.flags;
    return SLAM_OK;
}

}  // extern "C"
