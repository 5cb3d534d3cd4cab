// capi_gate.cpp — C ABI: innovation gating, the chi-square gate on the message the next step will process (gate_kernel.hip)
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_innovation.h"
#include "capi_run.h"
#include "gate_kernel.h"
#include "host/noise_pack.h"
#include "host/tick_chunks.h"

using namespace slam_capi;

namespace {

// *out = *cfg (NULL: the defaults), checked
int gate_config(const slam_gate_config* cfg, slam_gate_config* out) {
    if (cfg) *out = *cfg; else slam_gate_config_default(out);
    if (!(out->gate > 0.0)) return slam_internal_fail(SLAM_ERR_ARG, "gate config: gate = %g must be positive (+inf: nothing is rejected)", out->gate);
    if (!isfinite(out->nis_lo) || !isfinite(out->nis_hi) || out->nis_lo > out->nis_hi)
        return slam_internal_fail(SLAM_ERR_ARG, "gate config: the band nis_lo = %g .. nis_hi = %g must be finite and ordered", out->nis_lo, out->nis_hi);
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
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (need_out && (!meas_out || !count_out)) return slam_internal_fail(SLAM_ERR_ARG, "d_meas_out or d_count_out is NULL");
    if ((meas_out == meas) != (count_out == count))
        return slam_internal_fail(SLAM_ERR_ARG, "in place means both: meas_out == meas and count_out == meas_count, or neither");
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
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
    if (h->shadow) return slam_internal_fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
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
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
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
        return slam_internal_fail(SLAM_ERR_ARG, "the output message overlaps the input (only d_meas_out == d_meas with d_count_out == d_count is allowed) or itself");
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

}  // extern "C"

namespace {

// slam_gate_run and slam_gate_run_sim once their arguments are in order: T gated ticks with the commands of `csrc` on the messages of `msgs`
int gate_run(slam_handle* h, const char* who, const slam_gate_config& c, TickCmds::Source csrc, const float* cmds, TickMsgs& msgs, int T,
             double* recs, double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags) {
    const int k_stride = msgs.k_stride;
    TRY(run_enter(h, who, msgs.sim(), csrc == TickCmds::kNav, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    TickCmds tcmd;
    TRY(tcmd.init(h, csrc, cmds));
    // what a tick holds on the device: its rows of the series, of the commands (cmd_each) and of the messages
    const double per_tick = 8.0 * (nis_sum ? (double)B : 0.0) + 4.0 * (double)B * ((n_upd ? 1 : 0) + (flags ? 1 : 0) + (n_rej ? 1 : 0)) +
                            tcmd.bytes_per_tick(h) + msgs.bytes_per_tick(h, tcmd);
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(gate_reserve_step(h, k_stride, (size_t)chunk));
    TRY(msgs.reserve(h, tcmd, chunk));
    if (nis_sum) TRY(grow(h, h->inn.dlog, (size_t)chunk * B));
    TRY(grow(h, h->inn.dint, 2 * (size_t)chunk * B));
    int32_t* const d_upd = h->inn.dint;
    int32_t* const d_flags = h->inn.dint + (size_t)chunk * B;
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->gate.times,
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            return msgs.upload(h, t0, tc);
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each, *dm;
            const int32_t* dc;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(msgs.produce(h, tcmd, t, cmd, d_each, &dm, &dc));
            TRY(mark([&] {
                return gate_launch(h, c, cmd, d_each, dm, dc, k_stride, h->gate.dmeas,
                                   h->gate.dcount, h->inn.drec + (size_t)t * slam::kInnovRecLen, nis_sum ? h->inn.dlog + (size_t)t * B : nullptr,
                                   nullptr, nullptr, n_upd ? d_upd + (size_t)t * B : nullptr, flags ? d_flags + (size_t)t * B : nullptr, nullptr,
                                   h->gate.drej + (size_t)t * B, nullptr);
            }));
            TRY(launch_step(h, cmd, 0, h->gate.dmeas, h->gate.dcount, k_stride, d_each));
            return msgs.commit(h, t);
        },
        [&](int t0, int tc) -> int {
            TRY(msgs.download(h, tcmd, t0, tc));
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kInnovRecLen, h->inn.drec, sizeof(double) * (size_t)tc * slam::kInnovRecLen, hipMemcpyDeviceToHost));
            if (nis_sum) HIP_TRY(hipMemcpy(nis_sum + (size_t)t0 * B, h->inn.dlog, sizeof(double) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (n_upd) HIP_TRY(hipMemcpy(n_upd + (size_t)t0 * B, d_upd, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (flags) HIP_TRY(hipMemcpy(flags + (size_t)t0 * B, d_flags, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            if (n_rej) HIP_TRY(hipMemcpy(n_rej + (size_t)t0 * B, h->gate.drej, sizeof(int32_t) * (size_t)tc * B, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
}

}  // namespace

extern "C" {

int slam_gate_run(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                  int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags) {
    slam_gate_config c;
    TRY(gate_config(cfg, &c));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_log(meas, count, k_stride);
    return gate_run(h, "slam_gate_run", c, cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T, recs, nis_sum, n_upd, n_rej, flags);
}

int slam_gate_run_sim(slam_handle* h, const slam_gate_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                      double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags, const slam_sense_log* log) {
    slam_gate_config c;
    TickCmds::Source csrc;
    TRY(gate_config(cfg, &c));
    TRY(sim_run_source(source, cmds, &csrc));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_sim(log, k_stride);
    return gate_run(h, "slam_gate_run_sim", c, csrc, cmds, msgs, T, recs, nis_sum, n_upd, n_rej, flags);
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
    if (!x || !P || !cmd || !noise) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (count > 0 && !meas) return slam_internal_fail(SLAM_ERR_ARG, "meas is NULL");
    if (const char* f = slam_host::noise_bad_field(*noise)) return slam_internal_fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
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
