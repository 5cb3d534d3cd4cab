// capi_assoc.cpp — C ABI: maximum-likelihood association of detections without ids with the landmarks of the map (assoc_kernel.hip)
#include <math.h>
#include <string.h>

#include <vector>

#include "assoc_kernel.h"
#include "capi_assoc.h"
#include "ekf_kernel.h"

using namespace slam_capi;

namespace {

// the traffic model of `ticks` associations whose counts are in dint ([kAssocRows][stride] rows, the first ticks * B of each), summed on the stream
int assoc_sum_work(slam_handle* h, size_t ticks, size_t stride) {
    const int32_t* const di = h->assoc.dint;
    HIP_TRY(slam::launch_associate_work(row(di, kAssocLm, stride), row(di, kAssocMatch, stride), row(di, kAssocNew, stride), row(di, kAssocDrop, stride),
                                        ticks * (size_t)h->B, h->esz, h->assoc.dwork, h->stream));
    return SLAM_OK;
}

}  // namespace

namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int assoc_config(const slam_assoc_config* cfg, slam_assoc_config* out) {
    if (cfg) *out = *cfg; else slam_assoc_config_default(out);
    if (isnan(out->gate_match) || isnan(out->gate_new) || !(out->gate_match > 0.0) || out->gate_match > out->gate_new)
        return slam_internal_fail(SLAM_ERR_ARG, "assoc config: 0 < gate_match = %g <= gate_new = %g does not hold (gate_new may be +inf)",
                                  out->gate_match, out->gate_new);
    return SLAM_OK;
}

int assoc_supported(const slam_handle* h) {
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "association needs EKF_SLAM: the innovation covariance of the UKF kinds depends on all sigma points, so no block of P closes");
    if (!h->cfg.landmark_id_is_known)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "association labels messages for the known-id step: a handle with landmark_id_is_known = 0 associates inside its step");
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
    TRY(grow(h, h->assoc.dint, kAssocRows * ticks * B));
    TRY(grow(h, h->assoc.dwork, 3));
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, ticks * slam::kInnovRecLen));
    HIP_TRY(hipMemsetAsync(h->assoc.dwork, 0, 3 * sizeof(unsigned long long), h->stream));
    return SLAM_OK;
}

int read_traffic(slam_handle* h, Traffic& w) {
    unsigned long long wk[3];
    HIP_TRY(hipMemcpy(wk, w.dwork, sizeof(wk), hipMemcpyDeviceToHost));
    w.bytes = (double)wk[0] * h->esz + (double)wk[1];
    w.lines = 128.0 * (double)wk[2] + (double)wk[1];
    return SLAM_OK;
}

int last_traffic_work(const Traffic* w, const char* calls, double* bytes, double* part_ms, double* total_ms) {
    if (!w) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (w->bytes < 0.0) return slam_internal_fail(SLAM_ERR_STATE, "%s has not run on this handle", calls);
    if (bytes) { bytes[0] = w->bytes; bytes[1] = w->lines; }
    if (part_ms) *part_ms = w->times.part_ms;
    if (total_ms) *total_ms = w->times.total_ms;
    return SLAM_OK;
}

int AssocTicks::chunk_done(int, int tc) { return assoc_sum_work(h, (size_t)tc, cb); }

int AssocTicks::finish() {
    HIP_TRY(hipStreamSynchronize(h->stream));
    return read_traffic(h, h->assoc);
}

}  // namespace slam_capi

namespace {

struct AssocOut { double* rec; int32_t *n_match, *n_new, *n_drop, *flags, *verdict, *slot; double* det; };

// slam_associate (host: the message and per-instance commands are host arrays) and slam_associate_dev
int associate(slam_handle* h, bool host, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
              int k_stride, float* meas_out, int32_t* count_out, const AssocOut& to) {
    slam_assoc_config c;
    const float *cmd, *d_each;
    TRY(assoc_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride, meas_out, count_out, !host));
    TRY(filter_enter(h, assoc_supported));
    DevMsg out = {meas_out, count_out};
    if (!host) TRY(out_message_overlaps(h, meas, count, k_stride, out));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(assoc_reserve(h, host ? k_stride : 1, 1));
    if (host) {
        out = {h->assoc.dmeas, h->assoc.dcount};
        TRY(seed_out_message(h, out.meas, k_stride));
    }
    const size_t B = (size_t)h->B, nd = B * slam::kInnovMaxDet, nm = 3 * (size_t)k_stride * B;
    int32_t* const di = h->assoc.dint;
    if (to.verdict) TRY(grow(h, h->assoc.dverdict, nd));
    if (to.slot) TRY(grow(h, h->assoc.dslot, nd));
    if (to.det) TRY(grow(h, h->assoc.ddet, nd * slam::kAssocDetLen));
    const AssocDev d = {row(di, kAssocMatch, B), row(di, kAssocNew, B), row(di, kAssocDrop, B), row(di, kAssocFlags, B), row(di, kAssocLm, B),
                        to.verdict ? h->assoc.dverdict.get() : nullptr, to.slot ? h->assoc.dslot.get() : nullptr, to.det ? h->assoc.ddet.get() : nullptr};
    TRY(assoc_launch(h, c, cmd, d_each, meas, count, k_stride, out.meas, out.count, h->inn.drec, d));
    TRY(assoc_sum_work(h, 1, B));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(read_traffic(h, h->assoc));
    return copy_rows({{h->inn.drec, to.rec, slam::kInnovRecLen}, {d.n_match, to.n_match, B}, {d.n_new, to.n_new, B}, {d.n_drop, to.n_drop, B},
                      {d.flags, to.flags, B}, {d.verdict, to.verdict, nd}, {d.slot, to.slot, nd}, {d.det, to.det, nd * slam::kAssocDetLen},
                      {out.meas, host ? meas_out : nullptr, nm}, {out.count, host ? count_out : nullptr, B}}, 0, 1);
}

// slam_step_associated (host: as above) and slam_step_associated_dev: one associated timestep
int step_associated(slam_handle* h, bool host, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                    int k_stride, double* rec, int32_t* n_drop) {
    slam_assoc_config c;
    const float *cmd, *d_each;
    TRY(assoc_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride));
    TRY(filter_enter(h, assoc_supported));
    TRY(step_state(h, "an associated step"));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(assoc_reserve(h, k_stride, 1));
    int32_t* const d_drop = row(h->assoc.dint, kAssocDrop, (size_t)h->B);
    TRY(assoc_launch(h, c, cmd, d_each, meas, count, k_stride, h->assoc.dmeas, h->assoc.dcount, h->inn.drec,
                     {nullptr, nullptr, d_drop, nullptr, nullptr, nullptr, nullptr, nullptr}));
    TRY(launch_step(h, cmd, 0, h->assoc.dmeas, h->assoc.dcount, k_stride, d_each));
    return step_outputs(h, rec, d_drop, n_drop);
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
    return associate(h, true, cfg, cmds, cmd_each, meas, count, k_stride, meas_out, count_out, {rec, n_match, n_new, n_drop, flags, verdict, slot, det});
}

int slam_associate_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                       int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, int32_t* verdict,
                       int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out) {
    return associate(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out,
                     {rec, n_match, n_new, n_drop, flags, verdict, slot, det});
}

int slam_step_associated(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                         int k_stride, double rec[16], int32_t* n_drop) {
    return step_associated(h, true, cfg, cmds, cmd_each, meas, count, k_stride, rec, n_drop);
}

int slam_step_associated_dev(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop) {
    return step_associated(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, rec, n_drop);
}

int slam_associate_run(slam_handle* h, const slam_assoc_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                       int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags) {
    slam_assoc_config c;
    TickMsgs msgs;
    TRY(assoc_config(cfg, &c));
    TRY(run_args_log(cmds, meas, count, k_stride, T, &msgs));
    return run_filtered(h, "slam_associate_run", cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T,
                        AssocTicks{h, c, recs, n_match, n_new, n_drop, flags});
}

int slam_associate_run_sim(slam_handle* h, const slam_assoc_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                           int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, const slam_sense_log* log) {
    slam_assoc_config c;
    TickCmds::Source csrc;
    TickMsgs msgs;
    TRY(assoc_config(cfg, &c));
    TRY(run_args_sim(source, cmds, k_stride, T, log, &csrc, &msgs));
    return run_filtered(h, "slam_associate_run_sim", csrc, cmds, msgs, T, AssocTicks{h, c, recs, n_match, n_new, n_drop, flags});
}

int slam_last_associate_work(slam_handle* h, double* bytes, double* assoc_ms, double* total_ms) {
    return last_traffic_work(h ? &h->assoc : nullptr, "slam_associate, slam_associate_dev or slam_associate_run", bytes, assoc_ms, total_ms);
}

int slam_associate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                 const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                 const slam_assoc_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                                 double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out) {
    (void)lm_from_pred;   // (no update precedes a cost: x_pred and x_t hold the same landmark positions)
    slam_assoc_config c;
    InstanceHostArgs a;
    TRY(assoc_config(cfg, &c));
    TRY(a.init(x, P, ids, M, L_max, cmd, meas, count, k_stride, true, noise, f32_storage));
    std::vector<slam::AssocWork> ws(1);
    const slam::AssocResult v = slam::associate_instance_host(ws[0], a.load_x, a.load_P, ids, M, L_max, status, cmd[0], cmd[1], meas, count, k_stride,
                                                              a.nz, c.gate_match, c.gate_new, cost, verdict, slot, det, meas_out, count_out);
    if (rec) slam::assoc_record(v, rec);
    if (n_match) *n_match = v.n_match;
    if (n_new) *n_new = v.n_new;
    if (n_drop) *n_drop = v.n_drop;
    if (flags) *flags = v.flags;
    return SLAM_OK;
}

}  // extern "C"
