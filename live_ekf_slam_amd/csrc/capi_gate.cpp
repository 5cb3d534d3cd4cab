// capi_gate.cpp — C ABI: innovation gating, the chi-square gate on the message the next step will process (gate_kernel.hip)
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_filter.h"
#include "gate_kernel.h"

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

// the gate launches of one message on the handle's stream into the message `out`; the per-instance outputs may be NULL
int gate_launch(slam_handle* h, const slam_gate_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                const int32_t* d_count, int k_stride, DevMsg out, const InnovOut& d, int32_t* d_n_rej, int32_t* d_verdict) {
    const slam_innovation_config band = {c.nis_lo, c.nis_hi};
    slam::GateParams p;
    memset(&p, 0, sizeof(p));
    p.in = innovation_params(h, band, cmd, 0, d_meas, d_count, k_stride, d_cmd_each);
    p.in.nis_sum = d.nis_sum; p.in.post = d.post; p.in.det = d.det; p.in.n_upd = d.n_upd; p.in.flags = d.flags; p.in.n_new = d.n_new;
    p.in.rec = d.rec;
    p.gate = c.gate; p.meas_out = out.meas; p.count_out = out.count; p.n_rej = d_n_rej; p.verdict = d_verdict;
    HIP_TRY(slam::launch_gate(p, h->esz == 4, h->stream));
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

// slam_gate (host: the messages and per-instance commands are host arrays) and slam_gate_dev
int gate(slam_handle* h, bool host, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
         int k_stride, float* meas_out, int32_t* count_out, const InnovOut& to, int32_t* n_rej, int32_t* verdict) {
    slam_gate_config c;
    const float *cmd, *d_each;
    TRY(gate_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride, meas_out, count_out, !host));
    TRY(filter_enter(h, innovation_supported));
    DevMsg out = {meas_out, count_out};
    if (!host) TRY(out_message_overlaps(h, meas, count, k_stride, out));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    const size_t B = (size_t)h->B, nm = 3 * (size_t)k_stride * B, nd = B * slam::kInnovMaxDet;
    if (host) {
        TRY(grow(h, h->gate.dmeas, nm));
        TRY(grow(h, h->gate.dcount, B));
        out = {h->gate.dmeas, h->gate.dcount};
        TRY(seed_out_message(h, out.meas, k_stride));
    }
    InnovOut d;
    TRY(innovation_outputs(h, to.det != nullptr, &d));
    TRY(grow(h, h->gate.drej, B));
    if (verdict) TRY(grow(h, h->gate.dverdict, nd));
    TRY(gate_launch(h, c, cmd, d_each, meas, count, k_stride, out, d, h->gate.drej, verdict ? h->gate.dverdict.get() : nullptr));
    TRY(innovation_download(h, d, to));
    return copy_rows({{h->gate.drej, n_rej, B}, {h->gate.dverdict, verdict, nd},
                      {out.meas, host ? meas_out : nullptr, nm}, {out.count, host ? count_out : nullptr, B}}, 0, 1);
}

// slam_step_gated* (host: as above): one gated timestep
int step_gated(slam_handle* h, bool host, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
               int k_stride, double* rec, int32_t* n_rej) {
    slam_gate_config c;
    const float *cmd, *d_each;
    TRY(gate_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride));
    TRY(filter_enter(h, innovation_supported));
    TRY(step_state(h, "a gated step"));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(gate_reserve_step(h, k_stride, 1));
    TRY(gate_launch(h, c, cmd, d_each, meas, count, k_stride, {h->gate.dmeas, h->gate.dcount}, {h->inn.drec}, h->gate.drej, nullptr));
    TRY(launch_step(h, cmd, 0, h->gate.dmeas, h->gate.dcount, k_stride, d_each));
    return step_outputs(h, rec, h->gate.drej, n_rej);
}

// The gate as run_filtered's feature: the series the caller asked for decide which rows a tick holds.
struct GateTicks {
    slam_handle* h; const slam_gate_config& c;
    double *recs, *nis_sum; int32_t *n_upd, *n_rej, *flags;
    size_t B = 0, cb = 0;   // (set by reserve: the handle is checked by then)

    RunTimes& times() const { return h->gate.times; }
    double bytes_per_tick() const {
        return 8.0 * (nis_sum ? (double)h->B : 0.0) + 4.0 * (double)h->B * ((n_upd ? 1 : 0) + (flags ? 1 : 0) + (n_rej ? 1 : 0));
    }
    int reserve(int k_stride, int chunk) {
        B = (size_t)h->B; cb = (size_t)chunk * B;
        TRY(gate_reserve_step(h, k_stride, (size_t)chunk));
        if (nis_sum) TRY(grow(h, h->inn.dlog, cb));
        return grow(h, h->inn.dint, 2 * cb);
    }
    int chunk_begin() { return SLAM_OK; }
    DevMsg out() const { return {h->gate.dmeas, h->gate.dcount}; }
    template <class Mark>
    int filter(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int k_stride, Mark mark) {
        const size_t o = (size_t)t * B;
        int32_t* const di = h->inn.dint;
        return mark([&] {
            return gate_launch(h, c, cmd, d_each, dm, dc, k_stride, out(),
                               {h->inn.drec + (size_t)t * slam::kInnovRecLen, nis_sum ? h->inn.dlog + o : nullptr, nullptr, nullptr,
                                n_upd ? row(di, 0, cb, o) : nullptr, flags ? row(di, 1, cb, o) : nullptr, nullptr},
                               h->gate.drej + o, nullptr);
        });
    }
    template <class Mark> int after_step(int, int, Mark) { return SLAM_OK; }
    int chunk_done(int, int) { return SLAM_OK; }
    std::vector<TickRow> rows() const {
        return {{h->inn.drec, recs, slam::kInnovRecLen}, {h->inn.dlog, nis_sum, B}, {row(h->inn.dint, 0, cb), n_upd, B},
                {row(h->inn.dint, 1, cb), flags, B}, {h->gate.drej, n_rej, B}};
    }
    int finish() { return SLAM_OK; }
};

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
    return gate(h, true, cfg, cmds, cmd_each, meas, count, k_stride, meas_out, count_out, {rec, nis_sum, post, det, n_upd, flags, n_new}, n_rej, verdict);
}

int slam_gate_dev(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* d_meas, const int32_t* d_count,
                  int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post,
                  float* d_meas_out, int32_t* d_count_out, int32_t* n_rej, int32_t* verdict) {
    return gate(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out, {rec, nis_sum, post, det, n_upd, flags, n_new}, n_rej,
                verdict);
}

int slam_step_gated(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* meas, const int32_t* count, int k_stride,
                    double rec[16], int32_t* n_rej) {
    return step_gated(h, true, cfg, cmd, 0, meas, count, k_stride, rec, n_rej);
}

int slam_step_gated_dev(slam_handle* h, const slam_gate_config* cfg, const float cmd[2], const float* d_meas, const int32_t* d_count, int k_stride,
                        double rec[16], int32_t* n_rej) {
    return step_gated(h, false, cfg, cmd, 0, d_meas, d_count, k_stride, rec, n_rej);
}

int slam_step_gated_each(slam_handle* h, const slam_gate_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride,
                         double rec[16], int32_t* n_rej) {
    return step_gated(h, true, cfg, cmds, 1, meas, count, k_stride, rec, n_rej);
}

int slam_step_gated_each_dev(slam_handle* h, const slam_gate_config* cfg, const float* d_cmds, const float* d_meas, const int32_t* d_count,
                             int k_stride, double rec[16], int32_t* n_rej) {
    return step_gated(h, false, cfg, d_cmds, 1, d_meas, d_count, k_stride, rec, n_rej);
}

int slam_gate_run(slam_handle* h, const slam_gate_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                  int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags) {
    slam_gate_config c;
    TickMsgs msgs;
    TRY(gate_config(cfg, &c));
    TRY(run_args_log(cmds, meas, count, k_stride, T, &msgs));
    return run_filtered(h, "slam_gate_run", cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T,
                        GateTicks{h, c, recs, nis_sum, n_upd, n_rej, flags});
}

int slam_gate_run_sim(slam_handle* h, const slam_gate_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                      double* nis_sum, int32_t* n_upd, int32_t* n_rej, int32_t* flags, const slam_sense_log* log) {
    slam_gate_config c;
    TickCmds::Source csrc;
    TickMsgs msgs;
    TRY(gate_config(cfg, &c));
    TRY(run_args_sim(source, cmds, k_stride, T, log, &csrc, &msgs));
    return run_filtered(h, "slam_gate_run_sim", csrc, cmds, msgs, T, GateTicks{h, c, recs, nis_sum, n_upd, n_rej, flags});
}

int slam_last_gate_work(slam_handle* h, double* gate_ms, double* total_ms) {
    return last_work(h ? &h->gate.times : nullptr, "slam_gate_run", gate_ms, total_ms);
}

int slam_gate_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                            const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                            const slam_gate_config* cfg, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                            double* det, double* post, float* meas_out, int32_t* count_out, int32_t* n_rej, int32_t* verdict) {
    slam_gate_config c;
    InstanceHostArgs a;
    TRY(gate_config(cfg, &c));
    TRY(a.init(x, P, ids, M, L_max, cmd, meas, count, k_stride, true, noise, f32_storage));
    std::vector<slam::InnovWork> ws(1);
    int32_t rej = 0;
    const slam::InnovResult v = slam::gate_instance_host(ws[0], a.load_x, a.load_P, ids, M, L_max, status, cmd[0], cmd[1], meas, count, k_stride, a.nz,
                                                         lm_from_pred != 0, c.nis_lo, c.nis_hi, c.gate, det, meas_out, count_out, &rej, verdict);
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
