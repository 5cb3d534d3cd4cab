// capi_innovation.cpp — C ABI: innovation (NIS) statistics of the message the next step will process (innovation_kernel.hip), and the
// bodies of capi_filter.h
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_filter.h"
#include "ekf_kernel.h"
#include "host/noise_pack.h"

using namespace slam_capi;

namespace {

// *out = *cfg (NULL: the defaults), checked
int innovation_config(const slam_innovation_config* cfg, slam_innovation_config* out) {
    if (cfg) *out = *cfg; else slam_innovation_config_default(out);
    if (!isfinite(out->nis_lo) || !isfinite(out->nis_hi) || out->nis_lo > out->nis_hi)
        return slam_internal_fail(SLAM_ERR_ARG, "innovation config: the band nis_lo = %g .. nis_hi = %g must be finite and ordered", out->nis_lo, out->nis_hi);
    return SLAM_OK;
}

}  // namespace

namespace slam_capi {

int innovation_supported(const slam_handle* h) {
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "innovation statistics need EKF_SLAM: the innovation covariance of the UKF kinds depends on all sigma points, so no block of P closes");
    if (!h->cfg.landmark_id_is_known)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "innovation statistics need landmark_id_is_known = 1: the association of unknown ids reads every landmark of x_pred after every update");
    return SLAM_OK;
}

int innovation_reserve(slam_handle* h, bool det) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->inn.dval, (1 + 12 + slam::kInnovRecLen) * B));
    TRY(grow(h, h->inn.dpart, (size_t)slam::record_blocks(h->B) * slam::kInnovRecLen));
    if (det) TRY(grow(h, h->inn.ddet, B * slam::kInnovMaxDet * slam::kInnovDetLen));
    return SLAM_OK;
}

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

int innovation_outputs(slam_handle* h, bool det, InnovOut* d) {
    const size_t B = (size_t)h->B;
    TRY(innovation_reserve(h, det));
    TRY(grow(h, h->inn.drec, slam::kInnovRecLen));
    TRY(grow(h, h->inn.dint, 3 * B));
    *d = {h->inn.drec, h->inn.dval, h->inn.dval + B, det ? h->inn.ddet.get() : nullptr, h->inn.dint, h->inn.dint + B, h->inn.dint + 2 * B};
    return SLAM_OK;
}

int innovation_download(slam_handle* h, const InnovOut& d, const InnovOut& to) {
    const size_t B = (size_t)h->B;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{d.rec, to.rec, slam::kInnovRecLen}, {d.nis_sum, to.nis_sum, B}, {d.post, to.post, 12 * B},
                      {d.det, to.det, B * slam::kInnovMaxDet * slam::kInnovDetLen}, {d.n_upd, to.n_upd, B}, {d.flags, to.flags, B},
                      {d.n_new, to.n_new, B}}, 0, 1);
}

int innovation_upload_cmds(slam_handle* h, const float* cmds, size_t n) {
    TRY(grow(h, h->inn.dcmd, n));
    HIP_TRY(hipMemcpyAsync(h->inn.dcmd, cmds, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

int upload_messages(slam_handle* h, const float* meas, const int32_t* count, int k_stride, size_t ticks) {
    const size_t nc = ticks * h->B, nm = 3 * (size_t)k_stride * nc;
    TRY(grow(h, h->inn.dmeas, nm));
    TRY(grow(h, h->inn.dcount, nc));
    HIP_TRY(hipMemcpyAsync(h->inn.dmeas, meas, sizeof(float) * nm, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->inn.dcount, count, sizeof(int32_t) * nc, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

// ---- capi_filter.h --------------------------------------------------------------------------------------------------------------------------
int copy_rows(const std::vector<TickRow>& rows, int t0, int tc) {
    for (const TickRow& r : rows) {
        const size_t tick = r.per_tick * r.elem_bytes;
        if (r.host) HIP_TRY(hipMemcpy((char*)r.host + (size_t)t0 * tick, r.dev, (size_t)tc * tick, hipMemcpyDeviceToHost));
    }
    return SLAM_OK;
}

int message_args(const float* cmds, const void* meas, const void* count, int k_stride, const void* meas_out, const void* count_out, bool need_out) {
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (need_out && (!meas_out || !count_out)) return slam_internal_fail(SLAM_ERR_ARG, "d_meas_out or d_count_out is NULL");
    if ((meas_out == meas) != (count_out == count))
        return slam_internal_fail(SLAM_ERR_ARG, "in place means both: meas_out == meas and count_out == meas_count, or neither");
    return SLAM_OK;
}

bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb) {
    const char* const pa = (const char*)a; const char* const pb = (const char*)b;
    return pa < pb + nb && pb < pa + na;
}

int out_message_overlaps(const slam_handle* h, const float* d_meas, const int32_t* d_count, int k_stride, DevMsg out) {
    const size_t bm = sizeof(float) * 3 * (size_t)k_stride * h->B, bc = sizeof(int32_t) * (size_t)h->B;
    if ((out.meas != d_meas && ranges_overlap(out.meas, bm, d_meas, bm)) || (out.count != d_count && ranges_overlap(out.count, bc, d_count, bc)) ||
        ranges_overlap(out.meas, bm, d_count, bc) || ranges_overlap(out.count, bc, d_meas, bm) || ranges_overlap(out.meas, bm, out.count, bc))
        return slam_internal_fail(SLAM_ERR_ARG, "the output message overlaps the input (only d_meas_out == d_meas with d_count_out == d_count is allowed) or itself");
    return SLAM_OK;
}

int filter_enter(slam_handle* h, int (*supported)(const slam_handle*)) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(supported(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

int step_state(const slam_handle* h, const char* who) {
    if (h->shadow) return slam_internal_fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
    return SLAM_OK;
}

int stage_message(slam_handle* h, bool host, const float* cmds, int cmd_each, const float** meas, const int32_t** count, int k_stride,
                  const float** cmd, const float** d_each) {
    *cmd = cmd_each ? kNoCmd : cmds; *d_each = cmd_each ? cmds : nullptr;
    if (!host) return SLAM_OK;
    TRY(upload_messages(h, *meas, *count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * (size_t)h->B));
    *meas = h->inn.dmeas; *count = h->inn.dcount;
    if (cmd_each) *d_each = h->inn.dcmd;
    return SLAM_OK;
}

int seed_out_message(slam_handle* h, float* d_meas_out, int k_stride) {
    HIP_TRY(hipMemcpyAsync(d_meas_out, h->inn.dmeas, sizeof(float) * 3 * (size_t)k_stride * h->B, hipMemcpyDeviceToDevice, h->stream));
    return SLAM_OK;
}

int step_outputs(slam_handle* h, double* rec, const int32_t* d_n, int32_t* n) {
    if (!rec && !n) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{h->inn.drec, rec, slam::kInnovRecLen}, {d_n, n, (size_t)h->B}}, 0, 1);
}

int run_args_log(const float* cmds, const float* meas, const int32_t* count, int k_stride, int T, TickMsgs* msgs) {
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    TRY(message_args(cmds, meas, count, k_stride));
    msgs->init_log(meas, count, k_stride);
    return SLAM_OK;
}

int run_args_sim(int source, const float* cmds, int k_stride, int T, const slam_sense_log* log, TickCmds::Source* csrc, TickMsgs* msgs) {
    TRY(sim_run_source(source, cmds, csrc));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    msgs->init_sim(log, k_stride);
    return SLAM_OK;
}

int InstanceHostArgs::init(const double* x, const double* P, const int32_t* ids, int M, int L_max, const float cmd[2], const float* meas, int count,
                           int k_stride, bool strided, const slam_noise* noise, int f32_storage) {
    if (!x || !P || !cmd || !noise) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (strided && k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (strided && count > 0 && !meas) return slam_internal_fail(SLAM_ERR_ARG, "meas is NULL");
    if (!strided && (count < 0 || (count > 0 && !meas))) return slam_internal_fail(SLAM_ERR_ARG, "k = %d is negative, or meas is NULL", count);
    if (const char* f = slam_host::noise_bad_field(*noise)) return slam_internal_fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
    nz = {noise->v_d, noise->v_th, noise->w_r, noise->w_b, noise->V_00, noise->V_11, noise->W_00, noise->W_11};
    load_x = {x, f32_storage != 0};
    load_P = {P, 3 + 2 * M, f32_storage != 0};
    return SLAM_OK;
}

}  // namespace slam_capi

namespace {

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

// slam_innovation (host: the message and per-instance commands are host arrays) and slam_innovation_dev
int innovation(slam_handle* h, bool host, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* meas,
               const int32_t* count, int k_stride, const InnovOut& to) {
    slam_innovation_config c;
    const float *cmd, *d_each;
    TRY(innovation_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride));
    TRY(filter_enter(h, innovation_supported));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    return innovation_now(h, c, cmd, d_each, meas, count, k_stride, to);
}

}  // namespace

extern "C" {

int slam_innovation_config_default(slam_innovation_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->nis_lo = -2.0 * log(0.975); c->nis_hi = -2.0 * log(0.025);   // chi-square quantiles at 0.025 and 0.975, 2 degrees of freedom
    return SLAM_OK;
}

int slam_innovation(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                    int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags, double* det, double* post) {
    return innovation(h, true, cfg, cmds, cmd_each, meas, count, k_stride, {rec, nis_sum, post, det, n_upd, flags, n_new});
}

int slam_innovation_dev(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                        const int32_t* d_count, int k_stride, double rec[16], double* nis_sum, int32_t* n_upd, int32_t* n_new, int32_t* flags,
                        double* det, double* post) {
    return innovation(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, {rec, nis_sum, post, det, n_upd, flags, n_new});
}

int slam_innovation_run(slam_handle* h, const slam_innovation_config* cfg, int source, const float* cmds, const float* meas, const int32_t* count,
                        int k_stride, int T, double* recs, double* nis_sum, int32_t* n_upd, int32_t* flags) {
    slam_innovation_config c;
    TRY(innovation_config(cfg, &c));
    if (source != SLAM_INNOVATION_SHARED && source != SLAM_INNOVATION_EACH && source != SLAM_INNOVATION_NAV && source != SLAM_INNOVATION_LOG)
        return slam_internal_fail(SLAM_ERR_ARG, "unknown source %d", source);
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (source != SLAM_INNOVATION_NAV && !cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL: the sources SHARED, EACH and LOG read the commands from it");
    const bool log = source == SLAM_INNOVATION_LOG;
    if (log && (!meas || !count)) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL: the source LOG reads the messages from them");
    if (log && k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
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
            return copy_rows({{h->inn.drec, recs, slam::kInnovRecLen}, {h->inn.dlog, nis_sum, B}, {d_upd, n_upd, B}, {d_flags, flags, B}}, t0, tc);
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
    InstanceHostArgs a;
    TRY(a.init(x, P, ids, M, L_max, cmd, meas, k, 0, false, noise, f32_storage));
    std::vector<slam::InnovWork> ws(1);
    for (int i = 0; i < 3 * (k < slam::kInnovMaxDet ? k : slam::kInnovMaxDet); ++i) ws[0].meas[i] = meas[i];
    const slam::InnovResult v = slam::innovation_instance(slam::InnovSeq(), ws[0], a.load_x, a.load_P, ids, M, L_max, status, cmd[0], cmd[1], k, a.nz,
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
