// capi_innovation.cpp — C ABI: innovation (NIS) statistics of the message the next step will process (innovation_kernel.hip)
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_innovation.h"
#include "capi_run.h"
#include "ekf_kernel.h"
#include "host/noise_pack.h"
#include "host/tick_chunks.h"

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
    TRY(grow(h, h->inn.dpart, (size_t)slam::innovation_blocks(h->B) * slam::kInnovRecLen));
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
    if (to.rec) HIP_TRY(hipMemcpy(to.rec, d.rec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (to.nis_sum) HIP_TRY(hipMemcpy(to.nis_sum, d.nis_sum, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (to.post) HIP_TRY(hipMemcpy(to.post, d.post, sizeof(double) * 12 * B, hipMemcpyDeviceToHost));
    if (to.det) HIP_TRY(hipMemcpy(to.det, d.det, sizeof(double) * B * slam::kInnovMaxDet * slam::kInnovDetLen, hipMemcpyDeviceToHost));
    if (to.n_upd) HIP_TRY(hipMemcpy(to.n_upd, d.n_upd, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.flags) HIP_TRY(hipMemcpy(to.flags, d.flags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_new) HIP_TRY(hipMemcpy(to.n_new, d.n_new, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
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

// the checks slam_innovation and slam_innovation_dev share; the queued timesteps run first
int innovation_enter(slam_handle* h, const slam_innovation_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride,
                     slam_innovation_config* c) {
    TRY(innovation_config(cfg, c));
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
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
    if (!x || !P || !cmd || !noise) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (k < 0 || (k > 0 && !meas)) return slam_internal_fail(SLAM_ERR_ARG, "k = %d is negative, or meas is NULL", k);
    if (const char* f = slam_host::noise_bad_field(*noise)) return slam_internal_fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
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
