// capi_sense.cpp — C ABI: the simulator source with a sensor fault model (sense_kernel.hip): slam_set_sensor_each, slam_sense*,
// slam_sense_commit, the message source of the *_run_sim calls (TickMsgs, capi_run.h) and the host hook
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_filter.h"
#include "capi_sense.h"
#include "ekf_kernel.h"
#include "sense_kernel.h"

using namespace slam_capi;

namespace {

// the checks slam_sense and slam_sense_dev share, arguments first; the queued timesteps run first
int sense_enter(slam_handle* h, const float* cmds, const void* meas, const void* count, int k_stride, const char* who) {
    TRY(message_args(cmds, meas, count, k_stride));
    return run_enter(h, who, true, false, true);
}

size_t msg_row(const slam_handle* h, int k_stride) { return 3 * (size_t)k_stride * h->B; }

}  // namespace

namespace slam_capi {

int sense_reserve(slam_handle* h) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->sense.dnext, 3 * B));
    TRY(grow(h, h->sense.dstaged, B));
    TRY(grow(h, h->sense.dinst, B * slam::kSenseRecLen));
    TRY(grow(h, h->sense.dpart, (size_t)slam::record_blocks(h->B) * slam::kSenseRecLen));
    TRY(grow(h, h->sense.drec, slam::kSenseRecLen));
    return SLAM_OK;
}

int sense_launch(slam_handle* h, const float cmd[2], const float* d_cmd_each, float* d_meas, int32_t* d_count, int k_stride, int32_t* d_origin,
                 int32_t* d_fault, double* d_rec) {
    slam::SenseParams p;
    memset(&p, 0, sizeof(p));
    fill_ekf_params(h, p.s, cmd, 1, 0, nullptr, nullptr, 0, nullptr, 0, d_cmd_each);
    p.rows = h->sense.rows_set ? h->sense.drows.get() : nullptr;
    p.meas_out = d_meas; p.count_out = d_count; p.k_stride = k_stride; p.origin = d_origin; p.fault = d_fault;
    p.truth_next = h->sense.dnext; p.staged_ts = h->sense.dstaged;
    p.inst_rec = h->sense.dinst; p.partials = h->sense.dpart; p.rec = d_rec;
    HIP_TRY(slam::launch_sense(p, h->stream));
    return SLAM_OK;
}

int sense_commit_launch(slam_handle* h, double* d_err_pos, double* d_truth_out, double* d_rec) {
    slam::SenseCommitParams p;
    memset(&p, 0, sizeof(p));
    p.x = h->dx; p.xstride = h->xstride; p.f32_storage = h->esz == 4; p.B = h->B;
    p.timestep = h->dts; p.staged_ts = h->sense.dstaged;
    p.truth = h->dtruth; p.truth_next = h->sense.dnext; p.err_sum = h->derr;
    p.err_pos = d_err_pos; p.truth_out = d_truth_out;
    p.inst_rec = h->sense.dinst; p.partials = h->sense.dpart; p.rec = d_rec;
    HIP_TRY(slam::launch_sense_commit(p, h->stream));
    return SLAM_OK;
}

int sim_run_source(int source, const float* cmds, TickCmds::Source* out) {
    if (source == SLAM_INNOVATION_LOG) return slam_internal_fail(SLAM_ERR_ARG, "source LOG: the messages of a _sim run come from the simulator, use the run without _sim");
    if (source != SLAM_INNOVATION_SHARED && source != SLAM_INNOVATION_EACH && source != SLAM_INNOVATION_NAV)
        return slam_internal_fail(SLAM_ERR_ARG, "unknown source %d", source);
    if (source != SLAM_INNOVATION_NAV && !cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL: the sources SHARED and EACH read the commands from it");
    *out = source == SLAM_INNOVATION_EACH ? TickCmds::kEach : source == SLAM_INNOVATION_NAV ? TickCmds::kNav : TickCmds::kShared;
    return SLAM_OK;
}

// ---- TickMsgs (capi_run.h) ------------------------------------------------------------------------------------------------------------------
double TickMsgs::bytes_per_tick(const slam_handle* h, const TickCmds& tcmd) const {
    const double B = (double)h->B, ks = (double)k_stride;
    if (src == kLog) return 4.0 * 3.0 * ks * B + 4.0 * B;
    const bool msg = log.meas || log.count;   // (not logged: one row serves every tick; the commands of SHARED and EACH are the caller's own)
    return (msg ? 4.0 * 3.0 * ks * B + 4.0 * B : 0.0) + 4.0 * ks * B * ((log.origin ? 1 : 0) + (log.fault ? 1 : 0)) + (log.truth ? 24.0 * B : 0.0) +
           (log.err_pos ? 8.0 * B : 0.0) + (log.cmds && tcmd.src == TickCmds::kNav ? 8.0 * B : 0.0) + (log.recs ? 8.0 * slam::kSenseRecLen : 0.0);
}

int TickMsgs::reserve(slam_handle* h, const TickCmds& tcmd, int ticks) {
    chunk = ticks;
    if (src == kLog) return SLAM_OK;
    const size_t B = (size_t)h->B, n = (size_t)ticks, rows = (log.meas || log.count) ? n : 1;
    TRY(sense_reserve(h));
    TRY(grow(h, h->sense.dmeas, rows * msg_row(h, k_stride)));
    TRY(grow(h, h->sense.dcount, rows * B));
    if (log.origin) TRY(grow(h, h->sense.dorigin, n * (size_t)k_stride * B));
    if (log.fault) TRY(grow(h, h->sense.dfault, n * (size_t)k_stride * B));
    if (log.truth) TRY(grow(h, h->sense.dtruth, n * 3 * B));
    if (log.err_pos) TRY(grow(h, h->sense.derrpos, n * B));
    if (log.cmds && tcmd.src == TickCmds::kNav) TRY(grow(h, h->sense.dcmd, n * 2 * B));
    if (log.recs) TRY(grow(h, h->sense.drecs, n * slam::kSenseRecLen));
    return SLAM_OK;
}

int TickMsgs::upload(slam_handle* h, int t0, int tc) const {
    if (src == kSim) return SLAM_OK;
    return upload_messages(h, meas + (size_t)t0 * msg_row(h, k_stride), count + (size_t)t0 * h->B, k_stride, (size_t)tc);
}

int TickMsgs::produce(slam_handle* h, const TickCmds& tcmd, int t, const float cmd[2], const float* d_each, const float** d_meas,
                      const int32_t** d_count) {
    const size_t B = (size_t)h->B, mrow = msg_row(h, k_stride);
    if (src == kLog) {
        *d_meas = h->inn.dmeas + (size_t)t * mrow; *d_count = h->inn.dcount + (size_t)t * B;
        return SLAM_OK;
    }
    const size_t row = (log.meas || log.count) ? (size_t)t : 0, lrow = (size_t)t * k_stride * B;
    float* const m = h->sense.dmeas + row * mrow;
    int32_t* const c = h->sense.dcount + row * B;
    if (log.cmds && tcmd.src == TickCmds::kNav)   // (the controller's row is overwritten by the next tick; SHARED and EACH are the caller's own)
        HIP_TRY(hipMemcpyAsync(h->sense.dcmd + (size_t)t * 2 * B, d_each, sizeof(float) * 2 * B, hipMemcpyDeviceToDevice, h->stream));
    TRY(sense_launch(h, cmd, d_each, m, c, k_stride, log.origin ? h->sense.dorigin + lrow : nullptr, log.fault ? h->sense.dfault + lrow : nullptr,
                     nullptr));
    *d_meas = m; *d_count = c;
    return SLAM_OK;
}

int TickMsgs::commit(slam_handle* h, int t) {
    if (src == kLog) return SLAM_OK;
    const size_t B = (size_t)h->B;
    return sense_commit_launch(h, log.err_pos ? h->sense.derrpos + (size_t)t * B : nullptr, log.truth ? h->sense.dtruth + (size_t)t * 3 * B : nullptr,
                               log.recs ? h->sense.drecs + (size_t)t * slam::kSenseRecLen : nullptr);
}

int TickMsgs::download(slam_handle* h, const TickCmds& tcmd, int t0, int tc) const {
    if (src == kLog) return SLAM_OK;
    const size_t B = (size_t)h->B, n = (size_t)tc, o = (size_t)t0, mrow = msg_row(h, k_stride), lrow = (size_t)k_stride * B;
    TRY(copy_rows({{h->sense.dmeas, log.meas, mrow}, {h->sense.dcount, log.count, B}, {h->sense.dorigin, log.origin, lrow},
                   {h->sense.dfault, log.fault, lrow}, {h->sense.dtruth, log.truth, 3 * B}, {h->sense.derrpos, log.err_pos, B},
                   {h->sense.drecs, log.recs, slam::kSenseRecLen}}, t0, tc));
    if (log.cmds) {
        float* const dst = log.cmds + o * 2 * B;
        if (tcmd.src == TickCmds::kNav) HIP_TRY(hipMemcpy(dst, h->sense.dcmd, sizeof(float) * n * 2 * B, hipMemcpyDeviceToHost));
        else if (tcmd.src == TickCmds::kEach) memcpy(dst, tcmd.cmds + o * 2 * B, sizeof(float) * n * 2 * B);
        else
            for (size_t t = 0; t < n; ++t)
                for (size_t b = 0; b < B; ++b) { dst[(t * B + b) * 2] = tcmd.cmds[2 * (o + t)]; dst[(t * B + b) * 2 + 1] = tcmd.cmds[2 * (o + t) + 1]; }
    }
    return SLAM_OK;
}

}  // namespace slam_capi

extern "C" {

int slam_sensor_default(slam_sensor* row) {
    if (!row) return slam_internal_fail(SLAM_ERR_ARG, "row is NULL");
    memset(row, 0, sizeof(*row));
    return SLAM_OK;
}

int slam_set_sensor_each(slam_handle* h, const slam_sensor* rows) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    const size_t B = (size_t)h->B;
    for (size_t b = 0; rows && b < B; ++b)
        if (const char* f = slam::sense_bad_field(rows[b], h->range_max))
            return slam_internal_fail(SLAM_ERR_ARG, "instance %zu: sensor field %s is out of range (probabilities in [0, 1], spike_lo <= spike_hi finite, n_clutter in 0 .. %d, 0 <= clutter_r_min <= range_max = %g)",
                                      b, f, slam::kSenseMaxClutter, h->range_max);
    TRY(flush_lazy(h));   // the timesteps accepted so far keep the values they were accepted with
    HIP_TRY(hipSetDevice(h->device));
    if (!rows) {
        h->sense.rows_set = false;   // (the launches in flight keep reading drows: it stays allocated)
        return SLAM_OK;
    }
    if (h->sense.drows.cap() < B) {   // the new block first: a failure leaves the handle with the rows it had
        DevBuf<slam_sensor> d;
        HIP_TRY(d.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->sense.drows = std::move(d);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old rows are done
    }
    HIP_TRY(hipMemcpyAsync(h->sense.drows, rows, sizeof(slam_sensor) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->sense.rows_set = true;
    return SLAM_OK;
}

int slam_sense_dev(slam_handle* h, const float* cmds, int cmd_each, float* d_meas, int32_t* d_count, int k_stride, int32_t* d_origin,
                   int32_t* d_fault) {
    TRY(sense_enter(h, cmds, d_meas, d_count, k_stride, "slam_sense_dev"));
    HIP_TRY(hipSetDevice(h->device));
    TRY(sense_reserve(h));
    TRY(sense_launch(h, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, d_origin, d_fault, nullptr));
    h->sense.pending = true; h->sense.pending_step = h->step;
    return SLAM_OK;
}

int slam_sense(slam_handle* h, const float* cmds, int cmd_each, float* meas, int32_t* count, int k_stride, int32_t* origin, int32_t* fault,
               double* truth_next, double rec[16]) {
    TRY(sense_enter(h, cmds, meas, count, k_stride, "slam_sense"));
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B, mrow = msg_row(h, k_stride), lrow = (size_t)k_stride * B;
    TRY(sense_reserve(h));
    TRY(grow(h, h->sense.dmeas, mrow));
    TRY(grow(h, h->sense.dcount, B));
    if (origin) TRY(grow(h, h->sense.dorigin, lrow));
    if (fault) TRY(grow(h, h->sense.dfault, lrow));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * B));
    TRY(sense_launch(h, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->sense.dmeas, h->sense.dcount, k_stride,
                     origin ? h->sense.dorigin.get() : nullptr, fault ? h->sense.dfault.get() : nullptr, rec ? h->sense.drec.get() : nullptr));
    h->sense.pending = true; h->sense.pending_step = h->step;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(meas, h->sense.dmeas, sizeof(float) * mrow, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, h->sense.dcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (origin) HIP_TRY(hipMemcpy(origin, h->sense.dorigin, sizeof(int32_t) * lrow, hipMemcpyDeviceToHost));
    if (fault) HIP_TRY(hipMemcpy(fault, h->sense.dfault, sizeof(int32_t) * lrow, hipMemcpyDeviceToHost));
    if (truth_next) HIP_TRY(hipMemcpy(truth_next, h->sense.dnext, sizeof(double) * 3 * B, hipMemcpyDeviceToHost));
    if (rec) HIP_TRY(hipMemcpy(rec, h->sense.drec, sizeof(double) * slam::kSenseRecLen, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_sense_commit(slam_handle* h, double rec[16]) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(innovation_supported(h));
    if (!h->sense.pending) return slam_internal_fail(SLAM_ERR_STATE, "no sense is pending: slam_sense or slam_sense_dev comes first");
    TRY(flush_lazy(h));   // the caller's step, if it was queued
    HIP_TRY(hipSetDevice(h->device));
    TRY(sense_commit_launch(h, nullptr, nullptr, rec ? h->sense.drec.get() : nullptr));
    h->step = h->sense.pending_step + 1;   // one tick of the simulator, however many step calls ran on its message
    h->sense.pending = false;
    if (!rec) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(rec, h->sense.drec, sizeof(double) * slam::kSenseRecLen, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_sense_instance_host(uint64_t seed, int64_t instance, uint32_t step, const double truth[3], const float cmd[2], int32_t status,
                             const double* map_xy, int L, double d_max, double th_max, double range_max, double fov_min, double fov_max,
                             const double sim_noise[4], const slam_sensor* row, int k_stride, float* meas, int32_t* count, int32_t* origin,
                             int32_t* fault, double truth_next[3], int32_t* flags, double rec[16]) {
    if (!truth || !cmd || !map_xy || !sim_noise || !meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L <= 0) return slam_internal_fail(SLAM_ERR_ARG, "L = %d is not positive", L);
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    const slam_sensor r = row ? *row : slam::sense_default_row();
    if (const char* f = slam::sense_bad_field(r, range_max))
        return slam_internal_fail(SLAM_ERR_ARG, "sensor field %s is out of range (probabilities in [0, 1], spike_lo <= spike_hi finite, n_clutter in 0 .. %d, 0 <= clutter_r_min <= range_max = %g)",
                                  f, slam::kSenseMaxClutter, range_max);
    const slam::SenseSim sc = {seed, (uint64_t)instance, d_max, th_max, range_max, fov_min, fov_max, sim_noise[0], sim_noise[1], sim_noise[2], sim_noise[3]};
    std::vector<slam::SenseWork> ws(1);
    double tx = truth[0], ty = truth[1], tth = truth[2];
    slam::SenseResult v;
    const slam::InnovSeq w;
    if (status & slam::kInnovStatusFrozen) {
        v = slam::sense_frozen(w, k_stride, meas, origin, fault);
    } else {
        const int c_vis = slam::sense_clean_seq(sc, cmd[0], cmd[1], step, map_xy, L, tx, ty, tth, ws[0].meas);
        v = slam::sense_instance(w, ws[0], r, seed, (uint64_t)instance, step, c_vis, L, range_max, fov_min, fov_max, k_stride, meas, origin, fault);
    }
    *count = v.count;
    if (flags) *flags = v.flags;
    if (truth_next) { truth_next[0] = tx; truth_next[1] = ty; truth_next[2] = tth; }
    if (rec) slam::sense_record(v, k_stride, rec);
    return SLAM_OK;
}

}  // extern "C"
