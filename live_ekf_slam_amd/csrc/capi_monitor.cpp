// capi_monitor.cpp — C ABI: the run monitor, per-tick error and pose-NEES records (monitor_kernel.hip)
#include <math.h>
#include <string.h>

#include "capi_run.h"
#include "consistency_kernel.h"
#include "host/tick_chunks.h"
#include "monitor_kernel.h"

using namespace slam_capi;

namespace {

// *out = *cfg (NULL: the defaults), checked
int monitor_config(const slam_monitor_config* cfg, slam_monitor_config* out) {
    if (cfg) *out = *cfg; else slam_monitor_config_default(out);
    if (!isfinite(out->nees_lo) || !isfinite(out->nees_hi) || out->nees_lo > out->nees_hi)
        return slam_internal_fail(SLAM_ERR_ARG, "monitor config: the band nees_lo = %g .. nees_hi = %g must be finite and ordered", out->nees_lo, out->nees_hi);
    if (out->full_every < 0) return slam_internal_fail(SLAM_ERR_ARG, "monitor config: full_every = %d is negative", out->full_every);
    return SLAM_OK;
}

int monitor_full_supported(const slam_handle* h, const slam_monitor_config& c) {
    if (c.full_every != 0 && h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "monitor config: full_every = %d needs EKF_SLAM (slam_consistency is not defined for the UKF kinds); full_every = 0 runs", c.full_every);
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
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->nees_lo = 0.21579528262389785; c->nees_hi = 9.348403604496148;   // chi-square quantiles at 0.025 and 0.975, 3 degrees of freedom
    c->full_every = 0;
    return SLAM_OK;
}

int slam_monitor_now(slam_handle* h, const slam_monitor_config* cfg, double rec[16], double* err_pos, double* err_yaw, double* nees_pose, int32_t* flags) {
    slam_monitor_config c;
    TRY(monitor_config(cfg, &c));
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(monitor_full_supported(h, c));
    TRY(flush_lazy(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (!has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "no true map, so no simulated truth to compare with: call slam_set_map (or slam_set_maps) first");
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->mon.dpart, (size_t)slam::record_blocks(h->B) * slam::kMonRecLen));
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
    if (source != SLAM_MONITOR_SHARED && source != SLAM_MONITOR_EACH && source != SLAM_MONITOR_NAV) return slam_internal_fail(SLAM_ERR_ARG, "unknown command source %d", source);
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (source != SLAM_MONITOR_NAV && !cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL: the sources SHARED and EACH read the commands from it");
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
    TRY(grow(h, h->mon.dpart, (size_t)slam::record_blocks(h->B) * slam::kMonRecLen));
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
    if (filter_kind != SLAM_EKF_SLAM && filter_kind != SLAM_UKF_SLAM && filter_kind != SLAM_UKF_LOC) return slam_internal_fail(SLAM_ERR_ARG, "unknown filter kind %d", filter_kind);
    const bool ukf = filter_kind != SLAM_EKF_SLAM;
    if (!x || !truth || (!ukf && !P3)) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    const double zero[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    const slam::MonitorValue v = slam::monitor_instance(x, ukf ? zero : P3, truth, status, ukf);
    if (err_pos) *err_pos = v.err_pos;
    if (err_yaw) *err_yaw = v.err_yaw;
    if (nees_pose) *nees_pose = v.nees_pose;
    if (flags) *flags = v.flags;
    return SLAM_OK;
}

}  // extern "C"
