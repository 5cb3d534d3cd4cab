// capi_nav.cpp — C ABI: closed loop, pure-pursuit commands from each instance's estimate (nav_kernel.hip), and the definitions of what
// the per-tick runs share (capi_run.h)
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "capi_run.h"
#include "host/config_parse.h"
#include "host/tick_chunks.h"
#include "slam_math.h"

using namespace slam_capi;

int slam_capi::nav_reset(slam_handle* h) {
    if (!h->nav.set) return SLAM_OK;
    const size_t B = (size_t)h->B;
    HIP_TRY(hipMemsetAsync(h->nav.dhead, 0, sizeof(int32_t) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.dfinish, 0xff, sizeof(int32_t) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.dinteg, 0, sizeof(double) * B, h->stream));
    HIP_TRY(hipMemsetAsync(h->nav.derrp, 0, sizeof(double) * B, h->stream));
    h->nav.tick = 0;
    return SLAM_OK;
}

namespace {

int nav_check_config(const slam_nav_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "nav config is NULL");
    if (!(c->dt > 0.0) || !isfinite(c->dt)) return slam_internal_fail(SLAM_ERR_ARG, "nav config: dt = %g must be positive and finite", c->dt);
    if (!(c->lookahead_dist_init > 0.0) || !isfinite(c->lookahead_dist_init) || !(c->lookahead_dist_max > 0.0) || !isfinite(c->lookahead_dist_max))
        return slam_internal_fail(SLAM_ERR_ARG, "nav config: lookahead distances %g .. %g must be positive and finite", c->lookahead_dist_init, c->lookahead_dist_max);
    int radii = 0;
    for (double d = c->lookahead_dist_init; d <= c->lookahead_dist_max; d *= 1.25)
        if (++radii > slam::kNavMaxRadii) return slam_internal_fail(SLAM_ERR_ARG, "nav config: more than %d lookahead radii between %g and %g", slam::kNavMaxRadii, c->lookahead_dist_init, c->lookahead_dist_max);
    if (c->method != SLAM_NAV_PP && c->method != SLAM_NAV_DIRECT) return slam_internal_fail(SLAM_ERR_ARG, "nav config: unknown method %d", c->method);
    if (c->control != SLAM_NAV_LOOSE && c->control != SLAM_NAV_TIGHT) return slam_internal_fail(SLAM_ERR_ARG, "nav config: unknown control %d", c->control);
    return SLAM_OK;
}

// one path of P points: finite, 1 <= P <= cap, no two consecutive waypoints equal (choose_lookahead_pt would divide by a = 0)
int nav_check_path(const double* pts, int P, long long inst) {
    if (P < 1 || P > slam::kNavMaxWaypoints) return slam_internal_fail(SLAM_ERR_ARG, "path of %d waypoints (instance %lld): 1 .. %d are supported", P, inst, slam::kNavMaxWaypoints);
    for (int i = 0; i < P; ++i) {
        if (!isfinite(pts[2 * i]) || !isfinite(pts[2 * i + 1])) return slam_internal_fail(SLAM_ERR_ARG, "waypoint %d (instance %lld) is not finite", i, inst);
        if (i > 0 && pts[2 * i] == pts[2 * i - 2] && pts[2 * i + 1] == pts[2 * i - 1])
            return slam_internal_fail(SLAM_ERR_ARG, "waypoints %d and %d (instance %lld) are equal: the reference divides by zero there (pure_pursuit.py:124)", i - 1, i, inst);
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

}  // namespace

// ---- per-tick runs: the definitions of capi_run.h -------------------------------------------------------------------------------------------
namespace slam_capi {

int nav_params(slam_handle* h, slam::NavParams* out) {
    TRY(grow(h, h->each.dcmd_each, 2 * (size_t)h->B));
    slam::NavParams p;
    memset(&p, 0, sizeof(p));
    p.x = h->dx; p.flags = h->dflags; p.path = h->nav.dpath;
    p.P_each = h->nav.each ? h->nav.dP.get() : nullptr; p.P = h->nav.P; p.path_stride = h->nav.stride;
    p.B = h->B; p.xstride = h->xstride; p.ukf = h->kind != SLAM_EKF_SLAM;
    p.c = nav_consts(h->nav.cfg, h->cfg.d_max, h->cfg.th_max);
    p.head = h->nav.dhead; p.finish_tick = h->nav.dfinish; p.integ = h->nav.dinteg; p.err_prev = h->nav.derrp;
    p.cmd_out = h->each.dcmd_each;
    *out = p;
    return SLAM_OK;
}

int nav_launch(slam_handle* h, slam::NavParams& p) {
    p.tick = h->nav.tick;
    HIP_TRY(slam::launch_nav_tick(p, h->esz == 4, h->stream));
    h->nav.tick += 1;
    return SLAM_OK;
}

int run_enter(slam_handle* h, const char* who, bool runs_simulator, bool need_path, bool ekf_known_ids) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "%s: NULL handle", who);
    if (ekf_known_ids) TRY(innovation_supported(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "%s: slam_init has not been called", who);
    if (runs_simulator && !has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "%s runs the simulator: slam_set_map (or slam_set_maps) has not been called", who);
    if (need_path && !h->nav.set) return slam_internal_fail(SLAM_ERR_STATE, "%s: no path: call slam_nav_set_path or slam_nav_set_paths first", who);
    if (h->shadow) return slam_internal_fail(SLAM_ERR_STATE, "slam_track_instance is on: %s does not drive the shadow filter", who);
    // (checked before the first launch: a controller tick would overwrite the commands the pending update stage reads)
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev before %s", who);
    if (runs_simulator) TRY(sense_idle(h, who));   // (the truth it would advance is staged)
    return flush_lazy(h);
}

int last_work(const RunTimes* t, const char* run, double* part_ms, double* total_ms) {
    if (!t) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (t->total_ms < 0.0) return slam_internal_fail(SLAM_ERR_STATE, "%s has not run on this handle", run);
    if (part_ms) *part_ms = t->part_ms;
    if (total_ms) *total_ms = t->total_ms;
    return SLAM_OK;
}

}  // namespace slam_capi

extern "C" {

int slam_nav_config_default(slam_nav_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->dt = 0.05;                                                  // params.yaml:14
    c->lookahead_dist_init = 0.2; c->lookahead_dist_max = 2.0;     // params.yaml:83-84
    c->method = SLAM_NAV_PP; c->control = SLAM_NAV_LOOSE;          // params.yaml:81; sim_base.launch tight_control false
    return SLAM_OK;
}

int slam_nav_config_load(slam_nav_config* c, const char* path) {
    if (!c || !path) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    FILE* f = fopen(path, "r");
    if (!f) return slam_internal_fail(SLAM_ERR_IO, "cannot open %s", path);
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
        if (top && slam_host::parse_scalar(line, "dt", &v)) { if (isfinite(v)) c->dt = v; else rc = slam_internal_fail(SLAM_ERR_IO, "value of dt is not finite"); }
        else if (slam_host::parse_scalar(line, "lookahead_dist_init", &v)) { if (isfinite(v)) c->lookahead_dist_init = v; else rc = slam_internal_fail(SLAM_ERR_IO, "value of lookahead_dist_init is not finite"); }
        else if (slam_host::parse_scalar(line, "lookahead_dist_max", &v)) { if (isfinite(v)) c->lookahead_dist_max = v; else rc = slam_internal_fail(SLAM_ERR_IO, "value of lookahead_dist_max is not finite"); }
        else {
            const char* q = line;
            while (*q == ' ' || *q == '\t') ++q;
            if (strncmp(q, "nav_method:", 11) == 0) {
                char word[32] = "";
                sscanf(q + 11, " %*[\"']%31[A-Za-z_]", word);
                if (!word[0]) sscanf(q + 11, " %31[A-Za-z_]", word);
                if (strcmp(word, "pp") == 0) c->method = SLAM_NAV_PP;
                else if (strcmp(word, "direct") == 0 || strcmp(word, "simple") == 0) c->method = SLAM_NAV_DIRECT;
                else rc = slam_internal_fail(SLAM_ERR_IO, "nav_method \"%s\" is none of pp, direct, simple (goal_pursuit_node.py:45-53)", word);
            }
        }
    }
    fclose(f);
    return rc;
}

int slam_nav_set_path(slam_handle* h, const slam_nav_config* cfg, const double* pts, int P) {
    if (!h || !pts) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
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
    if (!h || !pts || !P) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(nav_check_config(cfg));
    if (P_stride < 1 || P_stride > slam::kNavMaxWaypoints) return slam_internal_fail(SLAM_ERR_ARG, "P_stride = %d: 1 .. %d are supported", P_stride, slam::kNavMaxWaypoints);
    const size_t B = (size_t)h->B;
    for (size_t b = 0; b < B; ++b) {
        if (P[b] > P_stride) return slam_internal_fail(SLAM_ERR_ARG, "instance %zu: %d waypoints exceed P_stride = %d", b, P[b], P_stride);
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
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
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
            return launch_step(h, kNoCmd, 1, nullptr, nullptr, 0, h->each.dcmd_each);
        },
        [&](int t0, int tc) -> int {
            if (cmds_out) HIP_TRY(hipMemcpy(cmds_out + (size_t)t0 * row, h->nav.dlog, sizeof(float) * (size_t)tc * row, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
}

int slam_nav_state(slam_handle* h, int32_t* remaining, int32_t* finish_tick, double* integ, double* err_prev) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (!h->nav.set) return slam_internal_fail(SLAM_ERR_STATE, "no path: call slam_nav_set_path or slam_nav_set_paths first");
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
    if (!h || !est) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
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
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    h->nav.time_ticks = per_tick != 0;
    return SLAM_OK;
}

int slam_last_nav_work(slam_handle* h, double* controller_ms, double* total_ms) {
    return last_work(h ? &h->nav.times : nullptr, "slam_nav_run", controller_ms, total_ms);
}

int slam_nav_tick_host(const slam_nav_config* cfg, double d_max, double th_max, const double* pts, int P, const float est[3], int frozen,
                       int tick, int32_t* head, int32_t* finish_tick, double* integ, double* err_prev, float cmd[2]) {
    if (!pts || !est || !head || !finish_tick || !integ || !err_prev || !cmd) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    TRY(nav_check_config(cfg));
    TRY(nav_check_path(pts, P, -1));
    if (*head < 0 || *head > P) return slam_internal_fail(SLAM_ERR_ARG, "head = %d outside [0, P = %d]", *head, P);
    slam::NavState s;
    s.head = *head; s.finish_tick = *finish_tick; s.integ = *integ; s.err_prev = *err_prev;
    slam::nav_tick(nav_consts(*cfg, d_max, th_max), slam::NavPathView{pts}, P, (double)est[0], (double)est[1], (double)est[2], frozen != 0, tick, s, cmd);
    *head = s.head; *finish_tick = s.finish_tick; *integ = s.integ; *err_prev = s.err_prev;
    return SLAM_OK;
}

}  // extern "C"
