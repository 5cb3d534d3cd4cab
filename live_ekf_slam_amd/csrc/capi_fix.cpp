// capi_fix.cpp — C ABI: absolute position and heading fixes of the EKF batch (fix_kernel.hip): slam_fix*, the simulated source
// slam_fix_sense*, the per-tick run slam_fix_run and the host hooks
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_filter.h"
#include "capi_innovation.h"
#include "capi_run.h"
#include "ekf_kernel.h"
#include "fix_kernel.h"
#include "host/tick_chunks.h"

using namespace slam_capi;

namespace {

// *out = *cfg (NULL: the defaults), checked
int fix_config(const slam_fix_config* cfg, slam_fix_config* out) {
    if (cfg) *out = *cfg; else slam_fix_config_default(out);
    if (!(out->gate_pos > 0.0)) return slam_internal_fail(SLAM_ERR_ARG, "fix config: gate_pos = %g is NaN or not positive", out->gate_pos);
    if (!(out->gate_yaw > 0.0)) return slam_internal_fail(SLAM_ERR_ARG, "fix config: gate_yaw = %g is NaN or not positive", out->gate_yaw);
    if (out->fix_every < 1) return slam_internal_fail(SLAM_ERR_ARG, "fix config: fix_every = %d is below 1", out->fix_every);
    return SLAM_OK;
}

// the handle, once the arguments are in order (map_enter's order); the queued timesteps run first
int fix_enter(slam_handle* h, const char* who, bool need_map, bool need_path) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "%s: NULL handle", who);
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "%s needs EKF_SLAM: the UKF's P is rank-deficient in its (cos, sin) yaw pair", who);
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "%s: slam_init has not been called", who);
    if (need_map && !has_map(h)) return slam_internal_fail(SLAM_ERR_STATE, "%s reads the simulator's truth: slam_set_map (or slam_set_maps) has not been called", who);
    if (need_path && !h->nav.set) return slam_internal_fail(SLAM_ERR_STATE, "%s: no path: call slam_nav_set_path or slam_nav_set_paths first", who);
    TRY(step_state(h, who));
    TRY(sense_idle(h, who));   // (a fix moves the pose: it belongs after the commit, as a merge does)
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

// the staged rows of `ticks` fixes, the record(s), the sums of the traffic model, the per-instance contributions
int fix_reserve(slam_handle* h, size_t ticks, size_t recs) {
    const size_t n = ticks * (size_t)h->B;
    TRY(grow(h, h->fix.dfix, slam::kFixRowLen * n));
    TRY(grow(h, h->fix.dkinds, n));
    TRY(grow(h, h->fix.dverdict, n));
    TRY(grow(h, h->fix.dnis, 2 * n));
    TRY(grow(h, h->fix.djumped, (size_t)h->B));
    TRY(grow(h, h->fix.drec, slam::kFixRecLen));
    if (recs) TRY(grow(h, h->fix.drecs, recs * slam::kFixRecLen));
    TRY(grow(h, h->fix.dwork, 2));
    return innovation_reserve(h, false);
}

int fix_zero_work(slam_handle* h) {
    HIP_TRY(hipMemsetAsync(h->fix.dwork, 0, 2 * sizeof(unsigned long long), h->stream));
    h->fix.work_set = true;
    return SLAM_OK;
}

// one fix on the handle's stream; d_verdict and d_nis are required here, d_rec NULL: no record
int fix_launch(slam_handle* h, const slam_fix_config& c, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict, double* d_nis, double* d_rec) {
    slam::FixParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.status = h->dflags;
    p.fix = d_fix; p.kinds = d_kinds; p.gate_pos = c.gate_pos; p.gate_yaw = c.gate_yaw;
    p.verdict = d_verdict; p.nis = d_nis;
    p.inst_rec = h->inn.dval + 13 * (size_t)h->B;   // (the places innovation_reserve gives the contributions and the partial records)
    p.partials = h->inn.dpart; p.rec = d_rec;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    HIP_TRY(slam::launch_fix(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

// the traffic model of the fix that has just been launched (M is what it saw: a fix does not change it)
int fix_sum_work(slam_handle* h, const int32_t* d_verdict) {
    HIP_TRY(slam::launch_fix_work(h->dM, d_verdict, (size_t)h->B, h->L_max, h->fix.dwork, h->stream));
    return SLAM_OK;
}

int fix_sense_launch(slam_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped) {
    slam::FixSenseParams p;
    memset(&p, 0, sizeof(p));
    p.truth = h->dtruth; p.rows = h->fix.rows_set ? h->fix.drows.get() : nullptr;
    p.seed = h->seed; p.inst0 = h->inst0; p.step = h->step;
    p.fix = d_fix; p.kinds = d_kinds; p.jumped = d_jumped; p.B = h->B;
    HIP_TRY(slam::launch_fix_sense(p, h->stream));
    return SLAM_OK;
}

// slam_fix* once the fix is on the device; the outputs' device places (NULL: the handle's)
int fix_now(slam_handle* h, const slam_fix_config& c, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict, double* d_nis, double* d_rec) {
    TRY(fix_zero_work(h));
    int32_t* const dv = d_verdict ? d_verdict : h->fix.dverdict.get();
    TRY(fix_launch(h, c, d_fix, d_kinds, dv, d_nis ? d_nis : h->fix.dnis.get(), d_rec));
    return fix_sum_work(h, dv);
}

}  // namespace

extern "C" {

int slam_fix_config_default(slam_fix_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->gate_pos = -2.0 * log(0.001);
    // chi-square with 1 degree of freedom is the square of a standard normal: its 0.999 quantile is z^2 with z the 0.9995 quantile of the
    // normal, z = sqrt(2) erfinv(0.999) = 3.2905267314919255
    c->gate_yaw = 10.827566170662733;
    c->fix_every = 10;
    return SLAM_OK;
}

int slam_fix(slam_handle* h, const slam_fix_config* cfg, const double* fix, const int32_t* kinds, int32_t* verdict, double* nis, double rec[16]) {
    slam_fix_config c;
    TRY(fix_config(cfg, &c));
    if (!fix) return slam_internal_fail(SLAM_ERR_ARG, "fix is NULL");
    if (!kinds) return slam_internal_fail(SLAM_ERR_ARG, "kinds is NULL");
    TRY(fix_enter(h, "slam_fix", false, false));
    const size_t B = (size_t)h->B;
    TRY(fix_reserve(h, 1, 0));
    HIP_TRY(hipMemcpyAsync(h->fix.dfix, fix, sizeof(double) * slam::kFixRowLen * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->fix.dkinds, kinds, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    TRY(fix_now(h, c, h->fix.dfix, h->fix.dkinds, nullptr, nullptr, rec ? h->fix.drec.get() : nullptr));
    if (!verdict && !nis && !rec) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{h->fix.dverdict, verdict, B}, {h->fix.dnis, nis, 2 * B}, {h->fix.drec, rec, slam::kFixRecLen}}, 0, 1);
}

int slam_fix_dev(slam_handle* h, const slam_fix_config* cfg, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict, double* d_nis,
                 double* d_rec) {
    slam_fix_config c;
    TRY(fix_config(cfg, &c));
    if (!d_fix) return slam_internal_fail(SLAM_ERR_ARG, "d_fix is NULL");
    if (!d_kinds) return slam_internal_fail(SLAM_ERR_ARG, "d_kinds is NULL");
    TRY(fix_enter(h, "slam_fix_dev", false, false));
    TRY(fix_reserve(h, 1, 0));
    return fix_now(h, c, d_fix, d_kinds, d_verdict, d_nis, d_rec);
}

int slam_fix_sensor_default(slam_fix_sensor* row) {
    if (!row) return slam_internal_fail(SLAM_ERR_ARG, "row is NULL");
    memset(row, 0, sizeof(*row));
    return SLAM_OK;
}

int slam_set_fix_sensor_each(slam_handle* h, const slam_fix_sensor* rows) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind != SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "slam_set_fix_sensor_each needs EKF_SLAM");
    const size_t B = (size_t)h->B;
    for (size_t b = 0; rows && b < B; ++b)
        if (const char* f = slam::fix_sensor_bad_field(rows[b]))
            return slam_internal_fail(SLAM_ERR_ARG, "instance %zu: fix sensor field %s is out of range (half-widths and sigmas finite and >= 0, probabilities in [0, 1], jump_lo <= jump_hi finite, kinds in 0 .. 3)",
                                      b, f);
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (!rows) {
        h->fix.rows_set = false;   // (the launches in flight keep reading drows: it stays allocated)
        return SLAM_OK;
    }
    if (h->fix.drows.cap() < B) {   // the new block first: a failure leaves the handle with the rows it had
        DevBuf<slam_fix_sensor> d;
        HIP_TRY(d.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->fix.drows = std::move(d);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old rows are done
    }
    HIP_TRY(hipMemcpyAsync(h->fix.drows, rows, sizeof(slam_fix_sensor) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fix.rows_set = true;
    return SLAM_OK;
}

int slam_fix_sense(slam_handle* h, double* fix, int32_t* kinds, int32_t* jumped) {
    if (!fix) return slam_internal_fail(SLAM_ERR_ARG, "fix is NULL");
    if (!kinds) return slam_internal_fail(SLAM_ERR_ARG, "kinds is NULL");
    TRY(fix_enter(h, "slam_fix_sense", true, false));
    const size_t B = (size_t)h->B;
    TRY(fix_reserve(h, 1, 0));
    TRY(fix_sense_launch(h, h->fix.dfix, h->fix.dkinds, h->fix.djumped));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{h->fix.dfix, fix, slam::kFixRowLen * B}, {h->fix.dkinds, kinds, B}, {h->fix.djumped, jumped, B}}, 0, 1);
}

int slam_fix_sense_dev(slam_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped) {
    if (!d_fix) return slam_internal_fail(SLAM_ERR_ARG, "d_fix is NULL");
    if (!d_kinds) return slam_internal_fail(SLAM_ERR_ARG, "d_kinds is NULL");
    TRY(fix_enter(h, "slam_fix_sense_dev", true, false));
    return fix_sense_launch(h, d_fix, d_kinds, d_jumped);
}

int slam_fix_run(slam_handle* h, const slam_fix_config* cfg, int source, const float* cmds, int T, double* recs, int32_t* verdict, double* nis,
                 const slam_fix_log* fix_log) {
    slam_fix_config c;
    TickCmds::Source csrc;
    TRY(fix_config(cfg, &c));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    TRY(sim_run_source(source, cmds, &csrc));
    TRY(fix_enter(h, "slam_fix_run", true, csrc == TickCmds::kNav));
    if (T == 0) return SLAM_OK;
    slam_fix_log log = {nullptr, nullptr};
    if (fix_log) log = *fix_log;
    const size_t B = (size_t)h->B;
    TickCmds tcmd;
    TRY(tcmd.init(h, csrc, cmds));
    // what a tick holds on the device: its per-instance commands and, when a per-instance series is wanted, its rows of all four (else one
    // row serves every tick); its record
    const bool keep = verdict || nis || log.fix || log.kinds;
    const double per_tick = tcmd.bytes_per_tick(h) + (keep ? (8.0 * slam::kFixRowLen + 4.0 + 4.0 + 16.0) * (double)B : 0.0) + 8.0 * slam::kFixRecLen;
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(fix_reserve(h, keep ? (size_t)chunk : 1, (size_t)chunk));
    TRY(fix_zero_work(h));
    const size_t rows = keep ? (size_t)chunk : 1;
    auto at = [&](int t) { return keep ? (size_t)t * B : (size_t)0; };
    return run_chunked(
        h, T, chunk, h->nav.time_ticks, h->fix.times,
        [&](int t0, int tc) -> int {   // (and the rows of the ticks without a fix: zeros, NaN for nis)
            TRY(tcmd.upload(h, t0, tc));
            HIP_TRY(hipMemsetAsync(h->fix.dfix, 0, sizeof(double) * slam::kFixRowLen * rows * B, h->stream));
            HIP_TRY(hipMemsetAsync(h->fix.dkinds, 0, sizeof(int32_t) * rows * B, h->stream));
            HIP_TRY(hipMemsetAsync(h->fix.dverdict, 0, sizeof(int32_t) * rows * B, h->stream));
            HIP_TRY(hipMemsetAsync(h->fix.dnis, 0xff, sizeof(double) * 2 * rows * B, h->stream));
            HIP_TRY(hipMemsetAsync(h->fix.drecs, 0, sizeof(double) * slam::kFixRecLen * (size_t)tc, h->stream));
            return SLAM_OK;
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(launch_step(h, cmd, 1, nullptr, nullptr, 0, d_each));
            const bool fixes = (t0 + t + 1) % c.fix_every == 0;
            double* const df = h->fix.dfix + slam::kFixRowLen * at(t);
            int32_t* const dk = h->fix.dkinds + at(t);
            int32_t* const dv = h->fix.dverdict + at(t);
            // (the marked group of a tick without a fix is empty: its event pair brackets nothing)
            TRY(mark([&]() -> int {
                if (!fixes) return SLAM_OK;
                TRY(fix_sense_launch(h, df, dk, nullptr));
                return fix_launch(h, c, df, dk, dv, h->fix.dnis + 2 * at(t), recs ? h->fix.drecs + (size_t)t * slam::kFixRecLen : nullptr);
            }));
            return fixes ? fix_sum_work(h, dv) : SLAM_OK;   // (here: the next tick's step changes M)
        },
        [&](int t0, int tc) -> int {
            return copy_rows({{h->fix.drecs, recs, slam::kFixRecLen}, {h->fix.dverdict, verdict, B}, {h->fix.dnis, nis, 2 * B},
                              {h->fix.dfix, log.fix, slam::kFixRowLen * B}, {h->fix.dkinds, log.kinds, B}}, t0, tc);
        });
}

int slam_last_fix_work(slam_handle* h, double* bytes, double* fix_ms, double* total_ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (!h->fix.work_set) return slam_internal_fail(SLAM_ERR_STATE, "slam_fix, slam_fix_dev or slam_fix_run has not run on this handle");
    if (bytes) {
        unsigned long long wk[2];
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(wk, h->fix.dwork, sizeof(wk), hipMemcpyDeviceToHost));
        *bytes = (double)wk[0] * h->esz + (double)wk[1];
    }
    if (fix_ms) *fix_ms = h->fix.times.part_ms;
    if (total_ms) *total_ms = h->fix.times.total_ms;
    return SLAM_OK;
}

int slam_fix_instance_host(double* x, double* P, int M, int L_max, int32_t status, int f32_storage, const slam_fix_config* cfg, const double row[5],
                           int32_t kinds, int32_t* verdict, double nis[2], double rec[16]) {
    slam_fix_config c;
    TRY(fix_config(cfg, &c));
    if (!x || !P || !row) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 1 || L_max > slam::kMapMaxLandmarks || M < 0 || M > L_max)
        return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d], or L_max is not in [1, %d]", M, L_max, slam::kMapMaxLandmarks);
    const int n = 3 + 2 * M;
    const bool skip = (status & slam::kMapStatusSkip) != 0;
    const double gates[2] = {c.gate_pos, c.gate_yaw};
    slam::FixResult o = {0, {__builtin_nan(""), __builtin_nan("")}, 0};
    // the instance's slab as the handle holds it: rows at the padded leading dimension, elements of the storage type
    auto run = [&](auto zero) {
        using ST = decltype(zero);
        const int ld = slam::ekf_ld(n, (int)sizeof(ST));
        std::vector<ST> Ps((size_t)n * ld, (ST)0), xs((size_t)n);
        for (int r = 0; r < n; ++r)
            for (int cc = 0; cc < n; ++cc) Ps[(size_t)r * ld + cc] = (ST)P[(size_t)r * n + cc];
        for (int i = 0; i < n; ++i) xs[i] = (ST)x[i];
        std::vector<double> ws((size_t)slam::fix_ws_len(n));
        o = slam::fix_instance<false>(slam::MapSeq(), Ps.data(), xs.data(), M, row, kinds, gates, ws.data());
        if (!o.written) return;   // (the caller's arrays keep their bytes)
        for (int r = 0; r < n; ++r)
            for (int cc = 0; cc < n; ++cc) P[(size_t)r * n + cc] = (double)Ps[(size_t)r * ld + cc];
        for (int i = 0; i < n; ++i) x[i] = (double)xs[i];
    };
    if (!skip) { if (f32_storage) run(0.0f); else run(0.0); }
    if (verdict) *verdict = o.verdict;
    if (nis) { nis[0] = o.nis[0]; nis[1] = o.nis[1]; }
    if (rec) slam::fix_record(o, skip, rec);
    return SLAM_OK;
}

int slam_fix_sense_instance_host(uint64_t seed, int64_t instance, uint32_t step, const double truth[3], const slam_fix_sensor* row, double fix[5],
                                 int32_t* kinds, int32_t* jumped) {
    if (!truth || !fix || !kinds) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    const slam_fix_sensor r = row ? *row : slam::fix_sensor_default_row();
    if (const char* f = slam::fix_sensor_bad_field(r))
        return slam_internal_fail(SLAM_ERR_ARG, "fix sensor field %s is out of range (half-widths and sigmas finite and >= 0, probabilities in [0, 1], jump_lo <= jump_hi finite, kinds in 0 .. 3)", f);
    const slam::FixSensed o = slam::fix_sense_instance(r, seed, (uint64_t)instance, step, truth[0], truth[1], truth[2]);
    memcpy(fix, o.row, sizeof(o.row));
    *kinds = o.kinds;
    if (jumped) *jumped = o.jumped;
    return SLAM_OK;
}

}  // extern "C"
