// pgs_capi_fix.cpp — C ABI: absolute position and heading fixes of the pose graph (include/slam_pgs.h "absolute fixes"; the factor: pgs_fix.h,
// the kernels: pgs_kernel.hip).  Host side only: owns the fix arrays and the staging, orders the launches on the handle's stream.
#include <math.h>
#include <string.h>

#include <vector>

#include "fix_kernel.h"
#include "pgs_handle.h"

#define fail slam_internal_fail

using pgs_capi::check;

static_assert((int)SLAM_FIX_POS == (int)slam::kPgsFixPos && (int)SLAM_FIX_YAW == (int)slam::kPgsFixYaw, "slam_fix_kinds and pgs_fix.h number the parts alike");
static_assert((int)PGS_FIX_ABSENT == (int)slam::kPgsFixAbsent && (int)PGS_FIX_STORED == (int)slam::kPgsFixStored && (int)PGS_FIX_INVALID == (int)slam::kPgsFixInvalid,
              "pgs_fix_verdict (slam_pgs.h) and pgs_fix.h number the verdicts alike");
static_assert(slam::kPgsFixRowLen == slam::kFixRowLen, "a fix row of the EKF batch goes into the pose graph unchanged");

namespace {

// what every call that touches the graph's fixes or the simulator's truth checks after its arguments
int fix_enter(pgs_handle* h, const char* who, bool need_map) {
    TRY(check(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "pgs_init must be called before %s", who);
    if (need_map && !h->p.map && !h->p.map_each) return fail(SLAM_ERR_STATE, "pgs_set_map or pgs_set_maps must be called before %s", who);
    return SLAM_OK;
}

// The fix arrays: allocated and zeroed by the first call that attaches a fix, both or neither.  From then on the solve launches the kernels
// built with the fixes' terms (pgs_kernel.h: pgs_has_fixes).
int ensure_fix_arrays(pgs_handle* h) {
    if (h->fix_kind) return SLAM_OK;
    const size_t n = (size_t)h->B * h->N_max;
    DevBuf<double> r; DevBuf<int32_t> k;
    if (r.reserve(slam::kPgsFixRowLen * n) != hipSuccess || k.reserve(n) != hipSuccess)
        return fail(SLAM_ERR_HIP, "out of device memory for the fixes (%zu bytes)", (sizeof(double) * slam::kPgsFixRowLen + sizeof(int32_t)) * n);
    HIP_TRY(hipMemsetAsync(r, 0, sizeof(double) * slam::kPgsFixRowLen * n, h->stream));
    HIP_TRY(hipMemsetAsync(k, 0, sizeof(int32_t) * n, h->stream));
    h->fix_row = std::move(r); h->fix_kind = std::move(k);
    h->p.fix_row = h->fix_row; h->p.fix_kind = h->fix_kind;
    return SLAM_OK;
}

int reserve_staging(pgs_handle* h) {
    const size_t B = (size_t)h->B;
    HIP_TRY(h->dfix.reserve(slam::kPgsFixRowLen * B));
    HIP_TRY(h->dfix_kinds.reserve(B));
    HIP_TRY(h->dfix_verdict.reserve(B));
    HIP_TRY(h->dfix_jumped.reserve(B));
    return SLAM_OK;
}

// one fix of every instance at the graph's newest pose, from device rows, in stream order
int attach(pgs_handle* h, const char* who, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict) {
    if (h->tick_dropped) return fail(SLAM_ERR_STATE, "%s: the handle's last update was dropped for pose capacity (N_max = %d): the fix has no pose", who, h->N_max);
    TRY(ensure_fix_arrays(h));
    h->p.N = h->timestep + 1;
    HIP_TRY(slam::pgs_launch_fix_attach(h->p, h->fix_row, h->fix_kind, d_fix, d_kinds, d_verdict, h->stream));
    h->invalidate_derived();
    return SLAM_OK;
}

int sense(pgs_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped) {
    // the RNG step of the next pgs_run_sim tick: the handle's timestep (pgs_capi.cpp: run_sim)
    HIP_TRY(slam::pgs_launch_fix_sense(h->p, h->fix_sensor_set ? h->fix_sensor.get() : nullptr, (uint32_t)h->timestep, d_fix, d_kinds, d_jumped, h->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int pgs_fix_dev(pgs_handle* h, const double* d_fix, const int32_t* d_kinds, int32_t* d_verdict) {
    if (!d_fix) return fail(SLAM_ERR_ARG, "pgs_fix_dev: d_fix is NULL");
    if (!d_kinds) return fail(SLAM_ERR_ARG, "pgs_fix_dev: d_kinds is NULL");
    TRY(fix_enter(h, "pgs_fix_dev", false));
    return attach(h, "pgs_fix_dev", d_fix, d_kinds, d_verdict);
}

int pgs_fix(pgs_handle* h, const double* fix, const int32_t* kinds, int32_t* verdict) {
    if (!fix) return fail(SLAM_ERR_ARG, "pgs_fix: fix is NULL");
    if (!kinds) return fail(SLAM_ERR_ARG, "pgs_fix: kinds is NULL");
    TRY(fix_enter(h, "pgs_fix", false));
    if (h->tick_dropped) return fail(SLAM_ERR_STATE, "pgs_fix: the handle's last update was dropped for pose capacity (N_max = %d): the fix has no pose", h->N_max);
    const size_t B = (size_t)h->B;
    TRY(reserve_staging(h));
    HIP_TRY(hipMemcpyAsync(h->dfix, fix, sizeof(double) * slam::kPgsFixRowLen * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->dfix_kinds, kinds, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    TRY(attach(h, "pgs_fix", h->dfix, h->dfix_kinds, h->dfix_verdict));
    if (verdict) HIP_TRY(hipMemcpyAsync(verdict, h->dfix_verdict, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host arrays are pageable and the staging is reused by the next call
    return SLAM_OK;
}

int pgs_set_fix_robust(pgs_handle* h, int kind, double k) {
    if (!pgs_capi::robust_args_ok(kind, k)) return fail(SLAM_ERR_ARG, "pgs_set_fix_robust: kind %d, k %g (kind 0 | 1 | 2; k finite and > 0 for a loss)", kind, k);
    TRY(check(h));
    h->fix_loss_kind = kind; h->fix_loss_k = kind == slam::kPgsLossNone ? 0.0 : k;
    h->invalidate_derived();   // what was computed belongs to the setting it was computed with
    return SLAM_OK;
}

int pgs_get_fix_robust(const pgs_handle* h, int* kind, double* k) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (kind) *kind = h->fix_loss_kind;
    if (k) *k = h->fix_loss_k;
    return SLAM_OK;
}

int pgs_get_fixes(pgs_handle* h, int inst, double* fix, int32_t* kinds, int cap, int32_t* n) {
    if (cap < 0 || (cap > 0 && !fix && !kinds)) return fail(SLAM_ERR_ARG, "pgs_get_fixes: bad output (cap = %d)", cap);
    TRY(fix_enter(h, "pgs_get_fixes", false));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    const size_t have = (size_t)h->timestep + 1, take = have < (size_t)cap ? have : (size_t)cap;
    if (n) *n = (int32_t)have;
    if (!take) return SLAM_OK;
    if (!h->fix_kind) {   // no fix was ever attached
        if (fix) memset(fix, 0, sizeof(double) * slam::kPgsFixRowLen * take);
        if (kinds) memset(kinds, 0, sizeof(int32_t) * take);
        return SLAM_OK;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (fix) HIP_TRY(hipMemcpy(fix, h->fix_row + (size_t)inst * h->N_max * slam::kPgsFixRowLen, sizeof(double) * slam::kPgsFixRowLen * take, hipMemcpyDeviceToHost));
    if (kinds) HIP_TRY(hipMemcpy(kinds, h->fix_kind + (size_t)inst * h->N_max, sizeof(int32_t) * take, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int pgs_fix_weights(pgs_handle* h, int which) {
    if (which != 0 && which != 1) return fail(SLAM_ERR_ARG, "which = %d (0: initial_estimate, 1: result)", which);
    TRY(fix_enter(h, "pgs_fix_weights", false));
    if (which == 1 && !h->solved) return fail(SLAM_ERR_STATE, "pgs_fix_weights(which = 1): no result yet (pgs_solve has not run since pgs_init)");
    h->fxw_valid = false;
    const size_t n = 2 * (size_t)h->B * h->N_max;
    if (!h->fxw) {   // one allocation: there or not
        DevBuf<double> a;
        if (a.reserve(n) != hipSuccess) return fail(SLAM_ERR_HIP, "pgs_fix_weights: out of device memory for the output (%zu bytes)", sizeof(double) * n);
        h->fxw = std::move(a);
    }
    if (!h->fix_kind) {   // no fix was ever attached: nothing is stored anywhere (all bits set is a NaN)
        HIP_TRY(hipMemsetAsync(h->fxw, 0xff, sizeof(double) * n, h->stream));
    } else {
        slam::PgsParams q = h->p;   // the setting of now; it needs none of the solve's work space
        q.N = h->timestep + 1; q.fix_loss_kind = h->fix_loss_kind; q.fix_loss_k = h->fix_loss_k;
        HIP_TRY(slam::pgs_launch_fix_weights(q, which, h->fxw, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fxw_valid = true;
    return SLAM_OK;
}

int pgs_get_fix_weights(pgs_handle* h, int inst, double* w, int cap, int32_t* n) {
    TRY(check(h));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    if (cap < 0 || (cap > 0 && !w)) return fail(SLAM_ERR_ARG, "bad output (w, cap = %d)", cap);
    if (!h->fxw_valid) return fail(SLAM_ERR_STATE, "no fix weights for the current values: call pgs_fix_weights after the last update / fix / solve");
    const size_t have = (size_t)h->timestep + 1, take = have < (size_t)cap ? have : (size_t)cap;
    if (take) HIP_TRY(hipMemcpy(w, h->fxw + 2 * (size_t)inst * h->N_max, sizeof(double) * 2 * take, hipMemcpyDeviceToHost));
    if (n) *n = (int32_t)have;
    return SLAM_OK;
}

int pgs_fix_weights_dev(pgs_handle* h, const double** d_w) {
    TRY(check(h));
    if (!h->fxw_valid) return fail(SLAM_ERR_STATE, "no fix weights for the current values: call pgs_fix_weights after the last update / fix / solve");
    if (d_w) *d_w = h->fxw;
    return SLAM_OK;
}

int pgs_set_fix_sensor_each(pgs_handle* h, const slam_fix_sensor* rows) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    const size_t B = (size_t)h->B;
    for (size_t b = 0; rows && b < B; ++b)
        if (const char* f = slam::fix_sensor_bad_field(rows[b]))
            return fail(SLAM_ERR_ARG, "instance %zu: fix sensor field %s is out of range (half-widths and sigmas finite and >= 0, probabilities in [0, 1], jump_lo <= jump_hi finite, kinds in 0 .. 3)",
                        b, f);
    TRY(check(h));
    if (!rows) {
        h->fix_sensor_set = false;   // (the launches in flight keep reading the rows: they stay allocated)
        return SLAM_OK;
    }
    if (h->fix_sensor.cap() < B) {   // the new block first: a failure leaves the handle with the rows it had
        DevBuf<slam_fix_sensor> d;
        HIP_TRY(d.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->fix_sensor = std::move(d);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old rows are done
    }
    HIP_TRY(hipMemcpyAsync(h->fix_sensor, rows, sizeof(slam_fix_sensor) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fix_sensor_set = true;
    return SLAM_OK;
}

int pgs_fix_sense_dev(pgs_handle* h, double* d_fix, int32_t* d_kinds, int32_t* d_jumped) {
    if (!d_fix) return fail(SLAM_ERR_ARG, "pgs_fix_sense_dev: d_fix is NULL");
    if (!d_kinds) return fail(SLAM_ERR_ARG, "pgs_fix_sense_dev: d_kinds is NULL");
    TRY(fix_enter(h, "pgs_fix_sense_dev", true));
    return sense(h, d_fix, d_kinds, d_jumped);
}

int pgs_fix_sense(pgs_handle* h, double* fix, int32_t* kinds, int32_t* jumped) {
    if (!fix) return fail(SLAM_ERR_ARG, "pgs_fix_sense: fix is NULL");
    if (!kinds) return fail(SLAM_ERR_ARG, "pgs_fix_sense: kinds is NULL");
    TRY(fix_enter(h, "pgs_fix_sense", true));
    const size_t B = (size_t)h->B;
    TRY(reserve_staging(h));
    TRY(sense(h, h->dfix, h->dfix_kinds, h->dfix_jumped));
    HIP_TRY(hipMemcpyAsync(fix, h->dfix, sizeof(double) * slam::kPgsFixRowLen * B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(kinds, h->dfix_kinds, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    if (jumped) HIP_TRY(hipMemcpyAsync(jumped, h->dfix_jumped, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int pgs_run_sim_fix(pgs_handle* h, const float* cmds, int T, int each, int fix_every) {
    if (!cmds || T <= 0) return fail(SLAM_ERR_ARG, "pgs_run_sim_fix: bad command sequence");
    if (each != 0 && each != 1) return fail(SLAM_ERR_ARG, "pgs_run_sim_fix: each = %d (0: cmds [T][2], 1: cmds [T][batch][2])", each);
    if (fix_every < 1) return fail(SLAM_ERR_ARG, "pgs_run_sim_fix: fix_every = %d is below 1", fix_every);
    TRY(fix_enter(h, "pgs_run_sim_fix", true));
    const size_t per_tick = 2 * (each ? (size_t)h->B : 1);
    if (each)
        for (size_t i = 0; i < per_tick * (size_t)T; ++i)
            if (!isfinite(cmds[i])) return fail(SLAM_ERR_ARG, "a command is not finite");
    if (h->timestep + T >= h->N_max) return fail(SLAM_ERR_STATE, "timestep %d + %d commands exceed the pose capacity N_max = %d", h->timestep, T, h->N_max);
    TRY(reserve_staging(h));
    // chunks that end after each tick t with (t + 1) % fix_every == 0, through the simulator calls themselves; then the source and the attach, in
    // stream order, the rows going from one to the other on the device unchanged
    for (int t0 = 0; t0 < T;) {
        int n = fix_every - t0 % fix_every;
        if (n > T - t0) n = T - t0;
        TRY(each ? pgs_run_sim_each(h, cmds + per_tick * (size_t)t0, n) : pgs_run_sim(h, cmds + per_tick * (size_t)t0, n));
        t0 += n;
        if (t0 % fix_every) continue;
        TRY(sense(h, h->dfix, h->dfix_kinds, nullptr));
        TRY(attach(h, "pgs_run_sim_fix", h->dfix, h->dfix_kinds, nullptr));
    }
    return SLAM_OK;
}

int pgs_fix_factor_host(const double pose[3], const double row[5], int32_t kinds, int loss_kind, double loss_k, double e[3], double J[9], double rho[2],
                        double w[2], int32_t* verdict) {
    if (!pose || !row || !e || !J || !rho || !w) return fail(SLAM_ERR_ARG, "pgs_fix_factor_host: NULL argument");
    if (!pgs_capi::robust_args_ok(loss_kind, loss_k)) return fail(SLAM_ERR_ARG, "pgs_fix_factor_host: kind %d, k %g (kind 0 | 1 | 2; k finite and > 0 for a loss)", loss_kind, loss_k);
    const int32_t v = slam::pgs_fix_factor(pose, row, kinds, loss_kind, loss_k, e, J, rho, w);
    if (verdict) *verdict = v;
    return SLAM_OK;
}

}  // extern "C"
