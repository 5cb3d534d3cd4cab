// slam_capi.cpp — C ABI (include/slam_batch.h) over the HIP kernels.  Host-side only: owns device memory,
// the stream, the step counter and the config; every compute entry point enqueues one fused kernel.
// There is NO CPU fallback: without a HIP device every compute call fails with SLAM_ERR_HIP.
// This unit: the error string, the config, creating and destroying a handle, its setters, the start state, the maps and the noise rows.
// The handle and what the other units of the ABI (capi_*.cpp) share with this one: slam_handle.h.
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <utility>
#include <vector>

#include "slam_handle.h"
#include "host/config_parse.h"
#include "host/noise_pack.h"
#include "ekf_kernel.h"
#include "slam_math.h"
#include "ukf_kernel.h"

using namespace slam_capi;

namespace {

thread_local char g_err[512] = "";

}  // namespace

extern "C" {

int slam_internal_fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

const char* slam_last_error(void) { return g_err; }
const char* slam_version(void) { return "live_ekf_slam_amd 0.1 (gfx950)"; }

int slam_config_default(slam_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->v_d = 0.0f; c->v_th = 0.0f; c->V_00 = 0.01; c->V_11 = 0.001;      // params.yaml:39-45
    c->w_r = 0.0f; c->w_b = 0.0f; c->W_00 = 0.01; c->W_11 = 0.01;        // params.yaml:46-52
    c->landmark_id_is_known = 1; c->min_landmark_separation = 0.1f;        // params.yaml:35-36
    c->d_max = 0.1; c->th_max = 0.0546;                                    // params.yaml:27-28
    c->range_max = 3.0; c->fov_min = -1.57; c->fov_max = 1.57;             // params.yaml:30-32
    c->init_x = 0.0; c->init_y = 0.0; c->init_yaw = 0.0;                   // params.yaml:19-22
    c->replicate_vw_quirk = 1;
    c->ukf_float_trig = 1;
    return SLAM_OK;
}

// The reference reads one YAML file with nested maps; the keys the hot path needs are unique leaf names
// except min_landmark_separation (constraints.measurements vs map), disambiguated by section tracking.  The reader
// itself is host/config_parse.h (host-only, also compiled under ASan + UBSan by `make -C oracle asan`).
int slam_config_load(slam_config* c, const char* path) {
    if (!c || !path) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    std::string err;
    const int rc = slam_host::config_parse_file(c, path, &err);
    if (rc) return slam_internal_fail(SLAM_ERR_IO, "%s", err.c_str());
    return SLAM_OK;
}

int slam_create(const slam_config* cfg, int kind, int batch, int L_max, int dtype, int device, slam_handle** out) {
    if (!cfg || !out) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (batch <= 0 || L_max <= 0) return slam_internal_fail(SLAM_ERR_ARG, "batch and L_max must be positive");
    if (kind != SLAM_EKF_SLAM && kind != SLAM_UKF_SLAM && kind != SLAM_UKF_LOC)
        return slam_internal_fail(SLAM_ERR_ARG, "unknown filter kind %d", kind);
    // The four quirk switches took over fields that were `reserved` until round 4: a caller compiled against that header may
    // have left anything there, and any non-zero value would silently switch a reference quirk off.  Only 0 and 1 are configurations.
    for (const int q : {cfg->ekf_abs_is_int, cfg->ekf_landmark_from_x_pred, cfg->ukf_accumulate_zest1, cfg->ukf_sensing_yaw_from_sigma})
        if (q != 0 && q != 1) return slam_internal_fail(SLAM_ERR_ARG, "slam_config quirk switch = %d: the switches (ekf_abs_is_int, ekf_landmark_from_x_pred, ukf_accumulate_zest1, "
                                                        "ukf_sensing_yaw_from_sigma) are 0 or 1 - zero-initialise the struct (slam_config_default)", q);
    if (kind == SLAM_UKF_LOC) L_max = 1;   // localisation only: the state never holds landmarks
    if (dtype != SLAM_F64 && !(dtype == SLAM_F32 && kind == SLAM_EKF_SLAM))
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "fp32 state storage is implemented for EKF_SLAM only");
    if (L_max > (kind != SLAM_EKF_SLAM ? slam::kUkfMaxLandmarks : slam::kEkfMaxLandmarks))
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "L_max %d exceeds the limit of this filter kind (EKF %d, UKF %d): the EKF beyond %d landmarks (fp32 storage: beyond %d) and the UKF beyond 50 run the HBM-streamed size classes, whose working set is 2 x n x n doubles per instance in HBM", L_max, slam::kEkfMaxLandmarks, slam::kUkfMaxLandmarks, slam::kEkfLdsMaxLandmarks, slam::kEkfLdsMaxLandmarksF32);
    HIP_TRY(hipSetDevice(device));
    slam_handle* h = new slam_handle();
    h->cfg = *cfg; h->kind = kind; h->B = batch; h->L_max = L_max; h->dtype = dtype; h->device = device;
    h->esz = dtype == SLAM_F32 ? 4 : 8;
    h->base = (kind == SLAM_EKF_SLAM) ? 3 : 4;
    h->n_max = h->base + 2 * L_max;
    // per-filter slab: n_max rows of the padded leading dimension (EKF: slam::ekf_ld, rows start on 16-byte boundaries;
    // the UKF packs n x n with n even), 256/512-byte aligned
    h->ld_max = kind == SLAM_EKF_SLAM ? slam::ekf_ld(h->n_max, h->esz) : h->n_max;
    h->pstride = round_up(h->n_max * h->ld_max + 4, 64);
    h->xstride = round_up(h->n_max + 1, 2);
    h->range_max = cfg->range_max; h->fov_min = cfg->fov_min; h->fov_max = cfg->fov_max;
    const char* env = getenv("SLAM_WAVES_PER_FILTER");
    if (env) h->waves_per_filter = atoi(env);
    env = getenv("SLAM_DEBUG_FLAGS");   // 4 / 32: phase and per-step timers.  The ablation bits (1, 2, 16: WRONG results) are
    if (env) h->dbg = atoi(env);        // compiled out of the release kernels (-DSLAM_ABLATE builds only)
#ifndef SLAM_ABLATE
    h->dbg &= (4 | 32);   // (the fault-injection bit 128 and the order-forcing bit 1024 are reachable through slam_set_debug_flags only: no
                          // environment variable can plant them)
#endif
    env = getenv("SLAM_UKF_SPLIT_MIN");   // batch size from which UKF run_sim splits the batch over two streams
    if (env) h->ukf.split_min = atoi(env);
    env = getenv("SLAM_UKF_PARTS");   // streams the UKF batch is split over in run_sim (2..4)
    if (env) h->ukf.parts = atoi(env);
    env = getenv("SLAM_LAZY_STEPS");   // slam_step_sim calls queued per multi-step launch (0 = one launch per call)
    if (env) { h->lazy_max = atoi(env); h->lazy_explicit = true; }
    env = getenv("SLAM_EAGER_FLUSH");   // queued steps from which an idle GPU is given work before the queue is full (0 = never)
    if (env) h->eager_init = h->eager_target = atoi(env);
    env = getenv("SLAM_RUN_CHUNK");   // timesteps per launch of slam_run_sim (1 = one launch per step)
    if (env) h->run_chunk = atoi(env);
    hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete h; return slam_internal_fail(SLAM_ERR_HIP, "hipStreamCreate -> %s", hipGetErrorString(e)); }
    h->own_stream = true;
    const size_t B = (size_t)batch;
    hipError_t errs[] = {
        h->dP.reserve((size_t)h->esz * B * h->pstride),
        h->dP2.reserve((size_t)h->esz * B * h->pstride),
        h->dx.reserve((size_t)h->esz * B * h->xstride),
        h->dM.reserve(B),
        h->dids.reserve(B * L_max),
        h->dflags.reserve(B),
        h->dts.reserve(B),
        h->dtruth.reserve(B * 3),
        h->derr.reserve(B),
        h->dscalar.reserve(4),
        (h->dbg & (4 | 32)) ? h->dprof.reserve(slam::kEkfProfSlots * B) : hipSuccess,
        h->dkhist.reserve(16),
        kind != SLAM_EKF_SLAM ? h->ukf.dsq.reserve(B * h->pstride) : hipSuccess,
        h->esz == 4 ? h->dscratch.reserve(B * h->pstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->ukf.dnsq.reserve(B) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->ukf.dxprev.reserve(B * h->xstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->ukf.dvt.reserve(B * h->pstride) : hipSuccess,
        (kind == SLAM_UKF_SLAM && L_max > slam::kUkfLdsMaxLandmarks) ? h->ukf.dbigws.reserve(B * 2 * h->pstride) : hipSuccess,
        kind != SLAM_EKF_SLAM ? h->ukf.dvage.reserve(B) : hipSuccess,
        (kind != SLAM_EKF_SLAM && h->n_max <= 44) ? h->ukf.drot.reserve(slam::kUkfQuadTabEntries) : hipSuccess,
    };
    for (hipError_t ee : errs)
        if (ee != hipSuccess) {
            slam_destroy(h);
            return slam_internal_fail(SLAM_ERR_HIP, "allocating device memory -> %s", hipGetErrorString(ee));
        }
    // every buffer a getter can read before slam_init is zeroed (M = 0, flags = 0, timestep = 0, ...)
    hipError_t zs[] = {
        hipMemsetAsync(h->dP, 0, (size_t)h->esz * B * h->pstride, h->stream),
        hipMemsetAsync(h->dP2, 0, (size_t)h->esz * B * h->pstride, h->stream),
        hipMemsetAsync(h->dx, 0, (size_t)h->esz * B * h->xstride, h->stream),
        hipMemsetAsync(h->dids, 0, sizeof(int32_t) * B * L_max, h->stream),
        hipMemsetAsync(h->dM, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dflags, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dts, 0, sizeof(int32_t) * B, h->stream),
        hipMemsetAsync(h->dtruth, 0, sizeof(double) * B * 3, h->stream),
        hipMemsetAsync(h->derr, 0, sizeof(double) * B, h->stream),
        hipMemsetAsync(h->dkhist, 0, sizeof(unsigned long long) * 16, h->stream),
        h->ukf.dnsq ? hipMemsetAsync(h->ukf.dnsq, 0, sizeof(int32_t) * B, h->stream) : hipSuccess,
        h->dprof ? hipMemsetAsync(h->dprof, 0, sizeof(unsigned long long) * slam::kEkfProfSlots * B, h->stream) : hipSuccess,
        h->ukf.drot ? slam::launch_ukf_quad_table(h->ukf.drot, h->stream) : hipSuccess,
    };
    for (hipError_t ee : zs)
        if (ee != hipSuccess) {
            slam_destroy(h);
            return slam_internal_fail(SLAM_ERR_HIP, "hipMemsetAsync -> %s", hipGetErrorString(ee));
        }
    *out = h;
    return SLAM_OK;
}

int slam_destroy(slam_handle* h) {
    if (!h) return SLAM_OK;
    if (h->shadow) { slam_destroy(h->shadow); h->shadow = nullptr; }
    flush_lazy(h);
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (auto& st : h->ukf.aux_stream) if (st) { hipStreamSynchronize(st); hipStreamDestroy(st); }
    for (auto& ev : h->ukf.aux_ev) if (ev) hipEventDestroy(ev);
    for (auto& ev : h->run_ev) if (ev) hipEventDestroy(ev);
    if (h->copy_stream) { hipStreamSynchronize(h->copy_stream); hipStreamDestroy(h->copy_stream); }
    if (h->shadow_ev) hipEventDestroy(h->shadow_ev);
    for (slam_handle::Stage* f : {&h->q.host[0], &h->q.host[1], &h->stage[0], &h->stage[1]})
        if (f->copied) { hipEventDestroy(f->copied); hipEventDestroy(f->used); }
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;   // the device and pinned buffers
    return SLAM_OK;
}

int slam_set_stream(slam_handle* h, void* s) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    if (h->stream) hipStreamSynchronize(h->stream);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    h->stream = (hipStream_t)s;
    h->own_stream = false;
    return SLAM_OK;
}
int slam_set_instance_offset(slam_handle* h, int64_t v) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->inst0 = v;
    return h->shadow ? slam_set_instance_offset(h->shadow, v + h->tracked) : SLAM_OK;
}
int slam_set_seed(slam_handle* h, uint64_t s) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->seed = s;
    return h->shadow ? slam_set_seed(h->shadow, s) : SLAM_OK;
}
int slam_set_vision(slam_handle* h, double range_max, double fov_min, double fov_max) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    h->range_max = range_max; h->fov_min = fov_min; h->fov_max = fov_max;
    return h->shadow ? slam_set_vision(h->shadow, range_max, fov_min, fov_max) : SLAM_OK;
}

int slam_init(slam_handle* h, float x0, float y0, float yaw0) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->kind == SLAM_EKF_SLAM) {
        slam::EkfInitParams p;
        memset(&p, 0, sizeof(p));   // (the per-instance pointers stay NULL: the shared start pose)
        p.P = h->dP; p.x = h->dx; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride; p.f32_storage = h->esz == 4;
        p.x0 = x0; p.y0 = y0; p.yaw0 = yaw0;
        // the simulator starts from the un-rounded YAML pose (sim_node.py:361); the filter gets float args
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        HIP_TRY(slam::launch_ekf_init(p, h->stream));
    } else {
        slam::UkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = (double*)h->dP.get(); p.x = (double*)h->dx.get(); p.n_sq = h->ukf.dnsq; p.v_age = h->ukf.dvage; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride;
        double s, c;   // x_t << x_0, y_0, cos(yaw_0), sin(yaw_0) with a float argument (ukf.cpp:33)
        slam::det_sincos((double)yaw0, &s, &c);
        p.x0 = x0; p.y0 = y0;
        p.c0 = h->cfg.ukf_float_trig ? (double)(float)c : c;
        p.s0 = h->cfg.ukf_float_trig ? (double)(float)s : s;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        HIP_TRY(slam::launch_ukf_init(p, h->stream));
    }
    h->step = 0;
    h->inited = true;
    h->sense.pending = false;
    TRY(nav_reset(h));
    TRY(map_track_reset(h));
    if (h->shadow) return slam_init(h->shadow, x0, y0, yaw0);
    return SLAM_OK;
}

int slam_set_map(slam_handle* h, const double* map_xy, int L) {
    if (!h || !map_xy || L <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad map");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (h->dmap) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(h->dmap.reserve(2 * (size_t)L));
    HIP_TRY(hipMemcpyAsync(h->dmap, map_xy, sizeof(double) * 2 * (size_t)L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->kind == SLAM_UKF_LOC) {   // trueMapCallback: filter->map = [id, x, y] float32 (localization_node.cpp:152-156)
        std::vector<float> trip((size_t)3 * L);
        for (int i = 0; i < L; ++i) { trip[3 * i] = (float)i; trip[3 * i + 1] = (float)map_xy[2 * i]; trip[3 * i + 2] = (float)map_xy[2 * i + 1]; }
        HIP_TRY(h->ukf.dmapf.reserve(trip.size()));
        HIP_TRY(hipMemcpy(h->ukf.dmapf, trip.data(), sizeof(float) * trip.size(), hipMemcpyHostToDevice));
    }
    h->L = L;
    h->each.maps_each = false;   // (after slam_set_maps: back to the shared map)
    h->hmap.assign(map_xy, map_xy + 2 * (size_t)L);
    if (h->shadow) { const int rs = slam_set_map(h->shadow, map_xy, L); if (rs) return rs; }
    return SLAM_OK;
}

// ---- heterogeneous batches: per-instance start poses, maps and commands ---------------------------------------------------------------
int slam_init_each(slam_handle* h, const float* pose0, const double* truth0) {
    if (!h || !pose0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    if (h->kind == SLAM_EKF_SLAM) {
        HIP_TRY(h->each.dpose_each.reserve(3 * B));
        if (truth0) HIP_TRY(h->each.dstart_each.reserve(3 * B));
        HIP_TRY(hipMemcpyAsync(h->each.dpose_each, pose0, sizeof(float) * 3 * B, hipMemcpyHostToDevice, h->stream));
        if (truth0) HIP_TRY(hipMemcpyAsync(h->each.dstart_each, truth0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, h->stream));
        slam::EkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = h->dP; p.x = h->dx; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride; p.f32_storage = h->esz == 4;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        p.pose_each = h->each.dpose_each; p.truth_each = truth0 ? h->each.dstart_each.get() : nullptr;
        HIP_TRY(slam::launch_ekf_init(p, h->stream));
    } else {
        // x_t << x_0, y_0, cos(yaw_0), sin(yaw_0) with a float argument (ukf.cpp:33), per instance as slam_init computes it
        std::vector<double> st(7 * B);
        for (size_t b = 0; b < B; ++b) {
            double sn, cs;
            slam::det_sincos((double)pose0[3 * b + 2], &sn, &cs);
            st[4 * b] = pose0[3 * b]; st[4 * b + 1] = pose0[3 * b + 1];
            st[4 * b + 2] = h->cfg.ukf_float_trig ? (double)(float)cs : cs;
            st[4 * b + 3] = h->cfg.ukf_float_trig ? (double)(float)sn : sn;
        }
        if (truth0) memcpy(st.data() + 4 * B, truth0, sizeof(double) * 3 * B);
        HIP_TRY(h->each.dstart_each.reserve(7 * B));
        HIP_TRY(hipMemcpyAsync(h->each.dstart_each, st.data(), sizeof(double) * (truth0 ? 7 : 4) * B, hipMemcpyHostToDevice, h->stream));
        slam::UkfInitParams p;
        memset(&p, 0, sizeof(p));
        p.P = (double*)h->dP.get(); p.x = (double*)h->dx.get(); p.n_sq = h->ukf.dnsq; p.v_age = h->ukf.dvage; p.M = h->dM; p.flags = h->dflags; p.timestep = h->dts; p.truth = h->dtruth; p.err_sum = h->derr;
        p.B = h->B; p.pstride = h->pstride; p.xstride = h->xstride;
        p.tx = h->cfg.init_x; p.ty = h->cfg.init_y; p.tyaw = h->cfg.init_yaw;
        p.x_each = h->each.dstart_each; p.truth_each = truth0 ? h->each.dstart_each + 4 * B : nullptr;
        HIP_TRY(slam::launch_ukf_init(p, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));   // (the host vector of the UKF is staged; the buffers are free for the next call)
    h->step = 0;
    h->inited = true;
    h->sense.pending = false;
    TRY(nav_reset(h));
    TRY(map_track_reset(h));
    if (h->shadow) return slam_init_each(h->shadow, pose0 + 3 * (size_t)h->tracked, truth0 ? truth0 + 3 * (size_t)h->tracked : nullptr);
    return SLAM_OK;
}

int slam_set_maps(slam_handle* h, const double* maps, const int32_t* L, int L_stride) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind == SLAM_UKF_LOC) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "UKF_LOC localises against one known map: slam_set_map");
    if (!maps || !L || L_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    const size_t B = (size_t)h->B;
    int Lmax = 0;
    for (size_t b = 0; b < B; ++b) {
        if (L[b] <= 0 || L[b] > L_stride) return slam_internal_fail(SLAM_ERR_ARG, "instance %zu: %d landmarks, outside [1, L_stride = %d]", b, L[b], L_stride);
        Lmax = L[b] > Lmax ? L[b] : Lmax;
    }
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    const size_t nm = 2 * (size_t)L_stride * B;
    if (h->each.dmaps.cap() < nm || h->each.dLs.cap() < B) {   // both new blocks first: a failure leaves the handle with the maps it had
        DevBuf<double> m; DevBuf<int32_t> l;
        HIP_TRY(m.reserve(nm)); HIP_TRY(l.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));     // the launches that read the old ones are done
        h->each.dmaps = std::move(m); h->each.dLs = std::move(l);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(hipMemcpyAsync(h->each.dmaps, maps, sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->each.dLs, L, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->each.maps_each = true; h->each.map_stride = L_stride; h->L = Lmax;
    if (h->kind == SLAM_EKF_SLAM) {   // the shadow of slam_track_instance (EKF handles only) takes its slice
        h->each.hmaps.assign(maps, maps + nm);
        h->each.hLs.assign(L, L + B);
    }
    if (h->shadow) return slam_set_maps(h->shadow, maps + (size_t)h->tracked * L_stride * 2, L + h->tracked, L_stride);
    return SLAM_OK;
}

int slam_noise_from_config(const slam_config* cfg, slam_noise* out) {
    if (!cfg || !out) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    slam_host::noise_from_config(*cfg, out);
    return SLAM_OK;
}

int slam_set_noise_each(slam_handle* h, const slam_noise* rows) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    const size_t B = (size_t)h->B;
    std::vector<slam::NoiseRow> packed(rows ? B : 0);
    if (rows) {
        size_t bad = 0; const char* field = nullptr;
        if (slam_host::noise_pack(rows, B, h->cfg.replicate_vw_quirk, packed.data(), &bad, &field))
            return slam_internal_fail(SLAM_ERR_ARG, "instance %zu: noise field %s is not finite", bad, field);
    }
    TRY(flush_lazy(h));   // the timesteps accepted so far keep the values they were accepted with
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    HIP_TRY(hipSetDevice(h->device));
    // the shadow of slam_track_instance first (its row, or back to its config): if that fails, the batch keeps the rows it had
    if (h->shadow) TRY(slam_set_noise_each(h->shadow, rows ? rows + h->tracked : nullptr));
    if (!rows) {
        h->each.noise_each = false; h->each.hnoise.clear();   // (the launches in flight keep reading dnoise: it stays allocated)
        return SLAM_OK;
    }
    if (h->each.dnoise.cap() < B) {   // the new block first: a failure leaves the handle with the rows it had
        DevBuf<slam::NoiseRow> d;
        HIP_TRY(d.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->each.dnoise = std::move(d);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));   // the launches that read the old rows are done
    }
    for (int i = 0; i < 3; ++i)
        if (h->ukf.aux_stream[i]) HIP_TRY(hipStreamSynchronize(h->ukf.aux_stream[i]));
    HIP_TRY(hipMemcpyAsync(h->each.dnoise, packed.data(), sizeof(slam::NoiseRow) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->each.noise_each = true;
    h->each.hnoise.assign(rows, rows + B);
    return SLAM_OK;
}

}  // extern "C"
