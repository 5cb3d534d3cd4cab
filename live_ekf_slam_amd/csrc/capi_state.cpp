// capi_state.cpp — C ABI: reading a handle back.  The getters, the error statistics, checkpoint save / load, slam_track_instance,
// slam_sync, the counters, kernel information and the debug reads.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "slam_handle.h"
#include "ekf_kernel.h"
#include "ukf_kernel.h"

using namespace slam_capi;

extern "C" {

// UKFState.X (ukf.cpp:92-101): the sigma points of the last predictionStage, column-major n x (2n+1):
// X = [x, x + offset i, x - offset i] with offset i = row i of sqtP (ukf.cpp:214-219) around the x_t that step started from.
int slam_get_sigma_points(slam_handle* h, int inst, double* X, int32_t* rows, int32_t* cols) {
    if (!h || inst < 0 || inst >= h->B) return slam_internal_fail(SLAM_ERR_ARG, "bad instance");
    TRY(flush_lazy(h));
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "sigma points exist for the UKF kinds only");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int32_t n = 0;
    HIP_TRY(hipMemcpy(&n, h->ukf.dnsq + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    n = n < 0 ? 0 : (n > h->n_max ? h->n_max : n);
    if (rows) *rows = n;
    if (cols) *cols = n > 0 ? 2 * n + 1 : 0;
    if (!X || n <= 0) return SLAM_OK;
    std::vector<double> x(n), S((size_t)n * n);
    HIP_TRY(hipMemcpy(x.data(), h->ukf.dxprev + (size_t)inst * h->xstride, sizeof(double) * n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(S.data(), h->ukf.dsq + (size_t)inst * h->pstride, sizeof(double) * (size_t)n * n, hipMemcpyDeviceToHost));
    // offset i = row i of sqtP, as ukf_step_kernel reads it: the symmetric eigen root (both halves written from one value) or, in
    // SLAM_UKF_SQRT_CHOLESKY mode, L^T row-major, whose row i is column i of L
    for (int r = 0; r < n; ++r) X[r] = x[r];
    for (int i = 0; i < n; ++i)
        for (int r = 0; r < n; ++r) {
            X[(size_t)(1 + i) * n + r] = x[r] + S[(size_t)i * n + r];
            X[(size_t)(1 + n + i) * n + r] = x[r] - S[(size_t)i * n + r];
        }
    return SLAM_OK;
}

// device -> host copy of `count` stored elements, widened to double when the storage type is fp32
static int fetch_elems(slam_handle* h, double* dst, const void* dbase, size_t elem_offset, size_t count) {
    if (h->esz == 8) {
        HIP_TRY(hipMemcpy(dst, (const char*)dbase + elem_offset * 8, count * 8, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp(count);
        HIP_TRY(hipMemcpy(tmp.data(), (const char*)dbase + elem_offset * 4, count * 4, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < count; ++i) dst[i] = (double)tmp[i];
    }
    return SLAM_OK;
}

int slam_get_state(slam_handle* h, int inst, double* x, double* P, int32_t* M, int32_t* ids, int32_t* ts) {
    if (!h || inst < 0 || inst >= h->B) return slam_internal_fail(SLAM_ERR_ARG, "bad instance");
    if (h->shadow && inst == h->tracked) return slam_get_state(h->shadow, 0, x, P, M, ids, ts);   // the batch's queue stays queued
    TRY(flush_lazy(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int32_t m = 0;
    HIP_TRY(hipMemcpy(&m, h->dM + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    m = m < 0 ? 0 : (m > h->L_max ? h->L_max : m);   // never index past the caller's n_max-sized buffers
    const int n = h->base + 2 * m;
    if (M) *M = m;
    int rc;
    if (x && (rc = fetch_elems(h, x, h->dx, (size_t)inst * h->xstride, n))) return rc;
    if (P) {   // rows of the device matrix are ld elements apart (pad columns beyond n); the caller gets packed n x n
        const int ld = h->kind == SLAM_EKF_SLAM ? slam::ekf_ld(n, h->esz) : n;
        std::vector<double> tmp((size_t)n * ld);
        if ((rc = fetch_elems(h, tmp.data(), h->dP, (size_t)inst * h->pstride, (size_t)n * ld))) return rc;
        for (int r = 0; r < n; ++r) memcpy(P + (size_t)r * n, tmp.data() + (size_t)r * ld, sizeof(double) * n);
    }
    if (ids && m > 0) HIP_TRY(hipMemcpy(ids, h->dids + (size_t)inst * h->L_max, sizeof(int32_t) * m, hipMemcpyDeviceToHost));
    if (ts) HIP_TRY(hipMemcpy(ts, h->dts + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_get_poses(slam_handle* h, double* poses) {
    if (!h || !poses) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->esz == 8) {
        HIP_TRY(hipMemcpy2D(poses, sizeof(double) * 3, h->dx, sizeof(double) * h->xstride, sizeof(double) * 3, h->B, hipMemcpyDeviceToHost));
    } else {
        std::vector<float> tmp((size_t)3 * h->B);
        HIP_TRY(hipMemcpy2D(tmp.data(), sizeof(float) * 3, h->dx, sizeof(float) * h->xstride, sizeof(float) * 3, h->B, hipMemcpyDeviceToHost));
        for (size_t i = 0; i < tmp.size(); ++i) poses[i] = (double)tmp[i];
    }
    return SLAM_OK;
}

static int copy_out(slam_handle* h, void* dst, const void* src, size_t bytes) {
    if (!h || !dst) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
    return SLAM_OK;
}
int slam_get_landmark_counts(slam_handle* h, int32_t* M) { return copy_out(h, M, h ? h->dM : nullptr, h ? sizeof(int32_t) * (size_t)h->B : 0); }
int slam_get_truth(slam_handle* h, double* t) { return copy_out(h, t, h ? h->dtruth : nullptr, h ? sizeof(double) * 3 * (size_t)h->B : 0); }
int slam_status(slam_handle* h, int32_t* f) { return copy_out(h, f, h ? h->dflags : nullptr, h ? sizeof(int32_t) * (size_t)h->B : 0); }

int slam_get_last_meas(slam_handle* h, float* meas, int32_t* count, int k_stride) {
    if (!h || !meas || !count || k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (!h->dump_meas || h->k_stride < k_stride) {
        // enable the dump for subsequent slam_step_sim calls; nothing recorded yet for past steps
        int rc = ensure_meas_buffers(h, k_stride);
        if (rc) return rc;
        if (!h->dump_meas) {
            h->dump_meas = true;
            memset(count, 0, sizeof(int32_t) * (size_t)h->B);
            return SLAM_OK;
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy2D(meas, sizeof(float) * 3 * k_stride, h->dmeas, sizeof(float) * 3 * h->k_stride,
                        sizeof(float) * 3 * k_stride, h->B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(count, h->dcount, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_error_stats(slam_handle* h, double* avg) {
    if (!h || !avg) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    std::vector<int32_t> ts(h->B);
    int rc = copy_out(h, avg, h->derr, sizeof(double) * (size_t)h->B);
    if (rc) return rc;
    rc = copy_out(h, ts.data(), h->dts, sizeof(int32_t) * (size_t)h->B);
    if (rc) return rc;
    for (int i = 0; i < h->B; ++i) avg[i] = ts[i] > 0 ? avg[i] / ts[i] : 0.0;  // sum(errors) / num_iters
    return SLAM_OK;
}

extern "C" int slam_internal_error_stats_dev(slam_handle* h, double* d_out, long long pad) {
    if (!h || !d_out || pad < h->B) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(slam::launch_avg_error(h->derr, h->dts, h->B, (int)pad, d_out, h->stream));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    return SLAM_OK;
}

// ---- checkpoint / resume (the reference keeps the filter only in memory) ------------------------------
namespace {
struct CkptHeader {
    char magic[8];            // "SLAMCKP1"
    int32_t kind, B, L_max, dtype, n_max, pstride, xstride, esz;
    uint32_t step;
    int32_t inited, reserved0;
    uint64_t seed;
    int64_t inst0;
};
struct CkptItem { void* dev; size_t bytes; };

std::vector<CkptItem> ckpt_items(slam_handle* h) {
    const size_t B = (size_t)h->B, e = (size_t)h->esz;
    std::vector<CkptItem> it = {
        {h->dP, e * B * h->pstride}, {h->dx, e * B * h->xstride}, {h->dM, sizeof(int32_t) * B}, {h->dids, sizeof(int32_t) * B * h->L_max},
        {h->dflags, sizeof(int32_t) * B}, {h->dts, sizeof(int32_t) * B}, {h->dtruth, sizeof(double) * B * 3}, {h->derr, sizeof(double) * B},
    };
    if (h->kind != SLAM_EKF_SLAM) {   // UKF: the square root of the last prediction stage and the warm-start eigenvectors
        it.push_back({h->ukf.dsq, sizeof(double) * B * h->pstride}); it.push_back({h->ukf.dnsq, sizeof(int32_t) * B});
        it.push_back({h->ukf.dxprev, sizeof(double) * B * h->xstride}); it.push_back({h->ukf.dvt, sizeof(double) * B * h->pstride});
        it.push_back({h->ukf.dvage, sizeof(int32_t) * B});
    }
    return it;
}
}  // namespace

int slam_save_state(slam_handle* h, const char* path) {
    if (!h || !path) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    TRY(sense_idle(h, "slam_save_state"));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    FILE* f = fopen(path, "wb");
    if (!f) return slam_internal_fail(SLAM_ERR_IO, "cannot write %s", path);
    CkptHeader hd;
    memset(&hd, 0, sizeof(hd));
    memcpy(hd.magic, "SLAMCKP1", 8);
    hd.kind = h->kind; hd.B = h->B; hd.L_max = h->L_max; hd.dtype = h->dtype; hd.n_max = h->n_max; hd.pstride = h->pstride; hd.xstride = h->xstride;
    hd.esz = h->esz; hd.step = h->step; hd.inited = h->inited ? 1 : 0; hd.seed = h->seed; hd.inst0 = h->inst0;
    bool ok = fwrite(&hd, sizeof(hd), 1, f) == 1;
    std::vector<char> buf((size_t)64 << 20);
    for (const CkptItem& it : ckpt_items(h))
        for (size_t off = 0; ok && off < it.bytes; off += buf.size()) {
            const size_t nb = it.bytes - off < buf.size() ? it.bytes - off : buf.size();
            if (hipMemcpy(buf.data(), (const char*)it.dev + off, nb, hipMemcpyDeviceToHost) != hipSuccess) { fclose(f); return slam_internal_fail(SLAM_ERR_HIP, "copying the state to the host failed"); }
            ok = fwrite(buf.data(), 1, nb, f) == nb;
        }
    ok = (fclose(f) == 0) && ok;
    return ok ? SLAM_OK : slam_internal_fail(SLAM_ERR_IO, "short write to %s", path);
}

int slam_load_state(slam_handle* h, const char* path) {
    if (!h || !path) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    FILE* f = fopen(path, "rb");
    if (!f) return slam_internal_fail(SLAM_ERR_IO, "cannot open %s", path);
    CkptHeader hd;
    if (fread(&hd, sizeof(hd), 1, f) != 1 || memcmp(hd.magic, "SLAMCKP1", 8) != 0) { fclose(f); return slam_internal_fail(SLAM_ERR_IO, "%s is not a state file of this library", path); }
    if (hd.kind != h->kind || hd.B != h->B || hd.L_max != h->L_max || hd.dtype != h->dtype || hd.pstride != h->pstride || hd.xstride != h->xstride || hd.esz != h->esz) {
        fclose(f);
        return slam_internal_fail(SLAM_ERR_ARG, "%s holds kind %d, batch %d, L_max %d, dtype %d; the handle is kind %d, batch %d, L_max %d, dtype %d", path, hd.kind, hd.B, hd.L_max,
                                  hd.dtype, h->kind, h->B, h->L_max, h->dtype);
    }
    if (hd.n_max != h->n_max) { fclose(f); return slam_internal_fail(SLAM_ERR_ARG, "%s was written for a state capacity of %d, the handle has %d", path, hd.n_max, h->n_max); }
    // The step kernels trust the per-instance counters (n = 3 + 2 M sizes every loop over LDS and the instance's slab), so a
    // corrupted or hand-made file must be refused BEFORE anything reaches the device: landmark counts, the size of the UKF's
    // stored square root and the timesteps are checked on the host first.
    {
        const std::vector<CkptItem> items = ckpt_items(h);
        std::vector<size_t> off(items.size() + 1, sizeof(hd));
        for (size_t i = 0; i < items.size(); ++i) off[i + 1] = off[i] + items[i].bytes;
        std::vector<int32_t> col((size_t)h->B);
        auto column = [&](size_t item, const char* what, int lo, int hi) -> int {
            if (fseek(f, (long)off[item], SEEK_SET) != 0 || fread(col.data(), sizeof(int32_t), col.size(), f) != col.size()) return slam_internal_fail(SLAM_ERR_IO, "%s is truncated", path);
            for (size_t b = 0; b < col.size(); ++b)
                if (col[b] < lo || col[b] > hi) return slam_internal_fail(SLAM_ERR_ARG, "%s: %s of instance %zu is %d, outside [%d, %d]", path, what, b, col[b], lo, hi);
            return SLAM_OK;
        };
        int rc = column(2, "the landmark count", 0, h->L_max);
        if (!rc) rc = column(5, "the timestep", 0, INT32_MAX);
        if (!rc && h->kind != SLAM_EKF_SLAM) rc = column(9, "the size of the stored square root", 0, h->n_max);
        // -1 is the cold-start marker (ukf_init_kernel, and both sqrt kernels after SLAM_INST_SQRT_FAILED); the kernels count the
        // age up to kUkfWarmMaxAge = 100 and start cold from there, so nothing a run can produce lies outside [-1, 100].
        if (!rc && h->kind != SLAM_EKF_SLAM) rc = column(12, "the age of the warm-start eigenvectors", -1, 100);
        if (rc) { fclose(f); return rc; }
        if (fseek(f, (long)sizeof(hd), SEEK_SET) != 0) { fclose(f); return slam_internal_fail(SLAM_ERR_IO, "cannot rewind %s", path); }
    }
    std::vector<char> buf((size_t)64 << 20);
    for (const CkptItem& it : ckpt_items(h))
        for (size_t off = 0; off < it.bytes; off += buf.size()) {
            const size_t nb = it.bytes - off < buf.size() ? it.bytes - off : buf.size();
            if (fread(buf.data(), 1, nb, f) != nb) { fclose(f); return slam_internal_fail(SLAM_ERR_IO, "%s is truncated", path); }
            if (hipMemcpy((char*)it.dev + off, buf.data(), nb, hipMemcpyHostToDevice) != hipSuccess) { fclose(f); return slam_internal_fail(SLAM_ERR_HIP, "copying the state to the device failed"); }
        }
    fclose(f);
    h->step = hd.step; h->inited = hd.inited != 0; h->seed = hd.seed; h->inst0 = hd.inst0;
    h->ukf.predicted = false;
    h->sense.pending = false;
    TRY(map_track_reset(h));   // (the counters are no part of a checkpoint)
    if (h->shadow) {   // the tracked instance restarts from the loaded state
        const int tr = h->tracked;
        const int rc = slam_track_instance(h, tr);
        if (rc) return rc;
    }
    return SLAM_OK;
}

int slam_track_instance(slam_handle* h, int inst) {
    if (!h || inst >= h->B) return slam_internal_fail(SLAM_ERR_ARG, "bad instance");
    TRY(flush_lazy(h));
    if (h->ukf.predicted) return slam_internal_fail(SLAM_ERR_STATE, "a prediction stage is pending: call slam_update_dev first");
    if (h->shadow) { slam_destroy(h->shadow); h->shadow = nullptr; h->tracked = -1; }
    if (inst < 0) return SLAM_OK;
    if (h->kind != SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "EKF handles only: the UKF launches every step at the call, there is no queue a getter would have to run");
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    slam_handle* s = nullptr;
    int rc = slam_create(&h->cfg, h->kind, 1, h->L_max, h->dtype, h->device, &s);
    if (rc) return rc;
    s->lazy_max = 0;                     // every step of the shadow is launched at the call
    s->seed = h->seed; s->inst0 = h->inst0 + inst;
    s->range_max = h->range_max; s->fov_min = h->fov_min; s->fov_max = h->fov_max;
    s->waves_per_filter = h->waves_per_filter;
    if (!h->hmap.empty()) rc = slam_set_map(s, h->hmap.data(), (int)(h->hmap.size() / 2));
    if (!rc && h->each.maps_each)   // the instance's own map (set after the shared one, which it replaces)
        rc = slam_set_maps(s, h->each.hmaps.data() + (size_t)inst * h->each.map_stride * 2, h->each.hLs.data() + inst, h->each.map_stride);
    if (!rc && h->each.noise_each) rc = slam_set_noise_each(s, h->each.hnoise.data() + inst);   // the instance's noise row
    if (!rc && h->inited) {
        // the instance's state as it is now: same slab layout (pstride / xstride depend on L_max and dtype only)
        const size_t b = (size_t)inst, e = (size_t)h->esz;
        hipError_t errs[] = {
            hipMemcpy(s->dP, (const char*)h->dP + b * h->pstride * e, (size_t)h->pstride * e, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dx, (const char*)h->dx + b * h->xstride * e, (size_t)h->xstride * e, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dM, h->dM + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dids, h->dids + b * h->L_max, sizeof(int32_t) * h->L_max, hipMemcpyDeviceToDevice),
            hipMemcpy(s->dflags, h->dflags + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dts, h->dts + b, sizeof(int32_t), hipMemcpyDeviceToDevice),
            hipMemcpy(s->dtruth, h->dtruth + 3 * b, sizeof(double) * 3, hipMemcpyDeviceToDevice),
            hipMemcpy(s->derr, h->derr + b, sizeof(double), hipMemcpyDeviceToDevice),
            h->ukf.dsq ? hipMemcpy(s->ukf.dsq, h->ukf.dsq + b * h->pstride, sizeof(double) * h->pstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->ukf.dnsq ? hipMemcpy(s->ukf.dnsq, h->ukf.dnsq + b, sizeof(int32_t), hipMemcpyDeviceToDevice) : hipSuccess,
            h->ukf.dxprev ? hipMemcpy(s->ukf.dxprev, h->ukf.dxprev + b * h->xstride, sizeof(double) * h->xstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->ukf.dvt ? hipMemcpy(s->ukf.dvt, h->ukf.dvt + b * h->pstride, sizeof(double) * h->pstride, hipMemcpyDeviceToDevice) : hipSuccess,
            h->ukf.dvage ? hipMemcpy(s->ukf.dvage, h->ukf.dvage + b, sizeof(int32_t), hipMemcpyDeviceToDevice) : hipSuccess,
        };
        for (hipError_t ee : errs)
            if (ee != hipSuccess) { slam_destroy(s); return slam_internal_fail(SLAM_ERR_HIP, "copying the tracked instance -> %s", hipGetErrorString(ee)); }
        s->step = h->step; s->inited = true;
    }
    if (rc) { slam_destroy(s); return rc; }
    h->shadow = s; h->tracked = inst;
    return SLAM_OK;
}

int slam_sync(slam_handle* h) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->eager_target = h->eager_init;   // the pipeline is drained: the next burst of calls fills it from small launches again
    return SLAM_OK;
}
int slam_batch(const slam_handle* h) { return h ? h->B : 0; }
int slam_state_dim_max(const slam_handle* h) { return h ? h->n_max : 0; }

// Per-timestep stamps of the EKF multi-step kernel (flag 32) / phase cycle counters (flag 4) for subsequent launches; 0 = off.
// The ablation bits are honoured by -DSLAM_ABLATE builds only.
int slam_set_debug_flags(slam_handle* h, int flags) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
#ifndef SLAM_ABLATE
    flags &= (4 | 32 | 128 | 1024);   // 128: tests only, provokes the watchdog of the EKF step kernel; 1024: tests only, every update of the
                                      // decoupled loop takes the deferred order (thin work before its ring slot), same results
#endif
    if ((flags & (4 | 32)) && !h->dprof) {
        HIP_TRY(h->dprof.reserve(slam::kEkfProfSlots * (size_t)h->B));
        HIP_TRY(hipMemset(h->dprof, 0, sizeof(unsigned long long) * h->dprof.cap()));
    }
    h->dbg = flags;
    return SLAM_OK;
}

int slam_variant_available(int L_max, int dtype, int variant) { return slam::ekf_variant_available(L_max, dtype == SLAM_F32, variant); }

int slam_k_histogram(slam_handle* h, uint64_t out[8], int reset) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(h->kind == SLAM_EKF_SLAM ? hipStreamSynchronize(h->stream) : hipDeviceSynchronize());
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "histogram element size");
    HIP_TRY(hipMemcpy(out, h->dkhist, sizeof(uint64_t) * 8, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist, 0, sizeof(uint64_t) * 8));
    return SLAM_OK;
}

int slam_traffic_counters(slam_handle* h, uint64_t out[4], int reset) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind != SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "the traffic counters are kept by the EKF step kernels");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->dkhist + slam::kEkfTrafficSlot, sizeof(uint64_t) * 4, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + slam::kEkfTrafficSlot, 0, sizeof(uint64_t) * 4));
    return SLAM_OK;
}

// Both counter sets zeroed IN STREAM ORDER, without a host round trip (round 6): a measurement that resets the counters between its
// warm-up and its timed launches no longer leaves the device idle for the reads and resets - profiles/r06a/launch_edges.txt: an idle
// device before a 20-step launch costs it 9 % (clocks).
int slam_reset_counters_async(slam_handle* h) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->dkhist, 0, sizeof(unsigned long long) * 16, h->stream));
    return SLAM_OK;
}

int slam_kernel_info(slam_handle* h, int multi_step, char* name, int name_cap, int32_t out[5]) {
    if (!h || (!name && !out)) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind != SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "EKF handles only");
    HIP_TRY(hipSetDevice(h->device));
    slam::EkfKernelInfo ki;
    HIP_TRY(slam::ekf_kernel_info(h->L_max, h->B, h->waves_per_filter, h->esz == 4, multi_step ? 1 : 0, &ki));
    if (name && name_cap > 0) { strncpy(name, ki.name, (size_t)name_cap - 1); name[name_cap - 1] = 0; }
    if (out) {
        hipDeviceProp_t pr;
        HIP_TRY(hipGetDeviceProperties(&pr, h->device));
        out[0] = ki.lds_bytes; out[1] = ki.vgprs; out[2] = ki.threads; out[3] = ki.wg_per_cu; out[4] = pr.multiProcessorCount;
    }
    return SLAM_OK;
}

int slam_ukf_sweep_stats(slam_handle* h, uint64_t out[2], int reset) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_STATE, "UKF handles only");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());   // the UKF splits large batches over two streams
    HIP_TRY(hipMemcpy(out, h->dkhist + 8, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + 8, 0, sizeof(uint64_t) * 2));
    return SLAM_OK;
}

int slam_ukf_set_sqrt_mode(slam_handle* h, int mode) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_ARG, "the square-root mode is a UKF setting");
    if (mode != SLAM_UKF_SQRT_EIGEN && mode != SLAM_UKF_SQRT_CHOLESKY) return slam_internal_fail(SLAM_ERR_ARG, "unknown square-root mode %d", mode);
    if (mode == SLAM_UKF_SQRT_CHOLESKY && h->L_max > slam::kUkfLdsMaxLandmarks)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "the Cholesky square root exists for the LDS size classes only (L_max <= %d), this handle has L_max %d",
                                  slam::kUkfLdsMaxLandmarks, h->L_max);
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    if (mode == SLAM_UKF_SQRT_CHOLESKY) HIP_TRY(h->ukf.dchol.reserve((size_t)h->B));
    h->ukf.chol = mode == SLAM_UKF_SQRT_CHOLESKY;
    return SLAM_OK;
}

int slam_ukf_sqrt_stats(slam_handle* h, uint64_t out[2], int reset) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (h->kind == SLAM_EKF_SLAM) return slam_internal_fail(SLAM_ERR_ARG, "UKF handles only");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipDeviceSynchronize());   // the UKF splits large batches over two streams
    HIP_TRY(hipMemcpy(out, h->dkhist + slam::kUkfCholSlot, sizeof(uint64_t) * 2, hipMemcpyDeviceToHost));
    if (reset) HIP_TRY(hipMemset(h->dkhist + slam::kUkfCholSlot, 0, sizeof(uint64_t) * 2));
    return SLAM_OK;
}

int slam_algorithmic_bytes(slam_handle* h, double* bytes) {
    if (!h || !bytes) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->dscalar, 0, sizeof(double), h->stream));
    HIP_TRY(slam::launch_algorithmic_bytes(h->dM, h->B, h->base, h->esz, h->dscalar, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(bytes, h->dscalar, sizeof(double), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// debug only (not declared in slam_batch.h): per-block phase cycles of the LAST launch, summed over blocks
// (SLAM_DEBUG_FLAGS & 4)
int slam_debug_read_prof(slam_handle* h, unsigned long long* out) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->dprof) return slam_internal_fail(SLAM_ERR_STATE, "SLAM_DEBUG_FLAGS has no timer bit (4 / 32) set");
    const size_t S = h->kind == SLAM_EKF_SLAM ? slam::kEkfProfSlots : 16;   // the UKF kernels use 16 slots per block
    std::vector<unsigned long long> buf(S * h->B);
    HIP_TRY(hipMemcpy(buf.data(), h->dprof, sizeof(unsigned long long) * buf.size(), hipMemcpyDeviceToHost));
    const int nslot = h->kind == SLAM_EKF_SLAM ? 64 : 16;   // out[64] for the EKF (slots 16.. = decoupled loop, 40.. = split control), out[16] for the UKF
    for (int i = 0; i < nslot; ++i) out[i] = 0;
    for (int b = 0; b < h->B; ++b)
        for (int i = 0; i < nslot; ++i) out[i] += buf[S * b + i];
    return SLAM_OK;
}

// debug only: the raw [B][16] buffer
int slam_debug_read_prof_raw(slam_handle* h, unsigned long long* out) {
    if (!h || !out) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (!h->dprof) return slam_internal_fail(SLAM_ERR_STATE, "SLAM_DEBUG_FLAGS has no timer bit (4 / 32) set");
    const size_t S = h->kind == SLAM_EKF_SLAM ? slam::kEkfProfSlots : 16;   // out: [B][S]
    HIP_TRY(hipMemcpy(out, h->dprof, sizeof(unsigned long long) * S * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// device math probe for the bit-exactness tests (a, b, out are HOST arrays; out has 8*n doubles)
int slam_math_probe(const double* a, const double* b, double* out, int n, int device) {
    if (!a || !b || !out || n <= 0) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> da, db, dout;   // (released on every return)
    HIP_TRY(da.reserve(n)); HIP_TRY(db.reserve(n)); HIP_TRY(dout.reserve(8 * (size_t)n));
    HIP_TRY(hipMemcpy(da, a, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(db, b, sizeof(double) * n, hipMemcpyHostToDevice));
    HIP_TRY(slam::launch_math_probe(da, db, dout, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * 8 * (size_t)n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// one shared function per call on HOST arrays (slam_batch.h); the kernel is in ukf_kernel.hip
int slam_math_probe2(int op, const double* a, const double* b, const double* c, const double* d, double* out, int out_per_item, int n, int device) {
    if (op < 0 || op >= slam::kProbeOps) return slam_internal_fail(SLAM_ERR_ARG, "unknown probe op");
    const int nin = slam::kProbeIn[op];
    const double* const in[4] = {a, b, c, d};
    for (int k = 0; k < nin; ++k)
        if (!in[k]) return slam_internal_fail(SLAM_ERR_ARG, "the op reads an input array that is NULL");
    if (!out || n <= 0 || out_per_item < slam::kProbeOut[op]) return slam_internal_fail(SLAM_ERR_ARG, "bad argument");
    HIP_TRY(hipSetDevice(device));
    DevBuf<double> din[4], dout;   // (released on every return)
    const double* dp[4] = {nullptr, nullptr, nullptr, nullptr};
    for (int k = 0; k < nin; ++k) {
        HIP_TRY(din[k].reserve(n));
        HIP_TRY(hipMemcpy(din[k], in[k], sizeof(double) * n, hipMemcpyHostToDevice));
        dp[k] = din[k];
    }
    const size_t nout = (size_t)out_per_item * (size_t)n;
    HIP_TRY(dout.reserve(nout));
    HIP_TRY(hipMemcpy(dout, out, sizeof(double) * nout, hipMemcpyHostToDevice));   // items beyond the op's outputs keep the caller's values
    HIP_TRY(slam::launch_math_probe2(op, dp[0], dp[1], dp[2], dp[3], dout, out_per_item, n, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(out, dout, sizeof(double) * nout, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

}  // extern "C"
