// capi_consistency.cpp — C ABI: NEES consistency statistics (consistency_kernel.hip)
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "slam_handle.h"
#include "consistency_kernel.h"
#include "ekf_kernel.h"

using namespace slam_capi;

int slam_capi::consistency_params(slam_handle* h, slam::ConsistencyParams* out, int* chunk_out) {
    const size_t B = (size_t)h->B;
    HIP_TRY(h->cons.dcons.reserve(3 * B));
    HIP_TRY(h->cons.dconsi.reserve(2 * B));
    // beyond the LDS classes the packed triangles live in a workspace of at most SLAM_CONSISTENCY_WS_BYTES (default 256 MiB; one
    // instance at least), and the batch is processed in chunks of as many instances as it holds
    const size_t per = slam::consistency_ws_per_instance(h->L_max);
    int chunk = h->B;
    if (per) {
        const char* env = getenv("SLAM_CONSISTENCY_WS_BYTES");
        const double budget = env ? atof(env) : 256.0 * 1024 * 1024;
        const double fit = budget / (8.0 * (double)per);
        chunk = fit >= (double)h->B ? h->B : (fit >= 1.0 ? (int)fit : 1);
        HIP_TRY(h->cons.dcons_ws.reserve(per * (size_t)chunk));
    }
    slam::ConsistencyParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.ids = h->dids; p.status = h->dflags; p.truth = h->dtruth;
    p.map = h->dmap; p.L = h->L;
    if (h->each.maps_each) { p.map_each = h->each.dmaps; p.L_each = h->each.dLs; p.map_stride = h->each.map_stride; }
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    p.id_known = h->cfg.landmark_id_is_known ? 1 : 0;
    p.nees_full = h->cons.dcons; p.nees_pose = h->cons.dcons + B; p.map_rms = h->cons.dcons + 2 * B; p.dof = h->cons.dconsi; p.flags = h->cons.dconsi + B;
    p.ws = h->cons.dcons_ws; p.ws_stride = per;
    *out = p; *chunk_out = chunk;
    return SLAM_OK;
}

extern "C" {

int slam_consistency(slam_handle* h, double* nees_full, double* nees_pose, double* map_rms, int32_t* dof, int32_t* flags) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "slam_consistency is defined for EKF_SLAM only: the UKF state carries (cos yaw, sin yaw), so its P is rank-deficient "
                                  "along the unit circle by construction and indefinite in most steps - a NEES there needs a definition first");
    TRY(flush_lazy(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->L <= 0 || !(h->each.maps_each ? (bool)h->each.dmaps : (bool)h->dmap))
        return slam_internal_fail(SLAM_ERR_STATE, "no true map to compare the landmarks with: call slam_set_map (or slam_set_maps) first");
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    slam::ConsistencyParams p;
    int chunk = 0;
    TRY(consistency_params(h, &p, &chunk));
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], h->stream);
    if (e == hipSuccess) e = slam::launch_consistency(p, h->esz == 4, chunk, h->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[1], h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    float ms = -1.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (e != hipSuccess) { (void)hipGetLastError(); return slam_internal_fail(SLAM_ERR_HIP, "slam_consistency -> %s", hipGetErrorString(e)); }
    std::vector<int32_t> hd(B);
    HIP_TRY(hipMemcpy(hd.data(), h->cons.dconsi, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    // the model: P once (the n rows of ld elements that are factored), x, ids, M, status, truth, the landmarks' map rows, the outputs
    double bytes = 0.0;
    for (size_t b = 0; b < B; ++b) {
        const int n = hd[b], m = (n - 3) / 2;
        const int nf = (!p.id_known && m > 0) ? 3 : n;
        bytes += (double)nf * slam::ekf_ld(n, h->esz) * h->esz + (double)nf * h->esz + 4.0 * (nf > 3 ? m : 0) + 8.0 + 24.0 + 16.0 * (nf > 3 ? m : 0) + 32.0;
    }
    h->cons.cons_bytes = bytes; h->cons.cons_ms = (double)ms;
    if (dof) memcpy(dof, hd.data(), sizeof(int32_t) * B);
    if (nees_full) HIP_TRY(hipMemcpy(nees_full, h->cons.dcons, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (nees_pose) HIP_TRY(hipMemcpy(nees_pose, h->cons.dcons + B, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (map_rms) HIP_TRY(hipMemcpy(map_rms, h->cons.dcons + 2 * B, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, h->cons.dconsi + B, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_last_consistency_work(slam_handle* h, double* bytes, double* ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->cons.cons_ms < 0.0) return slam_internal_fail(SLAM_ERR_STATE, "slam_consistency has not run on this handle");
    if (bytes) *bytes = h->cons.cons_bytes;
    if (ms) *ms = h->cons.cons_ms;
    return SLAM_OK;
}

}  // extern "C"
