// pgs_capi.cpp — C ABI (include/slam_pgs.h) over the pose-graph kernels.  Host side only: owns the device memory,
// the stream and the lockstep timestep; every numeric operation happens in pgs_kernel.hip.  No CPU fallback.
#include "../../include/slam_pgs.h"

#include <hip/hip_runtime.h>
#include <math.h>
#include <sched.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include <thread>
#include <vector>

#include "pgs_handle.h"

#define fail slam_internal_fail

using pgs_capi::apply_robust;
using pgs_capi::check;
using pgs_capi::robust_args_ok;

static_assert(PGS_LOSS_NONE == slam::kPgsLossNone && PGS_LOSS_HUBER == slam::kPgsLossHuber && PGS_LOSS_GEMAN_MCCLURE == slam::kPgsLossGemanMcClure,
              "pgs_loss_kind (slam_pgs.h) and pgs_robust.h number the losses alike");

namespace {

// a device array of `count` T (at least one) for the field *field into `set`; per_slot > 0: a per-slot array of per_slot T the clones copy
template <class T>
int add_array(std::vector<pgs_handle::Array>& set, T** field, size_t count, size_t per_slot = 0) {
    pgs_handle::Array a{{}, (void**)field, per_slot * sizeof(T)};
    HIP_TRY(a.buf.reserve(sizeof(T) * (count ? count : 1)));
    set.push_back(std::move(a));
    return SLAM_OK;
}

void bind_arrays(std::vector<pgs_handle::Array>& set) { for (pgs_handle::Array& a : set) *a.field = a.buf.get(); }

}  // namespace

// The handle's loss settings into the parameter block the kernels get.  A loss - on the landmark factors, or on the fixes of a handle that has
// fixes - needs lin0 (8 bytes per factor slot and lambda lane): allocated here once; if that fails the call returns the error and the handle
// - parameter block included - is what it was.
int pgs_capi::apply_robust(pgs_handle* h) {
    const bool loss = h->loss_kind != slam::kPgsLossNone || (h->fix_kind && h->fix_loss_kind != slam::kPgsLossNone);
    if (loss && !h->rb_lin0) {
        DevBuf<double> a;
        if (a.reserve((size_t)h->B * h->tune.lanes * h->N_max * h->KP) != hipSuccess)
            return fail(SLAM_ERR_HIP, "out of device memory for the robust loss' per-factor terms (%zu bytes)", sizeof(double) * (size_t)h->B * h->tune.lanes * h->N_max * h->KP);
        h->rb_lin0 = std::move(a);
        h->p.lin0 = h->rb_lin0;
    }
    h->p.loss_kind = h->loss_kind; h->p.loss_k = h->loss_k;
    h->p.fix_loss_kind = h->fix_loss_kind; h->p.fix_loss_k = h->fix_loss_k;
    return SLAM_OK;
}

bool pgs_capi::robust_args_ok(int kind, double k) {
    if (kind == slam::kPgsLossNone) return true;
    return (kind == slam::kPgsLossHuber || kind == slam::kPgsLossGemanMcClure) && k > 0.0 && k < (double)INFINITY;   // (NaN fails both)
}

namespace {

// the layout of Y for segments of SL poses (0: the sequential chain): the separators' rows live behind the pose rows (pgs_kernel.h: yr_rc, yr_sep)
void seg_geometry(const pgs_handle* h, slam::PgsParams& g, int SL) {
    g.nseg_max = SL > 0 ? (h->N_max - 2) / SL + 1 : 1;
    g.yr_sep = g.yr_rc + 6 * (int64_t)g.nseg_max;
    g.y_stride = (int64_t)(g.yr_sep + round_up(3 * g.nseg_max, 4)) * h->LD;
}

// The arrays whose size follows the number of segments of geometry g, into `set` (for h->p's fields, not yet bound): the plan (the lambda
// lanes get copies of it), the segments' outputs and Gram matrices (segT: if with_segT), and Y.  Nothing in them outlives a solve.
int alloc_seg_arrays(pgs_handle* h, const slam::PgsParams& g, bool with_segT, std::vector<pgs_handle::Array>& set) {
    slam::PgsParams& p = h->p;
    const size_t S = (size_t)h->B * h->tune.lanes, L = (size_t)h->L_max, G = (size_t)g.nseg_max;
    if (h->tune.seg_len > 0) {
        const size_t NB = (size_t)slam::seg_nb1(h->L_max);
        TRY(add_array(set, &p.seg_ncol, S * G, G)); TRY(add_array(set, &p.seg_lm, S * G * L, G * L)); TRY(add_array(set, &p.seg_inv, S * G * L, G * L));
        TRY(add_array(set, &p.seg_evt, S * G * L, G * L)); TRY(add_array(set, &p.seg_blk, S * G * NB, G * NB)); TRY(add_array(set, &p.sep_evt, S * G * L, G * L));
        TRY(add_array(set, &p.segout, S * G * 32)); TRY(add_array(set, &p.sepfac, S * G * 16));
        if (with_segT) TRY(add_array(set, &p.segT, S * G * (size_t)p.seg_tld * p.seg_tld));
    }
    TRY(add_array(set, &p.Y, S * (size_t)g.y_stride));
    return SLAM_OK;
}

// the segments' Gram matrices: [slots][nseg_max][seg_tld^2] doubles, only when a solve runs the segmented order (128 x 128 per
// segment whatever L_max, allocated also for handles whose every solve takes the sequential chain)
int ensure_segT(pgs_handle* h) {
    if (h->p.segT || h->tune.seg_len <= 0) return SLAM_OK;
    const size_t S = (size_t)h->B * h->tune.lanes;
    TRY(add_array(h->seg_arrays, &h->p.segT, S * (size_t)h->p.nseg_max * (size_t)h->p.seg_tld * h->p.seg_tld));
    bind_arrays(h->seg_arrays);
    return SLAM_OK;
}

// The segment-count-dependent arrays re-made for segments of SL poses, if they were sized for longer ones: the whole new set is allocated
// before the old one is released and the geometry and seg_alloc are committed.  Out of memory: the old set and geometry stay, *resized = false
// and the solve takes the sequential chain.  (Both sets at once: at most twice per handle, at 32 -> 16 and 16 -> 8 poses per segment.)
int resize_segments(pgs_handle* h, int SL, bool* resized) {
    *resized = true;
    if (SL >= h->seg_alloc) return SLAM_OK;
    HIP_TRY(hipDeviceSynchronize());
    slam::PgsParams g = h->p;
    seg_geometry(h, g, SL);
    std::vector<pgs_handle::Array> set;
    if (alloc_seg_arrays(h, g, h->p.segT != nullptr, set) != SLAM_OK) { *resized = false; return SLAM_OK; }   // (`set` is released)
    h->seg_arrays.swap(set);   // the old set is released with `set`
    bind_arrays(h->seg_arrays);
    h->p.nseg_max = g.nseg_max; h->p.yr_sep = g.yr_sep; h->p.y_stride = g.y_stride;
    h->seg_alloc = SL;
    return SLAM_OK;
}

// pgs_init[_each]: the graph is empty again and no pose carries a fix (the fix arrays, once allocated, stay)
int clear_fixes(pgs_handle* h) {
    h->tick_dropped = false;
    if (!h->fix_kind) return SLAM_OK;
    HIP_TRY(hipMemsetAsync(h->fix_row, 0, sizeof(double) * slam::kPgsFixRowLen * (size_t)h->B * h->N_max, h->stream));
    HIP_TRY(hipMemsetAsync(h->fix_kind, 0, sizeof(int32_t) * (size_t)h->B * h->N_max, h->stream));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int pgs_create(const slam_config* cfg, int batch, int N_max, int L_max, int k_per_pose, int device, pgs_handle** out) {
    if (!cfg || !out) return fail(SLAM_ERR_ARG, "NULL argument");
    if (batch <= 0 || N_max < 2 || L_max <= 0 || k_per_pose <= 0) return fail(SLAM_ERR_ARG, "batch, N_max (>= 2), L_max and k_per_pose must be positive");
    if (L_max > 255) return fail(SLAM_ERR_UNSUPPORTED, "L_max %d exceeds the pose-graph kernel limit 255", L_max);
    if (!cfg->landmark_id_is_known) return fail(SLAM_ERR_UNSUPPORTED, "PGS with unknown landmark ID is not supported (the reference throws: pose_graph.cpp:137)");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(SLAM_ERR_HIP, "no HIP device available (this library has no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(SLAM_ERR_ARG, "device %d out of range (%d devices)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    pgs_handle* h = new pgs_handle();
    h->cfg = *cfg; h->B = batch; h->N_max = N_max; h->L_max = L_max; h->KP = k_per_pose; h->device = device;
    { int cu = 0; if (hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cu > 0) h->cus = cu; }
    h->LD = round_up(2 * L_max + 1, 64);
    h->tune = slam_host::PgsTuning::from_env();
    h->seg_cur = h->seg_alloc = h->tune.seg_len;
    hipError_t e = hipStreamCreate(&h->stream);
    if (e != hipSuccess) { delete h; return fail(SLAM_ERR_HIP, "hipStreamCreate -> %s", hipGetErrorString(e)); }
    h->own_stream = true;
    slam::PgsParams& p = h->p;
    memset(&p, 0, sizeof(p));
    p.b_off = 0; p.b_cnt = batch;
    p.B = batch; p.N_max = N_max; p.L_max = L_max; p.KP = k_per_pose; p.LD = h->LD; p.N = 1;
    const size_t B = batch, N = N_max, L = L_max, K = (size_t)N_max * k_per_pose;
    // Every per-instance array has `lanes` slots per instance: slot b is instance b, slot j * B + b its j-th lambda lane (a
    // clone that pgs_solve fills from the instance; PgsParams::lanes_max).  Arrays only the instance itself uses keep B slots.
    {   // the lanes multiply the LM work space (Y alone is 3 N_max x LD doubles per slot): keep them within half of the free memory
        const double nsegx = h->tune.seg_len > 0 ? (double)((N_max - 2) / h->tune.seg_len + 1) : 0.0;
        const double per_slot = 8.0 * (((double)round_up(3 * N_max, 4) + 10.0 * nsegx) * h->LD + (double)h->LD * h->LD + (double)K * 29 + (double)N * 51 + (double)L * 12 + nsegx * (48 + (double)round_up(2 * (L_max < slam::kPgsSegMaxLm ? L_max : slam::kPgsSegMaxLm) + 1, 16) * round_up(2 * (L_max < slam::kPgsSegMaxLm ? L_max : slam::kPgsSegMaxLm) + 1, 16))) +
                                4.0 * ((double)K * 5 + (double)N + (double)L * 6 + nsegx * (4.0 * L + 16));
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            while (h->tune.lanes > 1 && per_slot * (double)B * h->tune.lanes > 0.5 * (double)free_b) h->tune.lanes -= 1;
    }
    const size_t S = B * (size_t)h->tune.lanes;
    p.lanes_max = h->tune.lanes; p.lanes = 1;
    int rc = SLAM_OK;
    auto A = [&](auto** ptr, size_t count) { if (rc == SLAM_OK) rc = add_array(h->arrays, ptr, count); };
    // AC: S slots, and the clones get the instance's content when a solve begins (per-slot element count given)
    auto AC = [&](auto** ptr, size_t per_slot) { if (rc == SLAM_OK) rc = add_array(h->arrays, ptr, S * per_slot, per_slot); };
    auto D = [&](auto& buf, size_t count) { if (rc == SLAM_OK && buf.reserve(count) != hipSuccess) rc = fail(SLAM_ERR_HIP, "out of device memory"); };
    A(&p.pose0, B * N * 3); A(&p.lm0, B * L * 2); A(&p.pose1, B * N * 3); A(&p.lm1, B * L * 2);
    A(&p.ids, B * L); AC(&p.M, 1); A(&p.flags, S);
    AC(&p.cnt, N); AC(&p.mlm, K); AC(&p.mnext, K); AC(&p.lm_head, L); AC(&p.lm_last, L); AC(&p.lm_first, L);
    AC(&p.mb, K); AC(&p.mr, K);
    D(h->dcmds, N * 2); p.cmds = h->dcmds;
    A(&p.cur, B * 3); A(&p.truth, B * 3); A(&p.truth_hist, B * N * 2); A(&p.prior, B * 3);
    AC(&p.pw, N * 3); AC(&p.lw, L * 2); A(&p.pn, S * N * 3); A(&p.ln, S * L * 2);
    A(&p.A, S * N * 9); A(&p.C, S * N * 9); A(&p.gp, S * N * 3); A(&p.E, S * K * 6); A(&p.Wl, S * K * 5);
    AC(&p.evt_start, L + 1); AC(&p.evt_pose, K); AC(&p.slot_pos, K); AC(&p.evt_slot, K); A(&p.Elm, S * K * 6);
    A(&p.PF, S * K * 12); A(&p.lin_ok, S); A(&p.fact_cnt, B); A(&p.seg_umax, B);
    A(&p.D, S * L * 3); A(&p.gl, S * L * 2); A(&p.Linv, S * N * 6); A(&p.G, S * N * 9);
    // segmented elimination: the segments' contributions to their separators' right-hand sides and the separators' rows of Y live
    // behind the pose rows of Y (pgs_kernel.h: yr_rc, yr_sep)
    p.seg_len = h->tune.seg_len; p.seg_on = 0; p.syrk_rows = -1; p.syrk_row0 = 0; p.syrk_first = nullptr;
    p.seg_back_global = h->tune.seg_back_global;
    p.yr_rc = round_up(3 * N_max, 4);
    seg_geometry(h, p, h->tune.seg_len);
    if (h->tune.seg_len > 0) {
        AC(&p.sep_first, L); A(&p.Gs, S * N * 9);
        // (segT, the segments' Gram matrices - the largest of these arrays - is allocated by the first solve that runs the segmented order: ensure_segT)
        p.seg_tld = round_up(2 * (L_max < slam::kPgsSegMaxLm ? L_max : slam::kPgsSegMaxLm) + 1, 16);
    }
    if (rc == SLAM_OK) rc = alloc_seg_arrays(h, p, false, h->seg_arrays);   // the plan, the segments' outputs, Y
    A(&p.S, S * (size_t)h->LD * h->LD);
    A(&p.dl, S * L * 2); A(&p.dp, S * N * 3);
    A(&p.lambda, S); A(&p.error, B); A(&p.cur_error, B); A(&p.err_init, B);
    A(&p.iters, B); A(&p.trials, B); A(&p.state, S + 1); AC(&p.solve_ok, 1); A(&p.n_active, 64); A(&p.alist, S); A(&p.inst_flop, B); A(&p.work, 3);
    A(&p.nl, B); A(&p.nlin, S); A(&p.nerr, S); A(&p.nok, S); A(&p.oldlin, S);
    D(h->dcount, B); D(h->dsec, B * 3); D(h->dout, B);
    D(h->d_cnt, (size_t)slam_host::kPgsMaxGroups * 16); D(h->d_wait, (size_t)slam_host::kPgsMaxGroups);
    if (getenv("SLAM_PGS_PROF")) { A(&p.prof, S * 24); }   // [S][8] chol phase timers, then [S][2][8] per-workgroup stamps of the fused chain
    if (rc != SLAM_OK) { pgs_destroy(h); return rc; }
    bind_arrays(h->arrays); bind_arrays(h->seg_arrays);
    hipMemsetAsync(p.truth_hist, 0, sizeof(double) * B * N * 2, h->stream);
    p.dead_slot = (int32_t)S; p.slots_cap = 0; p.n_list_dev = nullptr; p.wait_next = h->d_wait;
    hipMemsetD32Async((hipDeviceptr_t)(p.state + S), 1, 1, h->stream);   // the slot every kernel returns for at entry (pgs_slot)
    hipMemsetAsync(p.cnt, 0, sizeof(int32_t) * B * N, h->stream);
    // effective noise after Filter::readCommonParams (filter.h:105-121)
    double V00, V11, W00, W11;
    if (cfg->replicate_vw_quirk) { V00 = cfg->W_00; V11 = cfg->W_11; W00 = 1.0; W11 = 1.0; }
    else { V00 = cfg->V_00; V11 = cfg->V_11; W00 = cfg->W_00; W11 = cfg->W_11; }
    const double sp[3] = {1.3, 1.3, 1.2};                      // pose_graph.cpp:83
    for (int k = 0; k < 3; ++k) p.w_prior[k] = 1.0 / sp[k];
    p.w_btw[0] = 1.0 / V00; p.w_btw[1] = 1.0 / V00; p.w_btw[2] = 1.0 / V11;   // :52
    p.w_meas[0] = 1.0 / W11; p.w_meas[1] = 1.0 / W00;                          // :54 (bearing, range)
    p.sV00 = cfg->V_00; p.sV11 = cfg->V_11; p.sW00 = cfg->W_00; p.sW11 = cfg->W_11;
    p.d_max = cfg->d_max; p.th_max = cfg->th_max;
    p.range_max = cfg->range_max; p.fov_min = cfg->fov_min; p.fov_max = cfg->fov_max;
    p.seed = h->seed; p.inst0 = 0;
    *out = h;
    return SLAM_OK;
}

int pgs_destroy(pgs_handle* h) {
    if (!h) return SLAM_OK;
    hipSetDevice(h->device);
    if (h->stream) hipStreamSynchronize(h->stream);
    for (hipEvent_t e : h->events) hipEventDestroy(e);
    for (hipEvent_t e : h->gevents) hipEventDestroy(e);
    for (hipEvent_t e : h->ring_events) hipEventDestroy(e);
    for (hipEvent_t e : h->mg_ev) if (e) hipEventDestroy(e);
    for (hipStream_t st : h->gstreams) hipStreamDestroy(st);
    if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
    delete h;   // the device and pinned buffers
    return SLAM_OK;
}

int pgs_set_stream(pgs_handle* h, void* s) {
    TRY(check(h));
    if (h->own_stream && h->stream) { hipStreamSynchronize(h->stream); hipStreamDestroy(h->stream); }
    h->stream = (hipStream_t)s; h->own_stream = false;
    return SLAM_OK;
}
int pgs_set_instance_offset(pgs_handle* h, int64_t first) { TRY(check(h)); h->inst0 = first; h->p.inst0 = first; return SLAM_OK; }
int pgs_set_seed(pgs_handle* h, uint64_t seed) { TRY(check(h)); h->seed = seed; h->p.seed = seed; return SLAM_OK; }

int pgs_set_map(pgs_handle* h, const double* map_xy, int L) {
    TRY(check(h));
    if (!map_xy || L <= 0) return fail(SLAM_ERR_ARG, "bad map");
    if (h->map) hipStreamSynchronize(h->stream);
    HIP_TRY(h->map.reserve(2 * (size_t)L));
    HIP_TRY(hipMemcpyAsync(h->map, map_xy, sizeof(double) * 2 * (size_t)L, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->p.map = h->map; h->p.L = L;
    h->p.map_each = nullptr; h->p.L_each = nullptr; h->p.map_stride = 0;   // back from per-instance maps (pgs_set_maps)
    return SLAM_OK;
}

int pgs_set_maps(pgs_handle* h, const double* maps, const int32_t* L, int L_stride) {
    TRY(check(h));
    if (!maps || !L || L_stride <= 0 || L_stride > 255) return fail(SLAM_ERR_ARG, "bad argument (maps, L, 1 <= L_stride <= 255)");
    const size_t B = (size_t)h->B;
    for (size_t b = 0; b < B; ++b) {
        if (L[b] <= 0 || L[b] > L_stride) return fail(SLAM_ERR_ARG, "instance %zu: %d landmarks, outside [1, L_stride = %d]", b, L[b], L_stride);
        for (size_t k = 0; k < 2 * (size_t)L[b]; ++k)
            if (!isfinite(maps[b * L_stride * 2 + k])) return fail(SLAM_ERR_ARG, "instance %zu: landmark %zu is not finite", b, k / 2);
    }
    const size_t nm = 2 * (size_t)L_stride * B;
    if (h->dmaps.cap() < nm || h->dLs.cap() < B) {   // both new blocks first: a failure leaves the handle with the maps it had
        DevBuf<double> m; DevBuf<int32_t> l;
        HIP_TRY(m.reserve(nm)); HIP_TRY(l.reserve(B));
        HIP_TRY(hipStreamSynchronize(h->stream));     // the launches that read the old ones are done
        h->dmaps = std::move(m); h->dLs = std::move(l);
    } else {
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    HIP_TRY(hipMemcpyAsync(h->dmaps, maps, sizeof(double) * nm, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->dLs, L, sizeof(int32_t) * B, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->p.map_each = h->dmaps; h->p.L_each = h->dLs; h->p.map_stride = L_stride;
    return SLAM_OK;
}

int pgs_init(pgs_handle* h, float x0, float y0, float yaw0) {
    TRY(check(h));
    h->invalidate_derived();
    h->timestep = 0; h->p.N = 1;
    h->seg_cur = h->tune.seg_len;
    TRY(clear_fixes(h));
    HIP_TRY(slam::pgs_launch_init(h->p, x0, y0, yaw0, h->stream));
    h->inited = true; h->solved = false;
    return SLAM_OK;
}

namespace {

bool all_finite_f(const float* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!isfinite(v[i])) return false; return true; }
bool all_finite_d(const double* v, size_t n) { for (size_t i = 0; i < n; ++i) if (!isfinite(v[i])) return false; return true; }

// First per-instance command of the handle: its BetweenFactor measurements move from the shared row to one row per instance (dcmds_each,
// 8 B N_max bytes), and the ticks the handle already has are broadcast into every row - they stay part of every instance's graph.
int ensure_cmds_each(pgs_handle* h) {
    if (h->p.cmd_stride) return SLAM_OK;
    DevBuf<float> rows;
    HIP_TRY(rows.reserve((size_t)h->B * h->N_max * 2));
    HIP_TRY(slam::pgs_launch_put_cmds(h->p, rows, 2 * h->N_max, 0, h->timestep, h->dcmds, 2, 0, h->stream));
    h->dcmds_each = std::move(rows);
    h->p.cmds = h->dcmds_each; h->p.cmd_stride = 2 * h->N_max;
    return SLAM_OK;
}

// The BetweenFactor measurements of the next T ticks (the caller has checked that they fit N_max).  each: src [T][B][2], one per instance
// (moves the handle to per-instance rows first); else src [T][2], written for every instance.  src_dev: a device pointer read in the order
// of the handle's stream; else a host array, staged - pageable, so a caller that returns to ITS caller synchronises the stream first.
int put_commands(pgs_handle* h, const float* src, bool src_dev, int T, bool each) {
    if (each) TRY(ensure_cmds_each(h));
    const size_t n = 2 * (size_t)T * (each ? (size_t)h->B : 1);
    if (!h->p.cmd_stride) {   // the shared row: straight into place
        HIP_TRY(hipMemcpyAsync(h->dcmds + 2 * (size_t)h->timestep, src, sizeof(float) * n, src_dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
        return SLAM_OK;
    }
    if (!src_dev) {
        HIP_TRY(h->dcmd_stage.reserve(n));
        HIP_TRY(hipMemcpyAsync(h->dcmd_stage, src, sizeof(float) * n, hipMemcpyHostToDevice, h->stream));
        src = h->dcmd_stage;
    }
    // per-instance rows: the [T][B][2] layout is transposed into them on the device; a shared command goes into every row
    HIP_TRY(slam::pgs_launch_put_cmds(h->p, h->dcmds_each, h->p.cmd_stride, h->timestep, T, src, each ? 2 * h->B : 2, each ? 2 : 0, h->stream));
    return SLAM_OK;
}

bool meas_args_ok(const float* meas, const int32_t* count, int k_stride) { return k_stride == 0 || (k_stride > 0 && meas && count); }

// What a call that adds ticks brings: one command per instance (else one for all), commands in device memory (else a host array), a run of
// the simulator (else one appended tick of messages); kBadMeasArgs: the caller found its measurement arguments unsound (pgs_update_each).
enum TickFlags : unsigned { kShared = 0, kEach = 1, kDeviceSource = 2, kSim = 4, kBadMeasArgs = 8 };

// What every call that adds T ticks to the graphs does before its own work, in this order: the handle is initialised; a run of the simulator
// has a map; the commands are there; the measurement arguments are sound; host commands per instance are finite; the T poses fit.  Then the
// marginals no longer belong to the values and the commands go into place (put_commands).
int enter_ticks(pgs_handle* h, const char* who, const float* cmds, int T, unsigned flags) {
    const bool each = flags & kEach, src_dev = flags & kDeviceSource, sim = flags & kSim;
    if (!h->inited) return fail(SLAM_ERR_STATE, "pgs_init must be called before %s", who);
    if (sim && !h->p.map && !h->p.map_each) return fail(SLAM_ERR_STATE, "pgs_set_map%s must be called before %s", each ? " or pgs_set_maps" : "", who);
    if (sim && (!cmds || T <= 0)) return fail(SLAM_ERR_ARG, "bad command sequence");
    if (!cmds) return fail(SLAM_ERR_ARG, each ? "cmds is NULL" : "cmd is NULL");
    if (flags & kBadMeasArgs) return fail(SLAM_ERR_ARG, "bad measurement arguments");
    if (each && !src_dev && !all_finite_f(cmds, 2 * (size_t)T * h->B)) return fail(SLAM_ERR_ARG, "a command is not finite");
    if (h->timestep + T >= h->N_max) {
        h->tick_dropped = true;   // (pgs_fix: the graph's newest pose is not the one this update was for)
        return sim ? fail(SLAM_ERR_STATE, "timestep %d + %d commands exceed the pose capacity N_max = %d", h->timestep, T, h->N_max)
                   : fail(SLAM_ERR_STATE, "pose capacity N_max = %d reached", h->N_max);
    }
    h->tick_dropped = false;
    h->invalidate_derived();
    return put_commands(h, cmds, src_dev, T, each);
}

// the graphs have T more poses (p.N = timestep + 1 at every launch)
void advance(pgs_handle* h, int T) { h->timestep += T; h->p.N = h->timestep + 1; }

// updateNaiveVehPoseEstimate + update of one tick on device messages; the tick's commands are in place
int append_tick(pgs_handle* h, const float* d_meas, const int32_t* d_count, int k_stride, const double* d_sec) {
    HIP_TRY(slam::pgs_launch_append(h->p, d_meas, d_count, k_stride, d_sec, h->stream));
    advance(h, 1);
    return SLAM_OK;
}

// host messages of one tick into the handle's staging buffers (pgs_update, pgs_update_each); *ks = the stride the append kernel gets
int stage_messages(pgs_handle* h, const float* meas, const int32_t* count, int k_stride, const double* sec, int* ks) {
    *ks = k_stride > 0 ? k_stride : 1;
    HIP_TRY(h->dmeas.reserve((size_t)3 * *ks * h->B));
    if (k_stride > 0) {
        HIP_TRY(hipMemcpyAsync(h->dmeas, meas, sizeof(float) * 3 * (size_t)k_stride * h->B, hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->dcount, count, sizeof(int32_t) * (size_t)h->B, hipMemcpyHostToDevice, h->stream));
    } else {
        HIP_TRY(hipMemsetAsync(h->dcount, 0, sizeof(int32_t) * (size_t)h->B, h->stream));
    }
    if (sec) HIP_TRY(hipMemcpyAsync(h->dsec, sec, sizeof(double) * 3 * (size_t)h->B, hipMemcpyHostToDevice, h->stream));
    return SLAM_OK;
}

}  // namespace

int pgs_init_each(pgs_handle* h, const float* pose0, const double* truth0) {
    TRY(check(h));
    if (!pose0) return fail(SLAM_ERR_ARG, "pose0 is NULL");
    const size_t B = (size_t)h->B;
    if (!all_finite_f(pose0, 3 * B) || (truth0 && !all_finite_d(truth0, 3 * B))) return fail(SLAM_ERR_ARG, "a start pose is not finite");
    HIP_TRY(h->dpose_each.reserve(3 * B));
    if (truth0) HIP_TRY(h->dtruth_each.reserve(3 * B));
    HIP_TRY(hipMemcpyAsync(h->dpose_each, pose0, sizeof(float) * 3 * B, hipMemcpyHostToDevice, h->stream));
    if (truth0) HIP_TRY(hipMemcpyAsync(h->dtruth_each, truth0, sizeof(double) * 3 * B, hipMemcpyHostToDevice, h->stream));
    h->invalidate_derived();
    h->timestep = 0; h->p.N = 1;
    h->seg_cur = h->tune.seg_len;
    TRY(clear_fixes(h));
    HIP_TRY(slam::pgs_launch_init_each(h->p, h->dpose_each, truth0 ? h->dtruth_each.get() : nullptr, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // the host arrays are pageable
    h->inited = true; h->solved = false;
    return SLAM_OK;
}

int pgs_update_dev(pgs_handle* h, const float cmd[2], const float* d_meas, const int32_t* d_count, int k_stride, const double* d_sec) {
    TRY(check(h));
    TRY(enter_ticks(h, "pgs_update", cmd, 1, kShared));
    return append_tick(h, d_meas, d_count, k_stride, d_sec);
}

int pgs_update(pgs_handle* h, const float cmd[2], const float* meas, const int32_t* count, int k_stride, const double* sec) {
    TRY(check(h));
    if (!meas_args_ok(meas, count, k_stride)) return fail(SLAM_ERR_ARG, "bad measurement arguments");
    int ks = 1;
    TRY(stage_messages(h, meas, count, k_stride, sec, &ks));
    const int rc = pgs_update_dev(h, cmd, h->dmeas, h->dcount, ks, sec ? h->dsec : nullptr);
    // the staging buffers are reused by the next call and the host arrays are pageable: finish the copies now
    HIP_TRY(hipStreamSynchronize(h->stream));
    return rc;
}

int pgs_update_each_dev(pgs_handle* h, const float* d_cmds, const float* d_meas, const int32_t* d_count, int k_stride, const double* d_sec) {
    TRY(check(h));
    TRY(enter_ticks(h, "pgs_update_each", d_cmds, 1, kEach | kDeviceSource));
    return append_tick(h, d_meas, d_count, k_stride, d_sec);
}

int pgs_update_each(pgs_handle* h, const float* cmds, const float* meas, const int32_t* count, int k_stride, const double* sec) {
    TRY(check(h));
    TRY(enter_ticks(h, "pgs_update_each", cmds, 1, kEach | (meas_args_ok(meas, count, k_stride) ? 0u : kBadMeasArgs)));
    int ks = 1;
    TRY(stage_messages(h, meas, count, k_stride, sec, &ks));
    const int rc = append_tick(h, h->dmeas, h->dcount, ks, sec ? h->dsec : nullptr);
    HIP_TRY(hipStreamSynchronize(h->stream));   // as pgs_update: the staging buffers are free for the next call
    return rc;
}

namespace {

// T simulator iterations; each: one command per instance and tick - one copy and one transposing launch for the T ticks
int run_sim(pgs_handle* h, const char* who, const float* cmds, int T, bool each) {
    TRY(check(h));
    TRY(enter_ticks(h, who, cmds, T, kSim | (each ? kEach : kShared)));
    HIP_TRY(slam::pgs_launch_run_sim(h->p, T, (uint32_t)h->timestep, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));   // cmds is a pageable host array
    advance(h, T);
    return SLAM_OK;
}

}  // namespace

int pgs_run_sim(pgs_handle* h, const float* cmds, int T) { return run_sim(h, "pgs_run_sim", cmds, T, false); }
int pgs_run_sim_each(pgs_handle* h, const float* cmds, int T) { return run_sim(h, "pgs_run_sim_each", cmds, T, true); }

namespace {

// after pgs_launch_lm_begin on the same stream: the clones (lambda lanes) of the group's instances get the instance's graph,
// event lists, values and scalars - one contiguous copy per array and lane - and start inactive
int clone_instances(pgs_handle* h, const slam::PgsParams& p, hipStream_t stream, bool slabs = true) {
    const size_t B = (size_t)h->B, off = (size_t)p.b_off, cnt = (size_t)p.b_cnt;
    for (int j = 1; j < h->tune.lanes; ++j) {
        if (slabs)
            for (const auto* set : {&h->arrays, &h->seg_arrays})
                for (const pgs_handle::Array& a : *set)
                    if (const size_t sb = a.slot_bytes)
                        HIP_TRY(hipMemcpyAsync((char*)*a.field + ((size_t)j * B + off) * sb, (const char*)*a.field + off * sb, cnt * sb, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(p.state + (size_t)j * B + off), 1, cnt, stream));
    }
    return SLAM_OK;
}

// the slabs of the instances in the group's current list only, in one launch (pgs_clone_kernel): when the first trial with lanes is near
int clone_listed(pgs_handle* h, const slam::PgsParams& p, int n_list, hipStream_t stream) {
    slam::PgsCloneTable t;
    t.n = 0;
    for (const auto* set : {&h->arrays, &h->seg_arrays})
        for (const pgs_handle::Array& a : *set) {
            if (!a.slot_bytes) continue;
            if (t.n >= 28 || (a.slot_bytes & 3)) return fail(SLAM_ERR_STATE, "clone table: more than %d arrays, or %zu bytes per slot", t.n, a.slot_bytes);
            t.ptr[t.n] = *a.field; t.words[t.n] = (uint32_t)(a.slot_bytes / 4); t.n += 1;
        }
    slam::PgsParams q = p;
    q.n_list = n_list;
    HIP_TRY(slam::pgs_launch_clone(q, t, h->tune.lanes, stream));
    return SLAM_OK;
}

double now_ms() { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6; }

// What the host knows after the last trial it has counted, and the next trial starts from: the group's active instances scaled to the whole
// batch (x G: the lane and kernel rules go by the batch), the most lanes the decide step handed to any of them, the running slots it listed.
struct LmState { int32_t active, lanes, slots; };

// One solve group of a solve: a contiguous range of the batch whose LM loop runs on its own stream, driven by its own host thread.
struct SolveGroup {
    slam::PgsParams q;                       // the handle's parameter block with the group's range, counters, list and wait cursor
    hipStream_t stream = nullptr;
    int index = 0, G = 1;                    // group `index` of G
    int trials = 0;                          // trials launched so far
    int rc = SLAM_OK;                        // what its LM loop returned
    std::vector<int32_t> timeline;           // running slots of every trial (pgs_last_solve_timeline); its storage is the handle's, lent for the solve
    double launch_ms = 0.0, wait_ms = 0.0;   // tune.host_prof: host clock enqueuing trials / waiting for their counters
    SolveGroup() {}                          // (q is assigned by setup_groups: no zero-filling of a parameter block per solve)
    bool idle() const { return q.b_cnt <= 0; }
};

// The first two operations of a trial - clearing its counters and the linearisation - depend on nothing the host decides
// (kernel variants, lanes), so they are put on the stream BEFORE the host waits for the previous trial's active count: the
// linearize kernel covers the round trip of that wait and of the next launches.  Every slot is covered (inactive ones return).
int prelaunch_trial(pgs_handle* h, slam::PgsParams& p, hipStream_t stream) {
    p.lanes = h->tune.lanes;
    p.use_list = 0;   // the host does not know the list's length yet
    HIP_TRY(hipMemsetAsync(p.n_active, 0, 4 * sizeof(int32_t), stream));
    HIP_TRY(slam::pgs_launch_trial_kernel(p, 0, stream));
    return SLAM_OK;
}

// kWhole: the trial is enqueued from its first operation on; kPrelaunched: its first two operations are on the stream (prelaunch_trial);
// kStreaming: whole, and its decide step hands out one lane whatever is left (the streaming loop runs one slot per graph)
enum class TrialStart { kWhole, kPrelaunched, kStreaming };

// one tryLambda of the instances [p.b_off, p.b_off + p.b_cnt) on `stream`, from the state `s` the previous trial's pgs_decide_kernel reported
// (the first trial's: lm_begin's): s.lanes = the most slots any instance runs in this trial, s.slots = the slots listed for it
int launch_trial(pgs_handle* h, slam::PgsParams& p, hipStream_t stream, const LmState& s, int trial_index, TrialStart start) {
    const slam_host::PgsTuning& tune = h->tune;
    const bool profile = h->profiling, prelaunched = start == TrialStart::kPrelaunched;
    p.lanes = s.lanes < 1 ? 1 : (s.lanes > tune.lanes ? tune.lanes : s.lanes);
    p.use_list = tune.use_list ? 1 : 0; p.n_list = s.slots;
    p.fused = slam_host::pgs_fused(h->fused_ok, tune.fused_mode, p.use_list ? s.slots : p.b_cnt * p.lanes, h->cus);
    p.lanes_next = start == TrialStart::kStreaming ? 1 : slam_host::pgs_lanes_next(tune, s.active);
    p.syrk_wave_tile = slam_host::pgs_syrk_kernel(s.active, p.lanes, tune.syrk_inst_switch, h->syrk_inst_ok);
    if (profile) { if ((int)h->trial_fused.size() <= trial_index) h->trial_fused.resize(trial_index + 1); h->trial_fused[trial_index] = p.fused; }
    if (!prelaunched) HIP_TRY(hipMemsetAsync(p.n_active, 0, 4 * sizeof(int32_t), stream));
    for (int k = prelaunched ? 1 : 0; k < slam::kPgsTrialKernels; ++k) {
        if (profile) {
            const size_t need = (size_t)(trial_index + 1) * (slam::kPgsTrialKernels + 1);
            while (h->events.size() < need) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); h->events.push_back(e); }
            if (k == 0) HIP_TRY(hipEventRecord(h->events[(size_t)trial_index * (slam::kPgsTrialKernels + 1)], stream));
        }
        HIP_TRY(slam::pgs_launch_trial_kernel(p, k, stream));
        if (profile) HIP_TRY(hipEventRecord(h->events[(size_t)trial_index * (slam::kPgsTrialKernels + 1) + k + 1], stream));
    }
    return SLAM_OK;
}

// The plan for segments of SL poses (pgs_seg_plan_kernel; SL = 0: it only counts the factors - the grid of the per-factor kernels):
// *mx = the most landmarks the interior poses of any segment of any instance see
int plan_for_length(pgs_handle* h, int SL, int* mx) {
    h->p.seg_len = SL;
    HIP_TRY(slam::pgs_launch_seg_plan(h->p, h->stream));
    std::vector<int32_t> U((size_t)h->B), F((size_t)h->B);
    if (SL > 0) HIP_TRY(hipMemcpyAsync(U.data(), h->p.seg_umax, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(F.data(), h->p.fact_cnt, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int fx = 0;
    for (int32_t f : F) fx = f > fx ? f : fx;
    h->p.nfact_max = fx;
    *mx = 0;
    for (int32_t u : U) *mx = u > *mx ? u : *mx;
    return SLAM_OK;
}

// Segmented elimination of the pose chain (pgs_seg_impl.h): the path runs when no segment of any instance sees more than kPgsSegMaxLm
// landmarks (its columns fit the segment kernels) and the separators fit the separator kernel's staging.  The segment length of this solve:
// the longest of seg_cur, seg_cur / 2, ... (slam_host::pgs_seg_step) that does.  None - dense visibility on a big map: the sequential chain.
int plan_segments(pgs_handle* h) {
    h->seg_ok = false; h->p.seg_on = 0;
    int SL = h->tune.seg_len > 0 ? h->seg_cur : 0;
    for (;;) {
        int mx = 0;
        TRY(plan_for_length(h, SL, &mx));
        if (SL <= 0) break;
        const slam_host::PgsSegStep step = slam_host::pgs_seg_step(SL, mx, h->p.N);
        if (step.kind == slam_host::PgsSegStep::kAccept) h->seg_ok = true;
        if (step.kind != slam_host::PgsSegStep::kTry) break;
        bool resized = false;
        TRY(resize_segments(h, step.next, &resized));
        if (!resized) break;   // (no memory for the shorter segments' arrays: the sequential chain, on the arrays that exist)
        SL = step.next;
    }
    if (h->seg_ok) { h->seg_cur = SL; h->seg_used = SL; TRY(ensure_segT(h)); }
    else {   // (a graph only grows: what no segment length holds now, none will hold later - the next solves go straight to the sequential chain)
        h->p.seg_len = h->tune.seg_len > 0 ? h->seg_alloc : 0; h->seg_used = 0; h->seg_cur = 0;
    }
    h->p.seg_on = h->seg_ok ? 1 : 0;
    return SLAM_OK;
}

// Which chain / SYRK kernels the solve's graphs fit (slam_host::pgs_fit): asked for the sequential chain with a column of Y per lane only
int decide_paths(pgs_handle* h) {
    h->fused_ok = false; h->p.fused = 0; h->syrk_inst_ok = false;
    if (h->seg_ok || h->p.LD > 448) return SLAM_OK;
    std::vector<int32_t> M((size_t)h->B);
    HIP_TRY(hipMemcpyAsync(M.data(), h->p.M, sizeof(int32_t) * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    int mx = 0;
    for (int32_t m : M) mx = m > mx ? m : mx;
    const slam_host::PgsFit fit = slam_host::pgs_fit(mx, h->p.KP, h->tune.fused_mode);
    h->fused_ok = fit.fused_ok; h->syrk_inst_ok = fit.syrk_inst_ok;
    return SLAM_OK;
}

// The groups' streams must not share a hardware queue: two LM loops whose launches sit in ONE in-order queue wait for each other's
// queued trials at every host synchronisation (measured inside bench.py's driver command, where the earlier legs' streams shift the
// runtime's stream -> queue assignment: 3.40 k solves/s with two groups against 5.21 k with one and 5.66 k with two on distinct
// queues; profiles/r05_pgs/hw_queues.txt).  The runtime keeps separate queues per stream PRIORITY, so the groups alternate between
// the priority levels the device offers (SLAM_PGS_GROUP_PRIO=0: all at the default priority, the behaviour before).
int create_group_stream(pgs_handle* h, int g, hipStream_t* st) {
    int lo = 0, hi = 0;
    if (h->tune.group_prio && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && lo != hi) {
        const int nlev = lo - hi + 1;   // lo = least priority (numerically greatest), hi = greatest
        HIP_TRY(hipStreamCreateWithPriority(st, hipStreamNonBlocking, hi + (g % nlev)));
    } else {
        (void)hipGetLastError();
        HIP_TRY(hipStreamCreateWithFlags(st, hipStreamNonBlocking));
    }
    return SLAM_OK;
}

// What a solve of G groups needs and the handle keeps: the groups' streams and events, the pinned active counts and, if a group may
// stream (share > 0), the pinned ring of counter blocks with its events
int reserve_solve_resources(pgs_handle* h, int G, int share) {
    while (G > 1 && (int)h->gstreams.size() < G) {
        hipStream_t st;
        TRY(create_group_stream(h, (int)h->gstreams.size(), &st));
        h->gstreams.push_back(st);
    }
    while ((int)h->gevents.size() < G + 1) { hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->gevents.push_back(e); }
    HIP_TRY(h->h_active.reserve(64));
    if (share > 0) {
        HIP_TRY(h->h_ring.reserve(8 * slam_host::kPgsRing * slam_host::kPgsMaxGroups));
        while ((int)h->ring_events.size() < slam_host::kPgsRing * slam_host::kPgsMaxGroups) {
            hipEvent_t e; HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming)); h->ring_events.push_back(e);
        }
    }
    return SLAM_OK;
}

// The groups' parameter blocks and streams; every group that owns instances starts behind what the handle's stream holds so far, with
// pgs_lm_begin_kernel and its clones.  A group whose share of the slots covers its graphs runs lockstep (slots_cap = 0).
int setup_groups(pgs_handle* h, int share, std::vector<SolveGroup>& groups) {
    const int G = (int)groups.size();
    if (G > 1) HIP_TRY(hipEventRecord(h->gevents[G], h->stream));   // everything queued on the handle's stream so far comes first
    h->p.max_trials = h->tune.max_trials;   // the per-graph trial cap, applied by pgs_decide_kernel in every schedule
    h->timeline.resize((size_t)G);
    for (int g = 0; g < G; ++g) {
        SolveGroup& grp = groups[g];
        grp.timeline.swap(h->timeline[g]); grp.timeline.clear();   // (the last solve's storage: no allocation per solve)
        const slam_host::PgsRange r = slam_host::pgs_group_range(h->B, G, g);
        grp.index = g; grp.G = G;
        grp.stream = G > 1 ? h->gstreams[g] : h->stream;
        slam::PgsParams& q = grp.q = h->p;
        q.b_off = r.b_off; q.b_cnt = r.b_cnt;
        q.n_active = h->p.n_active + 4 * g;
        q.alist = h->p.alist + (size_t)r.b_off * h->tune.lanes;
        q.wait_next = h->d_wait + g;
        q.slots_cap = slam_host::pgs_stream_slots(share, r.b_cnt);
        q.n_list_dev = nullptr;
        if (grp.idle()) continue;
        if (G > 1) HIP_TRY(hipStreamWaitEvent(grp.stream, h->gevents[G], 0));
        HIP_TRY(slam::pgs_launch_lm_begin(q, grp.stream));
        TRY(clone_instances(h, q, grp.stream, /*slabs=*/!h->tune.use_list || h->profiling));   // (with the slot list: copied on demand, for the listed instances)
    }
    return SLAM_OK;
}

// the counters of streamed trial `seen` of the group (a blocking wait for its event) into last[8] and its running slots into the timeline
int read_streamed_trial(pgs_handle* h, SolveGroup& grp, int seen, int32_t last[8]) {
    constexpr int R = slam_host::kPgsRing;
    HIP_TRY(hipEventSynchronize(h->ring_events[(size_t)grp.index * R + seen % R]));
    memcpy(last, h->h_ring + ((size_t)grp.index * R + seen % R) * 8, 8 * sizeof(int32_t));
    if (h->tune.trace) fprintf(stderr, "pgs group %d trial %d (streaming): active %d, slots %d, next waiting %d of %d\n", grp.index, seen, last[0], last[2], last[4], grp.q.b_off + grp.q.b_cnt);
    grp.timeline.push_back(last[2]);
    return SLAM_OK;
}

// Streaming phase of a group (q.slots_cap > 0): the list of every trial is refilled on the device, its length read on the device, so the host
// enqueues trials `stream_depth` ahead and only looks at the counters of the trial that far back - to learn that the queue of waiting graphs
// is empty and few are left (then the lockstep phase takes over, with its lambda lanes), or none at all.  *s: the state the last trial left.
int stream_phase(pgs_handle* h, SolveGroup& grp, LmState* s) {
    constexpr int R = slam_host::kPgsRing;
    slam::PgsParams& q = grp.q;
    const int cap = q.slots_cap, G = grp.G, D = h->tune.stream_depth, wend = q.b_off + q.b_cnt;
    int32_t* dcnt = h->d_cnt + (size_t)grp.index * 16;
    int32_t* ring = h->h_ring + (size_t)grp.index * R * 8;
    int32_t* const n_active0 = q.n_active;
    // "the counters trial -1 left": the first `cap` graphs run (pgs_lm_begin_kernel listed them), the cursor stands behind them
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(dcnt + 2), cap, 1, grp.stream));
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)q.wait_next, q.b_off + cap, 1, grp.stream));
    int t = 0, seen = 0;   // trials enqueued / trials whose counters the host has read
    bool leave = false;    // nothing left, or nothing waiting and few enough running that the lanes pay: the lockstep phase finishes the group
    int32_t last[8] = {cap * G, 1, cap, 0, q.b_off + cap, 0, 0, 0};
    grp.timeline.push_back(cap);
    auto read_next = [&]() -> int {
        TRY(read_streamed_trial(h, grp, seen++, last));
        leave = leave || slam_host::pgs_stream_hands_over(last[0], last[4], wend, G, h->tune.lanes_switch);
        return SLAM_OK;
    };
    const long long bound = slam_host::pgs_stream_launch_bound(q.b_cnt, cap, h->tune.max_trials);
    while (!leave && t < bound) {
        q.n_list_dev = dcnt + 8 * (t & 1) + 2;
        q.n_active = dcnt + 8 * ((t + 1) & 1);
        TRY(launch_trial(h, q, grp.stream, LmState{cap * G, 1, cap}, t, TrialStart::kStreaming));
        HIP_TRY(hipMemcpyAsync(ring + 8 * (t % R), q.n_active, 8 * sizeof(int32_t), hipMemcpyDeviceToHost, grp.stream));
        HIP_TRY(hipEventRecord(h->ring_events[(size_t)grp.index * R + t % R], grp.stream));
        t += 1;
        while (!leave && t - seen >= D) TRY(read_next());
    }
    while (seen < t) TRY(read_next());   // the trials already enqueued are real ones (or return at entry): their counters are the state to go on from
    grp.timeline.pop_back();             // (the last entry is the list of a trial the lockstep phase launches and records itself)
    grp.trials = t;
    q.slots_cap = 0; q.n_list_dev = nullptr; q.n_active = n_active0;
    *s = LmState{last[0] * G, last[1] > 0 ? last[1] : 1, last[2]};
    // (graphs still waiting at the trial cap keep state 2: pgs_lm_end_kernel flags them NOT_CONVERGED)
    return SLAM_OK;
}

// Lockstep phase of a group, from state s: launch a trial, wait for its active count, choose the next trial's kernel variants and lanes from
// it.  The first two operations of the next trial are enqueued before that wait (prelaunch_trial) - not in a profiled solve: per-kernel
// timing wants every kernel of a trial between its own events.
int lockstep_phase(pgs_handle* h, SolveGroup& grp, LmState s) {
    slam::PgsParams& q = grp.q;
    hipStream_t st = grp.stream;
    const bool profile = h->profiling, host_prof = h->tune.host_prof;
    int32_t* hact = h->h_active + 4 * grp.index;
    // a bound that cannot bind first: every launch consumes at least one trial of every graph still running, and pgs_decide_kernel ends
    // a graph at its own max_trials-th trial
    const int trials_end = grp.trials + h->tune.max_trials;
    // the phase's first trial runs over the list it was handed; later ones have their first kernels enqueued ahead
    TrialStart start = TrialStart::kWhole;
    bool cloned = !h->tune.use_list || profile || h->tune.lanes <= 1;
    while (s.active > 0 && grp.trials < trials_end) {
        // the first trial whose decide step may hand out lanes: the instances it lists (every later list is a subset) get their clones now
        if (!cloned && slam_host::pgs_lanes_next(h->tune, s.active) > 1) { TRY(clone_listed(h, q, s.slots, st)); cloned = true; }
        grp.timeline.push_back(s.slots);
        const double ta = host_prof ? now_ms() : 0.0;
        TRY(launch_trial(h, q, st, s, grp.trials, start));
        HIP_TRY(hipMemcpyAsync(hact, q.n_active, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipEventRecord(h->gevents[grp.index], st));
        if (!profile) { TRY(prelaunch_trial(h, q, st)); start = TrialStart::kPrelaunched; }   // the next trial's linearisation runs while the host waits below
        const double tb = host_prof ? now_ms() : 0.0;
        HIP_TRY(hipEventSynchronize(h->gevents[grp.index]));
        if (host_prof) { grp.launch_ms += tb - ta; grp.wait_ms += now_ms() - tb; }
        s = LmState{hact[0] * grp.G, hact[1], hact[2]};
        grp.trials += 1;
        if (h->tune.trace) {
            static thread_local double t_prev = 0.0;
            const double now = now_ms();
            fprintf(stderr, "pgs group %d trial %d: %.2f ms, lanes %d -> active %d, lanes next %d\n", grp.index, grp.trials - 1, grp.trials > 1 ? now - t_prev : 0.0, (int)q.lanes, (int)hact[0], (int)s.lanes);
            t_prev = now;
        }
    }
    return SLAM_OK;
}

// the LM loop of one group, on the calling thread: the streaming phase if the group streams, the lockstep phase from the state it left
// (or from the start: every instance active, one lane, every slot listed), then the results
int drive_group(pgs_handle* h, SolveGroup& grp) {
    HIP_TRY(hipSetDevice(h->device));
    LmState s{grp.q.b_cnt * grp.G, 1, grp.q.b_cnt};
    if (grp.q.slots_cap > 0) TRY(stream_phase(h, grp, &s));
    TRY(lockstep_phase(h, grp, s));
    HIP_TRY(slam::pgs_launch_lm_end(grp.q, grp.stream));
    if (grp.G > 1) HIP_TRY(hipEventRecord(h->gevents[grp.index], grp.stream));
    return SLAM_OK;
}

// One host thread per group drives its LM loop (group 0: the caller's); the HIP runtime is thread-safe and the groups touch disjoint
// instance ranges and their own SolveGroup.  Returns when all of them have.
void run_groups(pgs_handle* h, std::vector<SolveGroup>& groups) {
    std::vector<std::thread> workers;
    for (size_t g = 1; g < groups.size(); ++g)
        if (!groups[g].idle()) workers.emplace_back([h, &grp = groups[g]]() { grp.rc = drive_group(h, grp); });
    if (!groups[0].idle()) groups[0].rc = drive_group(h, groups[0]);
    for (std::thread& w : workers) w.join();
}

// After the groups' threads: their timelines and host-clock sums into the handle, the handle's stream continues after every group
int join_groups(pgs_handle* h, std::vector<SolveGroup>& groups) {
    for (SolveGroup& grp : groups) {
        h->timeline[grp.index].swap(grp.timeline);
        h->host_launch_ms += grp.launch_ms; h->host_wait_ms += grp.wait_ms;
    }
    int most = 0;
    for (const SolveGroup& grp : groups) {
        if (grp.rc != SLAM_OK) return grp.rc;
        if (grp.G > 1 && !grp.idle()) HIP_TRY(hipStreamWaitEvent(h->stream, h->gevents[grp.index], 0));
        most = grp.trials > most ? grp.trials : most;
    }
    h->last_trials = most;
    return SLAM_OK;
}

// profiled solve: the HIP event times of every trial's kernels summed per kernel and per path
int total_profile(pgs_handle* h) {
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int k = 0; k < slam::kPgsTrialKernels; ++k) h->kernel_ms[k] = 0.0;
    for (int t = 0; t < h->last_trials; ++t)
        for (int k = 0; k < slam::kPgsTrialKernels; ++k) {
            float ms = 0.f;
            const size_t e0 = (size_t)t * (slam::kPgsTrialKernels + 1) + k;
            HIP_TRY(hipEventElapsedTime(&ms, h->events[e0], h->events[e0 + 1]));
            h->kernel_ms[k] += ms;
            const int tf = t < (int)h->trial_fused.size() ? h->trial_fused[t] : 0;
            if (k == 1 && tf) h->path_ms[1] += ms;      // chain + SYRK in one launch
            if (k == 2 && !tf) h->path_ms[h->seg_ok ? 2 : 0] += ms;     // the SYRK launch(es) of the two-launch path / of the segmented path
            if (h->tune.trace) fprintf(stderr, "%s%.3f%s", k == 0 ? "pgs trial kernels (ms): " : " ", ms, k + 1 == slam::kPgsTrialKernels ? "\n" : "");
        }
    return SLAM_OK;
}

}  // namespace

// The solve as its phases: plan the segments, decide the chain / SYRK paths, reserve what the groups need, set the groups up, drive them
// (lockstep: two groups on their own streams from batch 128 on - with the segmented elimination a trial's kernels are short enough for two
// LM loops to fill each other's gaps; profiles/r05_pgs/groups_and_lanes.txt), join, total the profile.  The rules: host/pgs_schedule.h.
int pgs_solve(pgs_handle* h) {
    TRY(check(h));
    if (!h->inited) return fail(SLAM_ERR_STATE, "pgs_init must be called before pgs_solve");
    TRY(apply_robust(h));
    h->invalidate_derived(); h->solved = true;
    h->p.N = h->timestep + 1;
    h->p.b_off = 0; h->p.b_cnt = h->B;
    TRY(plan_segments(h));
    TRY(decide_paths(h));
    HIP_TRY(hipMemsetAsync(h->p.work, 0, 3 * sizeof(double), h->stream));
    h->path_ms[0] = h->path_ms[1] = h->path_ms[2] = 0.0;
    const int G = slam_host::pgs_groups(h->tune.groups, h->B, h->profiling);
    const int share = slam_host::pgs_slot_share(h->tune.slots, G, h->profiling);
    TRY(reserve_solve_resources(h, G, share));
    std::vector<SolveGroup> groups((size_t)G);
    TRY(setup_groups(h, share, groups));
    run_groups(h, groups);
    TRY(join_groups(h, groups));
    return h->profiling ? total_profile(h) : SLAM_OK;
}

// Streaming: at most `slots` graphs of the batch in flight (0 = lockstep, every graph from the first trial on).  Results do not depend on it.
int pgs_set_slots(pgs_handle* h, int slots) { TRY(check(h)); h->tune.slots = slots < 0 ? 0 : slots; return SLAM_OK; }
// The last solve's running slots per trial of solve group `group`: slots[0 .. *n) (at most cap entries written); *groups = number of groups.
int pgs_last_solve_timeline(pgs_handle* h, int group, int32_t* slots, int cap, int32_t* n, int32_t* groups) {
    TRY(check(h));
    if (groups) *groups = (int32_t)h->timeline.size();
    if (group < 0 || group >= (int)h->timeline.size()) { if (n) *n = 0; return SLAM_OK; }
    const std::vector<int32_t>& tl = h->timeline[group];
    if (n) *n = (int32_t)tl.size();
    if (slots) for (int i = 0; i < (int)tl.size() && i < cap; ++i) slots[i] = tl[i];
    return SLAM_OK;
}

// number of solve groups (0 = automatic: slam_pgs.h)
int pgs_set_groups(pgs_handle* h, int groups) { TRY(check(h)); h->tune.groups = groups < 0 ? 0 : groups; return SLAM_OK; }

int pgs_adopt_result(pgs_handle* h) {
    TRY(check(h));
    h->invalidate_derived();
    HIP_TRY(slam::pgs_launch_adopt(h->p, h->stream));
    return SLAM_OK;
}

// solve_graph_every_iteration with the simulator on the device: T x { get_cmd + NaiveFilter + graph append (one tick of pgs_run_sim),
// pgs_solve, pgs_adopt_result }.  SLAM_PGS_ITER_PROF=1: the host clock per phase with a stream synchronisation after each (phase table only).
namespace {
int run_every_iteration(pgs_handle* h, int T, int32_t* counts);
}

int pgs_run_sim_every_iteration(pgs_handle* h, const float* cmds, int T, int32_t* counts) {
    TRY(check(h));
    TRY(enter_ticks(h, "pgs_run_sim_every_iteration", cmds, T, kSim | kShared));
    HIP_TRY(hipStreamSynchronize(h->stream));   // cmds is a pageable host array
    return run_every_iteration(h, T, counts);
}

// The same with one command per instance and tick, cmds [T][batch][2]: the commands of all T ticks go to the device at once, the ticks keep
// their structure.
int pgs_run_sim_every_iteration_each(pgs_handle* h, const float* cmds, int T, int32_t* counts) {
    TRY(check(h));
    TRY(enter_ticks(h, "pgs_run_sim_every_iteration_each", cmds, T, kSim | kEach));
    HIP_TRY(hipStreamSynchronize(h->stream));   // cmds is a pageable host array
    return run_every_iteration(h, T, counts);
}

namespace {

// the T ticks of pgs_run_sim_every_iteration[_each]; their commands are in place
int run_every_iteration(pgs_handle* h, int T, int32_t* counts) {
    HIP_TRY(h->d_tick.reserve((size_t)h->B * 2));
    HIP_TRY(h->d_tick_flop.reserve((size_t)h->B * 2));
    HIP_TRY(hipMemsetAsync(h->d_tick, 0, sizeof(int32_t) * 2 * (size_t)h->B, h->stream));
    HIP_TRY(hipMemsetAsync(h->d_tick_flop, 0, sizeof(double) * 2 * (size_t)h->B, h->stream));
    const bool prof = getenv("SLAM_PGS_ITER_PROF") != nullptr;
    for (int k = 0; k < 4; ++k) h->iter_ms[k] = 0.0;
    h->iter_trials = 0;
    // One solve group per tick unless the caller chose a number: a tick's solve is a handful of latency-bound trials - two groups gain 2 % in
    // a process of their own (15.2 k against 14.9 k graph-ticks/s) and lose 20 % when their streams land on one hardware queue behind other
    // handles' streams (bench.py's secondary leg: 12.3 k; the stream -> queue assignment of the runtime, profiles/r05_pgs/hw_queues.txt).
    struct GroupsGuard { pgs_handle* h; int saved; ~GroupsGuard() { h->tune.groups = saved; } } guard{h, h->tune.groups};
    if (h->tune.groups == 0) h->tune.groups = 1;
    for (int t = 0; t < T; ++t) {
        double t0 = prof ? now_ms() : 0.0;
        HIP_TRY(slam::pgs_launch_run_sim(h->p, 1, (uint32_t)h->timestep, h->stream));
        advance(h, 1);
        if (prof) { HIP_TRY(hipStreamSynchronize(h->stream)); const double t1 = now_ms(); h->iter_ms[0] += t1 - t0; t0 = t1; }
        TRY(pgs_solve(h));
        h->iter_trials += h->last_trials;
        if (prof) { HIP_TRY(hipStreamSynchronize(h->stream)); const double t1 = now_ms(); h->iter_ms[1] += t1 - t0; t0 = t1; }
        h->p.tick_acc = h->d_tick; h->p.tick_flop = h->d_tick_flop;
        const hipError_t e = slam::pgs_launch_adopt(h->p, h->stream);
        h->p.tick_acc = nullptr; h->p.tick_flop = nullptr;
        if (e != hipSuccess) return fail(SLAM_ERR_HIP, "pgs_launch_adopt -> %s", hipGetErrorString(e));
        if (prof) { HIP_TRY(hipStreamSynchronize(h->stream)); const double t1 = now_ms(); h->iter_ms[2] += t1 - t0; }
    }
    if (counts) {
        HIP_TRY(hipMemcpyAsync(counts, h->d_tick, sizeof(int32_t) * 2 * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (h->tune.host_prof) fprintf(stderr, "pgs host clock over the run's trials: %.0f ms enqueuing, %.0f ms waiting for the trials' counters\n", h->host_launch_ms, h->host_wait_ms);
    return SLAM_OK;
}

}  // namespace

// Host-clock phase times of the last pgs_run_sim_every_iteration under SLAM_PGS_ITER_PROF=1: ms in {simulator + append, solve, adopt}, and the
// LM trials launched over all ticks.
int pgs_last_iter_phases(pgs_handle* h, double ms[6]) {
    TRY(check(h));
    if (!ms) return fail(SLAM_ERR_ARG, "NULL output");
    ms[0] = h->iter_ms[0]; ms[1] = h->iter_ms[1]; ms[2] = h->iter_ms[2]; ms[3] = (double)h->iter_trials;
    ms[4] = ms[5] = 0.0;
    if (h->d_tick_flop) {   // algorithmic FLOP of the call's trials, summed over the batch: SYRK | Cholesky
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::vector<double> f((size_t)h->B * 2);
        HIP_TRY(hipMemcpy(f.data(), h->d_tick_flop, sizeof(double) * f.size(), hipMemcpyDeviceToHost));
        for (int b = 0; b < h->B; ++b) { ms[4] += f[2 * (size_t)b]; ms[5] += f[2 * (size_t)b + 1]; }
    }
    return SLAM_OK;
}

int pgs_get_graph(pgs_handle* h, int inst, int which, double* poses, double* lms, int32_t* timestep, int32_t* M, int32_t* ids) {
    TRY(check(h));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    HIP_TRY(hipStreamSynchronize(h->stream));
    int32_t m = 0;
    HIP_TRY(hipMemcpy(&m, h->p.M + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    const double* ps = (which ? h->p.pose1 : h->p.pose0) + (size_t)inst * h->N_max * 3;
    const double* ls = (which ? h->p.lm1 : h->p.lm0) + (size_t)inst * h->L_max * 2;
    if (poses) HIP_TRY(hipMemcpy(poses, ps, sizeof(double) * 3 * (size_t)(h->timestep + 1), hipMemcpyDeviceToHost));
    if (lms && m > 0) HIP_TRY(hipMemcpy(lms, ls, sizeof(double) * 2 * (size_t)m, hipMemcpyDeviceToHost));
    if (ids && m > 0) HIP_TRY(hipMemcpy(ids, h->p.ids + (size_t)inst * h->L_max, sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost));
    if (timestep) *timestep = h->timestep;
    if (M) *M = m;
    return SLAM_OK;
}

int pgs_get_connections(pgs_handle* h, int inst, int32_t* conn, int cap, int32_t* n) {
    TRY(check(h));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    HIP_TRY(hipStreamSynchronize(h->stream));
    const int N = h->timestep + 1;
    std::vector<int32_t> cnt(N), mlm((size_t)N * h->KP);
    HIP_TRY(hipMemcpy(cnt.data(), h->p.cnt + (size_t)inst * h->N_max, sizeof(int32_t) * N, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(mlm.data(), h->p.mlm + (size_t)inst * h->N_max * h->KP, sizeof(int32_t) * (size_t)N * h->KP, hipMemcpyDeviceToHost));
    int nc = 0;
    for (int i = 0; i < N; ++i)
        for (int s = 0; s < cnt[i]; ++s) {
            const int32_t v = mlm[(size_t)i * h->KP + s];
            if (conn && nc < cap) { conn[2 * nc] = i; conn[2 * nc + 1] = (v & slam::kPgsFirstBit) ? -1 : v; }
            nc += 1;
        }
    if (n) *n = nc;
    return SLAM_OK;
}

int pgs_get_stats(pgs_handle* h, int32_t* iterations, int32_t* trials, int32_t* flags, double* err_init, double* err_final, double* lambda) {
    TRY(check(h));
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = h->B;
    if (iterations) HIP_TRY(hipMemcpy(iterations, h->p.iters, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (trials) HIP_TRY(hipMemcpy(trials, h->p.trials, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (flags) HIP_TRY(hipMemcpy(flags, h->p.flags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (err_init) HIP_TRY(hipMemcpy(err_init, h->p.err_init, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (err_final) HIP_TRY(hipMemcpy(err_final, h->p.error, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (lambda) HIP_TRY(hipMemcpy(lambda, h->p.lambda, sizeof(double) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int pgs_error_stats(pgs_handle* h, int which, double* out) {
    TRY(check(h));
    if (!out) return fail(SLAM_ERR_ARG, "NULL output");
    h->p.N = h->timestep + 1;
    HIP_TRY(slam::pgs_launch_avg_error(h->p, which, h->dout, h->stream));
    HIP_TRY(hipMemcpyAsync(out, h->dout, sizeof(double) * (size_t)h->B, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return SLAM_OK;
}

int pgs_last_solve_work(pgs_handle* h, double* syrk_flop, int32_t* trials_launched) {
    TRY(check(h));
    // per trial and instance: what pgs_lm_begin_kernel priced one Schur-complement SYRK of the instance at (inst_flop: every stored
    // element of the lower triangle of S_ext over the rows of Y that can be non-zero in it - by the elimination order the solve ran,
    // sequential or segmented; independent of the kernels' tiling)
    HIP_TRY(hipStreamSynchronize(h->stream));
    const size_t B = h->B;
    std::vector<int32_t> tr(B);
    std::vector<double> fl(B);
    HIP_TRY(hipMemcpy(tr.data(), h->p.trials, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(fl.data(), h->p.inst_flop, sizeof(double) * B, hipMemcpyDeviceToHost));
    double tot = 0.0;
    for (size_t b = 0; b < B; ++b) tot += fl[b] * tr[b];
    if (syrk_flop) *syrk_flop = tot;
    if (trials_launched) *trials_launched = h->last_trials;
    return SLAM_OK;
}

// The last PROFILED solve by path: out = {algorithmic SYRK FLOP of the trials that ran pgs_syrk_*_kernel, of the trials that ran
// pgs_chain_syrk_kernel, ms in those SYRK launches, ms in those fused launches, FLOP of the trials of the segmented elimination, ms in
// its SYRK launches (tile kernel on the separator rows + pgs_seg_syrk_kernel), 1 if the solve ran the segmented elimination, segment length}
int pgs_last_solve_paths_v2(pgs_handle* h, double* out, int n) {
    TRY(check(h));
    if (!out || n < 0 || n > 8) return fail(SLAM_ERR_ARG, "bad output (n = %d, at most 8 entries)", n);
    HIP_TRY(hipStreamSynchronize(h->stream));
    double w[3];
    HIP_TRY(hipMemcpy(w, h->p.work, 3 * sizeof(double), hipMemcpyDeviceToHost));
    const double v[8] = {w[0], w[1], h->path_ms[0], h->path_ms[1], w[2], h->path_ms[2], h->seg_ok ? 1.0 : 0.0, (double)(h->seg_ok ? h->seg_used : h->tune.seg_len)};
    for (int i = 0; i < n; ++i) out[i] = v[i];
    return SLAM_OK;
}
int pgs_last_solve_paths(pgs_handle* h, double out[4]) { return pgs_last_solve_paths_v2(h, out, 4); }
int pgs_set_profiling(pgs_handle* h, int on) { TRY(check(h)); h->profiling = on != 0; return SLAM_OK; }
int pgs_last_solve_kernel_ms(pgs_handle* h, double ms[6]) {
    TRY(check(h));
    if (!ms) return fail(SLAM_ERR_ARG, "NULL output");
    for (int k = 0; k < slam::kPgsTrialKernels; ++k) ms[k] = h->kernel_ms[k];
    return SLAM_OK;
}
// debug only (not part of the ABI header): phase timers of the last chol launch, [batch][8] ticks of the 100 MHz clock
int pgs_debug_prof(pgs_handle* h, unsigned long long* out) {
    TRY(check(h));
    if (!h->p.prof) return fail(SLAM_ERR_STATE, "set SLAM_PGS_PROF before pgs_create");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->p.prof, sizeof(unsigned long long) * 8 * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}
// debug only: begin / end / HW_ID / XCC_ID of the two workgroups of every instance in the last fused chain launch + phase times, [batch][2][8]
int pgs_debug_prof2(pgs_handle* h, unsigned long long* out) {
    TRY(check(h));
    if (!h->p.prof) return fail(SLAM_ERR_STATE, "set SLAM_PGS_PROF before pgs_create");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out, h->p.prof + (size_t)h->B * h->tune.lanes * 8, sizeof(unsigned long long) * 16 * (size_t)h->B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// Marginal covariances of every pose and landmark of every instance at initial_estimate (which = 0) / result (1): the diagonal blocks of
// (J^T J)^-1 (pgs_marginals.h).  The factorisation runs in the instances' own LM work space (slot b of instance b; a later solve starts
// from pgs_lm_begin_kernel and reads none of it); the outputs and the flags the trial kernels see are this call's own arrays.
// SLAM_PGS_MARG_CHUNK = n: the batch in launches of n instances (results do not depend on it).
int pgs_marginals(pgs_handle* h, int which) {
    TRY(check(h));
    if (which != 0 && which != 1) return fail(SLAM_ERR_ARG, "which = %d (0: initial_estimate, 1: result)", which);
    if (!h->inited) return fail(SLAM_ERR_STATE, "pgs_init must be called before pgs_marginals");
    if (which == 1 && !h->solved) return fail(SLAM_ERR_STATE, "pgs_marginals(which = 1): no result yet (pgs_solve has not run since pgs_init)");
    TRY(apply_robust(h));
    h->mg_valid = false;
    const size_t B = (size_t)h->B;
    if (!h->mg_pose) {   // first call: everything or nothing (each owner is filled only once all allocations succeeded)
        DevBuf<double> a, b, c, d;
        DevBuf<int32_t> e, f;
        const size_t need = sizeof(double) * B * ((size_t)h->N_max * 9 + (size_t)h->L_max * 4 + 2) + sizeof(int32_t) * B * 4;
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && need > free_b)
            return fail(SLAM_ERR_HIP, "pgs_marginals: %zu bytes of output buffers exceed the %zu bytes of free device memory", need, free_b);
        if (a.reserve(B * (size_t)h->N_max * 9) != hipSuccess || b.reserve(B * (size_t)h->L_max * 4) != hipSuccess || c.reserve(B) != hipSuccess ||
            d.reserve(B) != hipSuccess || e.reserve(B) != hipSuccess || f.reserve(3 * B) != hipSuccess)
            return fail(SLAM_ERR_HIP, "pgs_marginals: out of device memory for the output buffers (%zu bytes)", need);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (hipEventCreate(&e0) != hipSuccess || hipEventCreate(&e1) != hipSuccess) {
            if (e0) hipEventDestroy(e0);
            (void)hipGetLastError();
            return fail(SLAM_ERR_HIP, "pgs_marginals: hipEventCreate failed");
        }
        h->mg_pose = std::move(a); h->mg_lm = std::move(b); h->mg_flop = std::move(c); h->mg_lambda = std::move(d);
        h->mg_status = std::move(e); h->mg_state = std::move(f);
        h->mg_ev[0] = e0; h->mg_ev[1] = e1;
    }
    int chunk = h->B;
    if (const char* e = getenv("SLAM_PGS_MARG_CHUNK")) { const int v = atoi(e); if (v > 0 && v < chunk) chunk = v; }
    slam::PgsParams q = h->p;
    q.N = h->timestep + 1;
    q.state = h->mg_state; q.lin_ok = h->mg_state + B; q.solve_ok = h->mg_state + 2 * B; q.lambda = h->mg_lambda;
    q.nfact_max = q.N * h->KP;   // an upper bound: the per-factor kernel returns beyond the instance's own count
    HIP_TRY(hipEventRecord(h->mg_ev[0], h->stream));
    for (int b0 = 0; b0 < h->B; b0 += chunk) {
        q.b_off = b0; q.b_cnt = h->B - b0 < chunk ? h->B - b0 : chunk;
        HIP_TRY(slam::pgs_launch_marginals(q, which, h->mg_pose, h->mg_lm, h->mg_status, h->mg_flop, h->stream));
    }
    HIP_TRY(hipEventRecord(h->mg_ev[1], h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, h->mg_ev[0], h->mg_ev[1]));
    h->mg_ms = ms;
    h->mg_valid = true;
    return SLAM_OK;
}

int pgs_get_marginals(pgs_handle* h, int inst, double* pose_cov, double* lm_cov, int32_t* status) {
    TRY(check(h));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    if (!h->mg_valid) return fail(SLAM_ERR_STATE, "no marginals for the current values: call pgs_marginals after the last update / solve");
    int32_t m = 0;
    HIP_TRY(hipMemcpy(&m, h->p.M + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    if (pose_cov) HIP_TRY(hipMemcpy(pose_cov, h->mg_pose + (size_t)inst * h->N_max * 9, sizeof(double) * 9 * (size_t)(h->timestep + 1), hipMemcpyDeviceToHost));
    if (lm_cov && m > 0) HIP_TRY(hipMemcpy(lm_cov, h->mg_lm + (size_t)inst * h->L_max * 4, sizeof(double) * 4 * (size_t)m, hipMemcpyDeviceToHost));
    if (status) HIP_TRY(hipMemcpy(status, h->mg_status + inst, sizeof(int32_t), hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int pgs_marginals_dev(pgs_handle* h, const double** d_pose_cov, const double** d_lm_cov, const int32_t** d_status) {
    TRY(check(h));
    if (!h->mg_valid) return fail(SLAM_ERR_STATE, "no marginals for the current values: call pgs_marginals after the last update / solve");
    if (d_pose_cov) *d_pose_cov = h->mg_pose;
    if (d_lm_cov) *d_lm_cov = h->mg_lm;
    if (d_status) *d_status = h->mg_status;
    return SLAM_OK;
}

// FLOP model per instance (pgs_marg_begin_kernel), N = poses, n = 2 M: 3N n^2 (Z = V X, counted dense) + 3N n 12 (recurrence + Gram)
// + 2 n^3 / 3 (R^-1 and its Gram) + 3N n^2 + n^3 / 3 (the lambda = 0 factorisation: Schur complement and Cholesky).
int pgs_last_marginals_work(pgs_handle* h, double* flop, double* ms) {
    TRY(check(h));
    if (!h->mg_valid) return fail(SLAM_ERR_STATE, "no marginals for the current values: call pgs_marginals after the last update / solve");
    if (flop) {
        std::vector<double> f((size_t)h->B);
        HIP_TRY(hipMemcpy(f.data(), h->mg_flop, sizeof(double) * f.size(), hipMemcpyDeviceToHost));
        double tot = 0.0;
        for (double v : f) tot += v;
        *flop = tot;
    }
    if (ms) *ms = h->mg_ms;
    return SLAM_OK;
}

// ---- robust loss on the bearing-range factors (pgs_robust.h) ----
int pgs_set_robust(pgs_handle* h, int kind, double k) {
    if (!robust_args_ok(kind, k)) return fail(SLAM_ERR_ARG, "pgs_set_robust: kind %d, k %g (kind 0 | 1 | 2; k finite and > 0 for a loss)", kind, k);
    TRY(check(h));
    h->loss_kind = kind; h->loss_k = kind == slam::kPgsLossNone ? 0.0 : k;
    h->invalidate_derived();   // what was computed belongs to the setting it was computed with
    return SLAM_OK;
}

int pgs_get_robust(const pgs_handle* h, int* kind, double* k) {
    if (!h) return fail(SLAM_ERR_ARG, "NULL handle");
    if (kind) *kind = h->loss_kind;
    if (k) *k = h->loss_k;
    return SLAM_OK;
}

int pgs_robust_loss_host(int kind, double k, double r, double* rho, double* w, double* sw) {
    if (!robust_args_ok(kind, k) || !rho || !w || !sw) return fail(SLAM_ERR_ARG, "pgs_robust_loss_host: kind %d, k %g, or a NULL output", kind, k);
    slam::pgs_robust_loss(kind, k, r * r, r, rho, w, sw);
    return SLAM_OK;
}

int pgs_factor_weights(pgs_handle* h, int which) {
    TRY(check(h));
    if (which != 0 && which != 1) return fail(SLAM_ERR_ARG, "which = %d (0: initial_estimate, 1: result)", which);
    if (!h->inited) return fail(SLAM_ERR_STATE, "pgs_init must be called before pgs_factor_weights");
    if (which == 1 && !h->solved) return fail(SLAM_ERR_STATE, "pgs_factor_weights(which = 1): no result yet (pgs_solve has not run since pgs_init)");
    h->fw_valid = false;
    if (!h->fw) {   // one allocation: there or not
        DevBuf<double> a;
        if (a.reserve((size_t)h->B * h->N_max * h->KP) != hipSuccess)
            return fail(SLAM_ERR_HIP, "pgs_factor_weights: out of device memory for the output (%zu bytes)", sizeof(double) * (size_t)h->B * h->N_max * h->KP);
        h->fw = std::move(a);
    }
    slam::PgsParams q = h->p;   // the setting of now; it needs none of the solve's work space (lin0 included)
    q.N = h->timestep + 1; q.loss_kind = h->loss_kind; q.loss_k = h->loss_k;
    HIP_TRY(slam::pgs_launch_factor_weights(q, which, h->fw, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->fw_valid = true;
    return SLAM_OK;
}

int pgs_get_factor_weights(pgs_handle* h, int inst, double* w, int cap, int32_t* n) {
    TRY(check(h));
    if (inst < 0 || inst >= h->B) return fail(SLAM_ERR_ARG, "instance %d out of range", inst);
    if (cap < 0 || (cap > 0 && !w)) return fail(SLAM_ERR_ARG, "bad output (w, cap = %d)", cap);
    if (!h->fw_valid) return fail(SLAM_ERR_STATE, "no factor weights for the current values: call pgs_factor_weights after the last update / solve");
    const size_t have = (size_t)(h->timestep + 1) * h->KP, take = have < (size_t)cap ? have : (size_t)cap;
    if (take) HIP_TRY(hipMemcpy(w, h->fw + (size_t)inst * h->N_max * h->KP, sizeof(double) * take, hipMemcpyDeviceToHost));
    if (n) *n = (int32_t)have;
    return SLAM_OK;
}

int pgs_factor_weights_dev(pgs_handle* h, const double** d_w) {
    TRY(check(h));
    if (!h->fw_valid) return fail(SLAM_ERR_STATE, "no factor weights for the current values: call pgs_factor_weights after the last update / solve");
    if (d_w) *d_w = h->fw;
    return SLAM_OK;
}

int pgs_sync(pgs_handle* h) { TRY(check(h)); HIP_TRY(hipStreamSynchronize(h->stream)); return SLAM_OK; }
int pgs_timestep(const pgs_handle* h) { return h ? h->timestep : -1; }

}  // extern "C"
