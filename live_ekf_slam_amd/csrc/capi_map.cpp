// capi_map.cpp — C ABI: map management of the EKF batch: removing landmarks, track evidence, the prune rule and the managed tick
// (map_kernel.hip)
#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "assoc_kernel.h"
#include "capi_map.h"
#include "ekf_kernel.h"
#include "map_kernel.h"

using namespace slam_capi;

namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int map_config(const slam_map_config* cfg, slam_map_config* out) {
    if (cfg) *out = *cfg; else slam_map_config_default(out);
    if (isnan(out->range_shrink) || isnan(out->fov_margin) || isnan(out->min_ratio))
        return slam_internal_fail(SLAM_ERR_ARG, "map config: range_shrink = %g, fov_margin = %g or min_ratio = %g is NaN", out->range_shrink,
                                  out->fov_margin, out->min_ratio);
    if (!(out->range_shrink > 0.0 && out->range_shrink <= 1.0))
        return slam_internal_fail(SLAM_ERR_ARG, "map config: range_shrink = %g is not in (0, 1]", out->range_shrink);
    if (out->fov_margin < 0.0) return slam_internal_fail(SLAM_ERR_ARG, "map config: fov_margin = %g is negative", out->fov_margin);
    if (out->min_expected < 1) return slam_internal_fail(SLAM_ERR_ARG, "map config: min_expected = %d is below 1", out->min_expected);
    if (!(out->min_ratio >= 0.0 && out->min_ratio <= 1.0))
        return slam_internal_fail(SLAM_ERR_ARG, "map config: min_ratio = %g is not in [0, 1]", out->min_ratio);
    if (out->prune_every < 1) return slam_internal_fail(SLAM_ERR_ARG, "map config: prune_every = %d is below 1", out->prune_every);
    return SLAM_OK;
}

// the handle, once the arguments are in order; the queued timesteps run first
int map_enter(slam_handle* h, const char* who) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "%s needs EKF_SLAM: the UKF's stored square root, eigenvectors and ages would have to follow a removal", who);
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    TRY(step_state(h, who));
    TRY(flush_lazy(h));
    HIP_TRY(hipSetDevice(h->device));
    return SLAM_OK;
}

// the track counters exist (zero when they are new)
int map_track(slam_handle* h) {
    if (h->map.tracked) return SLAM_OK;
    const size_t n = (size_t)h->B * h->L_max;
    HIP_TRY(h->map.dseen.reserve(n));
    HIP_TRY(h->map.dexpected.reserve(n));
    h->map.tracked = true;
    return map_track_reset(h);
}

// the rows of `ticks` removals, the record, the sums of the traffic model, the per-instance contributions
int map_reserve(slam_handle* h, size_t ticks) {
    TRY(grow(h, h->map.dint, kMapRows * ticks * (size_t)h->B));
    TRY(grow(h, h->map.drec, slam::kMapRecLen));
    TRY(grow(h, h->map.dwork, 3));
    return innovation_reserve(h, false);
}

int map_zero_work(slam_handle* h) {
    HIP_TRY(hipMemsetAsync(h->map.dwork, 0, 3 * sizeof(unsigned long long), h->stream));
    h->map.work_set = true;
    return SLAM_OK;
}

// one removal on the handle's stream: by the mask d_remove, or (NULL) by the prune rule of c on the counters
// (with_rec: the record is summed into map.drec, two more launches)
int map_compact_launch(slam_handle* h, const int32_t* d_remove, const slam_map_config& c, int32_t* d_n_removed, int32_t* d_m_before, bool with_rec) {
    slam::MapCompactParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.ids = h->dids;
    p.seen = h->map.tracked ? h->map.dseen.get() : nullptr; p.expected = h->map.tracked ? h->map.dexpected.get() : nullptr;
    p.remove = d_remove; p.min_expected = c.min_expected; p.min_ratio = c.min_ratio;
    p.n_removed = d_n_removed; p.m_before = d_m_before;
    p.inst_rec = h->inn.dval + 13 * (size_t)h->B;   // (the places innovation_reserve gives the contributions and the partial records)
    p.partials = h->inn.dpart; p.rec = with_rec ? h->map.drec.get() : nullptr;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    HIP_TRY(slam::launch_map_compact(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

int map_sum_work(slam_handle* h, const int32_t* d_n_removed, const int32_t* d_m_before, bool from_counters) {
    HIP_TRY(slam::launch_map_work(d_m_before, d_n_removed, (size_t)h->B, h->L_max, h->esz, from_counters, h->map.tracked, h->map.dwork, h->stream));
    return SLAM_OK;
}

// slam_remove_landmarks* and slam_map_prune once the mask (or nothing) is on the device
static int remove_now(slam_handle* h, const int32_t* d_remove, const slam_map_config& c, int32_t* n_removed, double* rec) {
    const size_t B = (size_t)h->B;
    TRY(map_reserve(h, 1));
    TRY(map_zero_work(h));
    int32_t* const di = h->map.dint;
    TRY(map_compact_launch(h, d_remove, c, row(di, kMapRemoved, B), row(di, kMapMBefore, B), rec != nullptr));
    TRY(map_sum_work(h, row(di, kMapRemoved, B), row(di, kMapMBefore, B), d_remove == nullptr));
    if (!n_removed && !rec) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{row(di, kMapRemoved, B), n_removed, B}, {h->map.drec, rec, slam::kMapRecLen}}, 0, 1);
}

// the tally of one message that is on the device, on the handle's stream
int tally_now(slam_handle* h, const slam_map_config& c, const float* d_meas, const int32_t* d_count, int k_stride, const int32_t* d_flags) {
    TRY(map_track(h));
    slam::MapTallyParams p;
    memset(&p, 0, sizeof(p));
    p.x = h->dx; p.M = h->dM; p.ids = h->dids; p.status = h->dflags;
    p.meas = d_meas; p.count = d_count; p.k_stride = k_stride; p.assoc_flags = d_flags;
    p.seen = h->map.dseen; p.expected = h->map.dexpected;
    p.r_lim = h->range_max * c.range_shrink; p.b_lo = h->fov_min + c.fov_margin; p.b_hi = h->fov_max - c.fov_margin;
    p.B = h->B; p.L_max = h->L_max; p.xstride = h->xstride;
    HIP_TRY(slam::launch_map_tally(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

static int tally_args(const slam_map_config* cfg, const float* meas, const int32_t* count, int k_stride, slam_map_config* c) {
    TRY(map_config(cfg, c));
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    return SLAM_OK;
}

// slam_step_managed (host: the message and per-instance commands are host arrays) and slam_step_managed_dev: one managed timestep
static int step_managed(slam_handle* h, bool host, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                        const float* meas, const int32_t* count, int k_stride, double* rec, int32_t* n_drop) {
    slam_assoc_config ac; slam_map_config mc;
    const float *cmd, *d_each;
    TRY(assoc_config(assoc_cfg, &ac));
    TRY(message_args(cmds, meas, count, k_stride));
    TRY(map_config(map_cfg, &mc));
    TRY(filter_enter(h, assoc_supported));
    TRY(step_state(h, "a managed step"));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(assoc_reserve(h, k_stride, 1));
    const size_t B = (size_t)h->B;
    int32_t* const d_drop = row(h->assoc.dint, kAssocDrop, B);
    int32_t* const d_flags = row(h->assoc.dint, kAssocFlags, B);
    TRY(assoc_launch(h, ac, cmd, d_each, meas, count, k_stride, h->assoc.dmeas, h->assoc.dcount, h->inn.drec,
                     {nullptr, nullptr, d_drop, d_flags, nullptr, nullptr, nullptr, nullptr}));
    TRY(launch_step(h, cmd, 0, h->assoc.dmeas, h->assoc.dcount, k_stride, d_each));
    TRY(tally_now(h, mc, h->assoc.dmeas, h->assoc.dcount, k_stride, d_flags));
    return step_outputs(h, rec, d_drop, n_drop);
}

int map_track_reset(slam_handle* h) {
    if (!h->map.tracked) return SLAM_OK;
    const size_t nb = sizeof(int32_t) * (size_t)h->B * h->L_max;
    HIP_TRY(hipSetDevice(h->device));
    HIP_TRY(hipMemsetAsync(h->map.dseen, 0, nb, h->stream));
    HIP_TRY(hipMemsetAsync(h->map.dexpected, 0, nb, h->stream));
    return SLAM_OK;
}

}  // namespace slam_capi

extern "C" {

int slam_map_config_default(slam_map_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->range_shrink = 0.9; c->fov_margin = 0.1; c->min_expected = 10; c->min_ratio = 0.3; c->prune_every = 10;
    return SLAM_OK;
}

int slam_remove_landmarks(slam_handle* h, const int32_t* remove, int32_t* n_removed, double rec[16]) {
    if (!remove) return slam_internal_fail(SLAM_ERR_ARG, "remove is NULL");
    TRY(map_enter(h, "slam_remove_landmarks"));
    const size_t n = (size_t)h->B * h->L_max;
    TRY(grow(h, h->map.dmask, n));
    HIP_TRY(hipMemcpyAsync(h->map.dmask, remove, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    slam_map_config c;
    slam_map_config_default(&c);
    return remove_now(h, h->map.dmask, c, n_removed, rec);
}

int slam_remove_landmarks_dev(slam_handle* h, const int32_t* d_remove, int32_t* n_removed, double rec[16]) {
    if (!d_remove) return slam_internal_fail(SLAM_ERR_ARG, "d_remove is NULL");
    TRY(map_enter(h, "slam_remove_landmarks_dev"));
    slam_map_config c;
    slam_map_config_default(&c);
    return remove_now(h, d_remove, c, n_removed, rec);
}

int slam_map_tally(slam_handle* h, const slam_map_config* cfg, const float* meas, const int32_t* count, int k_stride, const int32_t* assoc_flags) {
    slam_map_config c;
    TRY(tally_args(cfg, meas, count, k_stride, &c));
    TRY(map_enter(h, "slam_map_tally"));
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (assoc_flags) {   // (staged where a removal stages its mask: [B] of [B][L_max])
        TRY(grow(h, h->map.dmask, (size_t)h->B * h->L_max));
        HIP_TRY(hipMemcpyAsync(h->map.dmask, assoc_flags, sizeof(int32_t) * (size_t)h->B, hipMemcpyHostToDevice, h->stream));
    }
    return tally_now(h, c, h->inn.dmeas, h->inn.dcount, k_stride, assoc_flags ? h->map.dmask.get() : nullptr);
}

int slam_map_tally_dev(slam_handle* h, const slam_map_config* cfg, const float* d_meas, const int32_t* d_count, int k_stride,
                       const int32_t* d_assoc_flags) {
    slam_map_config c;
    TRY(tally_args(cfg, d_meas, d_count, k_stride, &c));
    TRY(map_enter(h, "slam_map_tally_dev"));
    return tally_now(h, c, d_meas, d_count, k_stride, d_assoc_flags);
}

int slam_map_prune(slam_handle* h, const slam_map_config* cfg, double rec[16], int32_t* n_removed) {
    slam_map_config c;
    TRY(map_config(cfg, &c));
    TRY(map_enter(h, "slam_map_prune"));
    TRY(map_track(h));
    return remove_now(h, nullptr, c, n_removed, rec);
}

int slam_map_get_track(slam_handle* h, int32_t* seen, int32_t* expected) {
    TRY(map_enter(h, "slam_map_get_track"));
    const size_t nb = sizeof(int32_t) * (size_t)h->B * h->L_max;
    if (!h->map.tracked) {
        if (seen) memset(seen, 0, nb);
        if (expected) memset(expected, 0, nb);
        return SLAM_OK;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (seen) HIP_TRY(hipMemcpy(seen, h->map.dseen, nb, hipMemcpyDeviceToHost));
    if (expected) HIP_TRY(hipMemcpy(expected, h->map.dexpected, nb, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_map_track_reset(slam_handle* h) {
    TRY(map_enter(h, "slam_map_track_reset"));
    return map_track_reset(h);
}

int slam_step_managed(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                      const float* meas, const int32_t* count, int k_stride, double rec[16], int32_t* n_drop) {
    return step_managed(h, true, assoc_cfg, map_cfg, cmds, cmd_each, meas, count, k_stride, rec, n_drop);
}

int slam_step_managed_dev(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                          const float* d_meas, const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop) {
    return step_managed(h, false, assoc_cfg, map_cfg, cmds, cmd_each, d_meas, d_count, k_stride, rec, n_drop);
}

int slam_manage_run(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const float* cmds, int cmd_each,
                    const float* meas, const int32_t* count, int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop,
                    int32_t* n_removed, int32_t* flags) {
    slam_assoc_config ac; slam_map_config mc;
    TickMsgs msgs;
    TRY(assoc_config(assoc_cfg, &ac));
    TRY(map_config(map_cfg, &mc));
    TRY(run_args_log(cmds, meas, count, k_stride, T, &msgs));
    return run_filtered(h, "slam_manage_run", cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T,
                        ManageTicks{{h, ac, recs, n_match, n_new, n_drop, flags}, mc, n_removed});
}

int slam_manage_run_sim(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, int source, const float* cmds,
                        int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* flags,
                        const slam_sense_log* log) {
    slam_assoc_config ac; slam_map_config mc;
    TickCmds::Source csrc;
    TickMsgs msgs;
    TRY(assoc_config(assoc_cfg, &ac));
    TRY(map_config(map_cfg, &mc));
    TRY(run_args_sim(source, cmds, k_stride, T, log, &csrc, &msgs));
    return run_filtered(h, "slam_manage_run_sim", csrc, cmds, msgs, T, ManageTicks{{h, ac, recs, n_match, n_new, n_drop, flags}, mc, n_removed});
}

int slam_last_map_work(slam_handle* h, double* bytes, double* prune_ms, double* total_ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (!h->map.work_set) return slam_internal_fail(SLAM_ERR_STATE, "slam_remove_landmarks, slam_map_prune or slam_manage_run has not run on this handle");
    if (bytes) {
        unsigned long long wk[3];
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(wk, h->map.dwork, sizeof(wk), hipMemcpyDeviceToHost));
        *bytes = (2.0 * (double)wk[0] + (double)wk[1]) * h->esz + (double)wk[2];
    }
    if (prune_ms) *prune_ms = h->map.times.part_ms;
    if (total_ms) *total_ms = h->map.times.total_ms;
    return SLAM_OK;
}

int slam_map_instance_host(double* x, double* P, int32_t* ids, int M, int L_max, int32_t status, const float* meas, int count, int k_stride,
                           int32_t assoc_flag, double range_max, double fov_min, double fov_max, int f32_storage, const slam_map_config* cfg,
                           int32_t* seen, int32_t* expected, const int32_t* remove, int prune, int32_t* mask_out, int32_t* M_out) {
    slam_map_config c;
    TRY(map_config(cfg, &c));
    if (!x || !P) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 1 || L_max > slam::kMapMaxLandmarks || M < 0 || M > L_max)
        return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d], or L_max is not in [1, %d]", M, L_max, slam::kMapMaxLandmarks);
    if (!ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (meas && k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if ((meas || (prune && !remove)) && (!seen || !expected)) return slam_internal_fail(SLAM_ERR_ARG, "seen or expected is NULL");
    if ((seen == nullptr) != (expected == nullptr)) return slam_internal_fail(SLAM_ERR_ARG, "seen and expected come together");
    const int n = 3 + 2 * M;
    const bool f32 = f32_storage != 0;
    if (f32) {   // what the handle stores
        for (int i = 0; i < n; ++i) x[i] = (double)(float)x[i];
        for (size_t i = 0; i < (size_t)n * n; ++i) P[i] = (double)(float)P[i];
    }
    if (meas && !(status & slam::kMapStatusSkip) && assoc_flag == 0) {
        int k = count < k_stride ? count : k_stride;
        k = k < 0 ? 0 : k;
        int32_t idbuf[slam::kMapIdBlock]; uint8_t okbuf[slam::kMapIdBlock];
        slam::map_tally_instance(slam::MapSeq(), [&](int i) { return x[i]; }, ids, M, meas, k, idbuf, okbuf, range_max * c.range_shrink,
                                 fov_min + c.fov_margin, fov_max - c.fov_margin, seen, expected);
    }
    std::vector<int32_t> mask((size_t)L_max, 0);
    for (int j = 0; j < M; ++j)
        mask[j] = remove ? (remove[j] != 0) : (prune ? slam::map_prune_decide(seen[j], expected[j], c.min_expected, c.min_ratio) : 0);
    if (mask_out) memcpy(mask_out, mask.data(), sizeof(int32_t) * (size_t)L_max);
    std::vector<uint16_t> kept((size_t)L_max);
    int Mk = M;
    // the instance's slab as the handle holds it: rows at the padded leading dimension, elements as integers of the storage type
    auto run = [&](auto zero) {
        using T = decltype(zero);
        using F = typename std::conditional<sizeof(T) == 4, float, double>::type;
        const int ld = slam::ekf_ld(n, (int)sizeof(T));
        std::vector<T> Ps((size_t)n * ld, 0), xs((size_t)n);
        auto bits = [](double v) { const F f = (F)v; T t; memcpy(&t, &f, sizeof(T)); return t; };
        auto value = [](T t) { F f; memcpy(&f, &t, sizeof(T)); return (double)f; };
        for (int r = 0; r < n; ++r)
            for (int cc = 0; cc < n; ++cc) Ps[(size_t)r * ld + cc] = bits(P[(size_t)r * n + cc]);
        for (int i = 0; i < n; ++i) xs[i] = bits(x[i]);
        Mk = slam::map_remove_instance_host(Ps.data(), xs.data(), ids, seen, expected, mask.data(), M, L_max, kept.data());
        if (Mk == M) return;
        const int n2 = 3 + 2 * Mk, ld2 = slam::ekf_ld(n2, (int)sizeof(T));
        for (int r = 0; r < n2; ++r)
            for (int cc = 0; cc < n2; ++cc) P[(size_t)r * n2 + cc] = value(Ps[(size_t)r * ld2 + cc]);
        for (int i = 0; i < n2; ++i) x[i] = value(xs[i]);
    };
    if (f32) run((uint32_t)0); else run((uint64_t)0);
    if (M_out) *M_out = Mk;
    return SLAM_OK;
}

}  // extern "C"
