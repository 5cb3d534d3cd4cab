// capi_merge.cpp — C ABI: merging duplicate landmarks of the EKF batch: the find, the fusion by a partner array, find + fuse + compact in
// one call and the managed run that merges (merge_kernel.hip; the compaction and the managed tick are capi_map.cpp's)
#include <math.h>
#include <string.h>

#include <type_traits>
#include <vector>

#include "assoc_kernel.h"
#include "capi_map.h"
#include "ekf_kernel.h"
#include "map_kernel.h"
#include "merge_kernel.h"

using namespace slam_capi;

namespace {

constexpr int kRows = 6;   // per merge and instance: candidates not mutual, eligible, pairs fused, pairs attempted, slots removed, M before
enum Row { kNotMutual = 0, kFindOn = 1, kFused = 2, kAttempted = 3, kRemoved = 4, kMBefore = 5 };

// *out = *cfg (NULL: the defaults), checked
int merge_config(const slam_merge_config* cfg, slam_merge_config* out) {
    if (cfg) *out = *cfg; else slam_merge_config_default(out);
    if (!(isfinite(out->gate_merge) && out->gate_merge > 0.0))
        return slam_internal_fail(SLAM_ERR_ARG, "merge config: gate_merge = %g is not finite and positive", out->gate_merge);
    if (!(isfinite(out->sigma) && out->sigma >= 0.0))
        return slam_internal_fail(SLAM_ERR_ARG, "merge config: sigma = %g is not finite and non-negative", out->sigma);
    if (out->merge_every < 1) return slam_internal_fail(SLAM_ERR_ARG, "merge config: merge_every = %d is below 1", out->merge_every);
    return SLAM_OK;
}

// the rows of `ticks` merges, the partner and mask arrays, the record, the sums of the traffic model, the per-instance contributions
int merge_reserve(slam_handle* h, size_t ticks, bool d2) {
    const size_t n = (size_t)h->B * h->L_max;
    TRY(grow(h, h->merge.dint, kRows * ticks * (size_t)h->B));
    TRY(grow(h, h->merge.dpartner, n));
    TRY(grow(h, h->merge.dmask, n));
    if (d2) TRY(grow(h, h->merge.dd2, n));
    TRY(grow(h, h->merge.drec, slam::kMergeRecLen));
    TRY(grow(h, h->merge.dwork, 5));
    return innovation_reserve(h, false);
}

int merge_zero_work(slam_handle* h) {
    HIP_TRY(hipMemsetAsync(h->merge.dwork, 0, 5 * sizeof(unsigned long long), h->stream));
    h->merge.work_set = true;
    return SLAM_OK;
}

// The find on the handle's stream into d_partner / d_d2 (NULL: not wanted), its counts into the rows at `rows` (stride cb; the caller
// zeroed them).  Rows an instance does not write keep the presets: -1, NaN (all bits set), 0.
int find_launch(slam_handle* h, const slam_merge_config& c, int32_t* d_partner, double* d_d2, int32_t* rows, size_t cb) {
    const size_t n = (size_t)h->B * h->L_max;
    HIP_TRY(hipMemsetAsync(d_partner, 0xff, sizeof(int32_t) * n, h->stream));
    if (d_d2) HIP_TRY(hipMemsetAsync(d_d2, 0xff, sizeof(double) * n, h->stream));
    slam::MergeFindParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.status = h->dflags;
    p.gate = c.gate_merge; p.sigma2 = c.sigma * c.sigma;
    p.partner = d_partner; p.d2 = d_d2; p.n_notmutual = row(rows, kNotMutual, cb); p.find_on = row(rows, kFindOn, cb);
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    HIP_TRY(slam::launch_merge_find(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

// the fusion by d_partner and the compaction of the slots it marks, on the handle's stream (with_rec: the record into merge.drec)
int fuse_launch(slam_handle* h, const slam_merge_config& c, const int32_t* d_partner, bool found, int32_t* rows, size_t cb, bool with_rec) {
    slam::MergeFuseParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.status = h->dflags;
    p.partner = d_partner; p.n_notmutual = found ? row(rows, kNotMutual, cb) : nullptr; p.sigma2 = c.sigma * c.sigma;
    p.seen = h->map.tracked ? h->map.dseen.get() : nullptr; p.expected = h->map.tracked ? h->map.dexpected.get() : nullptr;
    p.remove = h->merge.dmask; p.n_fused = row(rows, kFused, cb); p.n_attempted = row(rows, kAttempted, cb);
    p.inst_rec = h->inn.dval + 13 * (size_t)h->B;   // (the places innovation_reserve gives the contributions and the partial records)
    p.partials = h->inn.dpart; p.rec = with_rec ? h->merge.drec.get() : nullptr;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    HIP_TRY(slam::launch_merge_fuse(p, h->esz == 4, h->stream));
    slam_map_config mc;
    slam_map_config_default(&mc);
    return map_compact_launch(h, h->merge.dmask, mc, row(rows, kRemoved, cb), row(rows, kMBefore, cb), false);
}

// find (d_partner NULL), fuse and compact on the handle's stream
int merge_launches(slam_handle* h, const slam_merge_config& c, const int32_t* d_partner, int32_t* rows, size_t cb, bool with_rec) {
    if (!d_partner) TRY(find_launch(h, c, h->merge.dpartner, nullptr, rows, cb));
    return fuse_launch(h, c, d_partner ? d_partner : h->merge.dpartner.get(), d_partner == nullptr, rows, cb, with_rec);
}

// the traffic model of one merge whose rows are filled; m: the M the find and the fusion saw
int merge_sum_work(slam_handle* h, const int32_t* m, const int32_t* rows, size_t cb, bool compacted) {
    HIP_TRY(slam::launch_merge_work(m, row(rows, kFindOn, cb), row(rows, kAttempted, cb), row(rows, kFused, cb), (size_t)h->B, h->L_max, h->map.tracked,
                                    h->merge.dwork, h->stream));
    if (compacted)
        HIP_TRY(slam::launch_map_work(row(rows, kMBefore, cb), row(rows, kRemoved, cb), (size_t)h->B, h->L_max, h->esz, 0, h->map.tracked,
                                      h->merge.dwork + 2, h->stream));
    return SLAM_OK;
}

// slam_merge_landmarks* and slam_map_merge once the partner array (or nothing) is on the device
int merge_now(slam_handle* h, const slam_merge_config& c, const int32_t* d_partner, int32_t* n_merged, double* rec) {
    const size_t B = (size_t)h->B;
    TRY(merge_reserve(h, 1, false));
    TRY(merge_zero_work(h));
    int32_t* const rows = h->merge.dint;
    HIP_TRY(hipMemsetAsync(rows, 0, sizeof(int32_t) * kRows * B, h->stream));
    TRY(merge_launches(h, c, d_partner, rows, B, rec != nullptr));
    TRY(merge_sum_work(h, row(rows, kMBefore, B), rows, B, true));
    if (!n_merged && !rec) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return copy_rows({{row(rows, kRemoved, B), n_merged, B}, {h->merge.drec, rec, slam::kMergeRecLen}}, 0, 1);
}

// slam_map_duplicates* once the outputs' device places are known
int duplicates_now(slam_handle* h, const slam_merge_config& c, int32_t* d_partner, double* d_d2) {
    const size_t B = (size_t)h->B;
    TRY(merge_zero_work(h));
    int32_t* const rows = h->merge.dint;
    HIP_TRY(hipMemsetAsync(rows, 0, sizeof(int32_t) * kRows * B, h->stream));
    TRY(find_launch(h, c, d_partner, d_d2, rows, B));
    return merge_sum_work(h, h->dM, rows, B, false);
}

}  // namespace

extern "C" {

int slam_merge_config_default(slam_merge_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->gate_merge = -2.0 * log(0.05); c->sigma = 0.0; c->merge_every = 10;
    return SLAM_OK;
}

int slam_map_duplicates(slam_handle* h, const slam_merge_config* cfg, int32_t* partner, double* d2) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    if (!partner) return slam_internal_fail(SLAM_ERR_ARG, "partner is NULL");
    TRY(map_enter(h, "slam_map_duplicates"));
    TRY(merge_reserve(h, 1, d2 != nullptr));
    TRY(duplicates_now(h, c, h->merge.dpartner, d2 ? h->merge.dd2.get() : nullptr));
    const size_t n = (size_t)h->B * h->L_max;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(partner, h->merge.dpartner, sizeof(int32_t) * n, hipMemcpyDeviceToHost));
    if (d2) HIP_TRY(hipMemcpy(d2, h->merge.dd2, sizeof(double) * n, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_map_duplicates_dev(slam_handle* h, const slam_merge_config* cfg, int32_t* d_partner, double* d_d2) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    if (!d_partner) return slam_internal_fail(SLAM_ERR_ARG, "d_partner is NULL");
    TRY(map_enter(h, "slam_map_duplicates_dev"));
    TRY(merge_reserve(h, 1, false));
    return duplicates_now(h, c, d_partner, d_d2);
}

int slam_merge_landmarks(slam_handle* h, const slam_merge_config* cfg, const int32_t* partner, int32_t* n_merged, double rec[16]) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    if (!partner) return slam_internal_fail(SLAM_ERR_ARG, "partner is NULL");
    TRY(map_enter(h, "slam_merge_landmarks"));
    const size_t n = (size_t)h->B * h->L_max;
    TRY(merge_reserve(h, 1, false));
    // (staged where a find leaves its partner array)
    HIP_TRY(hipMemcpyAsync(h->merge.dpartner, partner, sizeof(int32_t) * n, hipMemcpyHostToDevice, h->stream));
    return merge_now(h, c, h->merge.dpartner, n_merged, rec);
}

int slam_merge_landmarks_dev(slam_handle* h, const slam_merge_config* cfg, const int32_t* d_partner, int32_t* n_merged, double rec[16]) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    if (!d_partner) return slam_internal_fail(SLAM_ERR_ARG, "d_partner is NULL");
    TRY(map_enter(h, "slam_merge_landmarks_dev"));
    return merge_now(h, c, d_partner, n_merged, rec);
}

int slam_map_merge(slam_handle* h, const slam_merge_config* cfg, double rec[16], int32_t* n_merged) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    TRY(map_enter(h, "slam_map_merge"));
    return merge_now(h, c, nullptr, n_merged, rec);
}

}  // extern "C"

namespace {

// slam_manage_merge_run as run_filtered's feature: the managed tick with a merge, every merge_every ticks, between its tally and its
// prune; the merge is the marked group
struct MergeTicks {
    ManageTicks m; const slam_merge_config& gc; int32_t* n_merged;

    RunTimes& times() const { return m.a.h->merge.times; }
    double bytes_per_tick() const { return m.bytes_per_tick() + kRows * 4.0 * (double)m.a.h->B; }
    int reserve(int k_stride, int chunk) {
        TRY(m.reserve(k_stride, chunk));
        TRY(merge_reserve(m.a.h, (size_t)chunk, false));
        return merge_zero_work(m.a.h);
    }
    int chunk_begin() {   // (and the rows of the ticks without a merge)
        TRY(m.chunk_begin());
        HIP_TRY(hipMemsetAsync(m.a.h->merge.dint, 0, sizeof(int32_t) * kRows * m.a.cb, m.a.h->stream));
        return SLAM_OK;
    }
    DevMsg out() const { return m.out(); }
    template <class Mark>
    int filter(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int k_stride, Mark mark) {
        return m.filter(t, cmd, d_each, dm, dc, k_stride, mark);
    }
    int32_t* at(int t) const { return m.a.h->merge.dint + (size_t)t * m.a.B; }   // the rows of tick t, at stride cb
    bool merges_after(int t_run) const { return (t_run + 1) % gc.merge_every == 0; }
    template <class Mark>
    int after_step(int t_run, int t, Mark mark) {
        TRY(m.tally(t));
        // (the marked group of a tick without a merge is empty: its event pair brackets nothing; the merge can move the pose)
        TRY(mark([&]() -> int { return merges_after(t_run) ? merge_launches(m.a.h, gc, nullptr, at(t), m.a.cb, false) : SLAM_OK; }));
        return m.prune(t_run, t);
    }
    int chunk_done(int t0, int tc) {
        for (int t = 0; t < tc; ++t) {
            if (merges_after(t0 + t)) TRY(merge_sum_work(m.a.h, row(at(t), kMBefore, m.a.cb), at(t), m.a.cb, true));
            TRY(m.sum_work(t0 + t, t));
        }
        return SLAM_OK;
    }
    std::vector<TickRow> rows() const {
        std::vector<TickRow> r = m.rows();
        r.push_back({row(at(0), kRemoved, m.a.cb), n_merged, m.a.B});
        return r;
    }
    int finish() { return m.finish(); }
};

}  // namespace

extern "C" {

int slam_manage_merge_run(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg, const slam_merge_config* merge_cfg,
                          const float* cmds, int cmd_each, const float* meas, const int32_t* count, int k_stride, int T, double* recs,
                          int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* n_merged, int32_t* flags) {
    slam_assoc_config ac; slam_map_config mc; slam_merge_config gc;
    TickMsgs msgs;
    TRY(assoc_config(assoc_cfg, &ac));
    TRY(map_config(map_cfg, &mc));
    TRY(merge_config(merge_cfg, &gc));
    TRY(run_args_log(cmds, meas, count, k_stride, T, &msgs));
    return run_filtered(h, "slam_manage_merge_run", cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T,
                        MergeTicks{{{h, ac, recs, n_match, n_new, n_drop, flags}, mc, n_removed}, gc, n_merged});
}

int slam_manage_merge_run_sim(slam_handle* h, const slam_assoc_config* assoc_cfg, const slam_map_config* map_cfg,
                              const slam_merge_config* merge_cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                              int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* n_removed, int32_t* n_merged, int32_t* flags,
                              const slam_sense_log* log) {
    slam_assoc_config ac; slam_map_config mc; slam_merge_config gc;
    TickCmds::Source csrc;
    TickMsgs msgs;
    TRY(assoc_config(assoc_cfg, &ac));
    TRY(map_config(map_cfg, &mc));
    TRY(merge_config(merge_cfg, &gc));
    TRY(run_args_sim(source, cmds, k_stride, T, log, &csrc, &msgs));
    return run_filtered(h, "slam_manage_merge_run_sim", csrc, cmds, msgs, T,
                        MergeTicks{{{h, ac, recs, n_match, n_new, n_drop, flags}, mc, n_removed}, gc, n_merged});
}

int slam_last_merge_work(slam_handle* h, double* bytes, double* merge_ms, double* total_ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (!h->merge.work_set)
        return slam_internal_fail(SLAM_ERR_STATE, "slam_map_duplicates, slam_merge_landmarks, slam_map_merge or slam_manage_merge_run has not run on this handle");
    if (bytes) {
        unsigned long long wk[5];
        HIP_TRY(hipSetDevice(h->device));
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(wk, h->merge.dwork, sizeof(wk), hipMemcpyDeviceToHost));
        *bytes = ((double)wk[0] + 2.0 * (double)wk[2] + (double)wk[3]) * h->esz + (double)wk[1] + (double)wk[4];
    }
    if (merge_ms) *merge_ms = h->merge.times.part_ms;
    if (total_ms) *total_ms = h->merge.times.total_ms;
    return SLAM_OK;
}

int slam_merge_instance_host(double* x, double* P, int32_t* ids, int M, int L_max, int32_t status, int f32_storage, const slam_merge_config* cfg,
                             int32_t* seen, int32_t* expected, const int32_t* partner_in, int fuse, int32_t* partner_out, double* d2_out,
                             double rec[16], int32_t* M_out) {
    slam_merge_config c;
    TRY(merge_config(cfg, &c));
    if (!x || !P) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 1 || L_max > slam::kMapMaxLandmarks || M < 0 || M > L_max)
        return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d], or L_max is not in [1, %d]", M, L_max, slam::kMapMaxLandmarks);
    if (!ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if ((seen == nullptr) != (expected == nullptr)) return slam_internal_fail(SLAM_ERR_ARG, "seen and expected come together");
    const int n = 3 + 2 * M;
    const bool f32 = f32_storage != 0, skip = (status & slam::kMapStatusSkip) != 0;
    const double sigma2 = c.sigma * c.sigma;
    std::vector<int32_t> nn((size_t)L_max, -1), partner((size_t)L_max, -1), mask((size_t)L_max, 0);
    std::vector<double> d2((size_t)L_max, __builtin_nan(""));
    std::vector<uint16_t> pi((size_t)L_max), pj((size_t)L_max), kept((size_t)L_max);
    double r16[slam::kMergeRecLen] = {0.0};
    int Mk = M;
    // the instance's slab as the handle holds it: rows at the padded leading dimension, elements of the storage type
    auto run = [&](auto zero) {
        using ST = decltype(zero);
        using T = typename std::conditional<sizeof(ST) == 4, uint32_t, uint64_t>::type;
        const int ld = slam::ekf_ld(n, (int)sizeof(ST));
        std::vector<ST> Ps((size_t)n * ld, (ST)0), xs((size_t)n);
        for (int r = 0; r < n; ++r)
            for (int cc = 0; cc < n; ++cc) Ps[(size_t)r * ld + cc] = (ST)P[(size_t)r * n + cc];
        for (int i = 0; i < n; ++i) xs[i] = (ST)x[i];
        int lonely = 0;
        if (!skip && M >= 2) {
            slam::merge_find_instance_host([&](int i) { return (double)xs[i]; }, [&](int r, int cc) { return (double)Ps[(size_t)r * ld + cc]; }, M,
                                           c.gate_merge, sigma2, nn.data(), d2.data());
            for (int s = 0; s < M; ++s) {
                const bool mutual = nn[s] >= 0 && nn[nn[s]] == s;
                partner[s] = mutual ? nn[s] : -1;
                lonely += (nn[s] >= 0 && !mutual) ? 1 : 0;
            }
        }
        if (!fuse) return;
        int ignored = 0;
        const int np = slam::merge_pairs_host(partner_in ? partner_in : partner.data(), M, L_max, skip, pi.data(), pj.data(), &ignored);
        if (np == 0) { r16[slam::kMrgNotMutual] = (double)(ignored + (partner_in ? 0 : lonely)); return; }
        std::vector<double> ws((size_t)4 * n + 2);
        const slam::MergeCounts cnt = slam::merge_fuse_instance(slam::MapSeq(), Ps.data(), xs.data(), M, pi.data(), pj.data(), np, sigma2, ws.data(),
                                                                mask.data(), seen, expected);
        r16[slam::kMrgTouched] = cnt.fused > 0 ? 1.0 : 0.0; r16[slam::kMrgFused] = (double)cnt.fused;
        r16[slam::kMrgNotMutual] = (double)(ignored + (partner_in ? 0 : lonely)); r16[slam::kMrgSingular] = (double)cnt.singular;
        r16[slam::kMrgUpdated] = (double)cnt.fused * ((double)n * (double)n);
        r16[slam::kMrgSumD2] = cnt.sum_d2; r16[slam::kMrgMaxD2] = cnt.max_d2;
        if (cnt.fused == 0) return;
        std::vector<T> Pi(Ps.size()), xi(xs.size());   // the compaction moves elements as integers of their size
        memcpy(Pi.data(), Ps.data(), sizeof(T) * Ps.size()); memcpy(xi.data(), xs.data(), sizeof(T) * xs.size());
        Mk = slam::map_remove_instance_host(Pi.data(), xi.data(), ids, seen, expected, mask.data(), M, L_max, kept.data());
        memcpy(Ps.data(), Pi.data(), sizeof(T) * Ps.size()); memcpy(xs.data(), xi.data(), sizeof(T) * xs.size());
        const int n2 = 3 + 2 * Mk, ld2 = slam::ekf_ld(n2, (int)sizeof(ST));
        for (int r = 0; r < n2; ++r)
            for (int cc = 0; cc < n2; ++cc) P[(size_t)r * n2 + cc] = (double)Ps[(size_t)r * ld2 + cc];
        for (int i = 0; i < n2; ++i) x[i] = (double)xs[i];
    };
    if (f32) run(0.0f); else run(0.0);
    if (partner_out) memcpy(partner_out, partner.data(), sizeof(int32_t) * (size_t)L_max);
    if (d2_out) memcpy(d2_out, d2.data(), sizeof(double) * (size_t)L_max);
    if (rec) memcpy(rec, r16, sizeof(r16));
    if (M_out) *M_out = Mk;
    return SLAM_OK;
}

}  // extern "C"
