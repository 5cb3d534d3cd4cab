// capi_score.cpp — C ABI: scoring the estimated map against the true map without ids (score_kernel.hip; the factorisation of
// nees_matched is consistency_kernel.hip's, on the rows the matching selects)
#include <math.h>
#include <string.h>

#include <vector>

#include "slam_handle.h"
#include "consistency_kernel.h"
#include "ekf_kernel.h"
#include "record_kernel.h"
#include "score_kernel.h"

using namespace slam_capi;

namespace {

constexpr int kVals = 3;   // per instance, doubles: map_rms, max_err, nees_matched
constexpr int kInts = 6;   // per instance, int32: n_matched, n_duplicate, n_spurious, dof_matched, flags, slots with a row

// *out = *cfg (NULL: the defaults), checked
int score_config(const slam_score_config* cfg, slam_score_config* out) {
    if (cfg) *out = *cfg; else slam_score_config_default(out);
    if (!(out->match_radius > 0.0))
        return slam_internal_fail(SLAM_ERR_ARG, "score config: match_radius = %g is not positive (+inf is allowed)", out->match_radius);
    if (!(isfinite(out->lm_lo) && isfinite(out->lm_hi) && out->lm_lo <= out->lm_hi))
        return slam_internal_fail(SLAM_ERR_ARG, "score config: the band lm_lo = %g .. lm_hi = %g must be finite and ordered", out->lm_lo, out->lm_hi);
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_score_config_default(slam_score_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->match_radius = INFINITY;
    c->lm_lo = -2.0 * log(0.975); c->lm_hi = -2.0 * log(0.025);   // chi-square quantiles at 0.025 and 0.975, 2 degrees of freedom
    c->full = 0;
    return SLAM_OK;
}

int slam_map_score(slam_handle* h, const slam_score_config* cfg, double rec[16], int32_t* n_matched, int32_t* n_duplicate, int32_t* n_spurious,
                   double* map_rms, double* max_err, double* nees_matched, int32_t* dof_matched, int32_t* flags, int32_t* row, int32_t* role,
                   double* lm_err, double* lm_nees) {
    slam_score_config c;
    TRY(score_config(cfg, &c));
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->kind != SLAM_EKF_SLAM)
        return slam_internal_fail(SLAM_ERR_UNSUPPORTED, "slam_map_score is defined for EKF_SLAM only (the UKF kinds are not covered, as for slam_consistency)");
    TRY(flush_lazy(h));
    if (!h->inited) return slam_internal_fail(SLAM_ERR_STATE, "slam_init has not been called");
    if (h->L <= 0 || !(h->each.maps_each ? (bool)h->each.dmaps : (bool)h->dmap))
        return slam_internal_fail(SLAM_ERR_STATE, "no true map to score the landmarks against: call slam_set_map (or slam_set_maps) first");
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B, n = B * (size_t)(h->L_max > 0 ? h->L_max : 1);
    slam_handle::Score& s = h->score;
    TRY(grow(h, s.dval, kVals * B));
    TRY(grow(h, s.dint, kInts * B));
    TRY(grow(h, s.dslot, 2 * n));
    TRY(grow(h, s.dsloti, 4 * n));
    TRY(grow(h, s.dinst, slam::kScoreRecLen * B));
    TRY(grow(h, s.dpart, slam::kScoreRecLen * (size_t)slam::record_blocks(h->B)));
    TRY(grow(h, s.drec, slam::kScoreRecLen));
    TRY(grow(h, s.dwork, 2));
    slam::ScoreParams p;
    memset(&p, 0, sizeof(p));
    p.P = h->dP; p.x = h->dx; p.M = h->dM; p.status = h->dflags; p.truth = h->dtruth;
    p.map = h->dmap; p.L = h->L;
    if (h->each.maps_each) { p.map_each = h->each.dmaps; p.L_each = h->each.dLs; p.map_stride = h->each.map_stride; }
    p.r2 = c.match_radius * c.match_radius; p.lm_lo = c.lm_lo; p.lm_hi = c.lm_hi;
    p.map_rms = s.dval; p.max_err = s.dval + B;
    double* const d_nees = s.dval + 2 * B;
    p.nees_matched = d_nees;
    p.n_matched = s.dint; p.n_duplicate = s.dint + B; p.n_spurious = s.dint + 2 * B;
    int32_t* const d_dof = s.dint + 3 * B;
    p.dof_matched = d_dof;
    p.flags = s.dint + 4 * B; p.n_with_row = s.dint + 5 * B;
    p.lm_err = s.dslot; p.lm_nees = s.dslot + n;
    p.row = s.dsloti; p.role = s.dsloti + n; p.sel = s.dsloti + 2 * n; p.sel_row = s.dsloti + 3 * n;
    p.inst_rec = s.dinst;
    p.B = h->B; p.L_max = h->L_max; p.pstride = h->pstride; p.xstride = h->xstride;
    // full: the factorisation of slam_consistency on the selected rows, with its workspace and chunks, writing into this call's buffers
    slam::ConsistencyParams q;
    int chunk = 0;
    if (c.full) {
        TRY(consistency_params(h, &q, &chunk));
        q.nees_full = d_nees; q.dof = d_dof; q.flags = p.flags; q.nees_pose = nullptr; q.map_rms = nullptr;
        q.sel = p.sel; q.sel_row = p.sel_row; q.n_sel = p.n_matched; q.inst_rec = p.inst_rec;
    }
    hipEvent_t ev[2] = {nullptr, nullptr};
    HIP_TRY(hipEventCreate(&ev[0]));
    hipError_t e = hipEventCreate(&ev[1]);
    if (e == hipSuccess) e = hipEventRecord(ev[0], h->stream);
    if (e == hipSuccess) e = slam::launch_score(p, h->esz == 4, h->stream);
    if (e == hipSuccess && c.full) e = slam::launch_consistency_selected(q, h->esz == 4, chunk, h->stream);
    if (e == hipSuccess) e = slam::launch_score_record(p.inst_rec, h->B, s.dpart, s.drec, h->stream);
    if (e == hipSuccess) e = hipEventRecord(ev[1], h->stream);
    // the traffic model, outside the timed part
    if (e == hipSuccess) e = hipMemsetAsync(s.dwork, 0, 2 * sizeof(unsigned long long), h->stream);
    if (e == hipSuccess) e = slam::launch_score_work(p, c.full, s.dwork, h->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
    float ms = -1.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
    (void)hipEventDestroy(ev[0]);
    if (ev[1]) (void)hipEventDestroy(ev[1]);
    if (e != hipSuccess) { (void)hipGetLastError(); return slam_internal_fail(SLAM_ERR_HIP, "slam_map_score -> %s", hipGetErrorString(e)); }
    unsigned long long wk[2];
    HIP_TRY(hipMemcpy(wk, s.dwork, sizeof(wk), hipMemcpyDeviceToHost));
    s.bytes = (double)wk[0] * h->esz + (double)wk[1]; s.ms = (double)ms;
    const size_t nl = B * (size_t)h->L_max;
    const struct { const void* src; void* dst; size_t bytes; } out[] = {
        {s.drec, rec, sizeof(double) * slam::kScoreRecLen}, {p.n_matched, n_matched, sizeof(int32_t) * B}, {p.n_duplicate, n_duplicate, sizeof(int32_t) * B},
        {p.n_spurious, n_spurious, sizeof(int32_t) * B}, {p.map_rms, map_rms, sizeof(double) * B}, {p.max_err, max_err, sizeof(double) * B},
        {d_nees, nees_matched, sizeof(double) * B}, {d_dof, dof_matched, sizeof(int32_t) * B}, {p.flags, flags, sizeof(int32_t) * B},
        {p.row, row, sizeof(int32_t) * nl}, {p.role, role, sizeof(int32_t) * nl}, {p.lm_err, lm_err, sizeof(double) * nl},
        {p.lm_nees, lm_nees, sizeof(double) * nl}};
    for (const auto& o : out)
        if (o.dst && o.bytes) HIP_TRY(hipMemcpy(o.dst, o.src, o.bytes, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_last_score_work(slam_handle* h, double* bytes, double* ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->score.ms < 0.0) return slam_internal_fail(SLAM_ERR_STATE, "slam_map_score has not run on this handle");
    if (bytes) *bytes = h->score.bytes;
    if (ms) *ms = h->score.ms;
    return SLAM_OK;
}

int slam_map_score_instance_host(const double* x, const double* P, int M, int L_max, int32_t status, const double truth[3], const double* map, int L,
                                 int f32_storage, const slam_score_config* cfg, int32_t* n_matched, int32_t* n_duplicate, int32_t* n_spurious,
                                 double* map_rms, double* max_err, int32_t* flags, int32_t* row, int32_t* role, double* lm_err, double* lm_nees) {
    slam_score_config c;
    TRY(score_config(cfg, &c));
    if (!x || !P || !truth) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || L_max > slam::kEkfMaxLandmarks || M < 0 || M > L_max)
        return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d], or L_max is not in [0, %d]", M, L_max, slam::kEkfMaxLandmarks);
    if (L < 1 || !map) return slam_internal_fail(SLAM_ERR_ARG, "no true map: L = %d", L);
    const int n = 3 + 2 * M;
    const bool f32 = f32_storage != 0;
    const size_t cap = (size_t)(L_max > 0 ? L_max : 1);
    std::vector<int32_t> wi(6 * cap);
    std::vector<double> wd(4 * cap);
    int32_t* const o_row = wi.data() + 2 * cap;
    int32_t* const o_role = wi.data() + 3 * cap;
    double* const o_err = wd.data() + 2 * cap;
    double* const o_nees = wd.data() + 3 * cap;
    // the stored values: rounded to the storage type, widened
    const slam::ScoreResult v = slam::score_instance(
        slam::ScoreSeq(), [&](int i) { return f32 ? (double)(float)x[i] : x[i]; },
        [&](int r, int cc) { const double e = P[(size_t)r * n + cc]; return f32 ? (double)(float)e : e; }, M, L_max, status, truth, map, L,
        c.match_radius * c.match_radius, c.lm_lo, c.lm_hi, wi.data(), wi.data() + cap, wd.data(), wd.data() + cap, o_row, o_role, o_err, o_nees,
        wi.data() + 4 * cap, wi.data() + 5 * cap);
    if (n_matched) *n_matched = v.n_matched;
    if (n_duplicate) *n_duplicate = v.n_duplicate;
    if (n_spurious) *n_spurious = v.n_spurious;
    if (map_rms) *map_rms = v.map_rms;
    if (max_err) *max_err = v.max_err;
    if (flags) *flags = v.flags;
    if (row) memcpy(row, o_row, sizeof(int32_t) * (size_t)L_max);
    if (role) memcpy(role, o_role, sizeof(int32_t) * (size_t)L_max);
    if (lm_err) memcpy(lm_err, o_err, sizeof(double) * (size_t)L_max);
    if (lm_nees) memcpy(lm_nees, o_nees, sizeof(double) * (size_t)L_max);
    return SLAM_OK;
}

}  // extern "C"
