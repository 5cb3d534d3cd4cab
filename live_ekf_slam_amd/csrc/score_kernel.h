// score_kernel.h — scoring the estimated map of an EKF instance against the true map WITHOUT ids (slam_map_score; gfx950).  With
// landmark_id_is_known = 0 the id stored with a slot says nothing about the true map, so slam_consistency has no landmark truth
// (NO_TRUTH); the evaluation every SLAM paper reports matches estimate and truth by position instead.  The per-instance semantics are
// defined here, ONCE, for the device kernel (score_kernel.hip: one wavefront per instance) and the host hook
// (slam_map_score_instance_host: one lane), both compiled with -ffp-contract=off.  Nothing is written but the outputs.
//
// All arithmetic is fp64 on the stored values, widened for fp32 storage.  M is clamped to [0, L_max] by the caller, Lb is the size of
// the instance's true map, r2 = match_radius * match_radius formed once on the host.
//   d2(j, r)   dx = x[3+2j] - map[2r], dy = x[4+2j] - map[2r+1], d2 = dx dx + dy dy (unfused)
//   row[j]     the r of least d2, ties to the lowest r (score_nearest: an ascending scan with a strict <); a d2 that is not finite never
//              wins.  No finite d2, or the least one > r2: row[j] = -1, SPURIOUS (d2 == r2 is inside; r2 = +inf takes every finite d2).
//   claims     among the slots with the same row the one of least d2 is MATCHED, ties to the lowest slot; the others are DUPLICATE
//              (score_beaten: slot k beats slot j iff row[k] == row[j] and (d2[k] < d2[j] or d2[k] == d2[j] and k < j)).
//   lm_err     sqrt(d2) of a MATCHED or DUPLICATE slot, NaN otherwise
//   lm_nees    of a MATCHED or DUPLICATE slot: the factorisation of slam_consistency (consistency_kernel.hip) on the slot's symmetrised
//              2 x 2 block with e = (dx, dy) appended (score_lm_nees); a pivot that is not > 0 and finite gives NaN and LM_NOT_PD.
//   summary    one lane, the slots in ascending order, one addition per slot: the counts of the roles, sum of d2 and the largest lm_err
//              over MATCHED, map_rms = sqrt(sum / n_matched) (0 over none), the finite lm_nees of MATCHED slots (their number, sum and
//              how many lie below lo / above hi), and the compacted list of the MATCHED slots with their true rows (sel, sel_row): the
//              rows of S the factorisation of nees_matched takes (launch_consistency_selected).
//   failed     status & (SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG), or a component of the pose error (x - x_true, y - y_true,
//              wrap2pi(yaw - yaw_true)) that is not finite: INSTANCE_FAILED alone, every value NaN, counts 0, row = -1, role NONE.
//   A landmark coordinate that is not finite fails nothing: every d2 of its slot is NaN, so the slot is SPURIOUS.
#pragma once
#include <math.h>
#include <stdint.h>

#include "slam_math.h"

namespace slam {

constexpr int kScoreRecLen = 16;                    // doubles of one record
// instances scored (not failed), failed, then over the scored ones: the sums of M, MATCHED, DUPLICATE and SPURIOUS slots, the sum of d2
// and the largest lm_err over MATCHED, the finite lm_nees of MATCHED slots (number, sum, below lm_lo, above lm_hi), the finite
// nees_matched (number, sum, the sum of their dof_matched: written by the factorisation, 0 with full = 0), instances with at least one
// DUPLICATE or SPURIOUS slot
enum ScoreRec { kScrScored = 0, kScrFailed = 1, kScrSumM = 2, kScrMatched = 3, kScrDuplicate = 4, kScrSpurious = 5, kScrSumD2 = 6, kScrMaxErr = 7,
                kScrLmN = 8, kScrLmSum = 9, kScrLmBelow = 10, kScrLmAbove = 11, kScrFullN = 12, kScrFullSum = 13, kScrFullDof = 14,
                kScrUnclean = 15 };
constexpr unsigned kScoreRecMax = 1u << kScrMaxErr;  // the entries joined by a maximum (record_kernel.h); every other is a sum

enum ScoreRole { kScoreNone = 0, kScoreMatched = 1, kScoreDuplicate = 2, kScoreSpurious = 3 };
constexpr int32_t kScoreMatchedNotPd = 1, kScoreLmNotPd = 4, kScoreFailed = 8;   // slam_score_flags
constexpr int32_t kScoreStatusFailed = 1 | 32;      // SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG

SLAM_HD bool score_finite(double v) { return fabs(v) < __builtin_inf(); }
SLAM_HD bool score_pivot_ok(double d) { return d > 0.0 && d < __builtin_inf(); }

// one lane: what the host hook runs the definition with
struct ScoreSeq {
    int lane() const { return 0; }
    int width() const { return 1; }
    void sync() const {}
    bool any(bool b) const { return b; }             // some lane holds true
};

// the nearest true row of the position (px, py), -1 if no d2 is finite; *d2 its distance squared (NaN if -1)
SLAM_HD int score_nearest(double px, double py, const double* map, int Lb, double* d2) {
    int best = -1;
    double bd = __builtin_nan("");
    for (int r = 0; r < Lb; ++r) {
        const double dx = px - map[2 * r], dy = py - map[2 * r + 1];
        const double d = dx * dx + dy * dy;
        if (score_finite(d) && (best < 0 || d < bd)) { best = r; bd = d; }
    }
    *d2 = bd;
    return best;
}

// slot k beats slot j for the true row both claim
SLAM_HD bool score_beaten(int j, int rj, double dj, int k, int rk, double dk) {
    return k != j && rk == rj && (dk < dj || (dk == dj && k < j));
}

// the NEES of (dx, dy) under the symmetrised block [[a, b], [b, c]], b = (p10 + p01) / 2; *ok: both pivots passed (else NaN)
SLAM_HD double score_lm_nees(double a, double p01, double p10, double c, double dx, double dy, bool* ok) {
    const double b = 0.5 * (p10 + p01);
    const double s0 = sqrt(a);
    const double y0 = dx / s0, l = b / s0;
    const double d = c - l * l;
    const double y1 = (dy - y0 * l) / sqrt(d);
    *ok = score_pivot_ok(a) && score_pivot_ok(d);
    return *ok ? y0 * y0 + y1 * y1 : __builtin_nan("");
}

// what the summary of one instance holds (valid in lane 0)
struct ScoreResult {
    int32_t M, n_matched, n_duplicate, n_spurious, flags;
    double sum_d2, map_rms, max_err;
    int32_t lm_n, lm_below, lm_above;
    double lm_sum;
};

// One instance.  load_x(i), load_P(r, c): the stored values widened; every index is below 3 + 2 M.  truth [3], map [Lb][2].
// ws_row, ws_role [M] and ws_d2, ws_nees [M]: the workspace the claims are resolved in and lane 0 sums up from (LDS on the device: no
// lane reads an output another lane wrote).  row, role, lm_err, lm_nees [L_max] each are written in full, sel and sel_row [>= M] up to
// n_matched (none may be NULL).  Every lane of the policy calls it with the same arguments.
template <class W, class LX, class LP>
SLAM_HD ScoreResult score_instance(const W& w, LX load_x, LP load_P, int M, int L_max, int32_t status, const double* truth, const double* map, int Lb,
                                   double r2, double lo, double hi, int32_t* ws_row, int32_t* ws_role, double* ws_d2, double* ws_nees, int32_t* row,
                                   int32_t* role, double* lm_err, double* lm_nees, int32_t* sel, int32_t* sel_row) {
    const double nan = __builtin_nan("");
    ScoreResult v = {M, 0, 0, 0, 0, nan, nan, nan, 0, 0, 0, 0.0};
    const double e0 = load_x(0) - truth[0], e1 = load_x(1) - truth[1], e2 = wrap2pi(load_x(2) - truth[2]);
    if ((status & kScoreStatusFailed) != 0 || !score_finite(e0) || !score_finite(e1) || !score_finite(e2)) {   // (alike in every lane)
        for (int j = w.lane(); j < L_max; j += w.width()) { row[j] = -1; role[j] = kScoreNone; lm_err[j] = nan; lm_nees[j] = nan; }
        v.flags = kScoreFailed;
        return v;
    }
    // the nearest true row of every slot (a lane owns the slots j = lane + k * width)
    for (int j = w.lane(); j < M; j += w.width()) {
        double d2;
        const int r = score_nearest(load_x(3 + 2 * j), load_x(4 + 2 * j), map, Lb, &d2);
        const bool in = r >= 0 && d2 <= r2;
        ws_row[j] = in ? r : -1; ws_d2[j] = d2;
    }
    w.sync();                                        // every slot's claim before it is compared with the others
    bool bad = false;
    for (int j = w.lane(); j < L_max; j += w.width()) {
        int rl = kScoreNone, rj = -1;
        double err = nan, nees = nan;
        if (j < M) {
            rj = ws_row[j];
            rl = kScoreSpurious;
            if (rj >= 0) {
                const double dj = ws_d2[j];
                bool beaten = false;
                for (int k = 0; k < M; ++k) beaten = beaten || score_beaten(j, rj, dj, k, ws_row[k], ws_d2[k]);
                rl = beaten ? kScoreDuplicate : kScoreMatched;
                err = sqrt(dj);
                const int i = 3 + 2 * j;
                bool ok;
                nees = score_lm_nees(load_P(i, i), load_P(i, i + 1), load_P(i + 1, i), load_P(i + 1, i + 1), load_x(i) - map[2 * rj],
                                     load_x(i + 1) - map[2 * rj + 1], &ok);
                bad = bad || !ok;
            }
        }
        row[j] = rj; role[j] = rl; lm_err[j] = err; lm_nees[j] = nees;
        if (j < M) { ws_role[j] = rl; ws_nees[j] = nees; }
    }
    w.sync();                                        // the roles and values lane 0 sums up
    if (w.any(bad)) v.flags |= kScoreLmNotPd;
    if (w.lane() != 0) return v;
    v.sum_d2 = 0.0; v.max_err = 0.0; v.map_rms = 0.0;
    for (int j = 0; j < M; ++j) {
        const int rl = ws_role[j];
        if (rl == kScoreSpurious) v.n_spurious += 1;
        if (rl == kScoreDuplicate) v.n_duplicate += 1;
        if (rl != kScoreMatched) continue;
        sel[v.n_matched] = j; sel_row[v.n_matched] = ws_row[j];
        v.n_matched += 1;
        v.sum_d2 += ws_d2[j];
        const double err = sqrt(ws_d2[j]);
        v.max_err = err > v.max_err ? err : v.max_err;
        const double q = ws_nees[j];
        if (score_finite(q)) {
            v.lm_n += 1; v.lm_sum += q;
            v.lm_below += q < lo ? 1 : 0; v.lm_above += q > hi ? 1 : 0;
        }
    }
    if (v.n_matched > 0) v.map_rms = sqrt(v.sum_d2 / (double)v.n_matched);
    return v;
}

// what one instance adds to a score record; entries 12 - 14 belong to the factorisation of nees_matched
SLAM_HD void score_record(const ScoreResult& v, double r[kScoreRecLen]) {
    for (int i = 0; i < kScoreRecLen; ++i) r[i] = 0.0;
    if (v.flags & kScoreFailed) { r[kScrFailed] = 1.0; return; }
    r[kScrScored] = 1.0; r[kScrSumM] = (double)v.M;
    r[kScrMatched] = (double)v.n_matched; r[kScrDuplicate] = (double)v.n_duplicate; r[kScrSpurious] = (double)v.n_spurious;
    r[kScrSumD2] = v.sum_d2; r[kScrMaxErr] = v.max_err;
    r[kScrLmN] = (double)v.lm_n; r[kScrLmSum] = v.lm_sum; r[kScrLmBelow] = (double)v.lm_below; r[kScrLmAbove] = (double)v.lm_above;
    r[kScrUnclean] = (v.n_duplicate + v.n_spurious) > 0 ? 1.0 : 0.0;
}

// The traffic model of one instance (slam_last_score_work), in elements of x / P and in other bytes.  Matching: x, the 2 x 2 diagonal
// block of every slot with a row, M, status and the truth, the map once, the outputs (four per-slot rows, the list of MATCHED slots, the
// eight per-instance values, the record).  A failed instance reads the pose only.  full: the factorisation reads the pose and the MATCHED
// slots of x again, the (3 + 2 n_matched)^2 elements of P it selects, the list and the map rows of the MATCHED slots.
struct ScoreTraffic { unsigned long long elems, other_bytes; };
SLAM_HD ScoreTraffic score_traffic(int M, int Lb, int L_max, int n_with_row, int n_matched, bool failed, bool full) {
    const unsigned long long m = (unsigned long long)(M < 0 ? 0 : M), lb = (unsigned long long)(Lb < 0 ? 0 : Lb), lmax = (unsigned long long)L_max;
    ScoreTraffic t = {3ull, 8ull + 24ull + 32ull * lmax + 48ull + 8ull * kScoreRecLen};
    if (failed) return t;
    t.elems += 2ull * m + 4ull * (unsigned long long)n_with_row;
    t.other_bytes += (m > 0 ? 16ull * lb : 0ull) + 8ull * (unsigned long long)n_matched;
    if (full) {
        const unsigned long long nf = 3ull + 2ull * (unsigned long long)n_matched;
        t.elems += nf + nf * nf;
        t.other_bytes += (8ull + 16ull) * (unsigned long long)n_matched;
    }
    return t;
}

#if defined(__HIPCC__)
// One scoring of every instance on `stream`: one launch, one wavefront per instance.  The record is reduced by launch_score_record, a
// call of its own, because with full = 1 the factorisation adds its entries to inst_rec in between.  Everything is read only but the outputs.
struct ScoreParams {
    const void* P; const void* x;     // [B][pstride], [B][xstride] in elements of the storage type
    const int32_t *M, *status;        // [B]
    const double* truth;              // [B][3]
    const double* map; int32_t L;     // the shared true map [L][2] ...
    const double* map_each; const int32_t* L_each; int32_t map_stride;   // ... or one per instance, as ConsistencyParams
    double r2, lm_lo, lm_hi;
    int32_t *n_matched, *n_duplicate, *n_spurious, *flags;   // [B] each
    double *map_rms, *max_err;        // [B] each
    double* nees_matched; int32_t* dof_matched;   // [B] each: written as NaN and 0; launch_consistency_selected then overwrites them
    int32_t *row, *role; double *lm_err, *lm_nees;           // [B][L_max] each
    int32_t *sel, *sel_row;           // [B][L_max] each: the MATCHED slots in ascending order and their true rows (n_matched entries)
    int32_t* n_with_row;              // [B]: MATCHED + DUPLICATE slots (the traffic model reads it)
    double* inst_rec;                 // [B][kScoreRecLen]
    int32_t B, L_max, pstride, xstride;
};
hipError_t launch_score(const ScoreParams& p, int f32_storage, hipStream_t stream);
// inst_rec -> rec [kScoreRecLen] through partials [record_blocks(B)][kScoreRecLen], join mask kScoreRecMax
hipError_t launch_score_record(const double* inst_rec, int B, double* partials, double* rec, hipStream_t stream);
// work [2] += the sums of score_traffic over the B instances
hipError_t launch_score_work(const ScoreParams& p, int full, unsigned long long* work, hipStream_t stream);
#endif

}  // namespace slam
