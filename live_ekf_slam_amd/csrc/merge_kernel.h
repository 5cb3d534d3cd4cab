// merge_kernel.h — merging duplicate landmarks of the EKF batch (slam_map_duplicates, slam_merge_landmarks, slam_map_merge,
// slam_manage_merge_run; gfx950).  A detection farther than gate_new from the map becomes a landmark; after drift or one outlier return a
// landmark that is already mapped is inserted a second time, and from then on the two copies split the detections.  The prune rule of
// map_kernel.h can only delete a copy; the correct operation is an EKF update with the pseudo-measurement l_i - l_j = 0 followed by the
// exact marginalisation of slot j.  The per-instance semantics are defined here, ONCE, for the device kernels (merge_kernel.hip) and the
// host hook (slam_merge_instance_host), both compiled with -ffp-contract=off; arithmetic goes through ekf_model.h (ekf_gain,
// ekf_state_update, ekf_downdate) and slam_math.h (inv2x2_lu) only.  No step, gate, innovation, association or map kernel changes.
//
// Indices: ii = 3 + 2 i, jj = 3 + 2 j, i < j.  All values are the stored ones, widened to double for fp32 storage.
// Cost of the pair (merge_pair_cost):
//   delta = (x[ii] - x[jj], x[ii+1] - x[jj+1])
//   S[a][b] = (P[ii+a][ii+b] - P[ii+a][jj+b]) - (P[jj+a][ii+b] - P[jj+a][jj+b]) + [a == b] sigma^2     (both off-diagonal blocks are read:
//             P is symmetric only to rounding)
//   Si = inv2x2_lu(S);  d2 = delta0 (Si00 delta0 + Si01 delta1) + delta1 (Si10 delta0 + Si11 delta1), unfused
//   d2 = NaN where Si failed or delta or S is not finite.
//   The cost is a function of the UNORDERED pair: whoever evaluates it passes the lower slot first, so it is symmetric by construction.
// Decision: nn(s) = the slot with the smallest finite d2 <= gate_merge against s, ties to the lowest slot (merge_consider), -1 if none.
//   (i, j), i < j, is a duplicate iff nn(i) == j && nn(j) == i: a slot is in at most one pair and no traversal order matters.  Instances
//   with status & kMapStatusSkip (non-finite, frozen, watchdog) or M < 2 have no pairs.
// Fusion (merge_fuse_instance), the pairs of one instance in ascending i, each on the state the previous one left:
//   c_r = (P[r][ii] - P[r][jj], P[r][ii+1] - P[r][jj+1]) for every row r;  g_c = (P[ii][c] - P[jj][c], P[ii+1][c] - P[jj+1][c]) for every column c
//   S[a][b] = (c_{ii+a}.b - c_{jj+a}.b) + [a == b] sigma^2 - the S of the cost, from the current state;  Si = inv2x2_lu(S)
//   Si failed or S not finite: the pair is skipped and counted SINGULAR (nothing is stored)
//   K_r = ekf_gain(c_r, Si);  x[r] = ekf_state_update(x[r], r, K_r.x, K_r.y, -delta0, -delta1)  (yaw wrapped as in the step)
//   P[r][c] = ekf_downdate(P[r][c], K_r.x, K_r.y, g_c.x, g_c.y) for all r and c; stored rounded to the storage type; pad columns stay zero.
// After the last pair: remove[j] = 1 for the slot j of every fused pair (the existing compaction takes it out: the kept slot is i, the
//   kept id ids[i]); with track counters expected' = max(expected[i], expected[j]), seen[i] = min(seen[i] + seen[j], expected'),
//   expected[i] = expected'.  Flags, timestep, truth and err_sum are untouched.  An instance without a fused pair is not written.
// Caller pairs: a partner row [L_max]; the entry of slot s is honoured iff s < M, 0 <= partner[s] < M, partner[s] != s and
//   partner[partner[s]] == s (merge_honoured); every other entry that is not -1 is ignored and counted.  A skipped instance honours none.
//
// Why the update of P may run IN PLACE (the barriers of merge_fuse_instance).  The rows ii, ii+1, jj, jj+1 and the same four columns are
// inputs of EVERY element (through c_r and g_c) and are themselves overwritten.  (1) All c_r, g_c and delta are gathered into the
// workspace (LDS on the device, 4 n + 2 doubles) and a workgroup barrier is passed before the first store of the pair: after it an
// element's new value depends on its own old value - read by the lane that stores it - and on the workspace alone.  (2) A second barrier
// after the stores and before the next pair's gather: that gather reads elements other lanes have just stored, and overwrites the
// workspace that slower lanes may still read.  No third barrier is needed: between (1) and (2) no lane reads an element of P or x that
// another lane writes, S, Si and the decision to skip are recomputed by every lane from the workspace (no broadcast to wait for), and the
// pair list is read-only once built.
#pragma once
#include <stdint.h>

#include "ekf_model.h"
#include "map_kernel.h"
#include "slam_math.h"

namespace slam {

constexpr int kMergeRecLen = 16;                    // doubles of one record
// instances touched, pairs fused, entries / candidates that were not mutual, pairs skipped SINGULAR, elements of P updated (n^2 per fused
// pair), the sum and the largest d2 of the fused pairs (0 without one); the rest 0
enum MergeRec { kMrgTouched = 0, kMrgFused = 1, kMrgNotMutual = 2, kMrgSingular = 3, kMrgUpdated = 4, kMrgSumD2 = 7, kMrgMaxD2 = 8 };
constexpr unsigned kMergeRecMax = 1u << kMrgMaxD2;   // the entries joined by a maximum (record_kernel.h); every other is a sum

SLAM_HD bool merge_finite(double v) { return fabs(v) < __builtin_inf(); }

// S of the pair from its four 2 x 2 blocks (row-major): Pll = P[lo][lo], Plh = P[lo][hi], Phl = P[hi][lo], Phh = P[hi][hi]; lo < hi
SLAM_HD void merge_S(const double Pll[4], const double Plh[4], const double Phl[4], const double Phh[4], double sigma2, double S[4]) {
    S[0] = ((Pll[0] - Plh[0]) - (Phl[0] - Phh[0])) + sigma2;
    S[1] = (Pll[1] - Plh[1]) - (Phl[1] - Phh[1]);
    S[2] = (Pll[2] - Plh[2]) - (Phl[2] - Phh[2]);
    S[3] = ((Pll[3] - Plh[3]) - (Phl[3] - Phh[3])) + sigma2;
}

// d2 from delta and S; *ok: Si is usable (inv2x2_lu succeeded and S is finite)
SLAM_HD double merge_d2(double d0, double d1, const double S[4], double Si[4], bool* ok) {
    *ok = inv2x2_lu(S, Si) && merge_finite(S[0]) && merge_finite(S[1]) && merge_finite(S[2]) && merge_finite(S[3]);
    const double d2 = d0 * (Si[0] * d0 + Si[1] * d1) + d1 * (Si[2] * d0 + Si[3] * d1);
    return (*ok && merge_finite(d0) && merge_finite(d1)) ? d2 : __builtin_nan("");
}

// the cost of the unordered pair {lo, hi}, lo < hi: xl, xh the two positions
SLAM_HD double merge_pair_cost(double xl0, double xl1, double xh0, double xh1, const double Pll[4], const double Plh[4], const double Phl[4],
                               const double Phh[4], double sigma2) {
    double S[4], Si[4];
    bool ok;
    merge_S(Pll, Plh, Phl, Phh, sigma2, S);
    return merge_d2(xl0 - xh0, xl1 - xh1, S, Si, &ok);
}

// slot t with cost d2 as a candidate of the running best (best_d2, best): smaller finite d2 within the gate, ties to the lower slot
SLAM_HD void merge_consider(double d2, int t, double gate, double* best_d2, int* best) {
    if (!(merge_finite(d2) && d2 <= gate)) return;
    if (*best < 0 || d2 < *best_d2 || (d2 == *best_d2 && t < *best)) { *best_d2 = d2; *best = t; }
}

// the entry of slot s of a partner row is an honoured pair
SLAM_HD bool merge_honoured(const int32_t* partner, int s, int M) {
    if (s >= M) return false;
    const int32_t e = partner[s];
    return e >= 0 && e < M && e != s && partner[e] == s;
}

// The nearest neighbours of one instance, sequentially (the host's find; the device maps the same two functions to a workgroup).
// load_x(i), load_P(r, c): the stored values widened.  nn [M], d2 [M] (NaN where nn = -1).
template <class LX, class LP>
void merge_find_instance_host(LX load_x, LP load_P, int M, double gate, double sigma2, int32_t* nn, double* d2) {
    auto block = [&](int r, int c, double B[4]) {
        B[0] = load_P(r, c); B[1] = load_P(r, c + 1); B[2] = load_P(r + 1, c); B[3] = load_P(r + 1, c + 1);
    };
    for (int s = 0; s < M; ++s) {
        int best = -1;
        double bd = __builtin_nan("");
        for (int t = 0; t < M; ++t) {
            if (t == s) continue;
            const int lo = s < t ? s : t, hi = s < t ? t : s, ll = 3 + 2 * lo, hh = 3 + 2 * hi;
            double Pll[4], Plh[4], Phl[4], Phh[4];
            block(ll, ll, Pll); block(ll, hh, Plh); block(hh, ll, Phl); block(hh, hh, Phh);
            merge_consider(merge_pair_cost(load_x(ll), load_x(ll + 1), load_x(hh), load_x(hh + 1), Pll, Plh, Phl, Phh, sigma2), t, gate, &bd, &best);
        }
        nn[s] = best; d2[s] = bd;
    }
}

struct MergeCounts { int fused, singular; double sum_d2, max_d2; };

// The fusion of one instance's pairs (pi[k] < pj[k], ascending pi; LDS on the device), in place.  ST: float or double, P at the leading
// dimension ld = ekf_ld(n), x [n].  ws: 4 n + 2 doubles (c_r at 2 r, g_c at 2 n + 2 c, delta at 4 n).  remove [>= M] receives 1 at the
// slot j of every fused pair (the caller zeroed it); seen / expected may be NULL.  Every lane of the policy calls it with the same
// arguments and gets the same counts.  The barriers: see the top of this file.
template <class W, class ST>
SLAM_HD MergeCounts merge_fuse_instance(const W& w, ST* P, ST* x, int M, const uint16_t* pi, const uint16_t* pj, int n_pairs, double sigma2,
                                        double* ws, int32_t* remove, int32_t* seen, int32_t* expected) {
    const int n = 3 + 2 * M, ld = ekf_ld(n, (int)sizeof(ST));
    MergeCounts cnt = {0, 0, 0.0, 0.0};
    double* const cr = ws;
    double* const gc = ws + 2 * n;
    for (int k = 0; k < n_pairs; ++k) {
        const int ii = 3 + 2 * (int)pi[k], jj = 3 + 2 * (int)pj[k];
        for (int r = w.lane(); r < n; r += w.width()) {
            cr[2 * r] = (double)P[r * ld + ii] - (double)P[r * ld + jj];
            cr[2 * r + 1] = (double)P[r * ld + ii + 1] - (double)P[r * ld + jj + 1];
            gc[2 * r] = (double)P[ii * ld + r] - (double)P[jj * ld + r];
            gc[2 * r + 1] = (double)P[(ii + 1) * ld + r] - (double)P[(jj + 1) * ld + r];
        }
        if (w.lane() == 0) {
            ws[4 * n] = (double)x[ii] - (double)x[jj];
            ws[4 * n + 1] = (double)x[ii + 1] - (double)x[jj + 1];
        }
        w.sync();                                    // (1): every input of the pair is in the workspace before its first store
        const double d0 = ws[4 * n], d1 = ws[4 * n + 1];
        double S[4], Si[4];
        S[0] = (cr[2 * ii] - cr[2 * jj]) + sigma2;
        S[1] = cr[2 * ii + 1] - cr[2 * jj + 1];
        S[2] = cr[2 * (ii + 1)] - cr[2 * (jj + 1)];
        S[3] = (cr[2 * (ii + 1) + 1] - cr[2 * (jj + 1) + 1]) + sigma2;
        bool ok;
        const double d2 = merge_d2(d0, d1, S, Si, &ok);
        if (!ok) cnt.singular += 1;
        else {
            cnt.fused += 1;
            if (merge_finite(d2)) { cnt.sum_d2 += d2; cnt.max_d2 = d2 > cnt.max_d2 ? d2 : cnt.max_d2; }
            const int total = n * ld;                // (<= 2003 * 2004: int)
            int r = w.lane() / ld, c = w.lane() - r * ld;
            const int dr = w.width() / ld, dc = w.width() - dr * ld;
            for (int e = w.lane(); e < total; e += w.width()) {
                if (c < n) {                         // (a pad column stays zero)
                    const EkfVec2 kr = ekf_gain(EkfVec2{cr[2 * r], cr[2 * r + 1]}, Si[0], Si[1], Si[2], Si[3]);
                    P[e] = (ST)ekf_downdate((double)P[e], kr.x, kr.y, gc[2 * c], gc[2 * c + 1]);
                }
                r += dr; c += dc;
                if (c >= ld) { c -= ld; r += 1; }
            }
            for (int q = w.lane(); q < n; q += w.width()) {
                const EkfVec2 kr = ekf_gain(EkfVec2{cr[2 * q], cr[2 * q + 1]}, Si[0], Si[1], Si[2], Si[3]);
                x[q] = (ST)ekf_state_update((double)x[q], q, kr.x, kr.y, -d0, -d1);
            }
            if (w.lane() == 0) {
                const int i = (int)pi[k], j = (int)pj[k];
                remove[j] = 1;
                if (seen) {
                    const int32_t ex = expected[i] > expected[j] ? expected[i] : expected[j];
                    const long long sn = (long long)seen[i] + (long long)seen[j];
                    seen[i] = sn < (long long)ex ? (int32_t)sn : ex;
                    expected[i] = ex;
                }
            }
        }
        w.sync();                                    // (2): the stores are done, and the workspace is free, before the next gather
    }
    return cnt;
}

// The pair list of a partner row as the kernel forms it (host): ascending i.  Returns the number of pairs; *ignored: the entries that are
// neither -1 nor honoured, over all L_max slots.
inline int merge_pairs_host(const int32_t* partner, int M, int L_max, bool skip, uint16_t* pi, uint16_t* pj, int* ignored) {
    int np = 0, ig = 0;
    for (int s = 0; s < L_max; ++s) {
        const bool hon = !skip && merge_honoured(partner, s, M);
        if (hon && partner[s] > s) { pi[np] = (uint16_t)s; pj[np] = (uint16_t)partner[s]; np += 1; }
        if (!hon && partner[s] != -1) ig += 1;
    }
    *ignored = ig;
    return np;
}

// The traffic model of one instance of a merge (slam_last_merge_work), in elements of P / x and in other bytes: the find reads P and x
// once (find_on: it ran and the instance was eligible); an attempted pair gathers 8 n elements and 2 of x; a fused pair reads and writes
// P and x once each; partner row, M, status and the counts; the compaction is map_traffic's.
struct MergeTraffic { unsigned long long elems, other_bytes; };
SLAM_HD MergeTraffic merge_traffic(int M, int find_on, int attempted, int fused, int L_max, bool counters) {
    const unsigned long long n = 3ull + 2ull * (unsigned long long)(M < 0 ? 0 : M);
    MergeTraffic t = {0ull, 8ull + 4ull * (unsigned long long)L_max + 16ull};   // M and status, the partner row, the four counts
    if (find_on) t.elems += n * n + n;
    t.elems += (unsigned long long)attempted * (8ull * n + 2ull) + (unsigned long long)fused * (2ull * n * n + 2ull * n);
    if (fused > 0) t.other_bytes += 4ull * (unsigned long long)(M < 0 ? 0 : M) + (counters ? 24ull : 0ull) * (unsigned long long)fused;
    return t;
}

#if defined(__HIPCC__)
// The find of every instance on `stream`.  partner / d2 / n_cand rows are written only by instances in which some slot has a candidate:
// the caller presets them (-1, NaN, 0).
struct MergeFindParams {
    const void* P; const void* x;     // [B][pstride], [B][xstride] in elements of the storage type
    const int32_t *M, *status;        // [B]
    double gate, sigma2;
    int32_t* partner;                 // [B][L_max]: the mutual partner of the slot, -1 if none
    double* d2;                       // [B][L_max] or NULL: the d2 of the slot's best candidate
    int32_t* n_notmutual;             // [B]: slots with a candidate that was not mutual
    int32_t* find_on;                 // [B] or NULL: 1 where the instance was eligible (the traffic model reads it)
    int32_t B, L_max, pstride, xstride;
};
hipError_t launch_merge_find(const MergeFindParams& p, int f32_storage, hipStream_t stream);

// The fusion of every instance by a partner array on `stream`, then - when rec is wanted - the record (two more launches).
struct MergeFuseParams {
    void* P; void* x;                 // updated in place
    const int32_t *M, *status;
    const int32_t* partner;           // [B][L_max]
    const int32_t* n_notmutual;       // [B] or NULL: added to the ignored entries of the record (the find's count)
    double sigma2;
    int32_t *seen, *expected;         // [B][L_max] or both NULL
    int32_t* remove;                  // [B][L_max]: the mask launch_map_compact then reads; every row is written up to L_max
    int32_t *n_fused, *n_attempted;   // [B] each
    double* inst_rec; double* partials; double* rec;   // as MapCompactParams
    int32_t B, L_max, pstride, xstride;
};
hipError_t launch_merge_fuse(const MergeFuseParams& p, int f32_storage, hipStream_t stream);

// work [2] += the sums of merge_traffic over n instances
hipError_t launch_merge_work(const int32_t* M, const int32_t* find_on, const int32_t* n_attempted, const int32_t* n_fused, size_t n, int L_max,
                             int counters, unsigned long long* work, hipStream_t stream);
#endif

}  // namespace slam
