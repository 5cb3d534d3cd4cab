// joint_kernel.h — joint-compatibility association (JCBB, Neira and Tardos) of detections that come WITHOUT landmark ids
// (slam_associate_joint, slam_step_associated_joint, slam_associate_joint_run; gfx950).  slam_associate (assoc_kernel.h) judges every
// detection alone; when the pose is uncertain relative to the landmark spacing every detection sits inside the individual gate of several
// landmarks, and the errors of all detections are tied together through the pose.  Here the hypothesis is judged as a whole: among the
// hypotheses whose STACKED innovation passes a chi-square test with 2 m degrees of freedom, the one that pairs the most detections.
// As there, a side kernel labels the message and the unmodified known-id step consumes it.
//
// joint_instance() below is THE definition: the device kernel (joint_kernel.hip) and the host test hook
// (slam_associate_joint_instance_host) compile this one function, with -ffp-contract=off on both sides, so the two give the same bits.
//
// 1  Costs.  d2[l][j], nu and the per-landmark H and S are those of associate_instance, bit for bit: assoc_cost_phase() and
//    assoc_landmark() of assoc_kernel.h, called by both.
// 2  Individual compatibility.  The candidates of detection l are the slots with finite d2 <= gate_match, ascending by (d2, j); the first
//    kJointMaxCand = 4 are kept.  A detection without a candidate is treated as in slam_associate: INVALID when M > 0 and it has no
//    finite cost, NEW when M == 0 or best > gate_new, else AMBIGUOUS; NEW ranks, ids, NO_ROOM, frozen and TOO_LONG instances and the
//    empty message are as there.
//    The distinct landmarks of the kept candidates go into a table of kJointMaxLm = 64 entries in (message order, candidate order); a
//    candidate whose landmark would be the 65th is never paired (flag kJointLmTable; it needs more than 64 landmarks inside individual
//    gates).  The table holds H (eight entries; H02 = 0, H12 = -1) and the lower triangle of S of every entry, from assoc_landmark().
// 3  Hypotheses.  Each detection with candidates is paired with one of them or left unpaired; a landmark is used at most once; at most
//    kJointMaxPair = 16 = kInnovMaxLm pairings, so a jointly labelled message is never TOO_LONG for slam_innovation / slam_gate
//    because of its matches.
// 4  Joint distance of (l_1, j_1) ... (l_m, j_m), pairing p taking rows 2 p, 2 p + 1 of the stacked system, in the order the search
//    adds them (l ascending):
//      nu      the cost phase's values
//      S       diagonal blocks: the cost phase's S_j, LOWER triangle read (s[0], s[2], s[3]).  Block (new pairing a, older pairing b)
//              = H_a P_pred[block a, block b] H_b^T with block x = {0, 1, 2, i_x, i_x + 1}: the 5 x 5 operand is read as
//              P[idx_a[r]][idx_b[c]] (the ROWS of the newer pairing's landmark) through load_P, so fp32 storage is rounded as the
//              handle holds it; every element goes through ekf_predicted (pose rows and columns predicted, the landmark - landmark
//              block as stored); then ekf_hp_col with H_a column by column and ekf_pht_row with H_b for the two rows.  Only these
//              lower blocks are formed.
//      L       Cholesky, two rows per pairing, right-looking: R[c] = R[c] / L[c][c], then R[cc] -= R[c] L[cc][c] for cc > c, c ascending
//              (every element sees its subtractions in ascending c, whatever the lane count); the corner d0 = S00 - sum R0[t]^2,
//              l10 = (S10 - sum R1[t] R0[t]) / l00, d1 = (S11 - sum R1[t]^2) - l10^2, sums ascending t.  Pivot test: > 0 and finite, no
//              floor.  A failed pivot makes the pairing incompatible and raises kJointSingular.
//      y       y0 = (nu0 - sum R0[t] y[t]) / l00, y1 = ((nu1 - sum R1[t] y[t]) - l10 y0) / l11;  d2_m = d2_{m-1} + (y0 y0 + y1 y1):
//              non-decreasing along a branch, in floating point too.
//      A hypothesis is compatible iff d2_m <= gate_joint[m - 1] (a NaN is incompatible).
// 5  Search.  Depth first over the detections with candidates in message order; at each the candidates in ascending (d2, j), then the
//    unpaired branch.  Best: most pairings, then smallest joint distance, then first found.  On entering a level with `pairs` pairings
//    and `remaining` detections: bound = pairs + min(remaining, 16 - pairs); the branch is cut when bound < best_pairs, or
//    bound == best_pairs and its distance >= the best's.  A NODE is one attempted pairing (one two-row extension); candidates whose
//    landmark is used or outside the table, and unpaired branches, are free.  When a pairing would be node max_nodes + 1 the search
//    stops: the branch at hand, its remaining detections unpaired, competes as a last hypothesis, flag kJointBudget.  The first dive
//    is sequential-compatibility nearest neighbour.
// 6  Verdicts.  MATCHED to the paired slot; kAssocJointUnpaired = 7: had candidates, the best hypothesis leaves it out, dropped (never
//    inserted as new).  The output message is built as step 5 of assoc_kernel.h.
// Per detection slot: verdict, slot (the paired slot when MATCHED, else the individual best or -1), det[4] = (d2, d2_second, nu_r, nu_b)
// as slam_associate, d2 and nu being those of the paired slot when MATCHED, and the number of candidates kept.
// Record (kInnovRecLen doubles): 0 evaluated, 1 FROZEN, 2 TOO_LONG, 3 detections in, 4 matched, 5 new, 6 ambiguous, 7 sum of d2_joint,
// 8 max of d2_joint, 9 unpaired, 10 no room, 11 invalid, 12 sum of nodes, 13 instances with kJointBudget, 14 instances with
// kJointSingular, 15 matched detections whose slot is not their individual best.  Entry 8 is a maximum, the rest sums (kJointRecMax).
// Out of scope: the UKF kinds, the simulator sources, slam_multi_*, the pose graph, joint association inside slam_manage_run /
// slam_manage_merge_run, the ln det S term, more than 16 pairings per message.
#pragma once
#include "assoc_kernel.h"

namespace slam {

constexpr int kJointMaxCand = 4;                     // SLAM_JOINT_MAX_CAND
constexpr int kJointMaxPair = 16;                    // SLAM_JOINT_MAX_PAIR
constexpr int kJointMaxLm = 64;                      // entries of the candidate-landmark table
constexpr int kJointN = 2 * kJointMaxPair;           // rows of the largest stacked system
constexpr int kJointMaxNodes = 65536;
constexpr int32_t kAssocJointUnpaired = 7;           // SLAM_ASSOC_JOINT_UNPAIRED
constexpr int32_t kJointBudget = 16, kJointSingular = 32, kJointLmTable = 64;   // slam_joint_flags, beside kInnovFrozen and kInnovTooLong
static_assert(kJointMaxPair == kInnovMaxLm, "a jointly labelled message is never TOO_LONG because of its matches");
static_assert(kJointMaxLm == 64 && kInnovMaxDet == 64, "the used-landmark set is one 64-bit word, one lane per table entry");

enum JointRec {
    kJntEval = 0, kJntFrozen = 1, kJntTooLong = 2, kJntDetIn = 3, kJntMatched = 4, kJntNew = 5, kJntAmbiguous = 6, kJntSumD2 = 7,
    kJntMaxD2 = 8, kJntUnpaired = 9, kJntNoRoom = 10, kJntInvalid = 11, kJntNodes = 12, kJntBudget = 13, kJntSingular = 14, kJntDiffer = 15
};
constexpr unsigned kJointRecMax = 1u << kJntMaxD2;   // the entries joined by a maximum (record_kernel.h)

// what one instance holds between its phases: LDS on the device (one per wavefront), plain memory on the host.  Arrays over detections
// and table entries are indexed [..][l]: lane l reads element l, consecutive banks.
struct JointWork {
    AssocWork a;
    double cd2[kJointMaxCand][kInnovMaxDet], cnu0[kJointMaxCand][kInnovMaxDet], cnu1[kJointMaxCand][kInnovMaxDet];   // the candidates' d2 and nu
    int32_t cj[kJointMaxCand][kInnovMaxDet], ct[kJointMaxCand][kInnovMaxDet];   // their slot and table entry (-1: outside the table)
    int32_t cn[kInnovMaxDet];                           // candidates kept
    int32_t dl[kInnovMaxDet];                           // level -> detection (those with candidates, message order)
    int32_t ci[kInnovMaxDet], asg[kInnovMaxDet], best[kInnovMaxDet];   // per level: next choice, the choice of the branch, of the best
    int32_t sel[kInnovMaxDet];                          // per detection: the candidate of the best hypothesis, -1 unpaired
    int32_t tab[kJointMaxLm];                           // table entry -> landmark slot
    double tH[8][kJointMaxLm], tS[3][kJointMaxLm];      // H and the lower triangle of S of the table's landmarks
    double L[kJointN * (kJointN + 1) / 2];              // the factor, lower triangle packed by rows
    double y[kJointN];
    double d2s[kJointMaxPair + 1];                      // the joint distance by pairing count
    double gj[kJointMaxPair];                           // gate_joint (the device's copy: its kernel fills it and passes it on)
    int32_t ptab[kJointMaxPair];                        // pairing -> table entry
};

struct JointResult {
    int32_t n_match, n_new, n_drop, flags;
    int32_t n_in, n_amb, n_unp, n_room, n_inv, count_out, nodes, n_diff;
    int32_t blocks;                                     // 2 x 2 landmark - landmark blocks of P read on demand (the traffic model)
    double d2_joint;
};

// The host's execution policy and (below) the device's: AssocSeq / AssocWave with a ballot and a find
struct JointSeq : AssocSeq {
    unsigned long long ballot(bool p) const { return p ? 1ull : 0ull; }
    int uni(int v) const { return v; }
    template <class F> int first(int n, F f) const {   // smallest i < n with f(i), -1 if none
        for (int i = 0; i < n; ++i)
            if (f(i)) return i;
        return -1;
    }
};

// the cost phase's sink: candidate lists.  The lanes holding a candidate of detection l insert it one after the other in ascending j.
struct JointSink {
    JointWork& ws;
    double gate_match;
    template <class W> SLAM_HD void pair(const W& w, int l, int j, bool fin, double d2, const EkfVec2& nu) const {
        unsigned long long m = w.ballot(fin && d2 <= gate_match);
        while (m != 0ull) {
            const int src = __builtin_ctzll(m);
            m &= m - 1ull;
            if (w.lane() == src) {
                const int n = ws.cn[l];
                int pos = 0;                          // (entries already there have lower j: they stay in front on a tie)
                for (int e = 0; e < n; ++e) pos += ws.cd2[e][l] <= d2 ? 1 : 0;
                if (pos < kJointMaxCand) {
                    for (int e = (n < kJointMaxCand ? n : kJointMaxCand - 1); e > pos; --e) {
                        ws.cd2[e][l] = ws.cd2[e - 1][l]; ws.cnu0[e][l] = ws.cnu0[e - 1][l]; ws.cnu1[e][l] = ws.cnu1[e - 1][l];
                        ws.cj[e][l] = ws.cj[e - 1][l];
                    }
                    ws.cd2[pos][l] = d2; ws.cnu0[pos][l] = nu.x; ws.cnu1[pos][l] = nu.y; ws.cj[pos][l] = j;
                    ws.cn[l] = n < kJointMaxCand ? n + 1 : kJointMaxCand;
                }
            }
            w.sync();
        }
    }
};

SLAM_HD EkfH joint_table_H(const JointWork& ws, int t) {
    return EkfH{ws.tH[0][t], ws.tH[1][t], ws.tH[2][t], ws.tH[3][t], ws.tH[4][t], ws.tH[5][t], ws.tH[6][t], ws.tH[7][t]};
}

// One node: the hypothesis of p pairings (ws.ptab, ws.L, ws.y, ws.d2s[p]) extended by table entry ta with innovation (nu0, nu1).  Writes
// rows 2 p and 2 p + 1 of L and y and ws.d2s[p + 1]; false: a pivot failed (nothing of the branch below p is touched either way).
template <class W, class LP>
SLAM_HD bool joint_extend(const W& w, JointWork& ws, LP load_P, const EkfMotion& m, const InnovNoise& nz, int p, int ta, double nu0, double nu1) {
    const int n0 = 2 * p, r0 = n0, r1 = n0 + 1;
    double* const R0 = ws.L + r0 * (r0 + 1) / 2;
    double* const R1 = ws.L + r1 * (r1 + 1) / 2;
    const int ia = 3 + 2 * ws.tab[ta];
    const EkfH ha = joint_table_H(ws, ta);
    const double q[2][2] = {{m.q00, m.q01}, {m.q10, m.q11}};
    // ---- the cross blocks against the pairings on the stack: lanes over them ----
    for (int b = w.lane(); b < p; b += w.width()) {
        const int tb = ws.ptab[b];
        const int ib = 3 + 2 * ws.tab[tb];
        const EkfH hb = joint_table_H(ws, tb);
        const int ra[5] = {0, 1, 2, ia, ia + 1}, cb[5] = {0, 1, 2, ib, ib + 1};
        double a2[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) a2[r] = load_P(ra[r], 2);
        EkfVec2 hp[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) {
            double a[5], pc[5];
#pragma unroll
            for (int r = 0; r < 5; ++r) a[r] = c == 2 ? a2[r] : load_P(ra[r], cb[c]);
#pragma unroll
            for (int r = 0; r < 5; ++r) pc[r] = ekf_predicted(a[r], r, c, a[2], a2[r], a2[2], m.fa, m.fb, (r < 2 && c < 2) ? q[r][c] : 0.0, nz.V11);
            hp[c] = ekf_hp_col(ha, pc[0], pc[1], pc[2], pc[3], pc[4]);
        }
        const EkfVec2 s0 = ekf_pht_row(hb, hp[0].x, hp[1].x, hp[2].x, hp[3].x, hp[4].x);
        const EkfVec2 s1 = ekf_pht_row(hb, hp[0].y, hp[1].y, hp[2].y, hp[3].y, hp[4].y);
        R0[2 * b] = s0.x; R0[2 * b + 1] = s0.y; R1[2 * b] = s1.x; R1[2 * b + 1] = s1.y;
    }
    w.sync();
    // ---- the two rows against the factor so far, right-looking: element cc sees its subtractions in ascending c ----
    for (int c = 0; c < n0; ++c) {
        const double lcc = ws.L[c * (c + 1) / 2 + c];
        for (int e = w.lane(); e < 2; e += w.width()) {
            double* const R = e ? R1 : R0;
            R[c] = R[c] / lcc;
        }
        w.sync();
        for (int e = w.lane(); e < 2 * kJointN; e += w.width()) {
            const int cc = e % kJointN;
            double* const R = e / kJointN ? R1 : R0;
            if (cc > c && cc < n0) R[cc] = R[cc] - R[c] * ws.L[cc * (cc + 1) / 2 + c];
        }
        w.sync();
    }
    // ---- the corner and y: every lane the same sums in ascending t (LDS broadcasts) ----
    const double s00 = ws.tS[0][ta], s10 = ws.tS[1][ta], s11 = ws.tS[2][ta];
    double d0 = s00;
    for (int t = 0; t < n0; ++t) d0 = d0 - R0[t] * R0[t];
    bool ok = d0 > 0.0 && innov_finite(d0);
    const double l00 = sqrt(ok ? d0 : 1.0);
    double o = s10;
    for (int t = 0; t < n0; ++t) o = o - R1[t] * R0[t];
    const double l10 = o / l00;
    double d1 = s11;
    for (int t = 0; t < n0; ++t) d1 = d1 - R1[t] * R1[t];
    d1 = d1 - l10 * l10;
    ok = ok && d1 > 0.0 && innov_finite(d1);
    const double l11 = sqrt(ok ? d1 : 1.0);
    double v0 = nu0, v1 = nu1;
    for (int t = 0; t < n0; ++t) v0 = v0 - R0[t] * ws.y[t];
    for (int t = 0; t < n0; ++t) v1 = v1 - R1[t] * ws.y[t];
    const double y0 = v0 / l00;
    const double y1 = (v1 - l10 * y0) / l11;
    const double d2 = ws.d2s[p] + (y0 * y0 + y1 * y1);
    w.sync();                                         // (every lane has read the rows before the corner is written)
    if (ok && w.lane() == 0) {
        R0[r0] = l00; R1[r0] = l10; R1[r1] = l11;
        ws.y[r0] = y0; ws.y[r1] = y1;
        ws.d2s[p + 1] = d2;
    }
    w.sync();
    return ok;
}

// One instance.  Arguments as associate_instance; gate_joint [kJointMaxPair], memory every lane can read; ncand [kInnovMaxDet] or NULL.
template <class W, class LX, class LP>
SLAM_HD JointResult joint_instance(const W& w, JointWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status,
                                   float fwd, float ang, int k, const InnovNoise& nz, double gate_match, double gate_new,
                                   const double* gate_joint, int max_nodes, double* cost, int32_t* verdict, int32_t* slot, double* det,
                                   int32_t* ncand, float* meas_out) {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    JointResult out;
    out.n_match = out.n_new = out.n_drop = out.flags = 0;
    out.n_in = out.n_amb = out.n_unp = out.n_room = out.n_inv = out.count_out = out.nodes = out.n_diff = out.blocks = 0;
    out.d2_joint = 0.0;
    if (status & kInnovStatusFrozen) out.flags = kInnovFrozen;
    else if (k > kInnovMaxDet) out.flags = kInnovTooLong;
    if (out.flags) {   // an empty message
        assoc_empty_message(w, k, verdict, slot, det, meas_out);
        if (ncand)
            for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) ncand[l] = 0;
        return out;
    }
    M = M < 0 ? 0 : (M > L_max ? L_max : M);
    AssocWork& as = ws.a;
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) { ws.cn[l] = 0; ws.sel[l] = -1; }

    // ---- 1, 2: costs and candidate lists ----
    JointSink sink = {ws, gate_match};
    const int idmax = assoc_cost_phase(w, as, load_x, load_P, ids, M, fwd, ang, k, nz, cost, sink);
    const long long base = M == 0 ? 0ll : 1ll + (long long)idmax;
    const int room = L_max - M;
    constexpr int32_t kCandNew = -1, kCandJoint = -2;   // classes that are not verdicts yet
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        int32_t c = kAssocNone;
        if (l < k) {
            const double b = as.best[l];
            if (ws.cn[l] > 0) c = kCandJoint;
            else if (M > 0 && !(b < inf)) c = kAssocInvalid;
            else if (M == 0 || b > gate_new) c = kCandNew;
            else c = kAssocAmbiguous;
        }
        as.cls[l] = c;
    }
    w.sync();
    int nd = 0;
    {
        auto has = [&](int i) { return as.cls[i] == kCandJoint; };
        for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
            const int pos = w.below(l, has);
            nd = w.total(has);
            if (has(l)) ws.dl[pos] = l;
        }
    }
    w.sync();
    nd = w.uni(nd);
    // the table of candidate landmarks, in (message order, candidate order)
    int nt = 0;
    int32_t flags = 0;
    for (int i = 0; i < nd; ++i) {
        const int l = w.uni(ws.dl[i]);
        const int n = w.uni(ws.cn[l]);
        for (int c = 0; c < n; ++c) {
            const int j = ws.cj[c][l];
            int t = w.first(nt, [&](int e) { return ws.tab[e] == j; });
            if (t < 0) {
                if (nt < kJointMaxLm) {
                    t = nt;
                    if (w.lane() == 0) ws.tab[nt] = j;
                    nt += 1;
                } else {
                    flags |= kJointLmTable;
                }
            }
            if (w.lane() == 0) ws.ct[c][l] = t;
            w.sync();
        }
    }
    const EkfMotion m = ekf_motion(load_x(0), load_x(1), load_x(2), fwd, ang, nz.v_d, nz.v_th, nz.V00);
    for (int e = w.lane(); e < nt; e += w.width()) {
        const AssocLandmark lm = assoc_landmark(load_x, load_P, m, nz, ws.tab[e]);
        ws.tH[0][e] = lm.h.h00; ws.tH[1][e] = lm.h.h01; ws.tH[2][e] = lm.h.h03; ws.tH[3][e] = lm.h.h04;
        ws.tH[4][e] = lm.h.h10; ws.tH[5][e] = lm.h.h11; ws.tH[6][e] = lm.h.h13; ws.tH[7][e] = lm.h.h14;
        ws.tS[0][e] = lm.Sm.s[0]; ws.tS[1][e] = lm.Sm.s[2]; ws.tS[2][e] = lm.Sm.s[3];
    }
    if (w.lane() == 0) ws.d2s[0] = 0.0;
    w.sync();

    // ---- 3 - 5: the search.  Its control state is the same in every lane: it comes from LDS and from sums every lane forms ----
    int level = 0, pairs = 0, nodes = 0, blocks = 0, best_pairs = -1;
    double best_d2 = 0.0;
    unsigned long long used = 0ull;
    bool entering = true;
    auto take_best = [&](int upto) {                  // the branch at hand, unpaired from level `upto` on, is the best so far
        best_pairs = pairs; best_d2 = ws.d2s[pairs];
        w.sync();
        for (int i = w.lane(); i < nd; i += w.width()) ws.best[i] = i < upto ? ws.asg[i] : -1;
        w.sync();
    };
    for (;;) {
        bool back = false;
        if (entering) {
            const int remaining = nd - level, left = kJointMaxPair - pairs;
            const int bound = pairs + (remaining < left ? remaining : left);
            const double d2cur = ws.d2s[pairs];
            const bool cut = bound < best_pairs || (bound == best_pairs && d2cur >= best_d2);
            if (!cut && level == nd) take_best(nd);
            if (cut || level == nd) back = true;
            else {
                if (w.lane() == 0) ws.ci[level] = 0;
                w.sync();
                entering = false;
            }
        }
        if (!back) {
            const int l = w.uni(ws.dl[level]);
            const int n = w.uni(ws.cn[l]);
            const int c = w.uni(ws.ci[level]);
            if (c > n) back = true;
            else {
                w.sync();
                if (w.lane() == 0) ws.ci[level] = c + 1;
                w.sync();
                if (c == n) {                         // the unpaired branch
                    if (w.lane() == 0) ws.asg[level] = -1;
                    w.sync();
                    level += 1; entering = true;
                    continue;
                }
                if (pairs == kJointMaxPair) continue;
                const int t = w.uni(ws.ct[c][l]);
                if (t < 0 || ((used >> t) & 1ull)) continue;
                if (nodes == max_nodes) {             // the budget: the branch at hand competes, then the search ends
                    flags |= kJointBudget;
                    const bool better = pairs > best_pairs || (pairs == best_pairs && ws.d2s[pairs] < best_d2);
                    if (better) take_best(level);
                    break;
                }
                nodes += 1;
                blocks += pairs;
                const bool ok = joint_extend(w, ws, load_P, m, nz, pairs, t, ws.cnu0[c][l], ws.cnu1[c][l]);
                if (!ok) { flags |= kJointSingular; continue; }
                if (!(ws.d2s[pairs + 1] <= gate_joint[pairs])) continue;
                if (w.lane() == 0) { ws.asg[level] = c; ws.ptab[pairs] = t; }
                w.sync();
                used |= 1ull << t;
                pairs += 1; level += 1; entering = true;
                continue;
            }
        }
        // back one level
        level -= 1;
        if (level < 0) break;
        if (w.uni(ws.asg[level]) >= 0) {
            pairs -= 1;
            used &= ~(1ull << w.uni(ws.ptab[pairs]));
        }
        entering = false;
    }
    for (int i = w.lane(); i < nd; i += w.width()) ws.sel[ws.dl[i]] = ws.best[i];
    w.sync();

    // ---- 6: verdicts, lanes over detections ----
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        int32_t c = as.cls[l];
        const double b = as.best[l];
        int j = as.slot[l];
        double d2 = b < inf ? b : nan, n0 = as.nu0[l], n1 = as.nu1[l];
        int32_t id = 0;
        if (c == kCandJoint) {
            const int s = ws.sel[l];
            c = s >= 0 ? kAssocMatched : kAssocJointUnpaired;
            if (s >= 0) {
                j = ws.cj[s][l]; d2 = ws.cd2[s][l]; n0 = ws.cnu0[s][l]; n1 = ws.cnu1[s][l];
                id = ids[j];
            }
        }
        const int rank = w.below(l, [&](int i) { return as.cls[i] == kCandNew; });
        if (c == kCandNew) {
            const bool fits = rank < room && base + rank < (long long)kAssocIdLimit;
            c = fits ? kAssocNew : kAssocNoRoom;
            id = fits ? (int32_t)(base + rank) : 0;
        }
        as.verdict[l] = c; as.id[l] = id;
        if (verdict) verdict[l] = c;
        if (slot) slot[l] = j;
        if (ncand) ncand[l] = l < k ? ws.cn[l] : 0;
        if (det) {
            double* const dl = det + (size_t)l * kAssocDetLen;
            dl[0] = d2; dl[1] = as.second[l] < inf ? as.second[l] : nan; dl[2] = n0; dl[3] = n1;
        }
    }
    w.sync();
    out.count_out = assoc_emit_message(w, as, k, meas_out);

    // ---- counts, ascending l (every lane walks all of them: LDS broadcasts) ----
    out.n_in = k;
    for (int l = 0; l < k; ++l) {
        const int32_t c = as.verdict[l];
        if (c == kAssocMatched) {
            out.n_match += 1;
            out.n_diff += ws.cj[ws.sel[l]][l] != as.slot[l];
        }
        out.n_new += c == kAssocNew; out.n_amb += c == kAssocAmbiguous; out.n_unp += c == kAssocJointUnpaired;
        out.n_room += c == kAssocNoRoom; out.n_inv += c == kAssocInvalid;
    }
    out.n_drop = out.n_amb + out.n_unp + out.n_room + out.n_inv;
    out.flags = flags; out.nodes = nodes; out.blocks = blocks;
    out.d2_joint = best_d2;
    return out;
}

// what one instance adds to a record
SLAM_HD void joint_record(const JointResult& v, double r[kInnovRecLen]) {
    for (int i = 0; i < kInnovRecLen; ++i) r[i] = 0.0;
    if (v.flags & kInnovFrozen) { r[kJntFrozen] = 1.0; return; }
    if (v.flags & kInnovTooLong) { r[kJntTooLong] = 1.0; return; }
    r[kJntEval] = 1.0;
    r[kJntDetIn] = (double)v.n_in; r[kJntMatched] = (double)v.n_match; r[kJntNew] = (double)v.n_new; r[kJntAmbiguous] = (double)v.n_amb;
    r[kJntSumD2] = v.d2_joint; r[kJntMaxD2] = v.d2_joint;
    r[kJntUnpaired] = (double)v.n_unp; r[kJntNoRoom] = (double)v.n_room; r[kJntInvalid] = (double)v.n_inv;
    r[kJntNodes] = (double)v.nodes;
    r[kJntBudget] = (v.flags & kJointBudget) ? 1.0 : 0.0; r[kJntSingular] = (v.flags & kJointSingular) ? 1.0 : 0.0;
    r[kJntDiffer] = (double)v.n_diff;
}

#if defined(__HIPCC__)
// the 64 lanes of one wavefront
struct JointWave : AssocWave {
    __device__ __forceinline__ unsigned long long ballot(bool p) const { return __ballot(p); }
    __device__ __forceinline__ int uni(int v) const { return __builtin_amdgcn_readfirstlane(v); }   // a value every lane holds
    template <class F> __device__ __forceinline__ int first(int n, F f) const {   // (n <= 64; called in wave-uniform control flow)
        const unsigned long long m = __ballot(ln < n && f(ln));
        return m != 0ull ? __ffsll((long long)m) - 1 : -1;
    }
};

// One joint association of every instance on `stream`: three launches, as launch_associate.
struct JointParams {
    EkfStepParams s;
    double gate_match, gate_new;
    double gate_joint[kJointMaxPair];
    int max_nodes;
    float* meas_out;            // [B][k_stride_in][3]
    int32_t* count_out;         // [B]
    int32_t *n_match, *n_new, *n_drop, *flags, *nodes;   // [B] each, any may be NULL
    double* d2_joint;           // [B] or NULL
    int32_t *verdict, *slot, *ncand;   // [B][kInnovMaxDet] or NULL
    double* det;                // [B][kInnovMaxDet][kAssocDetLen] or NULL
    int32_t *n_lm, *n_blk;      // [B]: landmarks compared with (-1: an empty message) and 2 x 2 blocks read on demand, or NULL
    double* inst_rec;           // [B][kInnovRecLen]
    double* partials;           // [record_blocks(B)][kInnovRecLen]
    double* rec;                // [kInnovRecLen]
};
hipError_t launch_associate_joint(const JointParams& p, int f32_storage, hipStream_t stream);
// work [3] += the sums of assoc_traffic over n instance-ticks, with 4 elements of P and one 128-byte line more per on-demand block
hipError_t launch_associate_joint_work(const int32_t* n_lm, const int32_t* n_match, const int32_t* n_new, const int32_t* n_drop, const int32_t* n_blk,
                                       size_t n, int esz, unsigned long long* work, hipStream_t stream);
#endif

// One instance on the host (slam_associate_joint_instance_host); arguments as associate_instance_host
template <class LX, class LP>
JointResult joint_instance_host(JointWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status, float fwd, float ang,
                                const float* meas, int count, int k_stride, const InnovNoise& nz, double gate_match, double gate_new,
                                const double* gate_joint, int max_nodes, double* cost, int32_t* verdict, int32_t* slot, double* det, int32_t* ncand,
                                float* meas_out, int32_t* count_out) {
    int k = count < k_stride ? count : k_stride;
    k = k < 0 ? 0 : k;
    for (int i = 0; i < 3 * (k < kInnovMaxDet ? k : kInnovMaxDet); ++i) ws.a.meas[i] = meas[i];
    const JointResult v = joint_instance(JointSeq(), ws, load_x, load_P, ids, M, L_max, status, fwd, ang, k, nz, gate_match, gate_new, gate_joint,
                                         max_nodes, cost, verdict, slot, det, ncand, meas_out);
    if (count_out) *count_out = v.count_out;
    return v;
}

}  // namespace slam
