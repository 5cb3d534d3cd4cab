// assoc_kernel.h — maximum-likelihood association of detections that come WITHOUT landmark ids (slam_associate, slam_step_associated,
// slam_associate_run; gfx950): nearest neighbour in Mahalanobis distance with a match gate and a new-landmark gate, with the EKF step
// kernels untouched.  A side kernel labels the message with ids; the unmodified known-id step (landmark_id_is_known = 1) consumes the
// labelled message on its fast path, and slam_innovation or slam_gate can be put in between.
//
// associate_instance() below is THE definition: the device kernel (assoc_kernel.hip) and the host test hook
// (slam_associate_instance_host) compile this one function, with -ffp-contract=off on both sides, so the two give the same bits.  Its
// arithmetic is the functions of ekf_model.h and slam_math.h, the ones the step kernels and the innovation replay call.
//
// Cost.  For detection l (r, b as floats; the id column of the incoming message is NOT READ) and mapped slot j < M, d2[l][j] is the nis that
// innovation_instance() (innovation_kernel.h) reports in slot 0 for the one-detection message [(ids[j], r_l, b_l)] at the same pre-step
// state, command and noise row, bit for bit: the predicted state after ekf_motion / ekf_predicted and before any update, on the block
// {0, 1, 2, ii, ii + 1} with ii = 3 + 2 j; nu with the float truncations of ekf.cpp:115,129-131; S in the oracle's association order;
// Si = inv2x2_lu(S); d2 = nu_r (Si00 nu_r + Si01 nu_b) + nu_b (Si10 nu_r + Si11 nu_b), unfused.  The 5 x 5 block, H, S and Si depend on the
// landmark alone and are formed once per landmark, and so is the predicted bearing of nu (ekf_predicted_bearing, the first half of
// ekf_innovation); the float differences of nu (ekf_innovation_from, its second half) and the quadratic form are formed per pair.  A
// cost is NaN where Si failed or where nu or S is not finite.  The quirk switch ekf_landmark_from_x_pred cannot matter: it chooses
// between x_t and x_pred for the landmark's position, and those differ only after an update of this message; no update precedes a cost.
//
// Decisions, per instance with count_in = min(max(count, 0), k_stride):
//   1  per detection the best finite cost (ties: lowest j) and the second-best finite cost (NaN if none)
//   2  INVALID: M > 0 and no finite cost;  NEW candidate: M == 0 or best > gate_new;  MATCH candidate: best <= gate_match;  AMBIGUOUS: the rest
//   3  a landmark is seen at most once per message: among the MATCH candidates of one slot the smallest (d2, l) wins, the others are
//      CONFLICT.  They are dropped, not reassigned.
//   4  NEW candidates in message order get rank 0, 1, ... and the id base + rank, base = 0 for M == 0, else 1 + max(ids[0 .. M)).  A
//      candidate is NO_ROOM when M + rank >= L_max or when its id is not below 2^24 (the message carries ids as floats and the step reads
//      (int)meas[3 l])
//   5  output message: the MATCHED and NEW detections in message order as ((float)id, r, b), r and b copied bit for bit; count_out = their
//      number; the triplets count_out .. count_in - 1 written as 0.0f; nothing written from count_in up.  The whole message is held
//      before the first write, so the output row may be the input row.
//   6  instances that cannot be associated emit an EMPTY message (count_out = 0, every verdict 0, the first count_in triplets zeroed), so
//      that an unlabelled id never reaches the step: status SLAM_INST_INDEX_OOR (flag FROZEN), more than kInnovMaxDet detections (flag
//      TOO_LONG).  There is no limit on distinct landmarks: no block larger than 5 x 5 is formed.
// Per detection slot: verdict, slot (best j or -1), det[4] = (d2_best, d2_second, nu_r, nu_b of the best), NaN where undefined.
// Record (kInnovRecLen doubles): 0 evaluated, 1 FROZEN, 2 TOO_LONG, 3 detections in, 4 matched, 5 new, 6 ambiguous, 7 sum of d2_best over
// the matched (ascending l), 8 max of d2_best over the matched (0 over none), 9 conflict, 10 no room, 11 invalid, 12 - 15 reserved, 0.
// Entry 8 is a maximum and every other a sum (kAssocRecMax).
#pragma once
#include "innovation_kernel.h"

namespace slam {

constexpr int kAssocDetLen = 4;                      // doubles per detection slot
constexpr int32_t kAssocNone = 0, kAssocMatched = 1, kAssocNew = 2, kAssocAmbiguous = 3, kAssocConflict = 4, kAssocNoRoom = 5,
                  kAssocInvalid = 6;                 // slam_assoc_verdict
constexpr int32_t kAssocIdLimit = 1 << 24;           // ids the float column of a message carries exactly

enum AssocRec {
    kAscEval = 0, kAscFrozen = 1, kAscTooLong = 2, kAscDetIn = 3, kAscMatched = 4, kAscNew = 5, kAscAmbiguous = 6, kAscSumD2 = 7,
    kAscMaxD2 = 8, kAscConflict = 9, kAscNoRoom = 10, kAscInvalid = 11
};
constexpr unsigned kAssocRecMax = 1u << kAscMaxD2;   // the entries joined by a maximum (record_kernel.h)

// what one instance holds between its phases: LDS on the device (one per wavefront), plain memory on the host.  The per-detection
// arrays are separate (not a struct per detection): lane l reads element l, consecutive banks.
struct AssocWork {
    double best[kInnovMaxDet], second[kInnovMaxDet];   // running best / second-best finite cost, +inf while there is none
    double nu0[kInnovMaxDet], nu1[kInnovMaxDet];       // nu of the best
    float meas[3 * kInnovMaxDet];                       // the message
    int32_t slot[kInnovMaxDet];                         // best j, -1 while there is none
    int32_t cls[kInnovMaxDet];                          // the candidate class
    int32_t verdict[kInnovMaxDet];                      // the verdict
    int32_t id[kInnovMaxDet];                           // the id a MATCHED or NEW detection is labelled with
};

struct AssocResult {
    int32_t n_match, n_new, n_drop, flags;             // flags: kInnovFrozen, kInnovTooLong
    int32_t n_in, n_amb, n_conf, n_room, n_inv, count_out;
    double sum_d2, max_d2;                              // over the matched, ascending l
};

// The host's execution policy; the device's is AssocWave (below).  Lanes run over landmarks in the cost phase and over detections
// afterwards; the arithmetic of an element does not depend on the lane.
struct AssocSeq {
    int lane() const { return 0; }
    int width() const { return 1; }
    void sync() const {}
    double xor_get(double v, int) const { return v; }   // (never called: the butterflies have log2(width) = 0 steps)
    int xor_get(int v, int) const { return v; }
    // number of i < l (below) or i < kInnovMaxDet (total) with f(i); called with l = every detection slot of this lane in turn
    template <class F> int below(int l, F f) const { int n = 0; for (int i = 0; i < l; ++i) n += f(i) ? 1 : 0; return n; }
    template <class F> int total(F f) const { return below(kInnovMaxDet, f); }
};

// the second smallest of the union of two pairs (a0 <= a1), (b0 <= b1)
SLAM_HD double assoc_second(double a0, double a1, double b0, double b1) {
    const double hi = a0 < b0 ? b0 : a0;        // the larger of the two minima
    const double lo = a1 < b1 ? a1 : b1;        // the smaller of the two seconds
    return hi < lo ? hi : lo;
}

// What the cost phase forms once per landmark slot jj, from the pre-step state: the offset and range, H, S of the predicted 5 x 5 block
// {0, 1, 2, ii, ii + 1} (ii = 3 + 2 jj), Si = inv2x2_lu(S) with `ok` (the inverse succeeded and S is finite) and the predicted bearing.
// The joint association (joint_kernel.h) calls it again for its candidate landmarks: the same function on the same operands, the same bits.
struct AssocLandmark { EkfRange rg; EkfH h; EkfS Sm; double Si[4]; bool ok; float angf; };
template <class LX, class LP>
SLAM_HD AssocLandmark assoc_landmark(LX load_x, LP load_P, const EkfMotion& m, const InnovNoise& nz, int jj) {
    AssocLandmark o;
    const int ii = 3 + 2 * jj;
    const int idx[5] = {0, 1, 2, ii, ii + 1};
    o.rg = ekf_range(load_x(ii), load_x(ii + 1), m.xp0, m.xp1);   // ekf.cpp:115 (no update precedes: x_pred[ii] = x_t[ii])
    o.h = ekf_jacobian(o.rg.dx, o.rg.dy, o.rg.dd, o.rg.d2);
    const double q[2][2] = {{m.q00, m.q01}, {m.q10, m.q11}};
    // P_pred on the block (ekf.cpp:61; block rows 3, 4 are rows >= 3 of the state) and H P, a column at a time: a column of the
    // prediction takes its own column of P and column 2
    double a2[5];
#pragma unroll
    for (int r = 0; r < 5; ++r) a2[r] = load_P(idx[r], 2);
    EkfVec2 hp[5];
#pragma unroll
    for (int c = 0; c < 5; ++c) {
        double a[5], pc[5];
#pragma unroll
        for (int r = 0; r < 5; ++r) a[r] = c == 2 ? a2[r] : load_P(idx[r], idx[c]);
#pragma unroll
        for (int r = 0; r < 5; ++r) pc[r] = ekf_predicted(a[r], r, c, a[2], a2[r], a2[2], m.fa, m.fb, (r < 2 && c < 2) ? q[r][c] : 0.0, nz.V11);
        hp[c] = ekf_hp_col(o.h, pc[0], pc[1], pc[2], pc[3], pc[4]);
    }
    o.Sm = ekf_S(o.h, hp[0], hp[1], hp[2], hp[3], hp[4], nz.W00, nz.W11);   // ekf.cpp:133
    o.ok = inv2x2_lu(o.Sm.s, o.Si) && innov_finite(o.Sm.s[0]) && innov_finite(o.Sm.s[1]) && innov_finite(o.Sm.s[2]) && innov_finite(o.Sm.s[3]);
    o.angf = ekf_predicted_bearing(o.rg.dx, o.rg.dy, m.xp2);
    return o;
}

// what the cost phase hands every pair (l, j) to, in wave-uniform control flow: nothing for slam_associate, the candidate lists of the
// joint association (joint_kernel.h)
struct AssocNoSink {
    template <class W> SLAM_HD void pair(const W&, int, int, bool, double, const EkfVec2&) const {}
};

// The cost phase: lanes over landmarks, width() of them at a time; per detection a butterfly arg-min with the (value, j) tie-break into
// ws.best / second / slot / nu0 / nu1 (initialised here).  Returns the largest id of the map (INT_MIN for M == 0) in every lane.
template <class W, class LX, class LP, class SINK>
SLAM_HD int assoc_cost_phase(const W& w, AssocWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, float fwd, float ang, int k,
                             const InnovNoise& nz, double* cost, SINK& sink) {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        ws.best[l] = inf; ws.second[l] = inf; ws.nu0[l] = nan; ws.nu1[l] = nan; ws.slot[l] = -1;
    }
    w.sync();
    const double x0 = load_x(0), x1 = load_x(1), x2 = load_x(2);
    const EkfMotion m = ekf_motion(x0, x1, x2, fwd, ang, nz.v_d, nz.v_th, nz.V00);   // ekf.cpp:41-59
    int idmax = -2147483647 - 1;
    for (int j0 = 0; j0 < M; j0 += w.width()) {
        const int j = j0 + w.lane();
        const bool mine = j < M;
        const int jj = mine ? j : 0;              // (a lane past the map computes on landmark 0 and discards: no index leaves the state)
        if (mine && ids[j] > idmax) idmax = ids[j];
        const AssocLandmark lm = assoc_landmark(load_x, load_P, m, nz, jj);
        const double (&Si)[4] = lm.Si;
        const bool ok = lm.ok;
        for (int l = 0; l < k; ++l) {
            const EkfVec2 nu = ekf_innovation_from(ws.meas[3 * l + 1], ws.meas[3 * l + 2], lm.rg.dist, lm.angf, nz.w_r, nz.w_b);   // ekf.cpp:129-131
            double d2 = nu.x * (Si[0] * nu.x + Si[1] * nu.y) + nu.y * (Si[2] * nu.x + Si[3] * nu.y);
            if (!ok || !innov_finite(nu.x) || !innov_finite(nu.y)) d2 = nan;
            if (cost && mine) cost[(size_t)l * M + j] = d2;
            const bool fin = mine && innov_finite(d2);
            const double own = fin ? d2 : inf;
            double b0 = own, b1 = inf;            // this group's best and second
            int bj = fin ? j : 2147483647;
            for (int s = 1; s < w.width(); s <<= 1) {
                const double o0 = w.xor_get(b0, s), o1 = w.xor_get(b1, s);
                const int oj = w.xor_get(bj, s);
                b1 = assoc_second(b0, b1, o0, o1);
                if (o0 < b0 || (o0 == b0 && oj < bj)) { b0 = o0; bj = oj; }
            }
            // into the running values: an earlier group holds lower j, so it keeps a tie
            const double r0 = ws.best[l], r1 = ws.second[l];
            const bool better = b0 < r0;
            if (w.lane() == 0) {
                ws.second[l] = assoc_second(r0, r1, b0, b1);
                if (better) { ws.best[l] = b0; ws.slot[l] = bj; }
            }
            if (better && fin && j == bj) { ws.nu0[l] = nu.x; ws.nu1[l] = nu.y; }
            sink.pair(w, l, j, fin, d2, nu);
        }
        w.sync();
    }
    for (int s = 1; s < w.width(); s <<= 1) {
        const int o = w.xor_get(idmax, s);
        idmax = o > idmax ? o : idmax;
    }
    return idmax;
}

// An instance that cannot be associated (step 6): every verdict 0, every slot -1, det NaN, the first k triplets of the row zeroed
template <class W>
SLAM_HD void assoc_empty_message(const W& w, int k, int32_t* verdict, int32_t* slot, double* det, float* meas_out) {
    const double nan = __builtin_nan("");
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        if (verdict) verdict[l] = kAssocNone;
        if (slot) slot[l] = -1;
        if (det)
            for (int i = 0; i < kAssocDetLen; ++i) det[l * kAssocDetLen + i] = nan;
    }
    if (meas_out)
        for (int i = w.lane(); i < 3 * k; i += w.width()) meas_out[i] = 0.0f;
}

// The labelled message (step 5) from ws.verdict / ws.id / ws.meas, in message order; returns count_out
template <class W>
SLAM_HD int assoc_emit_message(const W& w, const AssocWork& ws, int k, float* meas_out) {
    int count_out = 0;
    auto kept_at = [&](int i) { return ws.verdict[i] == kAssocMatched || ws.verdict[i] == kAssocNew; };
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        const int pos = w.below(l, kept_at);
        const int kept = w.total(kept_at);
        count_out = kept;
        if (!meas_out || l >= k) continue;        // every output index below is < 3 k <= 3 k_stride
        if (kept_at(l)) {
            meas_out[3 * pos] = (float)ws.id[l]; meas_out[3 * pos + 1] = ws.meas[3 * l + 1]; meas_out[3 * pos + 2] = ws.meas[3 * l + 2];
        } else {                                  // the dropped detections zero the tail kept .. k - 1, one triplet each
            const int t = kept + (l - pos);       // l - pos = dropped detections below l
            meas_out[3 * t] = 0.0f; meas_out[3 * t + 1] = 0.0f; meas_out[3 * t + 2] = 0.0f;
        }
    }
    return count_out;
}

// One instance.  ws.meas holds the message's first min(k, kInnovMaxDet) triplets already; k = count_in.  ids: lm_IDs[0 .. M); M is clamped
// to [0, L_max].  load_x(i) / load_P(r, c) as innovation_instance.  cost: [k][M] or NULL (the host hook's full matrix).  verdict, slot:
// [kInnovMaxDet], det: [kInnovMaxDet][kAssocDetLen], or NULL.  meas_out: the output row ([k_stride][3], may be the input row) or NULL.
// Every lane of the policy returns the same result; the lanes share the writes.
template <class W, class LX, class LP>
SLAM_HD AssocResult associate_instance(const W& w, AssocWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status,
                                       float fwd, float ang, int k, const InnovNoise& nz, double gate_match, double gate_new, double* cost,
                                       int32_t* verdict, int32_t* slot, double* det, float* meas_out) {
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    AssocResult out;
    out.n_match = out.n_new = out.n_drop = out.flags = 0;
    out.n_in = out.n_amb = out.n_conf = out.n_room = out.n_inv = out.count_out = 0;
    out.sum_d2 = out.max_d2 = 0.0;
    if (status & kInnovStatusFrozen) out.flags = kInnovFrozen;
    else if (k > kInnovMaxDet) out.flags = kInnovTooLong;
    if (out.flags) {   // an empty message
        assoc_empty_message(w, k, verdict, slot, det, meas_out);
        return out;
    }
    M = M < 0 ? 0 : (M > L_max ? L_max : M);
    // ---- costs (assoc_cost_phase) ----
    AssocNoSink sink;
    const int idmax = assoc_cost_phase(w, ws, load_x, load_P, ids, M, fwd, ang, k, nz, cost, sink);
    const long long base = M == 0 ? 0ll : 1ll + (long long)idmax;
    const int room = L_max - M;

    // ---- decisions: lanes over detections (on the device one lane each: below() and total() are a ballot and a popcount) ----
    constexpr int32_t kCandNew = -1, kCandMatch = -2;   // classes that are not verdicts yet
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        int32_t c = kAssocNone;
        if (l < k) {
            const double b = ws.best[l];
            if (M > 0 && !(b < inf)) c = kAssocInvalid;
            else if (M == 0 || b > gate_new) c = kCandNew;
            else if (b <= gate_match) c = kCandMatch;
            else c = kAssocAmbiguous;
        }
        ws.cls[l] = c;
    }
    w.sync();
    for (int l = w.lane(); l < kInnovMaxDet; l += w.width()) {
        int32_t c = ws.cls[l];
        const double b = ws.best[l];
        const int j = ws.slot[l];
        int32_t id = 0;
        if (c == kCandMatch) {                    // the smallest (d2, l) of a slot wins
            bool lost = false;
            for (int i = 0; i < k; ++i)
                if (i != l && ws.cls[i] == kCandMatch && ws.slot[i] == j && (ws.best[i] < b || (ws.best[i] == b && i < l))) lost = true;
            c = lost ? kAssocConflict : kAssocMatched;
            id = ids[j];
        }
        const int rank = w.below(l, [&](int i) { return ws.cls[i] == kCandNew; });
        if (c == kCandNew) {
            const bool fits = rank < room && base + rank < (long long)kAssocIdLimit;
            c = fits ? kAssocNew : kAssocNoRoom;
            id = fits ? (int32_t)(base + rank) : 0;
        }
        ws.verdict[l] = c; ws.id[l] = id;
        if (verdict) verdict[l] = c;
        if (slot) slot[l] = j;
        if (det) {
            double* const dl = det + (size_t)l * kAssocDetLen;
            dl[0] = b < inf ? b : nan; dl[1] = ws.second[l] < inf ? ws.second[l] : nan; dl[2] = ws.nu0[l]; dl[3] = ws.nu1[l];
        }
    }
    w.sync();

    // ---- the labelled message, in message order ----
    out.count_out = assoc_emit_message(w, ws, k, meas_out);

    // ---- counts and sums, ascending l (every lane walks all of them: LDS broadcasts) ----
    out.n_in = k;
    for (int l = 0; l < k; ++l) {
        const int32_t c = ws.verdict[l];
        if (c == kAssocMatched) {
            out.n_match += 1;
            out.sum_d2 = out.sum_d2 + ws.best[l];
            if (ws.best[l] > out.max_d2) out.max_d2 = ws.best[l];
        }
        out.n_new += c == kAssocNew; out.n_amb += c == kAssocAmbiguous; out.n_conf += c == kAssocConflict;
        out.n_room += c == kAssocNoRoom; out.n_inv += c == kAssocInvalid;
    }
    out.n_drop = out.n_amb + out.n_conf + out.n_room + out.n_inv;
    return out;
}

// what one instance adds to a record
SLAM_HD void assoc_record(const AssocResult& v, double r[kInnovRecLen]) {
    for (int i = 0; i < kInnovRecLen; ++i) r[i] = 0.0;
    if (v.flags & kInnovFrozen) { r[kAscFrozen] = 1.0; return; }
    if (v.flags & kInnovTooLong) { r[kAscTooLong] = 1.0; return; }
    r[kAscEval] = 1.0;
    r[kAscDetIn] = (double)v.n_in; r[kAscMatched] = (double)v.n_match; r[kAscNew] = (double)v.n_new; r[kAscAmbiguous] = (double)v.n_amb;
    r[kAscSumD2] = v.sum_d2; r[kAscMaxD2] = v.max_d2;
    r[kAscConflict] = (double)v.n_conf; r[kAscNoRoom] = (double)v.n_room; r[kAscInvalid] = (double)v.n_inv;
}

// The traffic model of one instance (slam_last_associate_work): elements of P (rows 0 - 2 whole, and per landmark P[ii .. ii + 1][0 .. 2]
// with the 2 x 2 diagonal block), bytes of everything else (x, ids, the message in and out, the count in and out), and the 128-byte
// lines the reads of P touch: the strided column reads take one line per row for columns 0 - 2 and one for the diagonal block.
struct AssocTraffic { unsigned long long p_elems, other_bytes, p_lines; };
SLAM_HD AssocTraffic assoc_traffic(int M, int k, int esz) {
    const unsigned long long n = 3ull + 2ull * (unsigned long long)M, kk = (unsigned long long)k;
    return AssocTraffic{3ull * n + 10ull * (unsigned long long)M, n * (unsigned long long)esz + 4ull * (unsigned long long)M + 24ull * kk + 8ull,
                        3ull * ((n * (unsigned long long)esz + 127ull) / 128ull) + 4ull * (unsigned long long)M};
}

#if defined(__HIPCC__)
// the 64 lanes of one wavefront
struct AssocWave {
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int width() const { return 64; }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ double xor_get(double v, int s) const { return __shfl_xor(v, s, 64); }
    __device__ __forceinline__ int xor_get(int v, int s) const { return __shfl_xor(v, s, 64); }
    // (called by all 64 lanes with l = their lane: one lane per detection)
    template <class F> __device__ __forceinline__ int below(int l, F f) const { return __popcll(__ballot(f(ln)) & ((1ull << l) - 1ull)); }
    template <class F> __device__ __forceinline__ int total(F f) const { return __popcll(__ballot(f(ln))); }
};
static_assert(kInnovMaxDet == 64, "one lane per detection of a message");

// One association of every instance on `stream`: three launches (the instances with their labelled messages, then the record as
// launch_innovation reduces it).  s is what the step that follows is launched with, message source meas_in / meas_count_in /
// k_stride_in (never the simulator).  meas_out / count_out may be the input pair itself and must not overlap it otherwise.
struct AssocParams {
    EkfStepParams s;
    double gate_match, gate_new;
    float* meas_out;            // [B][k_stride_in][3]
    int32_t* count_out;         // [B]
    int32_t *n_match, *n_new, *n_drop, *flags;   // [B] each, any may be NULL
    int32_t *verdict, *slot;    // [B][kInnovMaxDet] or NULL
    double* det;                // [B][kInnovMaxDet][kAssocDetLen] or NULL
    int32_t* n_lm;              // [B] landmarks the instance compared with (-1: it emitted an empty message), or NULL
    double* inst_rec;           // [B][kInnovRecLen]
    double* partials;           // [record_blocks(B)][kInnovRecLen]
    double* rec;                // [kInnovRecLen]
};
hipError_t launch_associate(const AssocParams& p, int f32_storage, hipStream_t stream);
// work [3] += the sums of assoc_traffic over n instance-ticks (n_lm as launch_associate wrote it, k = n_match + n_new + n_drop)
hipError_t launch_associate_work(const int32_t* n_lm, const int32_t* n_match, const int32_t* n_new, const int32_t* n_drop, size_t n, int esz,
                                 unsigned long long* work, hipStream_t stream);
#endif

// One instance on the host (slam_associate_instance_host).  meas: the message, count its detection count as given, k_stride the row's
// capacity (meas holds clamp(count, 0, k_stride) triplets); meas_out [k_stride][3] may be meas itself.
template <class LX, class LP>
AssocResult associate_instance_host(AssocWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status, float fwd, float ang,
                                    const float* meas, int count, int k_stride, const InnovNoise& nz, double gate_match, double gate_new,
                                    double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out) {
    int k = count < k_stride ? count : k_stride;
    k = k < 0 ? 0 : k;
    for (int i = 0; i < 3 * (k < kInnovMaxDet ? k : kInnovMaxDet); ++i) ws.meas[i] = meas[i];
    const AssocResult v = associate_instance(AssocSeq(), ws, load_x, load_P, ids, M, L_max, status, fwd, ang, k, nz, gate_match, gate_new, cost,
                                             verdict, slot, det, meas_out);
    if (count_out) *count_out = v.count_out;
    return v;
}

}  // namespace slam
