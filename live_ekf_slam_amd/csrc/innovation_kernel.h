// innovation_kernel.h — innovation (NIS) statistics of every detection of the message the next EKF step will process, computed from the
// PRE-step state without touching the step kernel (slam_innovation, slam_innovation_run; gfx950).
//
// innovation_instance() below is THE definition: the device kernel (innovation_kernel.hip) and the host test hook
// (slam_innovation_instance_host) compile this one function, with -ffp-contract=off on both sides, so the two give the same bits.  Its
// arithmetic is the functions of ekf_model.h, the ones the step kernels call; what is written here is the plan, the walk and the statistics.
//
// Why a side kernel can do it.  Let J = {0, 1, 2} U {ii, ii + 1 : landmark slot of a detection of this message that is already mapped}.
// In EKF::update (ekf.cpp:37-179, oracle/slam_oracle.cpp update_t / predict_fast / landmark_update_apply_fast) the prediction of rows and
// columns 0 - 1 of P, the products H P and P H^T, S, K, x_pred += K nu and the downdate P[r][c] -= k0 HP[c] + k1 HP[n + c], all RESTRICTED
// to r, c in J, read nothing outside x[J] and the J x J block of P; an insertion changes neither the pose nor an existing entry of P.  So
// the whole message is replayed on a (3 + 2 d) x (3 + 2 d) block, d = distinct mapped landmarks of the message, with the same scalar
// operations on the same operands as the full update: every nu and S is what the step computes, bit for bit, and so are the pose and the
// leading 3 x 3 block of P after the message.
//
// The walk (landmark_id_is_known = 1), per detection l in message order, id = (int)meas[3 l]:
//   found (first j < M with ids[j] == id)  -> UPDATE of landmark j: dist, d2, angf, nu0, nu1 with the float truncations of ekf.cpp:115,129-131,
//                                             H0 / H1, H P, P H^T, S in the oracle's association order, Si = inv2x2_lu(S) (PartialPivLU,
//                                             slam_math.h), K, x_pred += K nu, x_pred(2) = remainder(., 2 pi), the rank-2 downdate on the block
//   not found, first occurrence of the id  -> INSERTION while the map has room (M + insertions so far < L_max), else a capacity skip
//   not found, the id occurred before      -> its first occurrence was inserted by this message: the step raises SLAM_INST_INDEX_OOR and rolls
//                                             back (WOULD_FREEZE); it was skipped: skipped again
// Per update slot the six values (nis, nu_r, nu_b, S00, S01, S11), and
//   nis = nu_r * (Si00 * nu_r + Si01 * nu_b) + nu_b * (Si10 * nu_r + Si11 * nu_b)          (this order, no fused multiply-add)
// with Si what inv2x2_lu returned.  S01 = 0.5 * (S(0,1) + S(1,0)) of the S the step inverts: the downdate P -= K (H P) keeps P symmetric
// only to rounding, which accumulates over a run (S(0,1) - S(1,0) reaches some 1e-13 after 300 steps), and the step's Si is the inverse of
// that S, not of a symmetrised one.  nu^T S^-1 nu depends on S through its symmetric part up to (S(0,1) - S(1,0))^2 / (4 det S), so the
// reported triple reproduces nis to rounding; either off-diagonal entry alone does not.  nis is NaN where inv2x2_lu failed (S_SINGULAR; the replay goes on with the same Si the step uses) and
// where nu or S is not finite (no flag).  Slots that are insertions, capacity skips or beyond the count hold NaN.
// Per instance: nis_sum = the finite nis in ascending l (0 over none), n_upd = update slots, n_new = insertion slots including every
// capacity skip, post[12] = x_pred[0 .. 2] and the leading 3 x 3 block of P_pred (row-major) after the whole message, before the storage
// rounding, flags = slam_innovation_flags.  INSTANCE_FROZEN, WOULD_FREEZE and TOO_LONG leave every value NaN and the counts 0.
// A message that would freeze is WOULD_FREEZE whatever its number of landmarks; TOO_LONG is a message of more than kInnovMaxDet
// detections, or one that does not freeze and updates more than kInnovMaxLm distinct landmarks.
#pragma once
#include <stdint.h>

#include "ekf_model.h"
#if defined(__HIPCC__)
#include "ekf_kernel.h"
#include "record_kernel.h"
#endif

namespace slam {

constexpr int kInnovMaxDet = 64;                    // SLAM_INNOV_MAX_DET: detections of one message
constexpr int kInnovMaxLm = 16;                     // SLAM_INNOV_MAX_LM: distinct mapped landmarks of one message
constexpr int kInnovNb = 3 + 2 * kInnovMaxLm;       // rows of the largest block; also its row stride (odd: lanes that walk a column of
                                                    // doubles hit 32 different bank pairs)
constexpr int kInnovDetLen = 6;                     // doubles per detection slot
constexpr int kInnovRecLen = 16;                    // doubles of one record

constexpr int32_t kInnovFrozen = 1, kInnovWouldFreeze = 2, kInnovSingular = 4, kInnovTooLong = 8;   // slam_innovation_flags
constexpr int32_t kInnovStatusFrozen = 4;           // SLAM_INST_INDEX_OOR: the step kernel returns at once

// indices of a record (counts are stored as doubles)
enum InnovRec {
    kInnEval = 0, kInnFrozen = 1, kInnTooLong = 2, kInnWouldFreeze = 3, kInnSingular = 4, kInnUpd = 5, kInnNew = 6, kInnSumNis = 7,
    kInnMaxNis = 8, kInnBelow = 9, kInnAbove = 10, kInnSumNuR = 11, kInnSumNuB = 12, kInnSumNuR2 = 13, kInnSumNuB2 = 14, kInnReserved = 15
};
constexpr unsigned kInnovRecMax = 1u << kInnMaxNis;    // the entries joined by a maximum (record_kernel.h); every other is a sum

struct InnovNoise { float v_d, v_th, w_r, w_b; double V00, V11, W00, W11; };   // the instance's filter noise (effective V / W)

// everything the replay of one instance holds between its phases: LDS on the device (one per wavefront), plain memory on the host
struct InnovWork {
    double P[kInnovNb * kInnovNb];   // the J x J block, row stride kInnovNb
    double x[kInnovNb];              // x_t[J]
    double xp[kInnovNb];             // x_pred[J]
    double HP[2 * kInnovNb];         // (H P)[0][c], (H P)[1][c] of the update at hand
    double K[2 * kInnovNb];          // K[r][0 .. 1]
    float meas[3 * kInnovMaxDet];    // the message
    int32_t code[kInnovMaxDet];      // per detection: >= 0 pair of the block (update), -1 insertion, -2 capacity skip
    int32_t lm[kInnovMaxLm];         // pair of the block -> landmark number
};

struct InnovResult {
    double nis_sum;
    int32_t n_upd, n_new, flags;
    double post[12];
    // over the update slots with a finite nis, in ascending l: what the instance adds to a record (innovation_record)
    int32_t n_fin, n_below, n_above;
    double max_nis, s_nur, s_nub, s_nur2, s_nub2;
};

SLAM_HD bool innov_finite(double v) { return fabs(v) < __builtin_inf(); }

// The gating policy of innovation_instance(): InnovNoGate is the plain evaluation (slam_innovation; every `if constexpr` below drops
// out and the function is the code it was before there was a gate), InnovGate the chi-square gate of slam_gate (gate_kernel.h).
struct InnovNoGate { static constexpr bool on = false; };
struct InnovGate {
    static constexpr bool on = true;
    double gate;        // an update slot is REJECTED iff its nis is finite and nis > gate
    int32_t* verdict;   // [kInnovMaxDet], shared by the lanes like det: 0 not an update slot, 1 accepted, 2 rejected
    int32_t n_rej;      // out: rejected slots
};
constexpr int32_t kGateNone = 0, kGateAccepted = 1, kGateRejected = 2;

// The host's execution policy: one "lane" walks every loop.  The device's (innovation_kernel.hip) spreads the loops over the 64 lanes of
// a wavefront, finds by ballot and orders the phases by a wavefront fence; the arithmetic of an element does not depend on the lane.
struct InnovSeq {
    int lane() const { return 0; }
    int width() const { return 1; }
    void sync() const {}
    template <class F> int first(int n, F f) const {   // smallest i < n with f(i), -1 if none
        for (int i = 0; i < n; ++i)
            if (f(i)) return i;
        return -1;
    }
};

// state index of element s of the block
SLAM_HD int innov_full_index(const InnovWork& ws, int s) { return s < 3 ? s : 3 + 2 * ws.lm[(s - 3) >> 1] + ((s - 3) & 1); }

// One instance.  ws.meas holds the message's first min(k, kInnovMaxDet) triplets already; k: its detection count (clamped to the stride by
// the caller, >= 0).  ids: lm_IDs[0 .. M); M is clamped to [0, L_max].  status: slam_instance_flags.  load_x(i) / load_P(r, c): element i of
// x_t / element (r, c) of P_t as doubles (fp32 storage converted on load).  lo, hi: the band of the record's entries 9 and 10.
// det: [kInnovMaxDet][6] or NULL.  Every lane of the policy returns the same result; the lanes share the writes of det.
// g: the gating policy's state (NULL for InnovNoGate, the plain evaluation).  With InnovGate a rejected slot writes its six det values and is otherwise skipped: no K, no x_pred, no downdate, and
// it enters none of the sums and counts of the result except n_upd (the update slots of the plan, rejected or not) and g->n_rej; post is
// the state after the accepted updates.  A slot whose nis is not finite (S_SINGULAR, a non-finite nu or S) is never rejected: it goes
// through as the step has it.  INSTANCE_FROZEN, WOULD_FREEZE and TOO_LONG pass their message through: n_rej = 0, every verdict 0.
template <class W, class LX, class LP, class G = InnovNoGate>
SLAM_HD InnovResult innovation_instance(const W& w, InnovWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status,
                                        float fwd, float ang, int k, const InnovNoise& nz, bool lm_from_pred, double lo, double hi,
                                        double* det, G* g = nullptr) {
    const double nan = __builtin_nan("");
    if constexpr (G::on) {
        g->n_rej = 0;
        for (int e = w.lane(); e < kInnovMaxDet; e += w.width()) g->verdict[e] = kGateNone;
    }
    InnovResult out;
    out.nis_sum = nan; out.n_upd = 0; out.n_new = 0; out.flags = 0;
    out.n_fin = out.n_below = out.n_above = 0;
    out.max_nis = out.s_nur = out.s_nub = out.s_nur2 = out.s_nub2 = 0.0;
    for (int i = 0; i < 12; ++i) out.post[i] = nan;
    if (det)
        for (int e = w.lane(); e < kInnovMaxDet * kInnovDetLen; e += w.width()) det[e] = nan;
    if (status & kInnovStatusFrozen) { out.flags = kInnovFrozen; return out; }
    if (k > kInnovMaxDet) { out.flags = kInnovTooLong; return out; }
    M = M < 0 ? 0 : (M > L_max ? L_max : M);

    // ---- the plan: what becomes of every detection (ekf.cpp:99-108 and the rule for new ids, ekf_step_prestep.h) ----
    const int room = L_max - M;
    int d = 0, nfirst = 0, n_upd = 0, n_new = 0;
    bool freeze = false;
    for (int l = 0; l < k && !freeze; ++l) {
        const int id = (int)ws.meas[3 * l];
        const int j = w.first(M, [&](int i) { return ids[i] == id; });
        int code;
        if (j >= 0) {
            int q = w.first(d < kInnovMaxLm ? d : kInnovMaxLm, [&](int i) { return ws.lm[i] == j; });
            if (q < 0) {
                q = d;
                if (d < kInnovMaxLm && w.lane() == 0) ws.lm[d] = j;
                d += 1;   // (beyond kInnovMaxLm only counted: a later repeat of such a landmark counts again, the message is TOO_LONG either way)
            }
            code = q;
            n_upd += 1;
        } else {
            const int first = w.first(l, [&](int i) { return (int)ws.meas[3 * i] == id; });
            if (first < 0) {
                code = nfirst < room ? -1 : -2;
                nfirst += 1;
            } else if (ws.code[first] == -1) {
                freeze = true;
                code = -2;
            } else {
                code = -2;
            }
            n_new += 1;
        }
        if (w.lane() == 0) ws.code[l] = code;
        w.sync();
    }
    if (freeze) { out.flags = kInnovWouldFreeze; return out; }
    if (d > kInnovMaxLm) { out.flags = kInnovTooLong; return out; }
    const int nb = 3 + 2 * d;
    constexpr int LD = kInnovNb;

    // ---- gather x[J] and the J x J block ----
    for (int s = w.lane(); s < nb; s += w.width()) ws.x[s] = load_x(innov_full_index(ws, s));
    for (int e = w.lane(); e < nb * nb; e += w.width()) {
        const int r = e / nb, c = e - r * nb;
        ws.P[r * LD + c] = load_P(innov_full_index(ws, r), innov_full_index(ws, c));
    }
    w.sync();

    // ---- predict (ekf.cpp:41-61, predict_fast) ----
    {
        const EkfMotion m = ekf_motion(ws.x[0], ws.x[1], ws.x[2], fwd, ang, nz.v_d, nz.v_th, nz.V00);
        for (int cc = w.lane(); cc < nb; cc += w.width()) {   // rows 0, 1 of F_x P
            const double p2 = ws.P[2 * LD + cc];
            ws.P[cc] = ekf_pred_row(ws.P[cc], m.fa, p2);
            ws.P[LD + cc] = ekf_pred_row(ws.P[LD + cc], m.fb, p2);
            ws.xp[cc] = cc == 0 ? m.xp0 : (cc == 1 ? m.xp1 : (cc == 2 ? m.xp2 : ws.x[cc]));
        }
        w.sync();
        for (int r = w.lane(); r < nb; r += w.width()) {      // columns 0, 1 of (F_x P) F_x^T
            const double a2 = ws.P[r * LD + 2];
            ws.P[r * LD + 0] = ekf_pred_col(ws.P[r * LD + 0], a2, m.fa);
            ws.P[r * LD + 1] = ekf_pred_col(ws.P[r * LD + 1], a2, m.fb);
        }
        w.sync();
        if (w.lane() == 0) {                                   // + F_v V F_v^T
            ws.P[0] = ws.P[0] + m.q00;
            ws.P[1] = ws.P[1] + m.q01;
            ws.P[LD] = ws.P[LD] + m.q10;
            ws.P[LD + 1] = ws.P[LD + 1] + m.q11;
            ws.P[2 * LD + 2] = ws.P[2 * LD + 2] + nz.V11;
        }
        w.sync();
    }

    // ---- the message ----
    double nis_sum = 0.0;
    int32_t flags = 0;
    for (int l = 0; l < k; ++l) {
        const int q = ws.code[l];
        if (q < 0) continue;
        const int ii = 3 + 2 * q;
        const float r_m = ws.meas[3 * l + 1], b_m = ws.meas[3 * l + 2];
        const double* const xl = lm_from_pred ? ws.xp : ws.x;   // quirk D-2 (ekf.cpp:115-116): the landmark is read from x_t
        const EkfRange rg = ekf_range(xl[ii], xl[ii + 1], ws.xp[0], ws.xp[1]);   // ekf.cpp:115 (float)
        const EkfH h = ekf_jacobian(rg.dx, rg.dy, rg.dd, rg.d2);
        const EkfVec2 nu = ekf_innovation(r_m, b_m, rg.dist, rg.dx, rg.dy, ws.xp[2], nz.w_r, nz.w_b);   // ekf.cpp:129-131
        const double nu0 = nu.x, nu1 = nu.y;
        for (int c = w.lane(); c < nb; c += w.width()) {        // H P (H0[2] == 0 is skipped)
            const EkfVec2 hp = ekf_hp_col(h, ws.P[c], ws.P[LD + c], ws.P[2 * LD + c], ws.P[ii * LD + c], ws.P[(ii + 1) * LD + c]);
            ws.HP[c] = hp.x;
            ws.HP[kInnovNb + c] = hp.y;
        }
        w.sync();
        auto hp_col = [&](int c) -> EkfVec2 { return EkfVec2{ws.HP[c], ws.HP[kInnovNb + c]}; };
        const EkfS Sm = ekf_S(h, hp_col(0), hp_col(1), hp_col(2), hp_col(ii), hp_col(ii + 1), nz.W00, nz.W11);   // S = (H P) H^T + W (ekf.cpp:133)
        const double (&S)[4] = Sm.s;
        double Si[4];
        const bool ok = inv2x2_lu(S, Si);
        double nis = nu0 * (Si[0] * nu0 + Si[1] * nu1) + nu1 * (Si[2] * nu0 + Si[3] * nu1);
        if (!ok) { flags |= kInnovSingular; nis = nan; }
        if (!innov_finite(nu0) || !innov_finite(nu1) || !innov_finite(S[0]) || !innov_finite(S[1]) || !innov_finite(S[2]) || !innov_finite(S[3])) nis = nan;
        bool rejected = false;
        if constexpr (G::on) {
            rejected = innov_finite(nis) && nis > g->gate;
            if (w.lane() == 0) g->verdict[l] = rejected ? kGateRejected : kGateAccepted;
            if (rejected) g->n_rej += 1;
        }
        if (!rejected && innov_finite(nis)) {
            nis_sum = nis_sum + nis;
            out.n_fin += 1;
            if (nis > out.max_nis) out.max_nis = nis;
            if (nis < lo) out.n_below += 1;
            if (nis > hi) out.n_above += 1;
            out.s_nur = out.s_nur + nu0; out.s_nub = out.s_nub + nu1;
            out.s_nur2 = out.s_nur2 + nu0 * nu0; out.s_nub2 = out.s_nub2 + nu1 * nu1;
        }
        if (det && w.lane() == 0) {
            double* const dl = det + (size_t)l * kInnovDetLen;
            dl[0] = nis; dl[1] = nu0; dl[2] = nu1; dl[3] = S[0]; dl[4] = 0.5 * (S[1] + S[2]); dl[5] = S[3];
        }
        if constexpr (G::on) {
            if (rejected) {   // x_pred and P stay as they are; the next update's writes of HP come after this slot's reads of it
                w.sync();
                continue;
            }
        }
        for (int r = w.lane(); r < nb; r += w.width()) {        // K = (P H^T) S^-1 (ekf.cpp:135), x_pred += K nu (ekf.cpp:138)
            const double* const pr = ws.P + r * LD;
            const EkfVec2 kk = ekf_gain(ekf_pht_row(h, pr[0], pr[1], pr[2], pr[ii], pr[ii + 1]), Si[0], Si[1], Si[2], Si[3]);
            ws.K[2 * r] = kk.x; ws.K[2 * r + 1] = kk.y;
            ws.xp[r] = ekf_state_update(ws.xp[r], r, kk.x, kk.y, nu0, nu1);   // ekf.cpp:139
        }
        w.sync();
        for (int e = w.lane(); e < nb * nb; e += w.width()) {   // P_pred -= K (H P) (ekf.cpp:140, the rank-2 form)
            const int r = e / nb, c = e - r * nb;
            ws.P[r * LD + c] = ekf_downdate(ws.P[r * LD + c], ws.K[2 * r], ws.K[2 * r + 1], ws.HP[c], ws.HP[kInnovNb + c]);
        }
        w.sync();
    }
    out.nis_sum = nis_sum; out.n_upd = n_upd; out.n_new = n_new; out.flags = flags;
    for (int i = 0; i < 3; ++i) {
        out.post[i] = ws.xp[i];
        for (int j = 0; j < 3; ++j) out.post[3 + 3 * i + j] = ws.P[i * LD + j];
    }
    return out;
}

// what one instance adds to a record
SLAM_HD void innovation_record(const InnovResult& v, double r[kInnovRecLen]) {
    for (int i = 0; i < kInnovRecLen; ++i) r[i] = 0.0;
    if (v.flags & kInnovFrozen) { r[kInnFrozen] = 1.0; return; }
    if (v.flags & kInnovTooLong) { r[kInnTooLong] = 1.0; return; }
    if (v.flags & kInnovWouldFreeze) { r[kInnWouldFreeze] = 1.0; return; }
    r[kInnEval] = 1.0;
    if (v.flags & kInnovSingular) r[kInnSingular] = 1.0;
    r[kInnUpd] = (double)v.n_fin; r[kInnNew] = (double)v.n_new;
    r[kInnSumNis] = v.nis_sum; r[kInnMaxNis] = v.max_nis;
    r[kInnBelow] = (double)v.n_below; r[kInnAbove] = (double)v.n_above;
    r[kInnSumNuR] = v.s_nur; r[kInnSumNuB] = v.s_nub; r[kInnSumNuR2] = v.s_nur2; r[kInnSumNuB2] = v.s_nub2;
}

#if defined(__HIPCC__)
// the 64 lanes of one wavefront
struct InnovWave {
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int width() const { return 64; }
    // LDS written by some lanes is read by others of the same wavefront afterwards
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    template <class F> __device__ __forceinline__ int first(int n, F f) const {   // (called in wave-uniform control flow)
        for (int i0 = 0; i0 < n; i0 += 64) {
            const int i = i0 + ln;
            const unsigned long long m = __ballot(i < n && f(i));
            if (m != 0ull) return i0 + (__ffsll((long long)m) - 1);
        }
        return -1;
    }
};

// One evaluation of every instance on `stream`: three launches (the instances, then per-workgroup partial records and their sum in
// ascending order).  Everything is read only, except the outputs.
struct InnovParams {
    EkfStepParams s;            // exactly what the step that follows is launched with (state, ids, status, noise rows, command or cmd_each,
                                // the message source: meas_in / meas_count_in / k_stride_in, or sim with truth, maps, seed and step)
    double nis_lo, nis_hi;      // the band of record entries 9 and 10
    double* nis_sum; int32_t* n_upd; int32_t* n_new; int32_t* flags;   // [B] each, any may be NULL
    double* det;                // [B][kInnovMaxDet][kInnovDetLen] or NULL
    double* post;               // [B][12] or NULL
    double* inst_rec;           // [B][kInnovRecLen]
    double* partials;           // [record_blocks(B)][kInnovRecLen]
    double* rec;                // [kInnovRecLen]
};
hipError_t launch_innovation(const InnovParams& p, int f32_storage, hipStream_t stream);
#endif

}  // namespace slam
