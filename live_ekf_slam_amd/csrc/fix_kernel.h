// fix_kernel.h — absolute position and heading fixes of the EKF batch (slam_fix, slam_fix_sense, slam_fix_run; gfx950): a GPS position, a
// compass heading, a pose from a motion-capture system.  Every other measurement of the batch is a range-bearing detection of a landmark;
// a stretch without a landmark in view is dead reckoning whose error grows without bound, and a fix is what bounds it.  The per-instance
// semantics are defined here, ONCE, for the device kernels (fix_kernel.hip) and the host hooks (slam_fix_instance_host,
// slam_fix_sense_instance_host), both compiled with -ffp-contract=off; arithmetic goes through ekf_model.h (ekf_gain, ekf_state_update,
// ekf_downdate and their scalar forms ekf_gain1, ekf_state_update1, ekf_downdate1) and slam_math.h (inv2x2_lu, rem2pi, det_sincos) only.
// No step, gate, innovation, association, map, merge or sense kernel changes.
//
// A fix of instance b: one row {z_x, z_y, z_yaw, sigma_pos, sigma_yaw} of doubles and one int32 `kinds` (bit 0: the position part is
// present, bit 1: the heading part; other bits are ignored).  The parts are applied SEQUENTIALLY, position first, then heading, each on
// the state the previous one left.  All values are the stored ones, widened to double for fp32 storage; n = 3 + 2 M.
// Position part (H selects the entries 0 and 1):
//   c_r = (P[r][0], P[r][1]) for every row r;  g_c = (P[0][c], P[1][c]) for every column c  (both are read: P is symmetric only to rounding)
//   nu = (z_x - x[0], z_y - x[1]);  S = [c_0; c_1] + sigma_pos^2 I;  Si = inv2x2_lu(S)
//   nis = nu0 (Si00 nu0 + Si01 nu1) + nu1 (Si10 nu0 + Si11 nu1), unfused
//   accepted: K_r = ekf_gain(c_r, Si);  x[r] = ekf_state_update(x[r], r, K_r.x, K_r.y, nu0, nu1)  (yaw wrapped as in the step)
//             P[r][c] = ekf_downdate(P[r][c], K_r.x, K_r.y, g_c.x, g_c.y);  stored rounded to the storage type; pad columns stay zero
// Heading part (H selects entry 2):
//   c_r = P[r][2];  g_c = P[2][c];  nu = rem2pi(z_yaw - x[2]);  S = c_2 + sigma_yaw^2;  si = 1.0 / S;  nis = nu * (si * nu)
//   accepted: k_r = ekf_gain1(c_r, si);  x[r] = ekf_state_update1(x[r], r, k_r, nu);  P[r][c] = ekf_downdate1(P[r][c], k_r, g_c)
// Verdict of a part, in this order: 0 absent; 4 INVALID: a z or the sigma of the part is not finite, or sigma < 0; 3 SINGULAR: inv2x2_lu
//   failed or S is not finite (heading: S not finite or S <= 0); 2 REJECTED: nis is finite and nis > the part's gate (a nis equal to the
//   gate is accepted; a nis that is not finite is never rejected and ends as SINGULAR); 1 APPLIED.  Only APPLIED writes anything.
//   verdict = position | heading << 4.  nis [2]: the part's nis where it is APPLIED or REJECTED, NaN otherwise.
// Not written: an instance with status & kMapStatusSkip (non-finite, frozen, watchdog) reports verdict 0 and is not looked at; an instance
//   without an APPLIED part is not written at all.  M, ids, flags, timestep, truth, err_sum and the track counters are never touched.
// Record (16 doubles, every entry a sum, through the fixed-order reduction of the sense records): 0 instances written; 1 - 5 position
//   present / applied / rejected / singular / invalid; 6 - 10 the same for heading; 11, 12 the sums of the nis of the applied position and
//   heading parts; 13 instances skipped by status (they add to no other entry); 14, 15 reserved, 0.
//
// ONE PASS OVER P (fix_instance<true>, the device).  With both parts applied, the heading part's inputs are P'[r][2], P'[2][c], P'[2][2]
// and x'[2] of the state P', x' the position part leaves.  They follow from the position part's own inputs:
//   P'[r][2] = (ST)(P[r][2] - K_r . g_2),  P'[2][c] = (ST)(P[2][c] - K_2 . g_c),  x'[2] = (ST)ekf_state_update(x[2], 2, K_2, nu)
// (ST: the rounding to the storage type a store performs), so an element's final value is
//   (ST)( (double)(ST)(p - K_r . g_c) - ekf_gain1(P'[r][2], si) * P'[2][c] ):
// the operations of the two sequential passes (fix_instance<false>, the host hook) on the same operands in the same order, the rounding in
// between included, hence the same bits in fp64 and in fp32 storage - while P is read and written once.
//
// Why the update may run IN PLACE, and the barriers.  Rows and columns 0, 1, 2 of P and x[0 .. 2] are inputs of EVERY element and are
// themselves overwritten.  (1) They are gathered into the workspace (LDS on the device, 6 n + 3 doubles: the position part's c_r at 2 r
// and g_c at 2 n + 2 c, pairs a lane reads with one 16-byte load as in the merge; the heading part's c_r at 4 n + r and g_c at
// 5 n + c; x[0 .. 2] at 6 n) and a workgroup barrier is passed before the first
// store: after it an element's new value depends on its own old value - read by the lane that stores it - and on the workspace alone.
// (2) The sequential form passes a second barrier after the position part's stores and before the heading part's gather: that gather
// reads elements other lanes have just stored, and overwrites nothing they still read only because it comes after the barrier.  The
// one-pass form gathers once, so it has no store in front of a gather and needs (1) alone.  No further barrier: between (1) and the end
// no lane reads an element of P or x that another lane writes, and S, Si, si, K_2 and both verdicts are recomputed by every lane from the
// workspace and the fix row (no broadcast to wait for).
//
// Simulated source (fix_sense_instance): a fix of the TRUE pose for the runs and the tool.  Row per instance: slam_fix_sensor.  Draws of
// instance g at RNG step s - the step the next simulator step would use - at pair indices the clean generator and the fault model
// (F = 0x40000000) never use, G = 0x50000000:
//   (u0, u1) = pair G       z_x = (t_x + (2 a) u0) - a,  z_y = (t_y + (2 a) u1) - a,  a = pos_halfwidth
//   (v0, v1) = pair G + 1   z_yaw = rem2pi((t_yaw + (2 h) v0) - h),  h = yaw_halfwidth;  the position part is missed iff v1 < p_miss_pos
//   (j0, j1) = pair G + 2   a position part that was not missed jumps iff j0 < p_jump, by m = jump_lo + (jump_hi - jump_lo) * j1
//   (d0, d1) = pair G + 3   the direction phi = (kTwoPi * d0) - kPi: z_x = z_x + m * cos(phi), z_y = z_y + m * sin(phi) (det_sincos);  the
//                           heading part is missed iff d1 < p_miss_yaw
// kinds_out = row.kinds & 3 without the missed parts; the z of a part that is not in kinds_out is written as 0; sigma_pos and sigma_yaw are
// copied.  Every expression is evaluated as parenthesised, in fp64.  The all-zero row emits nothing: kinds 0 and a zero row.  The status
// is not consulted (the fix skips what it has to); the truth and the RNG step are read, never advanced.
#pragma once
#include <stdint.h>

#include "../../include/slam_batch.h"
#include "ekf_model.h"
#include "map_kernel.h"
#include "slam_math.h"
#include "slam_rng.h"

namespace slam {

constexpr int kFixRecLen = 16;
enum FixRec {
    kFixWritten = 0, kFixPosPresent = 1, kFixPosApplied = 2, kFixPosRejected = 3, kFixPosSingular = 4, kFixPosInvalid = 5,
    kFixYawPresent = 6, kFixYawApplied = 7, kFixYawRejected = 8, kFixYawSingular = 9, kFixYawInvalid = 10, kFixSumNisPos = 11,
    kFixSumNisYaw = 12, kFixSkipped = 13
};
constexpr unsigned kFixRecMax = 0u;                 // no entry is joined by a maximum (record_kernel.h): every one is a sum
enum FixVerdict { kFixAbsent = 0, kFixApplied = 1, kFixRejected = 2, kFixSingular = 3, kFixInvalid = 4 };
constexpr int kFixRowLen = 5;                       // doubles of one fix row
constexpr uint32_t kFixPair = 0x50000000u;          // G: the first pair index of the source's draws

SLAM_HD bool fix_finite(double v) { return fabs(v) < __builtin_inf(); }
constexpr int fix_ws_len(int n) { return 6 * n + 3; }   // doubles of the workspace of a state of n entries

// what the fix row alone says of a part: kFixAbsent, kFixInvalid, or -1: the part is evaluated against the state
SLAM_HD int fix_pre_pos(int kinds, const double* row) {
    if (!(kinds & 1)) return kFixAbsent;
    return (fix_finite(row[0]) && fix_finite(row[1]) && fix_finite(row[3]) && !(row[3] < 0.0)) ? -1 : kFixInvalid;
}
SLAM_HD int fix_pre_yaw(int kinds, const double* row) {
    if (!(kinds & 2)) return kFixAbsent;
    return (fix_finite(row[2]) && fix_finite(row[4]) && !(row[4] < 0.0)) ? -1 : kFixInvalid;
}

// the verdict of a nis that was formed with a usable inverse
SLAM_HD int fix_gate(bool ok, double nis, double gate) {
    if (!ok || !fix_finite(nis)) return kFixSingular;
    return nis > gate ? kFixRejected : kFixApplied;
}

struct FixPos { int verdict; double nis, nu0, nu1, Si[4]; };
SLAM_HD FixPos fix_pos_decide(double p00, double p01, double p10, double p11, double x0, double x1, const double* row, double gate) {
    FixPos d;
    d.nu0 = row[0] - x0; d.nu1 = row[1] - x1;
    const double s2 = row[3] * row[3];
    const double S[4] = {p00 + s2, p01, p10, p11 + s2};
    const bool ok = inv2x2_lu(S, d.Si) && fix_finite(S[0]) && fix_finite(S[1]) && fix_finite(S[2]) && fix_finite(S[3]);
    d.nis = d.nu0 * (d.Si[0] * d.nu0 + d.Si[1] * d.nu1) + d.nu1 * (d.Si[2] * d.nu0 + d.Si[3] * d.nu1);
    d.verdict = fix_gate(ok, d.nis, gate);
    return d;
}

struct FixYaw { int verdict; double nis, nu, si; };
SLAM_HD FixYaw fix_yaw_decide(double p22, double x2, const double* row, double gate) {
    FixYaw d;
    d.nu = rem2pi(row[2] - x2);
    const double S = p22 + row[4] * row[4];
    d.si = 1.0 / S;
    d.nis = d.nu * (d.si * d.nu);
    d.verdict = fix_gate(fix_finite(S) && S > 0.0, d.nis, gate);
    return d;
}

struct FixResult { int32_t verdict; double nis[2]; int written; };

SLAM_HD double fix_nis_out(int verdict, double nis) { return (verdict == kFixApplied || verdict == kFixRejected) ? nis : __builtin_nan(""); }

// One instance that is not skipped, in place.  ST: float or double, P at the leading dimension ekf_ld(n), x [n]; row [5], gates [2]
// (position, heading); ws: fix_ws_len(n) doubles (LDS on the device).  W: an execution policy of map_kernel.h (MapSeq on the host, the
// workgroup on the device).  ONE_PASS: every element of P and x is visited once, whatever the parts (the device); otherwise the two parts
// are two passes, each on the state the previous one left (the host hook: the definition).  The two give the same bits; the argument and
// the barriers are at the top of this file.  Every lane of the policy calls it with the same arguments and gets the same result.
template <bool ONE_PASS, class W, class ST>
SLAM_HD FixResult fix_instance(const W& w, ST* P, ST* x, int M, const double* row, int kinds, const double* gates, double* ws) {
    const int n = 3 + 2 * M, ld = ekf_ld(n, (int)sizeof(ST));
    const int total = n * ld;                        // (<= 2003 * 2004: int)
    double* const cr = ws;                           // c_r of the position part, pairs
    double* const gc = ws + 2 * n;                   // g_c of the position part, pairs
    double* const cy = ws + 4 * n;                   // c_r of the heading part
    double* const gy = ws + 5 * n;                   // g_c of the heading part
    double* const xs = ws + 6 * n;
    const double nan = __builtin_nan("");
    int vp = fix_pre_pos(kinds, row), vy = fix_pre_yaw(kinds, row);
    FixResult o = {0, {nan, nan}, 0};
    if (vp >= 0 && vy >= 0) {                        // (every lane alike: nothing is evaluated, P is not looked at)
        o.verdict = vp | (vy << 4);
        return o;
    }
    const bool ep = vp < 0, ey = vy < 0;             // the parts that are evaluated
    FixPos dp = {kFixAbsent, nan, 0.0, 0.0, {0.0, 0.0, 0.0, 0.0}};
    FixYaw dy = {kFixAbsent, nan, 0.0, 0.0};
    int r0 = w.lane() / ld, c0 = w.lane() - r0 * ld;
    const int dr = w.width() / ld, dc = w.width() - dr * ld;
    if (ONE_PASS) {
        for (int r = w.lane(); r < n; r += w.width()) {
            if (ep) {
                cr[2 * r] = (double)P[r * ld]; cr[2 * r + 1] = (double)P[r * ld + 1];
                gc[2 * r] = (double)P[r]; gc[2 * r + 1] = (double)P[ld + r];
            }
            if (ey) { cy[r] = (double)P[r * ld + 2]; gy[r] = (double)P[2 * ld + r]; }
        }
        if (w.lane() == 0) {
            if (ep) { xs[0] = (double)x[0]; xs[1] = (double)x[1]; }
            if (ey) xs[2] = (double)x[2];
        }
        w.sync();                                    // (1): every input of both parts is in the workspace before the first store
        bool ap = false, ay = false;
        EkfVec2 k2 = {0.0, 0.0};                     // K_2 of the position part
        if (ep) {
            dp = fix_pos_decide(cr[0], cr[1], cr[2], cr[3], xs[0], xs[1], row, gates[0]);
            vp = dp.verdict; ap = vp == kFixApplied;
        }
        if (ey) {
            double p22 = cy[2], x2 = xs[2];          // P[2][2] and x[2] as the position part leaves them
            if (ap) {
                k2 = ekf_gain(EkfVec2{cr[4], cr[5]}, dp.Si[0], dp.Si[1], dp.Si[2], dp.Si[3]);
                p22 = (double)(ST)ekf_downdate(p22, k2.x, k2.y, gc[4], gc[5]);
                x2 = (double)(ST)ekf_state_update(x2, 2, k2.x, k2.y, dp.nu0, dp.nu1);
            }
            dy = fix_yaw_decide(p22, x2, row, gates[1]);
            vy = dy.verdict; ay = vy == kFixApplied;
        }
        if (ap || ay) {
            const bool both = ap && ay;
            // 16 bytes of a row per lane and round trip: V elements that never straddle a row (ld is a multiple of V) and always hold
            // a real column (ld - n < V).  K_r and P'[r][2] are formed once per group.  A pad column is stored as it was read: zero.
            constexpr int V = 16 / (int)sizeof(ST);
            const int gpr = ld / V, groups = n * gpr;
            int r = w.lane() / gpr, gi = w.lane() - r * gpr;
            const int gdr = w.width() / gpr, gdi = w.width() - gdr * gpr;
            for (int g = w.lane(); g < groups; g += w.width()) {
                ST* const q = static_cast<ST*>(__builtin_assume_aligned(P + (size_t)g * V, 16));
                ST v[V];
                __builtin_memcpy(v, q, 16);
                EkfVec2 kr = {0.0, 0.0};
                double hc = ay ? cy[r] : 0.0;
                if (ap) {
                    kr = ekf_gain(EkfVec2{cr[2 * r], cr[2 * r + 1]}, dp.Si[0], dp.Si[1], dp.Si[2], dp.Si[3]);
                    if (both) hc = (double)(ST)ekf_downdate(hc, kr.x, kr.y, gc[4], gc[5]);         // P'[r][2]
                }
                const double kh = ekf_gain1(hc, dy.si);
#pragma unroll
                for (int u = 0; u < V; ++u) {
                    const int c = gi * V + u;
                    if (c < n) {
                        double p = (double)v[u];
                        double hg = ay ? gy[c] : 0.0;
                        if (ap) {
                            const double g0 = gc[2 * c], g1 = gc[2 * c + 1];
                            p = (double)(ST)ekf_downdate(p, kr.x, kr.y, g0, g1);
                            if (both) hg = (double)(ST)ekf_downdate(hg, k2.x, k2.y, g0, g1);       // P'[2][c]
                        }
                        if (ay) p = ekf_downdate1(p, kh, hg);
                        v[u] = (ST)p;
                    }
                }
                __builtin_memcpy(q, v, 16);
                r += gdr; gi += gdi;
                if (gi >= gpr) { gi -= gpr; r += 1; }
            }
            for (int q = w.lane(); q < n; q += w.width()) {
                double xv = (double)x[q];
                double hc = ay ? cy[q] : 0.0;
                if (ap) {
                    const EkfVec2 kq = ekf_gain(EkfVec2{cr[2 * q], cr[2 * q + 1]}, dp.Si[0], dp.Si[1], dp.Si[2], dp.Si[3]);
                    xv = (double)(ST)ekf_state_update(xv, q, kq.x, kq.y, dp.nu0, dp.nu1);
                    if (both) hc = (double)(ST)ekf_downdate(hc, kq.x, kq.y, gc[4], gc[5]);
                }
                if (ay) xv = ekf_state_update1(xv, q, ekf_gain1(hc, dy.si), dy.nu);
                x[q] = (ST)xv;
            }
            o.written = 1;
        }
    } else {
        if (ep) {                                    // ---- the position part
            for (int r = w.lane(); r < n; r += w.width()) {
                cr[2 * r] = (double)P[r * ld]; cr[2 * r + 1] = (double)P[r * ld + 1];
                gc[2 * r] = (double)P[r]; gc[2 * r + 1] = (double)P[ld + r];
            }
            if (w.lane() == 0) { xs[0] = (double)x[0]; xs[1] = (double)x[1]; }
            w.sync();                                // (1)
            dp = fix_pos_decide(cr[0], cr[1], cr[2], cr[3], xs[0], xs[1], row, gates[0]);
            vp = dp.verdict;
            if (vp == kFixApplied) {
                int r = r0, c = c0;
                for (int e = w.lane(); e < total; e += w.width()) {
                    if (c < n) {
                        const EkfVec2 kr = ekf_gain(EkfVec2{cr[2 * r], cr[2 * r + 1]}, dp.Si[0], dp.Si[1], dp.Si[2], dp.Si[3]);
                        P[e] = (ST)ekf_downdate((double)P[e], kr.x, kr.y, gc[2 * c], gc[2 * c + 1]);
                    }
                    r += dr; c += dc;
                    if (c >= ld) { c -= ld; r += 1; }
                }
                for (int q = w.lane(); q < n; q += w.width()) {
                    const EkfVec2 kq = ekf_gain(EkfVec2{cr[2 * q], cr[2 * q + 1]}, dp.Si[0], dp.Si[1], dp.Si[2], dp.Si[3]);
                    x[q] = (ST)ekf_state_update((double)x[q], q, kq.x, kq.y, dp.nu0, dp.nu1);
                }
                o.written = 1;
            }
            w.sync();                                // (2): the stores are done before the heading part's gather
        }
        if (ey) {                                    // ---- the heading part, on the state the position part left
            for (int r = w.lane(); r < n; r += w.width()) { cy[r] = (double)P[r * ld + 2]; gy[r] = (double)P[2 * ld + r]; }
            if (w.lane() == 0) xs[2] = (double)x[2];
            w.sync();                                // (1)
            dy = fix_yaw_decide(cy[2], xs[2], row, gates[1]);
            vy = dy.verdict;
            if (vy == kFixApplied) {
                int r = r0, c = c0;
                for (int e = w.lane(); e < total; e += w.width()) {
                    if (c < n) P[e] = (ST)ekf_downdate1((double)P[e], ekf_gain1(cy[r], dy.si), gy[c]);
                    r += dr; c += dc;
                    if (c >= ld) { c -= ld; r += 1; }
                }
                for (int q = w.lane(); q < n; q += w.width()) x[q] = (ST)ekf_state_update1((double)x[q], q, ekf_gain1(cy[q], dy.si), dy.nu);
                o.written = 1;
            }
        }
    }
    o.verdict = vp | (vy << 4);
    o.nis[0] = fix_nis_out(vp, dp.nis);
    o.nis[1] = fix_nis_out(vy, dy.nis);
    return o;
}

// what one instance adds to a record; skipped: its status carried kMapStatusSkip (o is then not looked at)
SLAM_HD void fix_record(const FixResult& o, bool skipped, double r[kFixRecLen]) {
    for (int i = 0; i < kFixRecLen; ++i) r[i] = 0.0;
    if (skipped) { r[kFixSkipped] = 1.0; return; }
    const int vp = o.verdict & 15, vy = (o.verdict >> 4) & 15;
    r[kFixWritten] = o.written ? 1.0 : 0.0;
    if (vp) { r[kFixPosPresent] = 1.0; r[kFixPosPresent + vp] = 1.0; }
    if (vy) { r[kFixYawPresent] = 1.0; r[kFixYawPresent + vy] = 1.0; }
    if (vp == kFixApplied) r[kFixSumNisPos] = o.nis[0];
    if (vy == kFixApplied) r[kFixSumNisYaw] = o.nis[1];
}

// The traffic model of one instance of a fix (slam_last_fix_work), in elements of P / x and in other bytes, from the verdict the instance
// reported: a part that was evaluated (APPLIED, REJECTED or SINGULAR) gathers 4 n + 2 (position) or 2 n + 1 (heading) elements; an
// instance that was written reads and writes P and x once each, whatever its parts; the fix row, kinds, M and status are read and the
// verdict and the two nis written by every instance.
struct FixTraffic { unsigned long long elems, other_bytes; };
SLAM_HD FixTraffic fix_traffic(int M, int32_t verdict) {
    const unsigned long long n = 3ull + 2ull * (unsigned long long)(M < 0 ? 0 : M);
    const int vp = verdict & 15, vy = (verdict >> 4) & 15;
    FixTraffic t = {0ull, 8ull * kFixRowLen + 4ull + 8ull + 4ull + 16ull};
    if (vp >= kFixApplied && vp <= kFixSingular) t.elems += 4ull * n + 2ull;
    if (vy >= kFixApplied && vy <= kFixSingular) t.elems += 2ull * n + 1ull;
    if (vp == kFixApplied || vy == kFixApplied) t.elems += 2ull * n * n + 2ull * n;
    return t;
}

// ---- the simulated source ----
SLAM_HD slam_fix_sensor fix_sensor_default_row() { return slam_fix_sensor{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0}; }
// the value checks of a row: NULL, or the name of the first bad field
inline const char* fix_sensor_bad_field(const slam_fix_sensor& r) {
    auto width = [](double v) { return fix_finite(v) && v >= 0.0; };
    auto prob = [](double p) { return fix_finite(p) && p >= 0.0 && p <= 1.0; };
    if (!width(r.pos_halfwidth)) return "pos_halfwidth";
    if (!width(r.yaw_halfwidth)) return "yaw_halfwidth";
    if (!width(r.sigma_pos)) return "sigma_pos";
    if (!width(r.sigma_yaw)) return "sigma_yaw";
    if (!prob(r.p_miss_pos)) return "p_miss_pos";
    if (!prob(r.p_miss_yaw)) return "p_miss_yaw";
    if (!prob(r.p_jump)) return "p_jump";
    if (!fix_finite(r.jump_lo)) return "jump_lo";
    if (!fix_finite(r.jump_hi) || r.jump_lo > r.jump_hi) return "jump_hi";
    if (r.kinds < 0 || r.kinds > 3) return "kinds";
    return nullptr;
}

struct FixSensed { double row[kFixRowLen]; int32_t kinds, jumped; };
// one instance's fix of its true pose (tx, ty, tth); g: the global instance id, s: the RNG step
SLAM_HD FixSensed fix_sense_instance(const slam_fix_sensor& sr, uint64_t seed, uint64_t g, uint32_t s, double tx, double ty, double tth) {
    FixSensed o = {{0.0, 0.0, 0.0, sr.sigma_pos, sr.sigma_yaw}, 0, 0};
    const int want = sr.kinds & 3;
    if (!want) return o;
    double u0, u1, v0, v1, j0, j1, d0, d1;
    noise_pair(seed, g, s, kFixPair, &u0, &u1);
    noise_pair(seed, g, s, kFixPair + 1u, &v0, &v1);
    noise_pair(seed, g, s, kFixPair + 2u, &j0, &j1);
    noise_pair(seed, g, s, kFixPair + 3u, &d0, &d1);
    const double a = sr.pos_halfwidth, hw = sr.yaw_halfwidth;
    double zx = (tx + (2 * a) * u0) - a;
    double zy = (ty + (2 * a) * u1) - a;
    const double zyaw = rem2pi((tth + (2 * hw) * v0) - hw);
    const bool pos = (want & 1) && !(v1 < sr.p_miss_pos);
    const bool yaw = (want & 2) && !(d1 < sr.p_miss_yaw);
    if (pos && j0 < sr.p_jump) {
        const double m = sr.jump_lo + (sr.jump_hi - sr.jump_lo) * j1;
        const double phi = (kTwoPi * d0) - kPi;
        double sn, cs;
        det_sincos(phi, &sn, &cs);
        zx = zx + m * cs;
        zy = zy + m * sn;
        o.jumped = 1;
    }
    if (pos) { o.row[0] = zx; o.row[1] = zy; }
    if (yaw) o.row[2] = zyaw;
    o.kinds = (pos ? 1 : 0) | (yaw ? 2 : 0);
    return o;
}

#if defined(__HIPCC__)
// The fix of every instance on `stream`: one launch, then - when rec is wanted - the record (two more launches).
struct FixParams {
    void* P; void* x;                 // [B][pstride], [B][xstride] in elements of the storage type; updated in place
    const int32_t *M, *status;        // [B]
    const double* fix;                // [B][5]
    const int32_t* kinds;             // [B]
    double gate_pos, gate_yaw;
    int32_t* verdict;                 // [B]
    double* nis;                      // [B][2]
    double* inst_rec;                 // [B][kFixRecLen]
    double* partials;                 // [record_blocks(B)][kFixRecLen]
    double* rec;                      // [kFixRecLen], or NULL: no record, and inst_rec / partials are not used
    int32_t B, L_max, pstride, xstride;
};
hipError_t launch_fix(const FixParams& p, int f32_storage, hipStream_t stream);

// The simulated source for every instance on `stream`.  rows NULL: the all-zero row (nothing is emitted).
struct FixSenseParams {
    const double* truth;              // [B][3]
    const slam_fix_sensor* rows;      // [B] or NULL
    uint64_t seed; int64_t inst0; uint32_t step;
    double* fix;                      // [B][5]
    int32_t* kinds;                   // [B]
    int32_t* jumped;                  // [B] or NULL
    int32_t B;
};
hipError_t launch_fix_sense(const FixSenseParams& p, hipStream_t stream);

// work [2] += the sums of fix_traffic over n instances
hipError_t launch_fix_work(const int32_t* M, const int32_t* verdict, size_t n, int L_max, unsigned long long* work, hipStream_t stream);
#endif

}  // namespace slam
