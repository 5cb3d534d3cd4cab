// monitor_kernel.h — the run monitor: position / heading error and pose NEES of every instance at the handle's current state, reduced to
// one 16-double record per tick (slam_monitor_now, slam_monitor_run; gfx950).
//
// monitor_instance() below is THE definition of the per-instance values: the device kernel (monitor_kernel.hip) and the host test hook
// (slam_monitor_instance_host) compile this one function, with -ffp-contract=off on both sides, so the two give the same bits;
// tests/monitor_reference.py restates it in numpy.
//
//   err_pos    sqrt(wx wx + wy wy), wx = (double)(float)x - x_true, wy likewise: the estimate in the float32 wire format of the state
//              message against the simulator's pose, i.e. exactly the summand the step kernels add to the handle's error sum
//              (plotting_node.py:209-212), so the mean of an instance's series over a run is its slam_error_stats
//   err_yaw    remainder(yaw - yaw_true, 2 pi); EKF: yaw = x_t(2); UKF kinds: yaw = remainder(det_atan2(x_t(3), x_t(2)), 2 pi) (ukf.cpp:71)
//   nees_pose  EKF only: e^T S^-1 e, S = (P + P^T) / 2 of the leading 3 x 3 block, e = (x - x_true, y - y_true, err_yaw) in fp64 - S, e and
//              the Cholesky steps are those of consistency_kernel.hip restricted to three rows (same operations in the same order, pivot
//              test "> 0 and finite, no floor"), so the value and the flags are slam_consistency's.  UKF kinds: NaN
//   flags      slam_consistency_flags restricted to POSE_NOT_PD and INSTANCE_FAILED (status carries NONFINITE or WATCHDOG, or e is not
//              finite: then the three values are NaN)
// A per-instance value does not depend on the batch the instance sits in.  A RECORD does: its sums run over the batch in a fixed order
// that depends on the batch size alone (256 consecutive instances per workgroup by a fixed tree, then the workgroups in ascending order:
// no atomics on values), so a record has the same bits on every run and under every chunking of a run, but the sum over a batch is not
// the sum of the sums over its parts to the last bit.
#pragma once
#include <stdint.h>

#include "slam_math.h"
#if defined(__HIPCC__)
#include "record_kernel.h"
#endif

namespace slam {

constexpr int kMonRecLen = 16;     // doubles of one record

// indices of a record (counts are stored as doubles); sums and maxima run over the counted instances, a maximum over none is 0
enum MonitorRec {
    kMonOk = 0, kMonFailed = 1, kMonNees = 2, kMonPoseNotPd = 3, kMonSumPos = 4, kMonSumPos2 = 5, kMonMaxPos = 6, kMonSumYaw2 = 7,
    kMonMaxYaw = 8, kMonSumNees = 9, kMonBelow = 10, kMonAbove = 11, kMonSumM = 12, kMonFull = 13, kMonSumFull = 14, kMonSumDof = 15
};
constexpr unsigned kMonRecMax = (1u << kMonMaxPos) | (1u << kMonMaxYaw);   // the entries joined by a maximum (record_kernel.h)

constexpr int32_t kMonFlagPoseNotPd = 2, kMonFlagFailed = 8;   // SLAM_CONSISTENCY_POSE_NOT_PD, SLAM_CONSISTENCY_INSTANCE_FAILED
constexpr int32_t kMonStatusDead = 1 | 32;                     // SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG: the state is undefined

struct MonitorValue {
    double err_pos, err_yaw, nees_pose;
    int32_t flags;
};

SLAM_HD bool mon_finite(double v) { return fabs(v) < __builtin_inf(); }
SLAM_HD bool mon_pivot_ok(double d) { return d > 0.0 && d < __builtin_inf(); }

// x: x_t[0 .. 2] (EKF) or x_t[0 .. 3] (UKF kinds) as doubles (fp32 storage converted on load); P3: the leading 3 x 3 block of P_t,
// row-major, as stored (not symmetrised; not read for the UKF kinds); truth: the simulator's pose; status: slam_instance_flags.
SLAM_HD MonitorValue monitor_instance(const double* x, const double* P3, const double* truth, int32_t status, bool ukf) {
    const double nan = __builtin_nan("");
    MonitorValue v;
    v.err_pos = v.err_yaw = v.nees_pose = nan;
    v.flags = kMonFlagFailed;
    if (status & kMonStatusDead) return v;
    const double e0 = x[0] - truth[0], e1 = x[1] - truth[1];
    const double yaw = ukf ? wrap2pi(det_atan2(x[3], x[2])) : x[2];
    const double e2 = wrap2pi(yaw - truth[2]);
    if (!mon_finite(e0) || !mon_finite(e1) || !mon_finite(e2)) return v;
    v.flags = 0;
    const double wx = (double)(float)x[0] - truth[0], wy = (double)(float)x[1] - truth[1];
    v.err_pos = sqrt(wx * wx + wy * wy);
    v.err_yaw = e2;
    if (ukf) return v;
    // the lower triangle of S: the lower element first, one exact halving of one sum (consistency_kernel.hip)
    const double a00 = P3[0], a10 = 0.5 * (P3[3] + P3[1]), a11 = P3[4];
    const double a20 = 0.5 * (P3[6] + P3[2]), a21 = 0.5 * (P3[7] + P3[5]), a22 = P3[8];
    // right-looking Cholesky over the rows (S, e): y = L^-1 e appears in the appended row, one component per column
    bool bad = !mon_pivot_ok(a00);
    const double s0 = sqrt(a00);
    const double l10 = a10 / s0, l20 = a20 / s0, y0 = e0 / s0;
    double acc = 0.0;
    acc += y0 * y0;
    const double d1 = a11 - l10 * l10;
    if (!mon_pivot_ok(d1)) bad = true;
    const double s1 = sqrt(d1);
    const double l21 = (a21 - l20 * l10) / s1;
    const double b22 = a22 - l20 * l20;
    const double y1 = (e1 - y0 * l10) / s1;
    const double f2 = e2 - y0 * l20;
    acc += y1 * y1;
    const double d2 = b22 - l21 * l21;
    if (!mon_pivot_ok(d2)) bad = true;
    const double s2 = sqrt(d2);
    const double y2 = (f2 - y1 * l21) / s2;
    acc += y2 * y2;
    if (bad) v.flags = kMonFlagPoseNotPd;
    else v.nees_pose = acc;
    return v;
}

#if defined(__HIPCC__)
// One evaluation of every instance on `stream`: two launches (per-workgroup partial records, then their sum in ascending order).
// Everything is read only, except the outputs.
struct MonitorParams {
    const void* P;            // [B][pstride] P_t, fp64 or fp32 storage; EKF: row-major with leading dimension ekf_ld(3 + 2 M, esz)
    const void* x;            // [B][xstride] x_t
    const int32_t* M;         // [B], clamped to [0, L_max] before it is used
    const int32_t* status;    // [B] slam_instance_flags
    const double* truth;      // [B][3]
    int32_t B, L_max, pstride, xstride;
    int32_t ukf;              // x_t = (x, y, cos yaw, sin yaw, ...), no NEES
    double nees_lo, nees_hi;  // the band of record entries 10 and 11
    const double* nees_full;  // [B] of a launch_consistency that ran before on the stream, with dof [B]; NULL: entries 13 - 15 are 0
    const int32_t* dof;
    double* err_pos; double* err_yaw; double* nees_pose; int32_t* flags;   // [B] each, any may be NULL
    double* partials;         // [record_blocks(B)][kMonRecLen]
    double* rec;              // [kMonRecLen]
};
hipError_t launch_monitor(const MonitorParams& p, int f32_storage, hipStream_t stream);
#endif

}  // namespace slam
