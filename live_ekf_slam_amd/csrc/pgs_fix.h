// pgs_fix.h — absolute position and heading fixes (GPS, compass, motion capture) as UNARY POSE FACTORS of the pose graph: the graph-side
// counterpart of the EKF batch's fix (fix_kernel.h).  One source for the device (pgs_kernel.hip: linearisation, evaluation, cost,
// pgs_fix_attach_kernel, pgs_fix_weights_kernel) and the host (pgs_fix_factor_host, the TEST HOOK of slam_pgs.h), both compiled with
// -ffp-contract=off: only + - * /, remainder and det_sincos, so the two sides agree bit for bit.  DESIGN.md 4.4 "Absolute fixes".
//
// A fix of instance b at pose i is the EKF's row {z_x, z_y, z_yaw, sigma_pos, sigma_yaw} (5 doubles; what slam_fix_sense* emits goes in
// unchanged) plus `kinds` (bit 0: the position part, bit 1: the heading part).  It is TWO independent factors on the pose (x, y, theta),
// in the local coordinates of the solver's retraction (retract_pose: t' = t + R(theta) d_xy, theta' = rem2pi(theta + d_theta)).  With
// (s, c) = det_sincos(theta), wp = 1 / sigma_pos, wy = 1 / sigma_yaw:
//   position (2 rows)   e = ((x - z_x) wp, (y - z_y) wp)           J = [[c wp, -s wp, 0], [s wp, c wp, 0]]
//   heading  (1 row)    e = remainder(theta - z_yaw, kTwoPi) wy    J = [0, 0, wy]
// The share of the pose's Hessian block is J^T J formed as the products' sums (add_JtJ), not the closed form wp^2 I: the rounding is that of
// the product, as for the between factor.  The share of the gradient is -J^T e.
// Each part may carry the fix loss (fix_loss_kind, fix_loss_k: the kinds and the function of pgs_robust.h) with ss = e0^2 + e1^2 for the
// position and ss = e^2 for the heading: the part is linearised as sw e, sw J with the weight at the linearisation point, costs rho and
// adds 0.5 (w ss) to the linearised cost at delta = 0 - the rules of the landmark factors' loss.
// Validation of a part when it is attached: ABSENT (0) its kinds bit is clear; INVALID (4) a z of the part or its sigma is not finite, or the
// sigma is <= 0 (unlike the EKF, where sigma = 0 is an exact fix: here it would be an infinite weight); STORED (1) otherwise.
// verdict = position | heading << 4.
#pragma once
#include <stdint.h>

#include "pgs_robust.h"
#include "slam_math.h"

namespace slam {

enum { kPgsFixPos = 1, kPgsFixYaw = 2 };                              // = SLAM_FIX_POS, SLAM_FIX_YAW (slam_batch.h)
enum { kPgsFixAbsent = 0, kPgsFixStored = 1, kPgsFixInvalid = 4 };    // = pgs_fix_verdict (slam_pgs.h)
constexpr int kPgsFixRowLen = 5;

SLAM_HD bool pgs_fix_finite(double v) { return fabs(v) < __builtin_inf(); }

SLAM_HD int pgs_fix_check_pos(int kinds, const double* row) {
    if (!(kinds & kPgsFixPos)) return kPgsFixAbsent;
    return (pgs_fix_finite(row[0]) && pgs_fix_finite(row[1]) && pgs_fix_finite(row[3]) && row[3] > 0.0) ? kPgsFixStored : kPgsFixInvalid;
}
SLAM_HD int pgs_fix_check_yaw(int kinds, const double* row) {
    if (!(kinds & kPgsFixYaw)) return kPgsFixAbsent;
    return (pgs_fix_finite(row[2]) && pgs_fix_finite(row[4]) && row[4] > 0.0) ? kPgsFixStored : kPgsFixInvalid;
}

// the position part at pose ps: whitened residual e [2] and (JAC) Jacobian J [2][3], without the loss
template <bool JAC>
SLAM_HD void pgs_fix_pos(const double* ps, const double* row, double e[2], double J[6]) {
    const double wp = 1.0 / row[3];
    e[0] = (ps[0] - row[0]) * wp;
    e[1] = (ps[1] - row[1]) * wp;
    if (JAC) {
        double s, c;
        det_sincos(ps[2], &s, &c);
        J[0] = c * wp; J[1] = -s * wp; J[2] = 0.0;
        J[3] = s * wp; J[4] = c * wp;  J[5] = 0.0;
    }
}

// the heading part: whitened residual (returned) and *wy, the one non-zero entry of J = [0, 0, wy]
SLAM_HD double pgs_fix_yaw(const double* ps, const double* row, double* wy) {
    *wy = 1.0 / row[4];
    return remainder(ps[2] - row[2], kTwoPi) * *wy;
}

// One fix factor as the kernels see it, both parts: e [3] and J [3][3] (rows 0, 1: position, row 2: heading) WITHOUT the loss - rows of a
// part that is not stored are zero -, rho [2] and w [2] of the parts under the loss (NaN where the part is not stored).  Returns the verdict.
SLAM_HD int32_t pgs_fix_factor(const double* ps, const double* row, int kinds, int loss_kind, double loss_k, double e[3], double J[9],
                               double rho[2], double w[2]) {
    const int vp = pgs_fix_check_pos(kinds, row), vy = pgs_fix_check_yaw(kinds, row);
    for (int a = 0; a < 3; ++a) e[a] = 0.0;
    for (int a = 0; a < 9; ++a) J[a] = 0.0;
    rho[0] = rho[1] = w[0] = w[1] = __builtin_nan("");
    double sw;
    if (vp == kPgsFixStored) {
        pgs_fix_pos<true>(ps, row, e, J);
        const double ss = e[0] * e[0] + e[1] * e[1];
        pgs_robust_loss(loss_kind, loss_k, ss, sqrt(ss), &rho[0], &w[0], &sw);
    }
    if (vy == kPgsFixStored) {
        double wy;
        e[2] = pgs_fix_yaw(ps, row, &wy);
        J[8] = wy;
        const double ss = e[2] * e[2];
        pgs_robust_loss(loss_kind, loss_k, ss, sqrt(ss), &rho[1], &w[1], &sw);
    }
    return vp | (vy << 4);
}

}  // namespace slam
