// pgs_robust.h — robust loss of the bearing-range factors (GTSAM's noiseModel::Robust on the measurement factors): rho, the IRLS weight w
// and its square root sw of one factor.  One source for the device (pgs_kernel.hip: linearisation, evaluation, cost, pgs_factor_weights_kernel)
// and the host (pgs_robust_loss_host, the TEST HOOK of slam_pgs.h).  DESIGN.md 4.4 "Robust loss".
//
// With e the whitened residual of a factor, ss = e0^2 + e1^2 and r = sqrt(ss):
//   kPgsLossNone            rho = 0.5 ss                                       w = 1                         sw = 1
//   kPgsLossHuber, k        rho = 0.5 ss (r <= k), k (r - 0.5 k) (r > k)       w = 1, k / r                  sw = 1, sqrt(k / r)
//   kPgsLossGemanMcClure, k rho = 0.5 k^2 (ss / (k^2 + ss))                    w = (k^2 / (k^2 + ss))^2      sw = k^2 / (k^2 + ss)
// Only + - * / and sqrt: correctly rounded on both sides, so device and host agree bit for bit (-ffp-contract=off).  The inlier branch of
// Huber takes 0.5 ss, not 0.5 r r: a Huber loss whose k no residual reaches gives the bits of the Gaussian cost.  A NaN in e gives NaN in
// all three (r <= k is false, k / NaN is NaN).  The linearised factor is sw e, sw J (weight taken at the linearisation point).
#pragma once
#include "slam_math.h"

namespace slam {

enum { kPgsLossNone = 0, kPgsLossHuber = 1, kPgsLossGemanMcClure = 2 };   // = pgs_loss_kind (slam_pgs.h)

SLAM_HD void pgs_robust_loss(int kind, double k, double ss, double r, double* rho, double* w, double* sw) {
    if (kind == kPgsLossHuber) {
        if (r <= k) { *rho = 0.5 * ss; *w = 1.0; *sw = 1.0; }
        else { const double q = k / r; *rho = k * (r - 0.5 * k); *w = q; *sw = sqrt(q); }
    } else if (kind == kPgsLossGemanMcClure) {
        const double k2 = k * k, s = k2 + ss, q = k2 / s;
        *rho = (0.5 * k2) * (ss / s); *w = q * q; *sw = q;
    } else {
        *rho = 0.5 * ss; *w = 1.0; *sw = 1.0;
    }
}

}  // namespace slam
