// ekf_model.h — the algebra of one EKF-SLAM step (EKF::update, reference ekf_ws/src/localization_pkg/src/ekf.cpp:37-179), defined ONCE.
//
// Every EKF kernel promises the oracle's bits, so every piece of device code that evaluates a part of the step must use the same IEEE
// operations in the same order.  The expressions live here, each in one function; the fused step kernel (ekf_step_*.h), the streamed
// size class (ekf_big_kernel.hip) and the innovation / gate replay (innovation_kernel.h, device and host) call them and keep only what
// is theirs: the parallel decomposition, where the operands live, barriers and flags.  OPERATION ORDER IS THE CONTRACT: a parenthesis
// moved here moves it everywhere, and tests/test_ekf_model_cpu.py checks a dense step written with these calls alone against the oracle
// (oracle/slam_oracle.cpp, which does NOT include this header: it is the independent statement) in bits, without a GPU.
//
// Scalars in, small structs out, no pointers and no kernel state; plain g++ and hipcc, -ffp-contract=off on both sides.
#pragma once
#include "slam_math.h"

namespace slam {

struct EkfVec2 { double x, y; };   // two rows of one column (H P) or two columns of one row (P H^T, K)

// ---- prediction -------------------------------------------------------------------------------------------------------------------
// Motion scalars (ekf.cpp:41-59): x_pred of the vehicle with the float add of :57, F_x(0,2), F_x(1,2) and F_v V F_v^T.
struct EkfMotion { double xp0, xp1, xp2, fa, fb, q00, q01, q10, q11; };   // x_pred[0 .. 2]; F_x(0,2), F_x(1,2); F_v V F_v^T (its (2,2) entry is V11)
SLAM_HD EkfMotion ekf_motion(double x0, double x1, double th, float fwd, float ang, float v_d, float v_th, double V00) {
    double sn, cs;
    det_sincos(th, &sn, &cs);
    const float dd = fwd + v_d;            // float add, ekf.cpp:57
    const double cv = cs * V00, sv = sn * V00;
    return EkfMotion{x0 + (double)dd * cs, x1 + (double)dd * sn, rem2pi((th + (double)ang) + (double)v_th),   // ekf.cpp:56-59
                     (double)(-1 * fwd) * sn, (double)fwd * cs,                                               // ekf.cpp:48-49
                     cv * cs, cv * sn, sv * cs, sv * sn};
}

// P_pred = F_x P F_x^T + F_v V F_v^T (ekf.cpp:61) with the sparse F_x: the two terms an element can take ...
SLAM_HD double ekf_pred_row(double t, double f_r, double p2c) { return t + f_r * p2c; }   // (F_x P)[r][c], r < 2: + F_x(r,2) P[2][c]
SLAM_HD double ekf_pred_col(double t, double a2, double f_c) { return t + a2 * f_c; }     // (. F_x^T)[r][c], c < 2: + (F_x P)[r][2] F_x(c,2)
// ... and one element (r, c) from t = P[r][c].  p2c = P[2][c] (read for r < 2), pr2 = P[r][2] (c < 2), p22 = P[2][2], q_rc = (F_v V F_v^T)[r][c]
// (r, c < 2); an operand the element does not take is not looked at.
SLAM_HD double ekf_predicted(double t, int r, int c, double p2c, double pr2, double p22, double fa, double fb, double q_rc, double V11) {
    const double f_r = r == 0 ? fa : fb;
    if (r < 2) t = ekf_pred_row(t, f_r, p2c);              // rows 0, 1 of F_x P
    if (c < 2) {                                           // cols 0, 1 of (F_x P) F_x^T
        double a2 = pr2;
        if (r < 2) a2 = ekf_pred_row(a2, f_r, p22);       // a2 + f_r * p22
        t = ekf_pred_col(t, a2, c == 0 ? fa : fb);
    }
    if (r < 2 && c < 2) t = t + q_rc;                      // + F_v V F_v^T
    if (r == 2 && c == 2) t = t + V11;
    return t;
}

// ---- landmark update, ekf.cpp:110-140 ------------------------------------------------------------------------------------------------
// Offset and range of a landmark with the float truncations of ekf.cpp:115: dist is a float, dist * dist a float product.
struct EkfRange { double dx, dy, dd, d2; float dist; };
SLAM_HD EkfRange ekf_range(double lx, double ly, double xp0, double xp1) {
    const double dx = lx - xp0, dy = ly - xp1;
    const float dist = (float)sqrt(dx * dx + dy * dy);
    return EkfRange{dx, dy, (double)dist, (double)(dist * dist), dist};
}

// Entry j of H = {H00, H01, H0i, H0i+1, H10, H11, H1i, H1i+1} (ekf.cpp:117-128; H02 = 0, H12 = -1): the fused kernel evaluates the eight
// quotients on eight lanes (j = lane), the serial callers with constant j through ekf_jacobian.
SLAM_HD double ekf_h_entry(int j, double dx, double dy, double dd, double d2) {
    const bool usey = (j == 1) || (j == 3) || (j == 4) || (j == 6);
    const bool neg = (j == 0) || (j == 1) || (j == 5) || (j == 6);
    double num = usey ? dy : dx;
    num = neg ? -num : num;
    return num / (j < 4 ? dd : d2);
}
struct EkfH { double h00, h01, h03, h04, h10, h11, h13, h14; };   // columns 0, 1, i, i + 1 of the two rows
SLAM_HD EkfH ekf_jacobian(double dx, double dy, double dd, double d2) {
    return EkfH{ekf_h_entry(0, dx, dy, dd, d2), ekf_h_entry(1, dx, dy, dd, d2), ekf_h_entry(2, dx, dy, dd, d2), ekf_h_entry(3, dx, dy, dd, d2),
                ekf_h_entry(4, dx, dy, dd, d2), ekf_h_entry(5, dx, dy, dd, d2), ekf_h_entry(6, dx, dy, dd, d2), ekf_h_entry(7, dx, dy, dd, d2)};
}

// Innovation (ekf.cpp:129-131): the bearing wrapped and truncated to float, both differences in float arithmetic.  In two halves: the
// predicted bearing depends on the landmark and the pose alone, the differences on the detection (the association forms the first once
// per landmark, assoc_kernel.h).
SLAM_HD float ekf_predicted_bearing(double dx, double dy, double xp2) { return (float)rem2pi(det_atan2(dy, dx) - xp2); }
SLAM_HD EkfVec2 ekf_innovation_from(float r_m, float b_m, float dist, float angf, float w_r, float w_b) {
    const float nu0f = r_m - dist - w_r;
    const float nu1f = b_m - angf - w_b;
    return EkfVec2{(double)nu0f, (double)nu1f};
}
SLAM_HD EkfVec2 ekf_innovation(float r_m, float b_m, float dist, double dx, double dy, double xp2, float w_r, float w_b) {
    return ekf_innovation_from(r_m, b_m, dist, ekf_predicted_bearing(dx, dy, xp2), w_r, w_b);
}

// Column c of H P from P[0][c], P[1][c], P[2][c], P[i][c], P[i+1][c] (ekf.cpp:133; H02 == 0 is skipped, H12 = -1)
SLAM_HD EkfVec2 ekf_hp_col(const EkfH h, double p0, double p1, double p2, double pi, double pj) {
    const double h12 = -1.0;
    return EkfVec2{((h.h00 * p0 + h.h01 * p1) + h.h03 * pi) + h.h04 * pj, (((h.h10 * p0 + h.h11 * p1) + h12 * p2) + h.h13 * pi) + h.h14 * pj};
}
// Row r of P H^T from P[r][0], P[r][1], P[r][2], P[r][i], P[r][i+1] (ekf.cpp:135); S = (H P) H^T takes its rows the same way
SLAM_HD EkfVec2 ekf_pht_row(const EkfH h, double q0, double q1, double q2, double qi, double qj) {
    const double h12 = -1.0;
    return EkfVec2{((q0 * h.h00 + q1 * h.h01) + qi * h.h03) + qj * h.h04, (((q0 * h.h10 + q1 * h.h11) + q2 * h12) + qi * h.h13) + qj * h.h14};
}
// S = (H P) H^T + W (ekf.cpp:133), row-major, from the columns 0, 1, 2, i, i + 1 of H P
struct EkfS { double s[4]; };
SLAM_HD EkfS ekf_S(const EkfH h, EkfVec2 g0, EkfVec2 g1, EkfVec2 g2, EkfVec2 gi, EkfVec2 gj, double W00, double W11) {
    const EkfVec2 r0 = ekf_pht_row(h, g0.x, g1.x, g2.x, gi.x, gj.x);
    const EkfVec2 r1 = ekf_pht_row(h, g0.y, g1.y, g2.y, gi.y, gj.y);
    return EkfS{{r0.x + W00, r0.y, r1.x, r1.y + W11}};
}
// Row r of K = (P H^T) S^-1 (ekf.cpp:135), Si = inv2x2_lu(S) row-major
SLAM_HD EkfVec2 ekf_gain(EkfVec2 ph, double si0, double si1, double si2, double si3) { return EkfVec2{ph.x * si0 + ph.y * si2, ph.x * si1 + ph.y * si3}; }
// x_pred[r] += K[r] nu (ekf.cpp:138), index 2 wrapped (ekf.cpp:139)
SLAM_HD double ekf_state_update(double x, int r, double k0, double k1, double nu0, double nu1) {
    double xv = x + (k0 * nu0 + k1 * nu1);
    if (r == 2) xv = rem2pi(xv);
    return xv;
}
// One element of P_pred -= K (H P) (ekf.cpp:140, the rank-2 form): P[r][c] with K[r][0 .. 1] and (H P)[0 .. 1][c]
SLAM_HD double ekf_downdate(double p, double k0, double k1, double h0, double h1) { return p - (k0 * h0 + k1 * h1); }

// ---- the same update for a scalar measurement of one state entry (fix_kernel.h: a heading fix; H is a unit row, so P H^T is a column
// of P and H P a row; si = 1 / S) ----
SLAM_HD double ekf_gain1(double ph, double si) { return ph * si; }
SLAM_HD double ekf_state_update1(double x, int r, double k, double nu) {
    double xv = x + k * nu;
    if (r == 2) xv = rem2pi(xv);
    return xv;
}
SLAM_HD double ekf_downdate1(double p, double k, double h) { return p - k * h; }

// ---- landmark insertion, ekf.cpp:141-173 ---------------------------------------------------------------------------------------------
// G_x(0,2) = G_z(0,1), G_x(1,2) = G_z(1,1), cos and sin of the bearing in the world frame (G_z's first column), the new landmark's position
struct EkfInsert { double g02, g12, c, s, lx, ly; };
SLAM_HD EkfInsert ekf_insert_geom(double xp0, double xp1, double xp2, float r_m, float b_m) {
    const double phi = xp2 + (double)b_m, rd = (double)r_m;
    double s, c;
    det_sincos(phi, &s, &c);
    return EkfInsert{-rd * s, rd * c, c, s, xp0 + rd * c, xp1 + rd * s};
}
SLAM_HD double ekf_insert_row(double p_ac, double g, double p_2c) { return p_ac + g * p_2c; }   // (G_x P[0:3, :])[a][c] = P[a][c] + G_x(a,2) P[2][c]
SLAM_HD double ekf_insert_col(double p_ra, double p_r2, double g) { return p_ra + p_r2 * g; }   // (P[:, 0:3] G_x^T)[r][a] = P[r][a] + P[r][2] G_x(a,2)
// The 2 x 2 corner (G_x P_vv) G_x^T + (G_z W) G_z^T from the entries 0 .. 2 of the two new rows
struct EkfCorner { double v00, v01, v10, v11; };
SLAM_HD EkfCorner ekf_insert_corner(double ra0, double ra1, double ra2, double rb0, double rb1, double rb2, double g02, double g12, double c,
                                    double s, double W00, double W11) {
    const double gw00 = c * W00, gw01 = g02 * W11;   // (G_z W) row 0
    const double gw10 = s * W00, gw11 = g12 * W11;   // (G_z W) row 1
    return EkfCorner{((ra0 + ra2 * g02) + gw00 * c) + gw01 * g02, ((ra1 + ra2 * g12) + gw00 * s) + gw01 * g12,
                     ((rb0 + rb2 * g02) + gw10 * c) + gw11 * g02, ((rb1 + rb2 * g12) + gw10 * s) + gw11 * g12};
}

// ---- the per-step position error (plotting_node.py:209-212) with the float32 wire format of EKFState.x_v / y_v ---------------------
SLAM_HD double ekf_position_error(double xp0, double xp1, double true_x, double true_y) {
    const double ex = (double)(float)xp0 - true_x, ey = (double)(float)xp1 - true_y;
    return sqrt(ex * ex + ey * ey);
}

}  // namespace slam
