"""Absolute fixes of the pose graph, the parts that need no device: the fix factor compiled for the host (pgs_fix_factor_host, the kernels'
source csrc/pgs_fix.h) against the reference (tests/pgs_fix_reference.py), a finite difference through the oracle's retraction and mpmath;
the verdict table; the argument checks that come before the handle; the reference itself; and the effect inputs the GPU test reuses."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import pgs_fix_reference as F
import pgs_robust_reference as RR
import pgs_step_reference as R
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.pose_graph import fix_factor_host

PI = 3.14159265358979323846
# e of a part is at most three correctly rounded operations from its inputs (a subtraction, 1 / sigma, a product; the remainder is exact):
# |e - exact| <= E_BOUND u max(|d|, |r|) / sigma with d the difference before the wrap and r after it.  (The subtraction's error is relative to
# d, not to r: next to a wrap r may be far smaller than d, so the bound is stated on that scale and not in ulps of e.)
E_BOUND = 3
# J's entries are cos / sin of the yaw (det_sincos, below 1 ulp: slam_math.h) times 1 / sigma (0.5 ulp), one product (0.5 ulp)
J_ULP_BOUND = 3
LOSS_ULP_BOUND = 4     # test_pgs_robust_cpu.py's bound of the loss function, fed r = |e| exactly here


def _mp():
    import mpmath as mp
    mp.mp.dps = 50
    return mp


def _wrap_exact(d):
    """remainder(d, kTwoPi) of an mpmath d, the IEEE rule (nearest multiple, ties to the even quotient)."""
    mp = _mp()
    T = mp.mpf(R.TWO_PI)
    q = mp.floor(d / T + mp.mpf(1) / 2)
    if d / T + mp.mpf(1) / 2 == q and int(q) % 2:      # a tie: the even quotient
        q -= 1
    return d - q * T


POSES = [(0.3, -1.2, 0.7), (-4.0, 2.5, -3.0), (10.25, 0.0, PI), (0.0, 0.0, -PI), (1e-3, 1e3, 1.5707963267948966)]
ROWS = [(0.25, -1.0, 0.5, 0.1, 0.05), (3.0, -2.0, 3.1, 2.0, 0.3), (-7.5, 0.125, -3.0, 0.01, 1.0)]
# heading residuals next to +-pi: the difference is exact (z_yaw = 0, or both multiples of 2^-40) so the wrap is the only event
NEAR_PI = [(th, 0.0) for th in (PI, np.nextafter(PI, 4.0), np.nextafter(PI, 0.0), -PI, np.nextafter(-PI, -4.0), np.nextafter(-PI, 0.0))]
NEAR_PI += [(3.0, 3.0 - round(PI * 2 ** 40) / 2 ** 40), (3.0, 3.0 - (round(PI * 2 ** 40) + 1) / 2 ** 40), (-3.0, -3.0 + (round(PI * 2 ** 40) + 1) / 2 ** 40)]


def test_the_host_factor_against_the_reference_and_mpmath():
    mp = _mp()
    worst_e = worst_J = 0.0
    cases = [(p, r) for p in POSES for r in ROWS] + [((0.5, 0.5, th), (0.0, 0.0, z, 1.0, 0.7)) for th, z in NEAR_PI]
    for pose, row in cases:
        got = fix_factor_host(pose, row, F.POS | F.YAW)
        assert got["verdict"] == (F.STORED | F.STORED << 4)
        ref = F.fix_parts(pose, row, F.POS | F.YAW)
        e_ref = np.r_[ref[0][1], ref[1][1]]
        J_ref = np.vstack([ref[0][2], ref[1][2]])
        # the residual: the reference performs the same IEEE operations, so the bits agree
        assert np.array_equal(got["e"], e_ref), (pose, row, got["e"], e_ref)
        x, y, th = (mp.mpf(v) for v in pose)
        zx, zy, zyaw, sp, sy = (mp.mpf(v) for v in row)
        d = [x - zx, y - zy, th - zyaw]
        r = [d[0], d[1], _wrap_exact(d[2])]
        exact = [r[0] / sp, r[1] / sp, r[2] / sy]
        for a in range(3):
            scale = max(abs(d[a]), abs(r[a])) / (sp if a < 2 else sy)
            err = abs(mp.mpf(float(got["e"][a])) - exact[a])
            if scale > 0:
                worst_e = max(worst_e, float(err / (mp.mpf(R.U) * scale)))
            assert err <= E_BOUND * R.U * scale, (pose, row, a, float(got["e"][a]), float(exact[a]))
        # the Jacobian: cos / sin by det_sincos on the device side, libm in the reference
        Jx = np.array([[float(mp.cos(th) / sp), float(-mp.sin(th) / sp), 0.0], [float(mp.sin(th) / sp), float(mp.cos(th) / sp), 0.0], [0.0, 0.0, float(1 / sy)]])
        for a in range(3):
            for c in range(3):
                if Jx[a, c] == 0.0 and (a == 2 or c == 2):
                    assert got["J"][a, c] == 0.0
                    continue
                ulps = abs(got["J"][a, c] - Jx[a, c]) / np.spacing(abs(Jx[a, c]))
                worst_J = max(worst_J, float(ulps))
                # (next to a zero of sin / cos one ulp of the ARGUMENT is many ulps of the value: an absolute floor of u / sigma)
                assert ulps <= J_ULP_BOUND or abs(got["J"][a, c] - Jx[a, c]) <= 2 * R.U / row[3], (pose, row, a, c, got["J"][a, c], Jx[a, c])
        assert np.all(np.abs(got["J"] - J_ref) <= 4 * R.U * np.abs(J_ref).max()), (pose, row)
        assert np.all(got["w"] == 1.0) and np.allclose(got["rho"], [0.5 * (e_ref[0] ** 2 + e_ref[1] ** 2), 0.5 * e_ref[2] ** 2], rtol=4 * R.U, atol=0)
    print(f"largest error of e: {worst_e:.2f} u max(|d|, |r|) / sigma (bound {E_BOUND}); of J: {worst_J:.2f} ulp (bound {J_ULP_BOUND})")


def test_the_wrap_takes_the_ieee_side_next_to_pi():
    for th, z in NEAR_PI:
        e = fix_factor_host((0.0, 0.0, th), (0.0, 0.0, z, 1.0, 1.0), F.YAW)["e"][2]
        assert e == math.remainder(th - z, R.TWO_PI) and abs(e) <= PI, (th, z, e)
    assert fix_factor_host((0.0, 0.0, PI), (0.0, 0.0, 0.0, 1.0, 1.0), F.YAW)["e"][2] == PI               # the tie stays (even quotient 0)
    assert fix_factor_host((0.0, 0.0, np.nextafter(PI, 4.0)), (0.0, 0.0, 0.0, 1.0, 1.0), F.YAW)["e"][2] < 0   # one ulp further wraps


def test_the_jacobian_against_a_central_difference_through_the_oracles_retraction():
    g = F.case("n2")["graphs"][0]
    h = 1e-6
    for pose in POSES:
        for row in ROWS:
            J = fix_factor_host(pose, row, F.POS | F.YAW)["J"]
            base = np.array([pose, pose], dtype=np.float64)
            for a in range(3):
                dp = np.zeros((2, 3)); dp[0, a] = h
                ep = fix_factor_host(g.retract(base, np.zeros(0), dp, np.zeros(0))[0][0], row, F.POS | F.YAW)["e"]
                em = fix_factor_host(g.retract(base, np.zeros(0), -dp, np.zeros(0))[0][0], row, F.POS | F.YAW)["e"]
                fd = (ep - em) / (2 * h)
                # e is linear in the translation and piecewise linear in the yaw: the difference quotient carries rounding only,
                # about u |e| / h, and the truncation of cos / sin of the retracted yaw's effect on nothing (x, y do not depend on it)
                tol = 1e-9 * max(1.0, float(np.abs(ep).max())) / min(row[3], row[4]) + 1e-9 * np.abs(J[:, a]).max()
                assert np.all(np.abs(fd - J[:, a]) <= tol), (pose, row, a, fd, J[:, a])


@pytest.mark.parametrize("kind,k", [(F.HUBER, 1.345), (F.GEMAN_MCCLURE, 3.0)])
def test_the_fix_loss_next_to_k_against_mpmath(kind, k):
    """r next to k: a position part with sigma 1 and z = 0 at (r, 0) has e = (r, 0) exactly, and sqrt(fl(r^2)) = r."""
    import test_pgs_robust_cpu as TR
    worst = 0.0
    for r in (k * (1 - 2.0 ** -52), k, k * (1 + 2.0 ** -52), 0.5 * k, 2.0 * k):
        got = fix_factor_host((r, 0.0, 0.3), (0.0, 0.0, 0.0, 1.0, 1.0), F.POS, kind, k)
        assert got["e"][0] == r and got["e"][1] == 0.0 and np.isnan(got["w"][1]) and np.isnan(got["rho"][1])
        rho, w, _ = TR._exact(kind, k, r)
        for name, gv, x in (("rho", got["rho"][0], rho), ("w", got["w"][0], w)):
            d = TR._ulps(gv, x)
            worst = max(worst, d)
            assert d <= LOSS_ULP_BOUND, (kind, k, r, name, gv, float(x), d)
        if r <= PI:   # and the heading part with the same norm (no wrap): e = yaw
            gy = fix_factor_host((0.0, 0.0, r), (0.0, 0.0, 0.0, 1.0, 1.0), F.YAW, kind, k)
            assert gy["e"][2] == r and gy["rho"][1] == got["rho"][0] and gy["w"][1] == got["w"][0]
    print(f"kind {kind}: largest error {worst:.2f} ulp")


def test_the_verdict_table():
    nan, inf = float("nan"), float("inf")
    good = [1.0, 2.0, 0.5, 0.1, 0.05]
    pose = (0.0, 0.0, 0.0)

    def v(row, kinds):
        got = fix_factor_host(pose, row, kinds)["verdict"]
        assert got == F.verdict(row, kinds), (row, kinds, got)
        return got & 15, got >> 4
    assert v(good, 0) == (0, 0) and v(good, F.POS) == (1, 0) and v(good, F.YAW) == (0, 1) and v(good, 3) == (1, 1)
    assert v(good, 4 | F.POS) == (1, 0)                                  # other bits are ignored
    for bad in (nan, inf, -inf):
        for idx in (0, 1, 3):                                            # a z or the sigma of the position part
            row = list(good); row[idx] = bad
            assert v(row, 3) == (4, 1), (idx, bad)
        for idx in (2, 4):                                               # ... of the heading part
            row = list(good); row[idx] = bad
            assert v(row, 3) == (1, 4), (idx, bad)
    for s in (0.0, -0.0, -1.0):                                          # sigma = 0 is INVALID here (an infinite weight), unlike the EKF
        row = list(good); row[3] = s
        assert v(row, 3) == (4, 1), s
        row = list(good); row[4] = s
        assert v(row, 3) == (1, 4), s
    row = [nan, nan, 0.5, nan, 0.05]                                     # a part that is absent is not looked at
    assert v(row, F.YAW) == (0, 1)
    # an INVALID part contributes nothing and leaves NaN weights
    got = fix_factor_host(pose, [1.0, 2.0, 0.5, 0.0, 0.05], 3)
    assert np.all(got["e"][:2] == 0) and np.all(got["J"][:2] == 0) and np.isnan(got["w"][0]) and got["w"][1] == 1.0


def test_argument_errors_that_come_before_the_handle():
    L = _lib.lib()
    err = lambda: L.slam_last_error().decode()   # noqa: E731
    d5, i1, f2 = (C.c_double * 5)(), (C.c_int32 * 1)(), (C.c_float * 2)()
    for kind, k in ((3, 1.0), (-1, 1.0), (1, float("nan")), (1, 0.0), (1, -1.0), (1, float("inf")), (2, 0.0)):
        assert L.pgs_set_fix_robust(None, kind, k) == -1 and "kind" in err() and "NULL handle" not in err(), (kind, k, err())
    assert L.pgs_set_fix_robust(None, 1, 1.345) == -1 and "NULL handle" in err()
    assert L.pgs_fix(None, None, i1, None) == -1 and "fix is NULL" in err()
    assert L.pgs_fix(None, d5, None, None) == -1 and "kinds is NULL" in err()
    assert L.pgs_fix(None, d5, i1, None) == -1 and "NULL handle" in err()
    assert L.pgs_fix_dev(None, None, None, None) == -1 and "d_fix is NULL" in err()
    assert L.pgs_fix_sense(None, None, i1, None) == -1 and "fix is NULL" in err()
    assert L.pgs_fix_sense(None, d5, i1, None) == -1 and "NULL handle" in err()
    assert L.pgs_run_sim_fix(None, None, 3, 0, 1) == -1 and "command" in err()
    assert L.pgs_run_sim_fix(None, f2, 0, 0, 1) == -1 and "command" in err()
    assert L.pgs_run_sim_fix(None, f2, 1, 0, 0) == -1 and "fix_every" in err()
    assert L.pgs_run_sim_fix(None, f2, 1, 2, 1) == -1 and "each" in err()
    assert L.pgs_run_sim_fix(None, f2, 1, 0, 1) == -1 and "NULL handle" in err()
    assert L.pgs_fix_weights(None, 2) == -1 and "which" in err()
    assert L.pgs_get_fix_robust(None, None, None) == -1 and "NULL handle" in err()
    with pytest.raises(_lib.SlamError):
        fix_factor_host((0, 0, 0), (0, 0, 0, 1, 1), 3, 5, 1.0)
    with pytest.raises(_lib.SlamError):
        fix_factor_host((0, 0, 0), (0, 0, 0, 1, 1), 3, F.HUBER, 0.0)


@pytest.mark.parametrize("kind,k", [(RR.NONE, 0.0), (RR.HUBER, 1.345), (RR.GEMAN_MCCLURE, 3.0)])
def test_without_fix_rows_the_reference_is_the_robust_reference_byte_for_byte(kind, k):
    sc = RR.case("n9")
    N = sc["N"]
    for g in sc["graphs"]:
        v = g.values(0)
        fg = F.FixGraph(g, np.zeros((N, 5)), np.zeros(N, dtype=int), fix_loss=(F.GEMAN_MCCLURE, 3.0), lm_loss=(kind, k))
        W, L = fg.weigh(v["poses"], v["landmarks"]), RR.weigh(g, v["poses"], v["landmarks"], kind, k)
        for key in ("rows", "cols", "vals", "e"):
            assert W[key].dtype == L[key].dtype and W[key].tobytes() == L[key].tobytes(), key
        a, b = F.lm_solve(fg), RR.lm_solve(g, kind, k)
        assert a["poses"].tobytes() == b["poses"].tobytes() and a["landmarks"].tobytes() == b["landmarks"].tobytes()
        assert {q: a[q] for q in a if q not in ("poses", "landmarks")} == {q: b[q] for q in b if q not in ("poses", "landmarks")}


def test_the_system_with_fix_rows_is_the_dense_product():
    sc = F.case("n9")
    fix, kinds = F.place_fixes(sc, "default")
    g = sc["graphs"][1]
    v = g.values(0)
    fg = F.FixGraph(g, fix[1], kinds[1], fix_loss=(F.HUBER, 1.345))
    S, W = F.system(fg, v["poses"], v["landmarks"], 1e-5)
    rows, cols, vals, e = g.jacobian(v["poses"], v["landmarks"])
    n_fix_rows = sum(2 * bool(k & 1) + bool(k & 2) for k in kinds[1])
    assert n_fix_rows > 0 and len(W["e"]) == len(e) + n_fix_rows
    J = np.zeros((len(W["e"]), S.n))
    J[W["rows"], W["cols"]] = W["vals"]
    A = J.T @ J + 1e-5 * np.eye(S.n)
    assert np.all(np.abs(S.A - A) <= 8 * R.U * (np.abs(J).T @ np.abs(J) + 1e-5 * np.eye(S.n)))
    # the fix rows touch their own pose's block only
    Jg = np.zeros((len(e), S.n)); Jg[rows, cols] = vals
    D = A - (Jg.T @ Jg + 1e-5 * np.eye(S.n))
    mask = np.zeros_like(D, dtype=bool)
    for i in np.flatnonzero(kinds[1]):
        mask[3 * i:3 * i + 3, 3 * i:3 * i + 3] = True
    assert np.all(np.abs(D[~mask]) <= 1e-12 * np.abs(A).max()) and np.abs(D[mask]).max() > 1.0


def test_a_tight_position_fix_pins_the_pose():
    sc = F.case("n9")
    g, N = sc["graphs"][2], sc["N"]
    fix, kinds = np.zeros((N, 5)), np.zeros(N, dtype=int)
    target = np.array([0.4321, -0.1234])
    fix[4] = (target[0], target[1], 0.0, 1e-6, 0.0)
    kinds[4] = F.POS
    r = F.lm_solve(F.FixGraph(g, fix, kinds))
    assert r["flags"] == 0
    free = RR.lm_solve(g, RR.NONE, 0.0)
    assert np.abs(free["poses"][4, :2] - target).max() > 0.05       # without the fix the pose is elsewhere
    assert np.abs(r["poses"][4, :2] - target).max() < 1e-8, r["poses"][4]


@functools.lru_cache(maxsize=None)
def effect_reference():
    """The Python LM on the effect inputs, per instance: (no fixes, clean fixes, jumps + Gaussian, jumps + Geman-McClure, its weights)."""
    ec = F.effect_case()
    N = ec["N"]
    out = []
    for b, g in enumerate(ec["graphs"]):
        none = F.lm_solve(F.FixGraph(g, np.zeros((N, 5)), np.zeros(N, dtype=int)))
        clean = F.lm_solve(F.FixGraph(g, ec["fix"][b], ec["kinds"][b]))
        gauss = F.lm_solve(F.FixGraph(g, ec["fix_jump"][b], ec["kinds"][b]))
        fgm = F.FixGraph(g, ec["fix_jump"][b], ec["kinds"][b], fix_loss=(F.GEMAN_MCCLURE, F.EFFECT_GM_K))
        gm = F.lm_solve(fgm)
        out.append(dict(none=none, clean=clean, gauss=gauss, gm=gm, w=fgm.weigh(gm["poses"], gm["landmarks"])["fix_w"]))
    return out


def test_the_effect_inputs_show_what_fixes_are_for():
    """Conditions (a) - (c) of the GPU test, on the Python LM alone.  Every fix row of the inputs is judged: none is excluded."""
    ec, ref = F.effect_case(), effect_reference()
    truth = ec["st"]["truth"]
    assert np.all(ec["kinds"][:, 1:] == F.POS) and ec["jumped"].sum(axis=1).min() >= 4
    for b, r in enumerate(ref):
        assert all(r[q]["flags"] == 0 for q in ("none", "clean", "gauss", "gm")), b
        e_none, e_fix = F.position_error(r["none"]["poses"], truth), F.position_error(r["clean"]["poses"], truth)
        d_gauss = float(np.abs(r["gauss"]["poses"][:, :2] - r["clean"]["poses"][:, :2]).max())
        d_gm = float(np.abs(r["gm"]["poses"][:, :2] - r["clean"]["poses"][:, :2]).max())
        w, j, stored = r["w"][:, 0], ec["jumped"][b], ec["kinds"][b] > 0
        print(f"effect[{b}]: mean position error {e_none:.4f} m without fixes, {e_fix:.4f} m with; with jumps the result is {d_gauss:.4f} m (Gaussian) / "
              f"{d_gm:.4f} m (Geman-McClure) from the clean-fix result; w of jumped parts <= {w[j & stored].max():.3g}, of clean parts >= {w[~j & stored].min():.3g}")
        assert e_fix < e_none, (b, e_fix, e_none)                                                    # (a)
        assert d_gm < d_gauss, (b, d_gm, d_gauss)                                                    # (b)
        assert np.all(w[j & stored] < 0.5) and np.all(w[~j & stored] >= 0.5), (b, w)                 # (c)
        assert np.isnan(w[~stored]).all()
