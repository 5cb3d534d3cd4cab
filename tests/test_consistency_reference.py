"""The host reference of slam_consistency (tests/consistency_reference.py) is itself checked: its longdouble NEES against mpmath at 50
digits, its flags on states of the CPU oracle and on matrices built to have one negative pivot, and consistency_summary's chi-square
interval against exact quantiles."""
import numpy as np
import pytest

import consistency_reference as R
from test_cholesky_highprec import _mpf, spd_graded, spd_with_condition


def _nees_mp(S, e, dps=50):
    import mpmath
    with mpmath.workdps(dps):
        L = mpmath.cholesky(mpmath.matrix(S.tolist()))
        n = S.shape[0]
        y = [mpmath.mpf(0)] * n
        for i in range(n):
            y[i] = (mpmath.mpf(float(e[i])) - mpmath.fsum(L[i, j] * y[j] for j in range(i))) / L[i, i]
        return mpmath.fsum(v * v for v in y)


@pytest.mark.parametrize("n", [3, 43, 103])
def test_longdouble_nees_is_a_reference_for_fp64(n):
    """Its error against 50 digits is below 1/100 of the error of the fp64 routes on the same input."""
    import mpmath
    rng = np.random.default_rng(500 + n)
    for kind in ("k1e1", "k1e4", "k1e8", "graded"):
        S = spd_graded(rng, n) if kind == "graded" else spd_with_condition(rng, n, float(kind[1:]))
        e = rng.standard_normal(n) * np.sqrt(np.diag(S))
        with mpmath.workdps(50):
            exact = _nees_mp(S, e)
            err_hp = abs(_mpf(R.nees_hp(S, e)) - exact) / exact
            err_d = max(abs(mpmath.mpf(r) - exact) / exact for r in R.nees_double_routes(S, e))
            print(f"n={n} {kind}: longdouble {float(err_hp):.3g}, fp64 routes {float(err_d):.3g}")
            assert err_hp * 100 <= err_d, (n, kind, float(err_hp), float(err_d))


@pytest.mark.parametrize("L,T", [(20, 400), (50, 300)])
def test_reference_on_oracle_states(oracle, L, T):
    """States of the CPU oracle: S is positive definite, no flag, every number finite and positive."""
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, T)
    B = 6
    for quirk in (1, 0):
        cfg = oracle.default_config()
        cfg.replicate_vw_quirk = quirk
        out = oracle.run_ekf_batch(lm, cmds, B, L, seed=2025, cfg=cfg)
        for b in range(B):
            M = int(out["M"][b]); n = 3 + 2 * M
            P = out["P"][b][:n * n].reshape(n, n)   # (the oracle packs n x n)
            r = R.reference(out["x"][b], P, M, out["ids"][b], out["truth"][b], lm, int(out["flags"][b]))
            assert r["flags"] == 0 and r["dof"] == n and M > 0
            for k in ("nees_full", "nees_pose", "map_rms"):
                assert np.isfinite(float(r[k])) and r[k] > 0, (b, k, r[k])
            assert r["nees_pose"] <= r["nees_full"]   # a marginal's NEES never exceeds the joint's


@pytest.mark.parametrize("n", [43, 103])
def test_not_pd_rule(n):
    rng = np.random.default_rng(n)
    for k in (0, 2, 3, n // 2, n - 1):
        S = R.not_pd_matrix(rng, n, k)
        assert np.array_equal(S, S.T) and 0.1 < np.linalg.norm(S, 2) < 10
        M = (n - 3) // 2
        x = np.concatenate([[0.1, 0.2, 0.3], rng.uniform(-1, 1, 2 * M)])
        r = R.reference(x, S, M, np.arange(M), np.zeros(3), np.zeros((M, 2)))
        assert r["flags"] == (R.FULL_NOT_PD | (R.POSE_NOT_PD if k < 3 else 0)), (k, r["flags"])
        assert np.isnan(float(r["nees_full"])) and np.isnan(float(r["nees_pose"])) == (k < 3) and np.isfinite(float(r["map_rms"]))


def test_flags_of_the_other_kinds():
    rng = np.random.default_rng(9)
    S = spd_with_condition(rng, 7, 1e2)
    x = rng.standard_normal(7); ids = np.array([1, 0]); m = rng.standard_normal((2, 2)); t = np.zeros(3)
    assert R.reference(x, S, 2, ids, t, m)["flags"] == 0
    for st in (R.NONFINITE, R.WATCHDOG, R.NONFINITE | 8):
        r = R.reference(x, S, 2, ids, t, m, status=st)
        assert r["flags"] == R.INSTANCE_FAILED and r["dof"] == 7 and np.isnan(float(r["nees_pose"]))
    assert R.reference(x, S, 2, ids, t, m, status=2 | 4 | 8 | 16)["flags"] == 0   # a frozen or truncated state is still a state
    for bad_ids in ([1, 2], [-1, 0]):
        r = R.reference(x, S, 2, np.array(bad_ids), t, m)
        assert r["flags"] == R.NO_TRUTH and np.isnan(float(r["nees_full"])) and np.isnan(float(r["map_rms"])) and r["nees_pose"] > 0
    r = R.reference(x, S, 2, ids, t, m, id_known=False)
    assert r["flags"] == R.NO_TRUTH and r["nees_pose"] > 0
    assert R.reference(x[:3], S[:3, :3], 0, ids[:0], t, m, id_known=False)["flags"] == 0   # M = 0: nothing to associate
    xn = x.copy(); xn[4] = np.nan
    assert R.reference(xn, S, 2, ids, t, m)["flags"] == R.INSTANCE_FAILED
    Sn = S.copy(); Sn[5, 1] = np.nan
    r = R.reference(x, Sn, 2, ids, t, m)
    assert r["flags"] == R.FULL_NOT_PD and r["nees_pose"] > 0
    # the heading error is wrapped, the truth's heading is not
    a = R.reference(x, S, 2, ids, np.array([0.0, 0.0, 0.25]), m)["nees_full"]
    b = R.reference(x, S, 2, ids, np.array([0.0, 0.0, 0.25 + 3 * R.TWO_PI]), m)["nees_full"]
    assert abs(float(a - b)) <= 1e-12 * float(a)


def test_summary_against_exact_chi_square_quantiles():
    from live_ekf_slam_amd.filters import chi2_quantile, consistency_summary
    for dof, row in R.CHI2_TABLE.items():
        for p, exact in zip(R.CHI2_P, row):
            assert abs(chi2_quantile(p, dof) / exact - 1) <= 0.004, (dof, p)
    # a batch of 65 536 instances of n = 103 (sum dof = 6 750 208), two of them flagged
    B = 65536 + 2
    dof = np.full(B, 103, dtype=np.int32); flags = np.zeros(B, dtype=np.int32); flags[[5, 77]] = [1, 8]
    nees = np.full(B, 51.5); nees[[5, 77]] = np.nan
    for alpha, lo, hi in ((0.05, 1, 4), (0.1, 2, 3), (0.01, 0, 5)):
        s = consistency_summary(nees, dof, flags, alpha)
        assert s["count"] == 65536 and s["left_out"] == 2 and abs(s["normalised"] - 0.5) < 1e-12
        row = R.CHI2_TABLE[6750208]
        assert abs(s["lower"] * 6750208 / row[lo] - 1) <= 0.004 and abs(s["upper"] * 6750208 / row[hi] - 1) <= 0.004
        assert s["lower"] < 1 < s["upper"]
    s = consistency_summary(np.full(10, 3.0), np.full(10, 3), np.zeros(10, dtype=np.int32))   # sum dof = 30: the smallest accepted
    assert abs(s["lower"] * 30 / R.CHI2_TABLE[30][1] - 1) <= 0.004 and abs(s["upper"] * 30 / R.CHI2_TABLE[30][4] - 1) <= 0.004


def test_summary_refuses_fewer_than_30_degrees_of_freedom():
    from live_ekf_slam_amd.filters import chi2_quantile, consistency_summary
    with pytest.raises(ValueError, match="30"):
        consistency_summary(np.ones(9), np.full(9, 3), np.zeros(9, dtype=np.int32))
    with pytest.raises(ValueError, match="30"):
        consistency_summary(np.ones(20), np.full(20, 3), np.r_[np.zeros(9, dtype=np.int32), np.ones(11, dtype=np.int32)])
    with pytest.raises(ValueError, match="30"):
        chi2_quantile(0.5, 29)
