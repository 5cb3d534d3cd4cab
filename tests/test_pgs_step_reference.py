"""The extended-precision reference of one LM step (tests/pgs_step_reference.py), checked before anything is compared with it:
the oracle's Jacobian export meets its contract, the refined step agrees with a 50-digit solve, the oracle's own eliminations meet the
backward-error bound the GPU test holds the device to, and the inverse of the retraction recovers a step within its stated error.

Calibration of the bound eta <= 8 n u (BOUND_C): Higham (Accuracy and Stability of Numerical Algorithms, Thm 10.4) bounds the backward
error of a Cholesky solve componentwise by gamma_{3n+1} |R^T| |R|, which in the infinity norm is at most about 3 n u |A| times the growth
of |R^T| |R| over |A| (at most n, in practice a small constant for these diagonally dominant systems).  The oracle's exact eliminations
(sequential Schur, dense, segmented at 32 / 16 / 8 / 5 poses) come out at eta ~ 1e-16 on these graphs, three to four orders of magnitude
below 8 n u (printed below): the constant is Higham's with room for the device's summation orders, not a fit to a measurement."""
import math

import numpy as np
import pytest

import pgs_step_reference as R
from live_ekf_slam_amd.config import default_config

LAMBDAS = (1e-5, 1e-2, 1e1, 1e4)


@pytest.fixture(scope="module")
def small(oracle):
    """N = 30 poses, M = 8 landmarks, 4 detections per message, one landmark first seen at the last pose, one seen from separators only."""
    cfg = default_config()
    N, KP = 30, 4
    st = R.make_streams(N, [8], 4, 7, window=10, at_last=1, sep_only=1, SL=8)
    g = R.build_oracle_graphs(oracle, cfg, st, N, 8, KP)[0]
    v = g.values(0)
    assert v["M"] == 8
    return g, v


@pytest.fixture(scope="module")
def medium(oracle):
    """Ragged: N = 100 poses; M = 0, 1, 17, 33 landmarks; messages of 10 detections into 8 slots (dropped detections, later first
    factors); poses without detections."""
    cfg = default_config()
    N, KP = 100, 8
    st = R.make_streams(N, [0, 1, 17, 33], 10, 11, window=40, new_last=True, empty_every=7, at_last=1, sep_only=2, SL=16)
    gs = R.build_oracle_graphs(oracle, cfg, st, N, 40, KP)
    return gs, st


def test_jacobian_meets_its_contract(oracle, medium):
    gs, _ = medium
    for b, g in enumerate(gs):
        v = g.values(0)
        rows, cols, vals, e = g.jacobian(v["poses"], v["landmarks"])
        assert np.array_equal(e, g.residuals(v["poses"], v["landmarks"])), b
        assert math.isclose(0.5 * float(np.sum(e.astype(np.longdouble) ** 2)), g.cost(0), rel_tol=1e-13), b
        S = R.system_of(g, v["poses"], v["landmarks"], 0.0)
        gp, gl = g.gradient(v["poses"], v["landmarks"])
        grad = R.pack(gp, gl)
        jte = np.asarray(S.JT(e.astype(np.longdouble)), dtype=np.float64)
        assert np.abs(jte - grad).max() <= 1e-13 * np.abs(grad).max(), (b, np.abs(jte - grad).max(), np.abs(grad).max())
        assert rows.max() == len(e) - 1 and cols.max() < S.n and np.all(np.diff(rows) >= 0)


def test_bearing_range_rows_match_central_differences(oracle, small):
    """J's bearing-range rows are the exact derivatives along the retraction (the Between / Prior rows are GTSAM's, which drop the rotation
    of the residual pose - test_minimiser_matches_scipy_least_squares pins those through the minimiser)."""
    g, v = small
    p0, l0 = v["poses"], v["landmarks"]
    N, M = p0.shape[0], l0.shape[0]
    n = 3 * N + 2 * M
    rows, cols, vals, e = g.jacobian(p0, l0)
    Jd = np.zeros((len(e), n))
    np.add.at(Jd, (rows, cols), vals)
    br = np.zeros(len(e), dtype=bool)    # rows of the bearing-range factors: the residual order is prior, then per pose between + detections
    r = 3
    conn = g.connections()
    per_pose = np.bincount(conn[:, 0], minlength=N)
    for i in range(N):
        r += 3 if i + 1 < N else 0
        br[r:r + 2 * per_pose[i]] = True
        r += 2 * per_pose[i]
    assert r == len(e) and br.sum() == 2 * len(conn)
    h = 1e-6
    fd = np.zeros((len(e), n))
    for k in range(n):
        d = np.zeros(n)
        d[k] = h
        pp, lp = g.retract(p0, l0, d[:3 * N].reshape(N, 3), d[3 * N:].reshape(M, 2))
        pm, lm_ = g.retract(p0, l0, -d[:3 * N].reshape(N, 3), -d[3 * N:].reshape(M, 2))
        fd[:, k] = (g.residuals(pp, lp) - g.residuals(pm, lm_)) / (2 * h)
    err = np.abs(fd[br] - Jd[br]).max()
    assert err < 1e-6 * max(1.0, np.abs(Jd[br]).max()), err


def test_refined_step_agrees_with_a_50_digit_solve(oracle, small):
    """The refinement's residuals carry a 64-bit mantissa, so the refined step is exact to about kappa 2^-64 |delta| (forward), not to a few
    u once kappa > 2^11: on this graph (kappa ~ 5e7) it lands ~1e-14 |delta| from the 50-digit solution.  That is 2^-11 of the forward
    tolerance the GPU test allows (BOUND_C n u kappa |delta|): the reference is exact for every comparison made with it."""
    import mpmath
    g, v = small
    S = R.system_of(g, v["poses"], v["landmarks"], 1e-5)
    d_ref, kappa, rounds = R.reference_step(S)
    mp = mpmath.mp
    mp.dps = 50
    n = S.n
    J = [[mp.mpf(0)] * n for _ in range(S.m)]
    for r, c, x in zip(S.rows.tolist(), S.cols.tolist(), S.vals.tolist()):
        J[r][c] += mp.mpf(x)
    Jm = mp.matrix(J)
    A = Jm.T * Jm + mp.mpf(S.lam) * mp.eye(n)
    b = -(Jm.T * mp.matrix([mp.mpf(x) for x in S.e.tolist()]))
    x = mp.lu_solve(A, b)
    exact = np.array([float(x[k]) for k in range(n)])
    dev = np.abs(np.asarray(d_ref, dtype=np.float64) - exact).max()
    scale = np.abs(exact).max()
    print(f"\nrefined step vs 50 digits: n = {n}, kappa_1 = {kappa:.3g}, {rounds} round(s), |d_ref - d_exact|_inf = {dev / scale:.3g} |d|_inf")
    assert dev <= max(4 * R.U, kappa * 2.0 ** -64) * scale, (dev, scale, kappa)
    assert dev <= 2.0 ** -11 * R.BOUND_C * n * R.U * kappa * scale


@pytest.mark.parametrize("lin", ["schur", "dense", "seg32", "seg16", "seg8", "seg5"])
def test_oracle_steps_meet_the_backward_error_bound(oracle, medium, lin):
    mode = {"schur": oracle.LIN_SCHUR, "dense": oracle.LIN_DENSE}.get(lin)
    if mode is None:
        mode = oracle.LIN_SEG | (int(lin[3:]) << 8)
    gs, _ = medium
    worst = []
    for lam in LAMBDAS:
        for b, g in enumerate(gs):
            v = g.values(0)
            S = R.system_of(g, v["poses"], v["landmarks"], lam)
            ok, dp, dl = g.step(v["poses"], v["landmarks"], lam, mode)
            assert ok, (lin, lam, b)
            eta = S.eta(R.pack(dp, dl))
            bound = R.BOUND_C * S.n * R.U
            assert eta <= bound, f"{lin} lam {lam:g} instance {b}: eta {eta:.3g} > bound {bound:.3g} (n = {S.n})"
            worst.append((eta, lam, b, bound))
    eta, lam, b, bound = max(worst)
    print(f"\noracle {lin}: largest eta {eta:.3g} (lam {lam:g}, instance {b}), bound {bound:.3g}")


def test_the_oracle_step_is_the_reference_step(oracle, medium):
    """The oracle's solve and the refined reference are the same step: forward error within the usual eta kappa."""
    gs, _ = medium
    for b, g in enumerate(gs):
        v = g.values(0)
        S = R.system_of(g, v["poses"], v["landmarks"], 1e-5)
        d_ref, kappa, _ = R.reference_step(S)
        assert S.eta(d_ref) < 1e3 * R.U * 2.0 ** -11, b         # refined well below double rounding
        ok, dp, dl = g.step(v["poses"], v["landmarks"], 1e-5, oracle.LIN_SCHUR)
        dref = np.asarray(d_ref, dtype=np.float64)
        err = np.abs(R.pack(dp, dl) - dref).max()
        assert err <= R.BOUND_C * S.n * R.U * kappa * np.abs(dref).max(), (b, err, kappa)


def test_recovering_the_step_from_the_retraction(oracle, medium):
    gs, st = medium
    rng = np.random.default_rng(3)
    for b, g in enumerate(gs):
        v = g.values(0)
        N, M = v["poses"].shape[0], v["M"]
        dp = rng.uniform(-0.5, 0.5, (N, 3))
        dp[::5, 2] = rng.uniform(-3.0, 3.0, len(dp[::5]))        # yaw steps that wrap
        dl = rng.uniform(-0.5, 0.5, (M, 2))
        p1, l1 = g.retract(v["poses"], v["landmarks"], dp, dl)
        delta, eps = R.recover_step(v["poses"], v["landmarks"], p1, l1[:M])
        assert np.all(np.abs(delta - R.pack(dp, dl)) <= eps), (b, np.max(np.abs(delta - R.pack(dp, dl)) - eps))


# The separator and pose-count edges of tests/test_pgs_step_gpu.py, written out: scenario -> (solve paths, N, segment length the search starts
# from, NS = (N - 2) / SL, the plan the solve must take: that length, or 0 = the sequential chain beyond 128 separators)
EDGE_TABLE = {"sep128": (("seg2",), 128, 2, 63, 2), "sep130": (("seg2",), 130, 2, 64, 2), "sep132": (("seg2",), 132, 2, 65, 2),
              "sep256": (("seg2",), 256, 2, 127, 2), "sep258": (("seg2",), 258, 2, 128, 2), "sep259": (("seg2",), 259, 2, 128, 2),
              "sep260": (("seg2",), 260, 2, 129, 0),
              "sep637": (("seg5",), 637, 5, 127, 5), "sep642": (("seg5", "seg5_back_global"), 642, 5, 128, 5), "sep646": (("seg5",), 646, 5, 128, 5),
              "sep647": (("seg5",), 647, 5, 129, 0),
              "sep1026": (("seg8",), 1026, 8, 128, 8), "sep1034": (("seg8",), 1034, 8, 129, 0),
              "lds1365": (("default", "back_global"), 1365, 32, 42, 32)}


def test_the_edge_table_is_the_gpu_tests_table():
    import test_pgs_step_gpu as T
    assert set(T.SEP_EDGES) | {"lds1365"} == set(EDGE_TABLE)
    want = {(n, p) for n, row in EDGE_TABLE.items() for p in row[0]}
    assert want <= set(T.CASES) and not {c for c in T.CASES if c[0] in EDGE_TABLE} - want
    assert T.FALLBACK == {n for n, row in EDGE_TABLE.items() if row[4] == 0}
    for name, (paths, N, SL, NS, _) in EDGE_TABLE.items():
        assert T.SCENARIOS[name][0] == N and (N - 2) // SL == NS, name
        for p in paths:
            assert int(T.SEG[p].get("SLAM_PGS_SEG", "32")) == SL, (name, p)
        if name in T.SEP_EDGES:
            assert T.SEP_EDGES[name] == (paths[0], NS) and T.SCENARIOS[name][5]["SL"] == SL, name
            assert T.SCENARIOS[name][5]["sep_last"] == (NS in (127, 128)), name
    # every count the edges are about: the lanes 63 | 64 of pgs_seg_chain_kernel (nseg = NS + 1), lane 128, the capacity and one beyond
    assert {row[3] for row in EDGE_TABLE.values()} >= {63, 64, 65, 127, 128, 129}
    assert {row[3] % 4 for n, row in EDGE_TABLE.items() if row[3] in (63, 64, 65)} == {3, 0, 1}


@pytest.mark.parametrize("name", list(EDGE_TABLE))
def test_premises_of_the_separator_and_pose_count_edges(oracle, name):
    """What test_pgs_step_gpu.py's cases at the separator capacity rest on, without a GPU: the plan (the forced length, the chain beyond 128
    separators), the landmark counts, a first trial the dense reference LM accepts, the landmark at the last separator, and factors in the
    segments whose lanes the cases are about."""
    import pgs_robust_reference as RR
    import test_pgs_step_gpu as T
    paths, N, SL, NS, plan = EDGE_TABLE[name]
    nseg = NS + 1
    sc = T.scenario(name)
    Ms = T.SCENARIOS[name][1]
    assert sc["N"] == N and len(sc["refs"]) == len(Ms)
    for p in paths:
        assert T.expected_plan(sc, name, p) == plan, (name, p)
    opt = T.SCENARIOS[name][5]
    with_last = 0
    for b, (g, (v, _, _, _, (pose, lm))) in enumerate(zip(sc["graphs"], sc["refs"])):
        assert v["M"] == Ms[b] and v["poses"].shape[0] == N, (name, b)
        first = RR.lm_solve(g, RR.NONE, 0.0, max_trials=1)
        assert (first["iterations"], first["trials"]) == (1, 1), (name, b, first["margin"])
        seg = np.minimum(np.where(pose == 0, 0, (pose - 1) // SL), NS)          # the segment of an interior pose (predict_plan's rule)
        interior = (pose % SL != 0) | (pose == 0) | (pose > NS * SL)
        assert seg.max(initial=0) < nseg
        j = R.sep_last_landmark(Ms[b], opt.get("at_last", 0), opt.get("sep_only", 0)) if opt.get("sep_last") else None
        if j is not None:     # the landmark of the last separator: factors at the last three separators and nowhere else
            k = int(np.flatnonzero(v["ids"] == 100 + j)[0])
            assert sorted(pose[lm == k].tolist()) == [(NS - 2) * SL, (NS - 1) * SL, NS * SL], (name, b, pose[lm == k])
            assert not interior[lm == k].any()
            with_last += 1
        if NS == 128 and Ms[b] == max(Ms):   # its segments 64 (first lane of wavefront 1), 127 and 128 (alone in wavefront 2) hold factors
            held = set(np.unique(seg[interior]).tolist())
            assert {64, 127, 128} <= held, (name, b, sorted({64, 127, 128} - held))
    if opt.get("sep_last"):
        assert NS in (127, 128) and with_last >= 2, (name, with_last)


def test_streams_hold_what_they_promise(oracle, medium):
    """M exactly as asked, messages longer than the 8 factor slots, poses without detections, and - from the detections those messages
    drop while their landmarks are still created - landmarks whose first FACTOR comes after that of a landmark numbered after them (the
    per-landmark first rows the SYRK's k-range trimming must take as a suffix minimum)."""
    gs, st = medium
    assert [g.values(0)["M"] for g in gs] == [0, 1, 17, 33]
    assert st["cnt"].max() == 10 and np.all(st["cnt"][:, 6::7] <= 1)      # over-long messages (8 slots), poses without detections
    v = gs[3].values(0)
    pose, lm = R.factor_pairs(gs[3], v["poses"], v["landmarks"])
    first = np.full(v["M"], np.iinfo(np.int64).max)
    np.minimum.at(first, lm, pose)
    seen = first < v["poses"].shape[0]      # (a landmark created by a dropped detection at the last pose has no factor at all)
    later = [j for j in range(v["M"] - 1) if seen[j] and first[j] > first[j + 1:][seen[j + 1:]].min(initial=first[j])]
    assert later, first
