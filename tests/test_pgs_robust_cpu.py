"""Robust loss of the pose graph, the parts that need no device: the loss function compiled for the host (pgs_robust_loss_host, the
kernels' source) against mpmath, pgs_set_robust's argument checks, and the reference the GPU tests lean on (tests/pgs_robust_reference.py):
its weighted system against a dense product, its LM loop against the oracle's on Gaussian graphs."""
import ctypes as C
import math

import numpy as np
import pytest

import pgs_robust_reference as RR
import pgs_step_reference as R
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import default_config
from live_ekf_slam_amd.pose_graph import robust_loss_host

KS = (0.1, 1.345, 30.0)
ULP_BOUND = 4      # every value is at most four correctly rounded operations away from its inputs (pgs_robust.h), each within half an ulp


def _rs(k):
    return [0.0, 5e-324, k * (1 - 2.0 ** -52), k, k * (1 + 2.0 ** -52), 1e-8 * k, 1e8 * k, 1e150]


def _exact(kind, k, r):
    import mpmath as mp
    mp.mp.dps = 50
    k, r = mp.mpf(k), mp.mpf(r)
    if kind == RR.NONE:
        return r * r / 2, mp.mpf(1), mp.mpf(1)
    if kind == RR.HUBER:
        if r <= k:
            return r * r / 2, mp.mpf(1), mp.mpf(1)
        return k * (r - k / 2), k / r, mp.sqrt(k / r)
    q = k * k / (k * k + r * r)
    return k * k / 2 * (r * r / (k * k + r * r)), q * q, q


def _ulps(got, exact):
    """|got - exact| in units of the spacing of float64 at exact (the smallest subnormal where exact underflows)."""
    import mpmath as mp
    ulp = float(np.spacing(abs(float(exact))))
    return float(abs(mp.mpf(got) - exact) / mp.mpf(ulp))


@pytest.mark.parametrize("kind", [RR.NONE, RR.HUBER, RR.GEMAN_MCCLURE])
def test_the_host_loss_against_mpmath(kind):
    worst = 0.0
    for k in KS:
        for r in _rs(k):
            got = robust_loss_host(kind, 0.0 if kind == RR.NONE else k, r)
            for name, g, x in zip(("rho", "w", "sw"), got, _exact(kind, k, r)):
                d = _ulps(g, x)
                worst = max(worst, d)
                assert d <= ULP_BOUND, (kind, k, r, name, g, float(x), d)
            ref = RR.loss(kind, k, np.array([r]))   # the Python reference of the GPU tests says the same
            for g, x in zip(got, ref):
                assert abs(g - float(x[0])) <= ULP_BOUND * np.spacing(abs(g)), (kind, k, r, g, float(x[0]))
    print(f"kind {kind}: largest error {worst:.2f} ulp")


@pytest.mark.parametrize("k", KS)
def test_huber_is_continuous_at_k(k):
    rho_in, w_in, sw_in = robust_loss_host(RR.HUBER, k, k)                       # the inlier branch holds r = k
    rho_out, w_out, sw_out = k * (k - 0.5 * k), k / k, math.sqrt(k / k)           # the outlier branch's expressions at r = k
    for a, b in ((rho_in, rho_out), (w_in, w_out), (sw_in, sw_out)):
        assert abs(a - b) <= 2 * np.spacing(abs(a)), (k, a, b)
    rho_up, w_up, sw_up = robust_loss_host(RR.HUBER, k, k * (1 + 2.0 ** -52))   # and one ulp of r further the outlier branch is taken
    assert rho_in <= rho_up <= rho_in * (1 + 8 * 2.0 ** -52) and 1 - 4 * 2.0 ** -52 <= w_up <= 1.0 and 1 - 4 * 2.0 ** -52 <= sw_up <= 1.0


def test_argument_errors_of_pgs_set_robust_in_the_documented_order():
    L = _lib.lib()
    err = lambda: L.slam_last_error().decode()   # noqa: E731
    # the arguments first, before the handle is looked at
    for kind, k in ((3, 1.0), (-1, 1.0), (1, float("nan")), (1, 0.0), (1, -1.0), (1, float("inf")), (2, float("nan")), (2, 0.0), (2, float("inf"))):
        assert L.pgs_set_robust(None, kind, k) == -1 and "kind" in err() and "NULL handle" not in err(), (kind, k, err())
    # then the handle
    for kind, k in ((0, 0.0), (0, float("nan")), (1, 1.345), (2, 3.0), (1, 1e300)):
        assert L.pgs_set_robust(None, kind, k) == -1 and "NULL handle" in err(), (kind, k, err())
    kind, k = C.c_int(7), C.c_double(7.0)
    assert L.pgs_get_robust(None, C.byref(kind), C.byref(k)) == -1 and "NULL handle" in err()
    with pytest.raises(_lib.SlamError):
        robust_loss_host(5, 1.0, 1.0)
    with pytest.raises(_lib.SlamError):
        robust_loss_host(RR.HUBER, 0.0, 1.0)


def _small_graph():
    """3 poses, 2 landmarks: landmark 0 seen from all poses, landmark 1 from the last two, one detection 3 m / 0.5 rad off."""
    from oracle import oracle as O
    g = O.OraclePoseGraph(default_config(), N_max=3, L_max=2, KP=2)
    g.init(0.0, 0.0, 0.0)
    g.updateNaiveVehPoseEstimate(np.array([0.12, 0.01, 0.03]))
    g.update(0.1, 0.03, np.array([[100, 1.5, 0.3], [101, 2.0, -0.4]], dtype=np.float32))
    g.updateNaiveVehPoseEstimate(np.array([0.19, 0.03, 0.08]))
    g.update(0.1, 0.03, np.array([[100, 1.42 + 3.0, 0.33 + 0.5], [101, 1.93, -0.45]], dtype=np.float32))
    return g


@pytest.mark.parametrize("kind,k", [(RR.HUBER, 1.345), (RR.GEMAN_MCCLURE, 3.0)])
def test_the_weighted_system_is_a_row_scaling(kind, k):
    g = _small_graph()
    v = g.values(0)
    assert v["poses"].shape[0] == 3 and v["M"] == 2
    S, L = RR.weighted_system(g, v["poses"], v["landmarks"], 1e-5, kind, k)
    rows, cols, vals, e = g.jacobian(v["poses"], v["landmarks"])
    J = np.zeros((len(e), S.n))
    J[rows, cols] = vals
    w_row = np.ones(len(e))
    w_row[L["first"]] = L["w"]
    w_row[L["first"] + 1] = L["w"]
    assert len(L["first"]) == 4 and L["w"].min() < 0.5 and (kind != RR.HUBER or (L["w"] == 1.0).any())
    b = -(J.T @ (w_row * e))
    tol = 8 * R.U * (np.abs(J).T @ np.abs(w_row * e))
    assert np.all(np.abs(S.b - b) <= tol), (S.b - b, tol)
    A = J.T @ (w_row[:, None] * J) + 1e-5 * np.eye(S.n)
    assert np.all(np.abs(S.A - A) <= 8 * R.U * (np.abs(J).T @ (w_row[:, None] * np.abs(J)) + 1e-5 * np.eye(S.n)))


def test_the_reference_lm_reproduces_the_oracle_on_gaussian_graphs():
    import pgs_marginals_reference as MR
    sc = MR.scenario("n34")
    for b, g in enumerate(sc["graphs"]):
        mine = RR.lm_solve(g, RR.NONE, 0.0)
        o = g.solve()
        assert (mine["iterations"], mine["trials"], mine["flags"]) == (o["iterations"], o["trials"], o["flags"]), (b, mine, o)
        vo = g.values(1)
        assert np.abs(mine["poses"] - vo["poses"]).max() < 1e-9, b


@pytest.mark.parametrize("name", ["n9", "n33", "n34"])
def test_the_outlier_streams_are_what_the_gpu_tests_assume(name):
    """Every seventh non-first detection is 3 m / 0.5 rad off, first detections are clean, and the oracle graphs store them."""
    sc = RR.case(name)
    d = sc["st"]["meas"].astype(np.float64) - sc["clean"]["meas"].astype(np.float64)
    assert np.all(d[~sc["bad"]] == 0.0) and sc["bad"].any()
    assert np.allclose(d[sc["bad"]][:, 1], RR.OUTLIER_RANGE, atol=1e-5) and np.allclose(d[sc["bad"]][:, 2], RR.OUTLIER_BEARING, atol=1e-5)
    for b, g in enumerate(sc["graphs"]):
        v = g.values(0)
        bad = RR.bad_factors(sc, b)
        L = RR.weigh(g, v["poses"], v["landmarks"], RR.HUBER, 1.345)
        assert len(bad) == len(L["w"]), (name, b)
        nonfirst = int(sum(sc["st"]["cnt"][b])) - v["M"]
        assert int(bad.sum()) == len(range(RR.SEED % RR.OUTLIER_EVERY and RR.OUTLIER_EVERY - RR.SEED % RR.OUTLIER_EVERY, nonfirst, RR.OUTLIER_EVERY)), (name, b)
        # a corrupted detection is an outlier at the initial estimate (3 m is about 3.5 sigma of the range noise: Huber's w is near 0.4)
        assert np.all(L["w"][bad] < 0.75) and (not bad.any() or L["w"][bad].min() < 0.5), (name, b, L["w"][bad])
