"""The reference and the yardstick of the marginal-covariance tests (tests/pgs_marginals_reference.py), on the CPU.

The GPU test (test_pgs_marginals_gpu.py) judges the device against judge(): an inverse of H = J^T J refined in np.longdouble, and a bar of
10 x the rounding spread of two double routes.  Here the reference is checked against a 50-digit inverse, and for every scenario the GPU
test uses (at the oracle's own solved result) the reference's last correction must be far below the smallest spread it judges and both
double routes inside the derived forward bound BOUND_C n u kappa_1."""
import functools

import numpy as np
import pytest

import pgs_marginals_reference as MR
import test_pgs_step_gpu as T

SMALL = [f"n{n}" for n in (2, 7, 8, 9, 31, 32, 33, 34)]
NAMES = ["ragged", "configs4", "ld512", "long", "ill", "fusable"] + SMALL


def test_the_reference_agrees_with_a_50_digit_inverse(oracle):
    import mpmath
    g = MR.scenario("n7")["graphs"][3]   # 7 poses, 8 landmarks: n = 37
    g.solve()
    v = g.values(1)
    poses, lms = v["poses"], v["landmarks"].reshape(-1, 2)
    j = MR.judge(g, poses, lms)
    N, M, n = j["N"], j["M"], j["n"]
    assert (N, M) == (7, 8)
    rows, cols, vals, e = g.jacobian(poses, lms)
    mp = mpmath.mp
    mp.dps = 50
    J = [[mp.mpf(0)] * n for _ in range(len(e))]
    for r, c, x in zip(rows.tolist(), cols.tolist(), vals.tolist()):
        J[r][c] += mp.mpf(x)
    Jm = mp.matrix(J)
    X = (Jm.T * Jm) ** -1
    Xd = np.array([[np.longdouble(mpmath.nstr(X[a, b], 30)) for b in range(n)] for a in range(n)], dtype=np.longdouble)
    fom = MR.figure_of_merit(j["pose_cov"], j["lm_cov"], *MR.split_blocks(Xd, N, M))
    print(f"reference vs 50 digits: {fom:.3g}; last correction {j['last_correction']:.3g}, spread {j['spread']:.3g}, kappa_1 {j['kappa']:.3g}")
    # long double carries 64 bits: kappa 2^-64 is the floor of the refinement
    assert fom <= max(4 * j["kappa"] * 2.0 ** -64, 2.0 ** -60) and fom <= 1e-3 * j["spread"]
    # and the figure of merit sees an error: one entry of one block off by 1e-9 relative
    bad = np.array(j["pose_cov"], dtype=np.float64)
    bad[2, 1, 1] *= 1 + 1e-9
    assert MR.figure_of_merit(bad, j["lm_cov"], j["pose_cov"], j["lm_cov"]) > 0.5e-9 * abs(bad[2, 1, 1]) / np.abs(bad[2]).max()


@functools.lru_cache(maxsize=None)
def judged_at_result(name, b):
    g = MR.scenario(name)["graphs"][b]
    g.solve()
    v = g.values(1)
    return MR.judge(g, v["poses"], v["landmarks"])


@pytest.mark.parametrize("name", NAMES)
def test_the_yardstick(oracle, name):
    """(i) the reference's last correction <= 0.1 x the smallest spread it judges; (ii) both double routes inside the derived bound."""
    js = [judged_at_result(name, b) for b in range(len(MR.scenario(name)["graphs"]))]
    js = [j for j in js if "singular" not in j]
    for b, j in enumerate(js):
        print(f"{name}[{b}]: N {j['N']} M {j['M']} spread chol {j['spread_chol']:.3g} lu {j['spread_lu']:.3g} bar {j['bar']:.3g} bound {j['bound']:.3g} "
              f"kappa_1 {j['kappa']:.3g} last correction {j['last_correction']:.3g} ({j['rounds']} rounds)")
    smallest = min(j["spread"] for j in js)
    assert max(j["last_correction"] for j in js) <= 0.1 * smallest
    for j in js:
        assert 0.0 < j["spread_chol"] <= j["bound"] and 0.0 < j["spread_lu"] <= j["bound"]
        assert j["bar"] == min(MR.MARGIN * j["spread"], j["bound"])


def test_the_singular_instances_are_the_two_known_ones(oracle):
    """A landmark that was created but has no stored factor (both Jacobian columns empty) makes H singular.  In the scenario table as it
    stands: n2 instance 4 (9 of its 17 landmarks) and fusable instance 13 (one landmark), and no other."""
    found = {}
    for name in NAMES + ["ragged207"]:
        for b, g in enumerate(MR.scenario(name)["graphs"]):
            v = g.values(0)
            loose = MR.unconstrained_landmarks(g, v["poses"], v["landmarks"])
            if len(loose):
                found[(name, b)] = len(loose)
    assert found == {("n2", 4): 9, ("fusable", 13): 1}, found
    j = MR.judge(MR.scenario("n2")["graphs"][4], *(lambda v: (v["poses"], v["landmarks"]))(MR.scenario("n2")["graphs"][4].values(0)))
    assert "singular" in j and len(j["singular"]) == 9
    assert T.SCENARIOS["n2"][1][4] == 17
