"""CPU reference for the Cholesky square-root mode of the UKF (SLAM_UKF_SQRT_CHOLESKY, include/slam_batch.h): a numpy
transliteration of ukf.cpp whose matrix square root is a parameter - "eigh" (nearestSPD + sqrt, the reference) or "cholesky"
(Y = L L^T, sigma-point offsets = columns of L, eigen fallback for a pivot <= 1e-8 or a non-finite one).  The oracle under
oracle/ implements the reference only, so this module is the reference of the new mode; tests/test_ukf_chol_gpu.py checks the
device against it."""
import math

import numpy as np
import pytest

from conftest import load_golden

F32 = np.float32
TWO_PI = 2 * 3.14159265358979323846
PIVOT_FLOOR = 1e-8   # nearestSPD's cwiseMax(0.00000001) (ukf.cpp:119), reused as the Cholesky pivot floor


def _rem(x):
    return math.remainder(x, TWO_PI)


def cholesky_lower(Y):
    """Lower-triangular L with L L^T = Y, or None if a pivot d_k = Y_kk - sum_j L_kj^2 is <= 1e-8 or not finite."""
    n = len(Y)
    L = np.zeros((n, n))
    for k in range(n):
        d = Y[k, k] - L[k, :k] @ L[k, :k]
        if not (d > PIVOT_FLOOR and np.isfinite(d)):
            return None
        L[k, k] = math.sqrt(d)
        L[k + 1:, k] = (Y[k + 1:, k] - L[k + 1:, :k] @ L[k, :k]) / L[k, k]
    return L


def eigen_sqrt(Y):
    D, Qv = np.linalg.eigh(Y)
    return (Qv * np.sqrt(np.maximum(D, PIVOT_FLOOR))) @ Qv.T


class NumpyUKF:
    """ukf.cpp:3-45,106-372 with numpy (float casts of SURVEY.md Appendix B, float overload of cos/sin), the square root
    selectable.  A copy of NumpyUKF of tests/test_oracle_ukf.py with `sqrt` added; shares nothing with the C++ oracle."""

    def __init__(self, sqrt="eigh", V00=0.01, V11=0.01, W00=1.0, W11=1.0, v_d=0.0, v_th=0.0, w_r=0.0, w_b=0.0):
        assert sqrt in ("eigh", "cholesky")
        self.sqrt = sqrt
        self.V = np.diag([V00, V11]); self.W = np.diag([W00, W11])   # V/W quirk on: V = (W_00, W_11), W = I
        self.v_d, self.v_th, self.w_r, self.w_b = F32(v_d), F32(v_th), F32(w_r), F32(w_b)
        self.W0 = F32(0.2)
        self.M = 0; self.ids = []
        self.P = np.diag([1e-4, 1e-4, 2.5e-5, 2.5e-5])
        self.factorisations = 0; self.fallbacks = 0

    def init(self, x0, y0, yaw0):
        yaw0 = F32(yaw0)
        self.x = np.array([F32(x0), F32(y0), F32(math.cos(yaw0)), F32(math.sin(yaw0))], dtype=np.float64)

    @staticmethod
    def _yaw(v):
        return F32(_rem(math.atan2(v[3], v[2])))

    def _motion(self, x, u_d, u_th):
        xp = x.copy()
        yaw = self._yaw(x)
        dd = F32(u_d + self.v_d)
        xp[0] = x[0] + float(F32(dd * F32(math.cos(yaw))))
        xp[1] = x[1] + float(F32(dd * F32(math.sin(yaw))))
        ny = F32(_rem(float(F32(F32(yaw + u_th) + self.v_th))))
        xp[2] = float(F32(math.cos(ny))); xp[3] = float(F32(math.sin(ny)))
        return xp

    def _sense(self, x, li):
        yaw = self._yaw(self.x)
        dx, dy = x[li] - x[0], x[li + 1] - x[1]
        return np.array([math.sqrt(dx * dx + dy * dy) + float(self.w_r),
                         _rem(math.atan2(dy, dx) - float(yaw) + float(self.w_b))])

    def scaled(self):
        """Y = 0.5 (P + P^T) * float((2M+4)/(1-W_0)) (ukf.cpp:114), the matrix both square roots take."""
        return 0.5 * (self.P + self.P.T) * float(F32(F32(2 * self.M + 4) / (F32(1) - self.W0)))

    def square_root(self):
        """Sigma-point offsets: column i-1 gives X_i = x + offset, X_{i+n} = x - offset."""
        Y = self.scaled()
        if self.sqrt == "cholesky":
            L = cholesky_lower(Y)
            if L is not None:
                self.factorisations += 1
                return L
            self.fallbacks += 1
        return eigen_sqrt(Y)

    def update(self, fwd, ang, meas):
        u_d, u_th = F32(fwd), F32(ang)
        n = 2 * self.M + 4
        w = float(F32((F32(1) - self.W0) / F32(2 * n)))
        Wts = np.full(2 * n + 1, w); Wts[0] = float(self.W0)
        yaw = self._yaw(self.x)
        Q = np.zeros((n, n))
        Q[0, 0] = self.V[0, 0] * float(F32(math.cos(yaw))); Q[1, 1] = self.V[0, 0] * float(F32(math.sin(yaw)))
        Q[2, 2] = self.V[1, 1] * float(F32(math.cos(yaw))); Q[3, 3] = self.V[1, 1] * float(F32(math.sin(yaw)))
        sq = self.square_root()
        X = np.zeros((n, 2 * n + 1))
        X[:, 0] = self.x
        for i in range(1, n + 1):
            X[:, i] = self.x + sq[:, i - 1]; X[:, i + n] = self.x - sq[:, i - 1]
        Xp = np.stack([self._motion(X[:, i], u_d, u_th) for i in range(2 * n + 1)], axis=1)
        xp = np.zeros(n)
        for i in range(2 * n + 1):
            xp = xp + Wts[i] * Xp[:, i]
        Pp = np.zeros((n, n))
        for i in range(2 * n + 1):
            d = Xp[:, i] - xp
            Pp = Pp + np.outer(Wts[i] * d, d)
        Pp = Pp + Q
        fresh = []
        for (idf, r, b) in meas:
            idn = int(idf)
            if idn in self.ids:
                li = 2 * self.ids.index(idn) + 4
                Z = np.stack([self._sense(Xp[:, i], li) for i in range(2 * n + 1)], axis=1)
                z_est = np.array([sum(Wts[i] * Z[0, i] for i in range(2 * n + 1)), 0.0])
                S = np.zeros((2, 2)); Cm = np.zeros((n, 2))
                for i in range(2 * n + 1):
                    d = Z[:, i] - z_est; d[1] = _rem(d[1])
                    S = S + np.outer(Wts[i] * d, d)
                    Cm = Cm + np.outer(Wts[i] * (Xp[:, i] - xp), d)
                S = S + self.W
                K = Cm @ np.linalg.inv(S)
                inn = np.array([float(F32(r)), float(F32(b))]) - z_est; inn[1] = _rem(inn[1])
                xp = xp + K @ inn
                Pp = Pp - K @ S @ K.T
            else:
                fresh.append((idn, F32(r), F32(b)))
        for idn, r, b in fresh:
            nn = len(xp)
            yw = self._yaw(xp)
            a = F32(yw + b)
            xp = np.concatenate([xp, [xp[0] + float(F32(r * F32(math.cos(a)))), xp[1] + float(F32(r * F32(math.sin(a))))]])
            Pn = np.zeros((nn + 2, nn + 2)); Pn[:nn, :nn] = Pp; Pn[nn:, nn:] = self.W
            Pp = Pn
            self.ids.append(idn); self.M += 1
        self.x, self.P = xp, Pp


def run_stream(g, T, sqrt):
    """T steps of a golden measurement stream; returns the filter and the position error after every step."""
    f = NumpyUKF(sqrt); f.init(0, 0, 0)
    err = np.empty(T)
    for t in range(T):
        k = int(g["meas_count"][t])
        f.update(g["cmds"][t, 0], g["cmds"][t, 1], [tuple(r) for r in g["meas"][t, :k]])
        err[t] = math.hypot(f.x[0] - g["truth"][t, 0], f.x[1] - g["truth"][t, 1])
    return f, err


def test_eigh_variant_matches_the_oracle(oracle):
    """The transliteration with sqrt="eigh" is the reference: within 1e-8 of the C++ oracle over 120 steps (the bound of
    tests/test_oracle_ukf.py for the numpy UKF it was copied from)."""
    g = load_golden("sim_seed1_L20_T400.npz")
    u = oracle.OracleUKF(L_max=20, math=oracle.MATH_LIBM); u.init(0, 0, 0)
    ref = NumpyUKF("eigh"); ref.init(0, 0, 0)
    worst = 0.0
    for t in range(120):
        k = int(g["meas_count"][t]); m = g["meas"][t, :k]
        u.update(g["cmds"][t, 0], g["cmds"][t, 1], m)
        ref.update(g["cmds"][t, 0], g["cmds"][t, 1], [tuple(r) for r in m])
        s = u.state()
        assert s["M"] == ref.M and list(s["ids"]) == ref.ids
        worst = max(worst, np.abs(s["x"] - ref.x).max(), np.abs(s["P"] - ref.P).max())
    assert ref.M >= 1
    assert worst < 1e-8, worst


def test_cholesky_factor_is_lower_triangular_and_exact():
    rng = np.random.default_rng(7)
    for n in (4, 10, 44, 104):
        A = rng.normal(size=(n, n)); Y = A @ A.T / n + np.diag(rng.uniform(1e-3, 1.0, n))
        L = cholesky_lower(Y)
        assert L is not None and np.array_equal(L, np.tril(L)) and np.all(np.diag(L) > 0)
        assert np.abs(L @ L.T - Y).max() < 1e-13 * np.abs(Y).max()
        np.testing.assert_allclose(L, np.linalg.cholesky(Y), rtol=0, atol=1e-12)


def test_pivot_rule_sends_an_indefinite_P_to_the_eigen_path():
    """A pivot <= 1e-8 (or a non-finite one) falls back to nearestSPD + sqrt for that step, counted; a positive definite P
    factors."""
    f = NumpyUKF("cholesky"); f.init(0, 0, 0)
    f.P = np.diag([1e-4, 1e-4, 2.5e-5, -1e-6])           # indefinite: the last pivot is negative
    sq = f.square_root()
    assert (f.factorisations, f.fallbacks) == (0, 1)
    np.testing.assert_array_equal(sq, eigen_sqrt(f.scaled()))
    assert cholesky_lower(np.diag([1.0, 1e-8])) is None  # the floor itself is refused (cwiseMax keeps 1e-8: <= falls back)
    assert cholesky_lower(np.diag([1.0, np.nan])) is None and cholesky_lower(np.diag([np.inf, 1.0])) is None
    f.P = np.diag([1e-4, 1e-4, 2.5e-5, 2.5e-5])
    L = f.square_root()
    assert (f.factorisations, f.fallbacks) == (1, 1)
    np.testing.assert_allclose(L @ L.T, f.scaled(), rtol=1e-14)


# Cholesky vs eigen square root on a reference measurement stream.  The reference's process noise is signed (Q = diag(V00 cos yaw,
# V00 sin yaw, V11 cos yaw, V11 sin yaw), ukf.cpp:183-186), so P is indefinite on many steps - nearestSPD clamps those eigenvalues -
# and there the Cholesky mode takes the eigen path (sim_seed1_L20: 328 of 400 steps; sim_seed2_L50: 130 of 200).  On the other
# steps its sigma points have the same first two moments in other directions, and the quirk-laden filter drifts apart from the
# eigen one: mean position errors measured 1.80 vs 2.02 m (+12 %) and 0.84 vs 0.78 m (-7 %).  Stated tolerance: 25 %.
CHOL_MEAN_ERR_RTOL = 0.25


@pytest.mark.parametrize("fixture,T", [("sim_seed1_L20_T400.npz", 400), ("sim_seed2_L50_T1000.npz", 200)])
def test_cholesky_variant_tracks_like_the_eigen_variant(fixture, T):
    g = load_golden(fixture)
    fe, ee = run_stream(g, T, "eigh")
    fc, ec = run_stream(g, T, "cholesky")
    assert fc.M == fe.M and fc.ids == fe.ids and fc.M >= 2
    assert fc.factorisations > 0 and fc.fallbacks > 0 and fc.factorisations + fc.fallbacks == T
    assert np.all(np.isfinite(fc.P)) and np.abs(fc.P - fc.P.T).max() < 1e-9
    assert abs(ec.mean() - ee.mean()) <= CHOL_MEAN_ERR_RTOL * ee.mean(), (ec.mean(), ee.mean())
