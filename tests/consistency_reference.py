"""The reference of slam_consistency (include/slam_batch.h) on the host, in np.longdouble, the three fp64 routes that serve as the
yardstick of its rounding error, and the rule the GPU tests judge the device's values with.  A helper: no tests in here.

Definitions: S = (P + P^T) / 2, e = (x - x_true, y - y_true, remainder(yaw - yaw_true, 2 pi), landmark slot j: x_t[3+2j : 5+2j] -
map[ids[j]]), nees_full = e^T S^-1 e, nees_pose the same with the leading 3 x 3 block, map_rms the root mean square landmark error.
S and e are formed in fp64 exactly as the device forms them (one subtraction, one exact halving of one sum per element), so the
reference differs from the device in the factorisation and the solve alone."""
import math

import numpy as np

from test_cholesky_highprec import EPS, cholesky_hp

FULL_NOT_PD, POSE_NOT_PD, NO_TRUTH, INSTANCE_FAILED = 1, 2, 4, 8
NONFINITE, WATCHDOG = 1, 32            # the two slam_instance_flags after which the state is undefined
TWO_PI = 2 * 3.14159265358979323846    # filter.h:42

# exact chi-square quantiles (scipy.stats.chi2.ppf, recorded), dof -> values at P
CHI2_P = (0.005, 0.025, 0.05, 0.95, 0.975, 0.995)
CHI2_TABLE = {
    30: (13.78671985950272, 16.79077226556663, 18.49266098195347, 43.77297182574219, 46.97924224367115, 53.671961930240585),
    100: (67.32756330547916, 74.22192747492373, 77.92946516501726, 124.34211340400407, 129.5611971858366, 140.1694894423138),
    1000: (888.5635231814683, 914.257153799259, 927.594363020979, 1074.679448803441, 1089.5309127749135, 1118.9480663231916),
    6750208: (6740747.409621069, 6743008.416024964, 6744165.465996011, 6756252.808061891, 6757411.372586716, 6759676.103574161),
}


def symmetric_part(P):
    P = np.asarray(P, dtype=np.float64)
    return 0.5 * (P + P.T)


def error_vector(x, M, ids, truth, map_xy):
    """e in fp64, the device's operations: a subtraction per component, the heading wrapped by the IEEE remainder (math.remainder is
    C's remainder: x - n y with n = x / y rounded to nearest, ties to even)."""
    e = np.empty(3 + 2 * M)
    e[0] = x[0] - truth[0]
    e[1] = x[1] - truth[1]
    e[2] = math.remainder(x[2] - truth[2], TWO_PI) if np.isfinite(x[2] - truth[2]) else np.nan
    for j in range(M):
        e[3 + 2 * j:5 + 2 * j] = x[3 + 2 * j:5 + 2 * j] - map_xy[ids[j]]
    return e


def solve_hp(S, e):
    """(y, z, bad): y = L^-1 e and z = S^-1 e in longdouble from the right-looking longdouble Cholesky factor S = L L^T; bad = index
    of the first pivot that is not positive and finite (then y, z are None), else None."""
    L, piv = cholesky_hp(S)
    fin = np.isfinite(piv.astype(np.float64)) & (piv > 0)
    if L is None or not fin.all():
        return None, None, int(np.argmin(fin))
    n = S.shape[0]
    e = np.asarray(e, dtype=np.float64).astype(np.longdouble)
    y = np.zeros(n, dtype=np.longdouble)
    for i in range(n):
        y[i] = (e[i] - L[i, :i] @ y[:i]) / L[i, i]
    z = np.zeros(n, dtype=np.longdouble)
    for i in range(n - 1, -1, -1):
        z[i] = (y[i] - L[i + 1:, i] @ z[i + 1:]) / L[i, i]
    return y, z, None


def nees_hp(S, e):
    y, _, bad = solve_hp(S, e)
    return None if bad is not None else y @ y


def nees_double_routes(S, e):
    """e^T S^-1 e by three plain fp64 routes: LAPACK Cholesky + triangular solve, LU solve, explicit inverse."""
    S = np.asarray(S, dtype=np.float64); e = np.asarray(e, dtype=np.float64)
    out = []
    try:
        y = _forward(np.linalg.cholesky(S), e)
        out.append(float(y @ y))
    except np.linalg.LinAlgError:
        out.append(float("nan"))
    out.append(float(e @ np.linalg.solve(S, e)))
    out.append(float(e @ (np.linalg.inv(S) @ e)))
    return out


def _forward(L, e):
    try:
        from scipy.linalg import solve_triangular
        return solve_triangular(L, e, lower=True)
    except ImportError:   # scipy is not required: plain fp64 forward substitution
        y = np.zeros_like(e)
        for i in range(e.size):
            y[i] = (e[i] - L[i, :i] @ y[:i]) / L[i, i]
        return y


def reference(x, P, M, ids, truth, map_xy, status=0, id_known=True):
    """All five outputs for one instance, plus what the judging rule needs: dict(nees_full, nees_pose, map_rms [longdouble or NaN],
    dof, flags, S, e, z_full, z_pose).  x [n], P [n][n], ids [M], truth [3], map_xy [L][2]; the rules of slam_consistency_flags."""
    n = 3 + 2 * M
    nan = np.longdouble("nan")
    out = dict(nees_full=nan, nees_pose=nan, map_rms=nan, dof=n, flags=0, S=None, e=None, z_full=None, z_pose=None)
    if status & (NONFINITE | WATCHDOG):
        out["flags"] = INSTANCE_FAILED
        return out
    x = np.asarray(x, dtype=np.float64)[:n]; ids = np.asarray(ids)[:M]; map_xy = np.asarray(map_xy, dtype=np.float64)
    no_truth = (not id_known and M > 0) or bool(np.any((ids < 0) | (ids >= map_xy.shape[0])))
    e = error_vector(x, 0 if no_truth else M, ids, truth, map_xy)
    if not np.all(np.isfinite(e)):
        out["flags"] = INSTANCE_FAILED
        return out
    nf = e.size
    S = symmetric_part(np.asarray(P, dtype=np.float64)[:n, :n])[:nf, :nf]
    out["S"], out["e"] = S, e
    flags = NO_TRUTH if no_truth else 0
    y, z, bad = solve_hp(S, e)
    if bad is not None:
        flags |= FULL_NOT_PD | (POSE_NOT_PD if bad < 3 else 0)
        if bad >= 3:
            y3, z3, _ = solve_hp(S[:3, :3], e[:3])
            out["nees_pose"], out["z_pose"] = y3 @ y3, z3
    else:
        out["nees_pose"] = y[:3] @ y[:3]
        out["z_pose"] = solve_hp(S[:3, :3], e[:3])[1]
        if not no_truth:
            out["nees_full"], out["z_full"] = y @ y, z
    if not no_truth:
        d = e[3:].astype(np.longdouble)
        out["map_rms"] = np.sqrt((d @ d) / M) if M > 0 else np.longdouble(0)
    out["flags"] = flags
    return out


# ---- the judging rule ---------------------------------------------------------------------------------------------------------------
# For an instance with reference value v, z = S^-1 e and n rows, a backward error of gamma_n ||S|| in the solve moves e^T S^-1 e by
# n u ||S||_2 ||z||_2^2 to first order (u = 2^-53).  The figure of a computed value w is g = |w - v| / (n u ||S||_2 ||z||_2^2).  A pool
# is the set of instances of one kind; G is the largest g any of the three fp64 routes reaches on any instance of the pool.  The bar
# for every instance of the pool: g <= 10 G (the project's margin for sums formed in another order), and never above 4
# (gamma_{3n+1} ~ 4 n u is Higham's constant for the Cholesky solve).
MARGIN, CAP = 10.0, 4.0


def figure(w, v, S, z):
    n = S.shape[0]
    unit = n * EPS * float(np.linalg.norm(S, 2)) * float(z @ z)
    return abs(float(np.longdouble(w) - v)) / unit


def judge(pool):
    """pool: [(device value, reference value v, S, e, z)] of one kind.  Returns (G, g_dev_max, bar, [index of every instance above
    the bar or not finite])."""
    G, gd = 0.0, []
    for w, v, S, e, z in pool:
        for r in nees_double_routes(S, e):
            G = max(G, figure(r, v, S, z))
        gd.append(figure(w, v, S, z) if np.isfinite(w) else float("inf"))
    bar = min(MARGIN * G, CAP)
    return G, max(gd), bar, [i for i, g in enumerate(gd) if not g <= bar]


def map_rms_bound(M):
    """relative error of the fp64 map_rms: M squared terms, a sum, a division, a square root."""
    return (2 * M + 4) * EPS


def not_pd_matrix(rng, n, k, dk=-1e-6):
    """S = L D L^T, exactly symmetric, ||S|| ~ 1: L unit lower-triangular with small entries, D in [0.5, 1] except D_k = dk.  The
    exact Cholesky pivots of S are the D_j, so pivot k is the first that is not positive (rounding S to fp64 moves it by ~1e-16)."""
    L = np.tril(rng.uniform(-0.3, 0.3, (n, n)) / np.sqrt(n), -1).astype(np.longdouble) + np.eye(n, dtype=np.longdouble)
    D = rng.uniform(0.5, 1.0, n).astype(np.longdouble)
    D[k] = dk
    S = ((L * D[None, :]) @ L.T).astype(np.float64)
    return np.tril(S) + np.tril(S, -1).T
