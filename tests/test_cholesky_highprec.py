"""A high-precision Cholesky factor and the SPD test matrices that tests/test_ukf_chol_kernel_gpu.py feeds ukf_chol_kernel, checked on
the CPU: the factor against LAPACK and against mpmath at 50 digits, the matrices against the condition numbers and pivots they are
built to have."""
import numpy as np
import pytest

EPS = 2.0 ** -53
LD_EPS = float(np.finfo(np.longdouble).eps)


def cholesky_hp(Y):
    """Right-looking Cholesky of the fp64 matrix Y (lower triangle read) in np.longdouble (64-bit significand on x86-64).
    Returns (L, pivots): L in longdouble, or None when a pivot is not positive; pivots d_k = L_kk^2 up to the first bad one."""
    A = np.tril(np.asarray(Y, dtype=np.float64)).astype(np.longdouble)
    n = A.shape[0]
    L = np.zeros_like(A)
    piv = []
    for k in range(n):
        d = A[k, k]
        piv.append(d)
        if not d > 0:
            return None, np.array(piv)
        L[k, k] = np.sqrt(d)
        col = A[k + 1:, k] / L[k, k]
        L[k + 1:, k] = col
        A[k + 1:, k + 1:] -= np.tril(np.outer(col, col))
    return L, np.array(piv)


def gamma(k):
    return k * EPS / (1 - k * EPS)


def spd_with_condition(rng, n, kappa, top=10.0):
    """A A^T + c I with A of n/2 columns (so A A^T is singular and the shift alone sets the smallest eigenvalue), scaled to a largest
    eigenvalue near `top`: condition number about kappa.  Exactly symmetric."""
    A = rng.standard_normal((n, max(1, n // 2)))
    G = A @ A.T
    lmax = np.linalg.eigvalsh(G)[-1]
    c = lmax / (kappa - 1.0) if kappa > 1 else 1.0
    Y = (G + c * np.eye(n)) * (top / (lmax + c))
    return np.tril(Y) + np.tril(Y, -1).T


def spd_graded(rng, n, lo=1e-6, hi=1e6):
    """D^1/2 C D^1/2: a well-conditioned correlation matrix C graded by a diagonal D from lo to hi.  Exactly symmetric."""
    C = spd_with_condition(rng, n, 10.0)
    s = 1.0 / np.sqrt(np.diag(C))
    C = C * s[:, None] * s[None, :]
    d = np.sqrt(np.logspace(np.log10(lo), np.log10(hi), n))
    Y = C * d[:, None] * d[None, :]
    return np.tril(Y) + np.tril(Y, -1).T


def spd_with_pivot(rng, n, k, pivot):
    """A matrix whose exact k-th Cholesky pivot is `pivot` (the others near 1): L0 L0^T for a lower-triangular L0 with unit-scale
    entries and L0[k, k] = sqrt(pivot), formed in longdouble and rounded once.  Exactly symmetric."""
    L0 = np.tril(rng.uniform(-0.5, 0.5, (n, n))).astype(np.longdouble)
    L0[np.diag_indices(n)] = rng.uniform(0.8, 1.2, n)
    L0[k, k] = np.sqrt(np.longdouble(pivot))
    Y = (L0 @ L0.T).astype(np.float64)
    return np.tril(Y) + np.tril(Y, -1).T


def _mp_cholesky(Y, dps=50):
    import mpmath
    with mpmath.workdps(dps):
        A = mpmath.matrix(Y.tolist())
        return np.array(mpmath.cholesky(A).tolist(), dtype=object)


@pytest.mark.parametrize("n", [4, 17, 44, 104])
def test_matches_lapack(n):
    rng = np.random.default_rng(n)
    for kappa in (1e1, 1e4, 1e8):
        Y = spd_with_condition(rng, n, kappa)
        L, piv = cholesky_hp(Y)
        Ln = np.linalg.cholesky(Y)
        assert np.all(np.triu(L, 1) == 0) and np.all(piv > 0)
        err = np.linalg.norm((L - Ln).astype(np.float64)) / np.linalg.norm(Ln, 2)
        assert err <= n * EPS * kappa, (kappa, err)


@pytest.mark.parametrize("n,kappa", [(6, 1e1), (12, 1e8), (24, 1e4)])
def test_matches_mpmath_at_50_digits(n, kappa):
    """The longdouble factor is a reference for fp64: its error against a 50-digit factor is far below fp64's own n eps kappa."""
    Y = spd_with_condition(np.random.default_rng(7 * n), n, kappa)
    L, _ = cholesky_hp(Y)
    Lm = _mp_cholesky(Y)
    err = max(abs(float(Lm[i, j] - _mpf(L[i, j]))) for i in range(n) for j in range(n)) / float(np.abs(L).max())
    assert err <= 16 * n * LD_EPS * kappa, err


def _mpf(v):
    """A longdouble as an exact mpmath number: its 64-bit significand split into two fp64 halves."""
    import mpmath
    hi = np.float64(v)
    lo = np.float64(v - np.longdouble(hi))
    return mpmath.mpf(float(hi)) + mpmath.mpf(float(lo))


def test_refuses_an_indefinite_matrix():
    Y = spd_with_condition(np.random.default_rng(1), 10, 1e2)
    Y[9, 9] = -1.0
    L, piv = cholesky_hp(Y)
    assert L is None and len(piv) == 10 and piv[-1] < 0


@pytest.mark.parametrize("n", [4, 44, 104])
def test_constructed_matrices_have_their_condition_and_pivots(n):
    rng = np.random.default_rng(100 + n)
    for kappa in (1e1, 1e4, 1e8):
        Y = spd_with_condition(rng, n, kappa)
        ev = np.linalg.eigvalsh(Y)
        assert np.array_equal(Y, Y.T) and 0.5 * kappa <= ev[-1] / ev[0] <= 2 * kappa and 5 <= ev[-1] <= 20
    G = spd_graded(rng, n)
    assert np.array_equal(G, G.T) and cholesky_hp(G)[0] is not None
    assert np.isclose(G[0, 0], 1e-6) and np.isclose(G[-1, -1], 1e6)
    for k in sorted({0, n // 2, min(43, n - 1), min(44, n - 1), n - 1}):
        for p in (2e-8, 5e-9):
            Y = spd_with_pivot(rng, n, k, p)
            L, piv = cholesky_hp(Y)
            assert np.array_equal(Y, Y.T) and L is not None
            assert abs(float(piv[k]) / p - 1) < 1e-2, (k, piv[k])   # rounding Y to fp64 moves it by ~1e-12
            others = np.delete(piv.astype(np.float64), k)
            assert others.size == 0 or others.min() > 1e-3
