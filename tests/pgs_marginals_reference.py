"""Reference and yardstick for the marginal covariances of the pose-graph solver (pgs_marginals), shared by
tests/test_pgs_marginals_reference.py (CPU: the reference itself) and tests/test_pgs_marginals_gpu.py (the device against it).

For an oracle graph g at values (poses, lms), J = the whitened Jacobian of all factors (OraclePoseGraph.jacobian) and H = J^T J without
damping: the marginal covariance of a variable is its diagonal block of H^-1 (gtsam::Marginals::marginalCovariance).  The reference
inverts H with a double Cholesky and refines X <- X + H^-1 (I - J^T (J X)) with J sparse in np.longdouble until the correction stops
shrinking: it ends 2 - 7e-18 relative on every diagonal block, far below anything it is compared with.

Figure of merit of a computed set of blocks: max over the diagonal blocks of max|S - S_ref| / max|S_ref| (maxima over a block's entries).

The bar of a computed set (judge()): kappa_1(H) is 1e9 - 3e11 here (the prior is loose against the odometry), so the derived forward
bound BOUND_C n u kappa_1 is 1e3 - 1e6 times looser than what double arithmetic does and alone would pass a wrong kernel.  The bar is
therefore 10 x the rounding spread of the instance - the larger figure of merit of two independent double routes on the CPU, LAPACK's
Cholesky solve and LU inverse of H - and never above the derived bound.  10 is the project's margin for results whose sums the MFMA
forms in another order.  A plain helper module (no fixtures)."""
import functools

import numpy as np

import pgs_step_reference as R

MARGIN = 10.0
PRIOR_SIGMAS = (1.3, 1.3, 1.2)      # pose_graph.cpp:83


def split_blocks(X, N, M):
    """Diagonal blocks of a dense (3N + 2M)^2 matrix: (pose [N][3][3], landmark [M][2][2])."""
    ip = 3 * np.arange(N)[:, None] + np.arange(3)[None, :]
    il = 3 * N + 2 * np.arange(M)[:, None] + np.arange(2)[None, :]
    return X[ip[:, :, None], ip[:, None, :]], X[il[:, :, None], il[:, None, :]]


def figure_of_merit(pose_cov, lm_cov, ref_pose, ref_lm):
    """max over diagonal blocks of max|S - S_ref| / max|S_ref|."""
    worst = 0.0
    for a, r in ((pose_cov, ref_pose), (lm_cov, ref_lm)):
        a, r = np.asarray(a, dtype=np.longdouble), np.asarray(r, dtype=np.longdouble)
        if r.shape[0] == 0:
            continue
        assert a.shape == r.shape, (a.shape, r.shape)
        d = np.abs(a - r).reshape(r.shape[0], -1).max(axis=1) / np.abs(r).reshape(r.shape[0], -1).max(axis=1)
        if not np.all(np.isfinite(d.astype(np.float64))):
            return float("inf")
        worst = max(worst, float(d.max()))
    return worst


def unconstrained_landmarks(g, poses, lms):
    """Landmarks of the oracle graph without any factor (both Jacobian columns empty): H is singular, GTSAM throws
    IndeterminantLinearSystemException, the device reports status 1."""
    poses = np.asarray(poses, dtype=np.float64)
    M = np.asarray(lms).reshape(-1, 2).shape[0]
    _, cols, _, _ = g.jacobian(poses, np.asarray(lms, dtype=np.float64).reshape(-1, 2))
    used = np.zeros(3 * poses.shape[0] + 2 * M, dtype=bool)
    used[cols] = True
    lm_used = used[3 * poses.shape[0]:].reshape(M, 2)
    return np.flatnonzero(~lm_used.any(axis=1))


def judge(g, poses, lms, max_rounds=8):
    """Reference blocks, yardstick and bar of the oracle graph g at (poses [N][3], lms [M][2]).  Returns dict(pose_cov, lm_cov
    (np.longdouble), last_correction, rounds, kappa, bound, spread, spread_chol, spread_lu, bar, n); for a structurally singular
    graph dict(singular=[landmarks without a factor])."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.linalg.lapack import dpocon
    from scipy.sparse import csr_matrix
    poses = np.ascontiguousarray(poses, dtype=np.float64)
    lms = np.ascontiguousarray(lms, dtype=np.float64).reshape(-1, 2)
    N, M = poses.shape[0], lms.shape[0]
    n = 3 * N + 2 * M
    loose = unconstrained_landmarks(g, poses, lms)
    if len(loose):
        return dict(singular=loose, n=n)
    rows, cols, vals, e = g.jacobian(poses, lms)
    m = len(e)
    J = csr_matrix((vals, (rows, cols)), shape=(m, n))
    H = (J.T @ J).toarray()
    c, low = cho_factor(H, lower=True)
    eye = np.eye(n)
    X_chol = cho_solve((c, low), eye)
    X_lu = np.linalg.inv(H)
    Jl = csr_matrix((vals.astype(np.longdouble), (rows, cols)), shape=(m, n))
    JlT = Jl.T.tocsr()
    X = X_chol.astype(np.longdouble)
    eye_l = np.eye(n, dtype=np.longdouble)
    last, rounds = np.inf, 0
    for rounds in range(1, max_rounds + 1):
        res = eye_l - JlT @ (Jl @ X)
        D = cho_solve((c, low), res.astype(np.float64))
        Xn = X + D.astype(np.longdouble)
        dp, dl = split_blocks(D, N, M)
        xp, xl = split_blocks(Xn, N, M)
        corr = float(max((np.abs(a).reshape(a.shape[0], -1).max(axis=1) / np.abs(b).reshape(b.shape[0], -1).max(axis=1)).max()
                         for a, b in ((dp, xp), (dl, xl)) if a.shape[0]))
        if corr > 0.5 * last:      # the long-double limit is reached: keep the iterate before a correction that no longer shrinks
            break
        X, last = Xn, corr
    normH = float(np.abs(H).sum(axis=1).max())
    rcond, info = dpocon(c, normH, uplo="L")
    assert info == 0
    kappa = 1.0 / rcond if rcond > 0 else np.inf
    ref_p, ref_l = split_blocks(X, N, M)
    s_chol = figure_of_merit(*split_blocks(X_chol, N, M), ref_p, ref_l)
    s_lu = figure_of_merit(*split_blocks(X_lu, N, M), ref_p, ref_l)
    spread = max(s_chol, s_lu)
    bound = R.BOUND_C * n * R.U * kappa
    return dict(pose_cov=ref_p, lm_cov=ref_l, last_correction=last, rounds=rounds, kappa=kappa, bound=bound, spread=spread,
                spread_chol=s_chol, spread_lu=s_lu, bar=min(MARGIN * spread, bound), n=n, N=N, M=M)


@functools.lru_cache(maxsize=None)
def scenario(name):
    """Streams and oracle graphs of one scenario of tests/test_pgs_step_gpu.py's table (the device graphs are built from the same
    streams by test_pgs_step_gpu._device)."""
    import test_pgs_step_gpu as T
    from live_ekf_slam_amd.config import default_config
    from oracle import oracle as O
    N, Ms, per_pose, KP, L_max, opt = T.SCENARIOS[name]
    cfg = default_config()
    st = R.make_streams(N, Ms, per_pose, 1000 + len(name) * 7 + N, **opt)
    gs = R.build_oracle_graphs(O, cfg, st, N, L_max, KP)
    return dict(st=st, N=N, KP=KP, L_max=L_max, cfg=cfg, graphs=gs, Ms=list(Ms))


@functools.lru_cache(maxsize=None)
def judged_at_initial(name, instance):
    """judge() of one instance of a scenario at the oracle's own initial estimate (the CPU yardstick test)."""
    g = scenario(name)["graphs"][instance]
    v = g.values(0)
    return judge(g, v["poses"], v["landmarks"])
