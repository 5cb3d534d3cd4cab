"""Float64 reference of the pose graph's robust loss (Huber, Geman-McClure on the bearing-range factors), shared by
tests/test_pgs_robust_cpu.py and tests/test_pgs_robust_gpu.py.  Built on tests/pgs_step_reference.py, which it changes nothing in.

The oracle exports the Gaussian graph: whitened residuals e and the sparse Jacobian J.  A robust factor with r = |e_factor| is
linearised as sw e, sw J (sw = sqrt(w), weight at the linearisation point) and costs rho(r):

    NONE            rho = 0.5 r^2                                   w = 1
    HUBER, k        rho = 0.5 r^2 (r <= k), k (r - 0.5 k) (r > k)   w = 1, k / r
    GEMAN_MCCLURE   rho = 0.5 k^2 r^2 / (k^2 + r^2)                 w = (k^2 / (k^2 + r^2))^2

so the weighted system is a row scaling of the oracle's.  lm_solve() is a dense Levenberg-Marquardt loop with pgs_decide_kernel's
constants and logic, oldLin being the linearised cost at delta = 0 (the Gaussian terms + sum 0.5 w r^2); it records how close each of its
comparisons came to its threshold.  corrupt() builds the outlier streams the tests use.  A plain helper module (no fixtures)."""
import numpy as np

import pgs_step_reference as R

NONE, HUBER, GEMAN_MCCLURE = 0, 1, 2
LAMBDA0, LAMBDA_FACTOR, LAMBDA_UPPER, MIN_FIDELITY, REL_TOL, ABS_TOL, MAX_ITER, MAX_TRIALS = 1e-5, 10.0, 1e5, 1e-3, 1e-5, 1e-5, 100, 400
FLAG_NOT_CONVERGED, FLAG_NONFINITE = 8, 16
OUTLIER_RANGE, OUTLIER_BEARING, OUTLIER_EVERY = 3.0, 0.5, 7


def loss(kind, k, r):
    """(rho, w, sw) of residual norms r (float64 array)."""
    r = np.asarray(r, dtype=np.float64)
    one = np.ones_like(r)
    if kind == NONE:
        return 0.5 * r * r, one, one
    if kind == HUBER:
        out = r > k
        safe = np.where(out, r, 1.0)
        w = np.where(out, k / safe, 1.0)
        return np.where(out, k * (r - 0.5 * k), 0.5 * r * r), w, np.sqrt(w)
    if kind == GEMAN_MCCLURE:
        q = (k * k) / (k * k + r * r)
        return 0.5 * k * k * (r * r / (k * k + r * r)), q * q, q
    raise ValueError(kind)


def factor_rows(g, poses, lms):
    """First row of every bearing-range factor of the oracle graph, in the order of its residuals (pose-major, slot order) - the rule of
    pgs_step_reference.factor_pairs: the rows with landmark entries, four entries (2 rows x 2 columns) per factor.  The second row follows."""
    rows, cols, _, _ = g.jacobian(poses, lms)
    lm_entry = cols >= 3 * np.asarray(poses).shape[0]
    first = rows[lm_entry][::4].astype(np.int64)
    assert np.array_equal(np.unique(rows[lm_entry]), np.sort(np.r_[first, first + 1]))
    return first


def weigh(g, poses, lms, kind, k):
    """The weighted linearisation at (poses, lms): dict(rows, cols, vals, e (scaled), first (factor rows), r, w, sw, rho (per factor),
    e0 (the oracle's residual), row_sw (per row), n)."""
    rows, cols, vals, e = g.jacobian(poses, lms)
    first = factor_rows(g, poses, lms)
    r = np.sqrt(e[first] * e[first] + e[first + 1] * e[first + 1])
    rho, w, sw = loss(kind, k, r)
    row_sw = np.ones(len(e))
    row_sw[first] = sw
    row_sw[first + 1] = sw
    n = 3 * np.asarray(poses).shape[0] + 2 * np.asarray(lms).reshape(-1, 2).shape[0]
    return dict(rows=rows, cols=cols, vals=vals * row_sw[rows], e=e * row_sw, first=first, r=r, w=w, sw=sw, rho=rho, e0=e, row_sw=row_sw, n=n)


def weighted_system(g, poses, lms, lam, kind, k):
    """(StepSystem of the weighted graph, the linearisation of weigh())."""
    L = weigh(g, poses, lms, kind, k)
    return R.StepSystem(L["rows"], L["cols"], L["vals"], L["e"], L["n"], lam), L


class WeightedGraph:
    """The oracle graph seen through the loss: jacobian() returns the weighted rows (for pgs_marginals_reference.judge)."""

    def __init__(self, g, kind, k):
        self.g, self.kind, self.k = g, kind, k

    def jacobian(self, poses, lms):
        L = weigh(self.g, np.asarray(poses, dtype=np.float64), np.asarray(lms, dtype=np.float64).reshape(-1, 2), self.kind, self.k)
        return L["rows"], L["cols"], L["vals"], L["e"]


def cost(g, first, poses, lms, kind, k):
    """sum rho: 0.5 |e|^2 of the prior and between rows, rho(r) of every bearing-range factor."""
    e = g.residuals(poses, lms)
    br = np.zeros(len(e), dtype=bool)
    br[first] = True
    br[first + 1] = True
    r = np.sqrt(e[first] ** 2 + e[first + 1] ** 2)
    return float(0.5 * np.sum(e[~br] ** 2) + np.sum(loss(kind, k, r)[0]))


def _margin(a, b):
    d = max(abs(a), abs(b))
    return abs(a - b) / d if d > 0 else 1.0


def lm_solve(g, kind, k, solver="chol", max_trials=MAX_TRIALS):
    """Dense LM from the oracle graph's initial estimate with pgs_decide_kernel's logic.  Returns dict(poses, landmarks, iterations,
    trials, flags, err_init, err_final, lam, margin): margin = the smallest relative distance of any accept / stop comparison from its
    threshold.  solver: "chol" (normal equations) or "qr" (the damped least-squares problem, no normal equations)."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.sparse import csr_matrix
    v = g.values(0)
    poses, lms = v["poses"].copy(), v["landmarks"].copy().reshape(-1, 2)
    N, M = poses.shape[0], lms.shape[0]
    first = factor_rows(g, poses, lms)
    error = cost(g, first, poses, lms, kind, k)
    err_init = cur_error = error
    lam, iters, trials, flags, margin = LAMBDA0, 0, 0, 0, 1.0
    done = False
    while not done:
        L = weigh(g, poses, lms, kind, k)
        n = L["n"]
        J = csr_matrix((L["vals"], (L["rows"], L["cols"])), shape=(len(L["e"]), n)).toarray()
        ew = L["e"]
        old_lin = error if kind == NONE else float(0.5 * np.sum(ew * ew))
        H, b = J.T @ J, -(J.T @ ew)
        end_inner = False
        while not end_inner and trials < max_trials:
            ok, success, stop = True, False, False
            try:
                if solver == "chol":
                    delta = cho_solve(cho_factor(H + lam * np.eye(n), lower=True), b)
                else:
                    delta = np.linalg.lstsq(np.vstack([J, np.sqrt(lam) * np.eye(n)]), np.r_[-ew, np.zeros(n)], rcond=None)[0]
            except np.linalg.LinAlgError:
                ok = False
            if ok:
                v_lin = J @ delta + ew
                new_lin = float(0.5 * np.sum(v_lin * v_lin))
                pn, ln = g.retract(poses, lms, delta[:3 * N].reshape(N, 3), delta[3 * N:].reshape(M, 2))
                ln = ln.reshape(-1, 2)[:M]
                new_error = cost(g, first, pn, ln, kind, k)
                lin_change = old_lin - new_lin
                # (lin_change >= 0 and lin_change > eps old_lin share the threshold eps old_lin: at 0 itself only the sign counts, and the
                # rounding of old_lin - new_lin is a few u old_lin, the same scale)
                margin = min(margin, _margin(lin_change, 2.220446049250313e-16 * old_lin))
                if lin_change >= 0.0:
                    cost_change = error - new_error
                    if lin_change > 2.220446049250313e-16 * old_lin:
                        success = cost_change / lin_change > MIN_FIDELITY
                        margin = min(margin, _margin(cost_change / lin_change, MIN_FIDELITY))
                    if abs(cost_change) < REL_TOL * error:
                        stop = True
                    margin = min(margin, _margin(abs(cost_change), REL_TOL * error))
            trials += 1
            if success:
                lam, error, iters, end_inner = lam / LAMBDA_FACTOR, new_error, iters + 1, True
                poses, lms = pn, ln
            elif not stop:
                lam *= LAMBDA_FACTOR
                if lam >= LAMBDA_UPPER:
                    end_inner = True
            else:
                end_inner = True
            if success:
                break
        if end_inner:
            abs_dec = cur_error - error
            rel_dec = abs_dec / cur_error
            if not np.isfinite(error):
                done, flags = True, FLAG_NONFINITE
            elif iters >= MAX_ITER:
                done, flags = True, FLAG_NOT_CONVERGED
            else:
                if abs_dec != 0.0:
                    margin = min(margin, _margin(rel_dec, REL_TOL), _margin(abs_dec, ABS_TOL))
                if error <= 0.0 or rel_dec <= REL_TOL or abs_dec <= ABS_TOL:
                    done = True
                else:
                    cur_error = error
        if not done and trials >= max_trials:
            done, flags = True, FLAG_NOT_CONVERGED
    return dict(poses=poses, landmarks=lms, iterations=iters, trials=trials, flags=flags, err_init=err_init, err_final=error, lam=lam,
                margin=margin)


def corrupt(st, seed):
    """A copy of the streams of pgs_step_reference.make_streams with outliers: of the non-first detections of every instance (message
    order; a landmark's first detection initialises it and stays clean) every OUTLIER_EVERY-th, from number seed % OUTLIER_EVERY on, gets
    +OUTLIER_RANGE m on its range and +OUTLIER_BEARING rad on its bearing.  Returns (streams, bad): bad [B][T][K] marks them."""
    out = dict(st)
    meas = st["meas"].copy()
    B, T, K, _ = meas.shape
    bad = np.zeros((B, T, K), dtype=bool)
    for b in range(B):
        seen, c = set(), seed % OUTLIER_EVERY
        for t in range(T):
            for s in range(int(st["cnt"][b, t])):
                i = int(meas[b, t, s, 0])
                if i not in seen:
                    seen.add(i)
                    continue
                if c % OUTLIER_EVERY == 0:
                    meas[b, t, s, 1] += np.float32(OUTLIER_RANGE)
                    meas[b, t, s, 2] += np.float32(OUTLIER_BEARING)
                    bad[b, t, s] = True
                c += 1
    out["meas"] = meas
    return out, bad


SEED = 3          # the outlier streams of the tests: chosen on the CPU so that the premises of tests/test_pgs_robust_gpu.py hold
_CASES = {}


def case(name, seed=SEED):
    """Scenario `name` of tests/test_pgs_step_gpu.py's table with outliers (corrupt(streams, seed)): dict(st (corrupted streams), clean,
    bad [B][T][K], N, KP, L_max, cfg, graphs (one oracle graph per instance, built from the corrupted streams), Ms).  Computed once."""
    if (name, seed) not in _CASES:
        import test_pgs_step_gpu as T
        from live_ekf_slam_amd.config import default_config
        from oracle import oracle as O
        N, Ms, per_pose, KP, L_max, opt = T.SCENARIOS[name]
        cfg = default_config()
        clean = R.make_streams(N, Ms, per_pose, 1000 + len(name) * 7 + N, **opt)
        st, bad = corrupt(clean, seed)
        gs = R.build_oracle_graphs(O, cfg, st, N, L_max, KP)
        _CASES[(name, seed)] = dict(st=st, clean=clean, bad=bad, N=N, KP=KP, L_max=L_max, cfg=cfg, graphs=gs, Ms=list(Ms))
    return _CASES[(name, seed)]


def bad_factors(sc, b):
    """Per stored factor of instance b, in the oracle's residual order (pose-major, slot order): True where the detection was corrupted.
    Detections beyond k_per_pose are not stored."""
    cnt, KP = sc["st"]["cnt"][b], sc["KP"]
    return np.concatenate([sc["bad"][b, t, :min(int(cnt[t]), KP)] for t in range(len(cnt))] + [np.zeros(0, dtype=bool)])
