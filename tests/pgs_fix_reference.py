"""Float64 reference of the pose graph's absolute fixes (unary position / heading factors on a pose), shared by tests/test_pgs_fix_cpu.py and
tests/test_pgs_fix_gpu.py.  Built by composition on tests/pgs_robust_reference.py and tests/pgs_step_reference.py, which it changes nothing in.

The oracle exports the Gaussian graph of prior, between and bearing-range factors.  A fix at pose i (x, y, th) is the row
{z_x, z_y, z_yaw, sigma_pos, sigma_yaw} with kinds (1: position, 2: heading) and APPENDS rows to the oracle's Jacobian and residual, in the
local coordinates of the oracle's retraction (translation in the pose's frame, then yaw):

    position   e = ((x - z_x) / sigma_pos, (y - z_y) / sigma_pos)       J = [[c, -s, 0], [s, c, 0]] / sigma_pos
    heading    e = remainder(th - z_yaw, 2 pi) / sigma_yaw               J = [0, 0, 1 / sigma_yaw]

Each part may carry the fix loss (pgs_robust_reference.loss on r = |e_part|): it is linearised as sw e, sw J with the weight at the
linearisation point and costs rho; the landmark factors' own loss goes through pgs_robust_reference.weigh.  FixGraph.jacobian() returns the
weighted rows (for pgs_step_reference.StepSystem and pgs_marginals_reference.judge).  lm_solve() is the dense Levenberg-Marquardt loop with
pgs_decide_kernel's constants and logic of pgs_robust_reference.lm_solve over such a graph: oldLin is the cost itself while no factor carries
a loss, and the weighted linearised cost at delta = 0 as soon as one does.  A plain helper module (no fixtures)."""
import math

import numpy as np

import pgs_robust_reference as RR
import pgs_step_reference as R

POS, YAW = 1, 2
ABSENT, STORED, INVALID = 0, 1, 4
NONE, HUBER, GEMAN_MCCLURE = RR.NONE, RR.HUBER, RR.GEMAN_MCCLURE


def verdict(row, kinds):
    """position | heading << 4 of one row as pgs_fix validates it."""
    row = np.asarray(row, dtype=np.float64)

    def part(bit, zs, sigma):
        if not kinds & bit:
            return ABSENT
        return STORED if all(math.isfinite(v) for v in zs) and math.isfinite(sigma) and sigma > 0.0 else INVALID
    return part(POS, row[:2], row[3]) | (part(YAW, row[2:3], row[4]) << 4)


def fix_parts(pose, row, kinds):
    """The stored parts of one fix at `pose`, position before heading: [(part index 0 | 1, e (rows,), J (rows, 3))], without the loss."""
    x, y, th = (float(v) for v in pose)
    out = []
    if kinds & POS:
        wp = 1.0 / row[3]
        c, s = math.cos(th), math.sin(th)
        out.append((0, np.array([(x - row[0]) * wp, (y - row[1]) * wp]), np.array([[c * wp, -s * wp, 0.0], [s * wp, c * wp, 0.0]])))
    if kinds & YAW:
        wy = 1.0 / row[4]
        out.append((1, np.array([math.remainder(th - row[2], R.TWO_PI) * wy]), np.array([[0.0, 0.0, wy]])))
    return out


def _loss1(kind, k, ss):
    rho, w, sw = RR.loss(kind, k, np.array([math.sqrt(ss)]))
    return float(rho[0]), float(w[0]), float(sw[0])


class FixGraph:
    """An oracle graph g with fixes: fix [N][5], kinds [N] (0: none at that pose; only STORED parts), the fix loss and the landmark loss
    as (kind, k).  values() and retract() are the oracle's."""

    def __init__(self, g, fix, kinds, fix_loss=(NONE, 0.0), lm_loss=(NONE, 0.0)):
        self.g = g
        self.fix = np.asarray(fix, dtype=np.float64).reshape(-1, 5)
        self.kinds = np.asarray(kinds, dtype=np.int64).reshape(-1)
        self.fix_loss, self.lm_loss = fix_loss, lm_loss

    def values(self, which=0):
        return self.g.values(which)

    def retract(self, poses, lms, dp, dl):
        return self.g.retract(poses, lms, dp, dl)

    @property
    def any_loss(self):
        return self.lm_loss[0] != NONE or (self.fix_loss[0] != NONE and bool(self.kinds.any()))

    def weigh(self, poses, lms):
        """The weighted linearisation at (poses, lms): the oracle's rows through pgs_robust_reference.weigh (the landmark loss), then the
        fix rows in pose order, position before heading.  dict(rows, cols, vals, e, n, lm (that weigh's dict), fix_w, fix_rho [N][2]: NaN
        where no part is stored)."""
        poses = np.asarray(poses, dtype=np.float64)
        lms = np.asarray(lms, dtype=np.float64).reshape(-1, 2)
        L = RR.weigh(self.g, poses, lms, *self.lm_loss)
        N = poses.shape[0]
        rows, cols, vals, e = [], [], [], []
        m = len(L["e"])
        fw, frho = np.full((N, 2), np.nan), np.full((N, 2), np.nan)
        for i in np.flatnonzero(self.kinds[:N]):
            for part, ep, Jp in fix_parts(poses[i], self.fix[i], int(self.kinds[i])):
                rho, w, sw = _loss1(self.fix_loss[0], self.fix_loss[1], float(np.sum(ep * ep)))
                fw[i, part], frho[i, part] = w, rho
                for r in range(len(ep)):
                    rows += [m] * 3
                    cols += [3 * i, 3 * i + 1, 3 * i + 2]
                    vals += [sw * Jp[r, 0], sw * Jp[r, 1], sw * Jp[r, 2]]
                    e.append(sw * ep[r])
                    m += 1
        return dict(rows=np.concatenate([L["rows"], np.asarray(rows, dtype=L["rows"].dtype)]),
                    cols=np.concatenate([L["cols"], np.asarray(cols, dtype=L["cols"].dtype)]),
                    vals=np.concatenate([L["vals"], np.asarray(vals, dtype=np.float64)]),
                    e=np.concatenate([L["e"], np.asarray(e, dtype=np.float64)]), n=L["n"], lm=L, fix_w=fw, fix_rho=frho)

    def jacobian(self, poses, lms):
        W = self.weigh(poses, lms)
        return W["rows"], W["cols"], W["vals"], W["e"]

    def cost(self, poses, lms):
        """sum rho: pgs_robust_reference.cost of the oracle's factors plus rho of every stored fix part."""
        poses = np.asarray(poses, dtype=np.float64)
        lms = np.asarray(lms, dtype=np.float64).reshape(-1, 2)
        c = RR.cost(self.g, RR.factor_rows(self.g, poses, lms), poses, lms, *self.lm_loss)
        for i in np.flatnonzero(self.kinds[:poses.shape[0]]):
            for _, ep, _ in fix_parts(poses[i], self.fix[i], int(self.kinds[i])):
                c += _loss1(self.fix_loss[0], self.fix_loss[1], float(np.sum(ep * ep)))[0]
        return float(c)


def system(fg, poses, lms, lam):
    """(StepSystem of the graph with its fixes, the linearisation of FixGraph.weigh)."""
    W = fg.weigh(poses, lms)
    return R.StepSystem(W["rows"], W["cols"], W["vals"], W["e"], W["n"], lam), W


def lm_solve(fg, solver="chol", max_trials=RR.MAX_TRIALS):
    """pgs_robust_reference.lm_solve over a FixGraph (the same loop, constants and margins; see there for the returned dict)."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.sparse import csr_matrix
    v = fg.values(0)
    poses, lms = v["poses"].copy(), v["landmarks"].copy().reshape(-1, 2)
    N, M = poses.shape[0], lms.shape[0]
    error = fg.cost(poses, lms)
    err_init = cur_error = error
    lam, iters, trials, flags, margin = RR.LAMBDA0, 0, 0, 0, 1.0
    done = False
    while not done:
        W = fg.weigh(poses, lms)
        n = W["n"]
        J = csr_matrix((W["vals"], (W["rows"], W["cols"])), shape=(len(W["e"]), n)).toarray()
        ew = W["e"]
        old_lin = float(0.5 * np.sum(ew * ew)) if fg.any_loss else error
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
                pn, ln = fg.retract(poses, lms, delta[:3 * N].reshape(N, 3), delta[3 * N:].reshape(M, 2))
                ln = ln.reshape(-1, 2)[:M]
                new_error = fg.cost(pn, ln)
                lin_change = old_lin - new_lin
                margin = min(margin, RR._margin(lin_change, 2.220446049250313e-16 * old_lin))
                if lin_change >= 0.0:
                    cost_change = error - new_error
                    if lin_change > 2.220446049250313e-16 * old_lin:
                        success = cost_change / lin_change > RR.MIN_FIDELITY
                        margin = min(margin, RR._margin(cost_change / lin_change, RR.MIN_FIDELITY))
                    if abs(cost_change) < RR.REL_TOL * error:
                        stop = True
                    margin = min(margin, RR._margin(abs(cost_change), RR.REL_TOL * error))
            trials += 1
            if success:
                lam, error, iters, end_inner = lam / RR.LAMBDA_FACTOR, new_error, iters + 1, True
                poses, lms = pn, ln
            elif not stop:
                lam *= RR.LAMBDA_FACTOR
                if lam >= RR.LAMBDA_UPPER:
                    end_inner = True
            else:
                end_inner = True
            if success:
                break
        if end_inner:
            abs_dec = cur_error - error
            rel_dec = abs_dec / cur_error
            if not np.isfinite(error):
                done, flags = True, RR.FLAG_NONFINITE
            elif iters >= RR.MAX_ITER:
                done, flags = True, RR.FLAG_NOT_CONVERGED
            else:
                if abs_dec != 0.0:
                    margin = min(margin, RR._margin(rel_dec, RR.REL_TOL), RR._margin(abs_dec, RR.ABS_TOL))
                if error <= 0.0 or rel_dec <= RR.REL_TOL or abs_dec <= RR.ABS_TOL:
                    done = True
                else:
                    cur_error = error
        if not done and trials >= max_trials:
            done, flags = True, RR.FLAG_NOT_CONVERGED
    return dict(poses=poses, landmarks=lms, iterations=iters, trials=trials, flags=flags, err_init=err_init, err_final=error, lam=lam,
                margin=margin)


# ----------------------------------------------------------------------------------------------------------------------------
# the cases of the tests
# ----------------------------------------------------------------------------------------------------------------------------
_CASES = {}


def case(name):
    """Scenario `name` of tests/test_pgs_step_gpu.py's table with its clean streams: dict(st, N, KP, L_max, cfg, graphs, Ms).  Once."""
    if name not in _CASES:
        import test_pgs_step_gpu as T
        from live_ekf_slam_amd.config import default_config
        from oracle import oracle as O
        N, Ms, per_pose, KP, L_max, opt = T.SCENARIOS[name]
        cfg = default_config()
        st = R.make_streams(N, Ms, per_pose, 1000 + len(name) * 7 + N, **opt)
        _CASES[name] = dict(st=st, N=N, KP=KP, L_max=L_max, cfg=cfg, graphs=R.build_oracle_graphs(O, cfg, st, N, L_max, KP), Ms=list(Ms))
    return _CASES[name]


def placement(N, path):
    """The poses of the placement test's fixes in a graph of N poses: pose 0 (with the prior), separators of the path's segmentation,
    segment-interior poses, the last pose.  (Separators are the multiples of the segment length: 5, 10 under seg5, 2, 4 under seg2, 32, 64
    by default; the sequential chain has none and gets seg5's poses.)  A graph of more than 64 separators also gets them at the separators
    64 and 65 (the segments beside them run in the first lanes of the segment chain kernel's second wavefront), at the last separator
    NS = (N - 2) / sl (the last row of what the separator kernel stages) and at the one before."""
    lengths = {"seg5": 5, "seg2": 2, "default": 32}
    sl = lengths.get(path, 5)
    want = [0, 3, sl, 2 * sl, 2 * sl + 1, sl + 2, N - 1]
    NS = (N - 2) // sl
    if path in lengths and NS > 64:
        want += [64 * sl, 65 * sl, (NS - 1) * sl, NS * sl]
    return sorted({i for i in want if 0 <= i < N})


def place_fixes(sc, path, seed=0):
    """Fixes for every instance of case `sc` at placement(): rows near the truth (0.05 m, 0.02 rad off, sigma 0.1 m / 0.05 rad), the kinds
    cycling position-only, heading-only, both; the LAST instance of the batch carries none.  Returns (fix [B][N][5], kinds [B][N])."""
    rng = np.random.default_rng(4242 + seed)
    st, N = sc["st"], sc["N"]
    B = st["cnt"].shape[0]
    fix, kinds = np.zeros((B, N, 5)), np.zeros((B, N), dtype=np.int32)
    for b in range(B - 1):
        for q, i in enumerate(placement(N, path)):
            x, y, th = st["truth"][i]
            fix[b, i] = (x + rng.uniform(-0.05, 0.05), y + rng.uniform(-0.05, 0.05), math.remainder(th + rng.uniform(-0.02, 0.02), R.TWO_PI), 0.1, 0.05)
            kinds[b, i] = (POS, YAW, POS | YAW)[(q + b) % 3]
            if not kinds[b, i] & POS:
                fix[b, i, [0, 1, 3]] = 0.0     # what pgs_get_fixes returns of a part that was never stored
            if not kinds[b, i] & YAW:
                fix[b, i, [2, 4]] = 0.0
    return fix, kinds


# The effect inputs (chosen on the CPU, tests/test_pgs_fix_cpu.py): 34 poses whose landmarks are out of view on the poses 11 .. 22, an
# odometry that reads 4 % long and 0.004 rad per step to the left - inside its sigmas of 0.01 m / 0.01 rad per step, so the graph cannot
# tell - and a position fix of sigma EFFECT_SIGMA at every pose from 1 on, EFFECT_NOISE m off the truth at most.
EFFECT_N, EFFECT_MS, EFFECT_SIGMA, EFFECT_NOISE, EFFECT_JUMP, EFFECT_JUMP_EVERY = 34, [0, 5, 9, 12], 0.1, 0.03, 3.0, 7
EFFECT_GM_K = 3.0


def effect_case():
    """dict(st (streams with the biased odometry), N, KP, L_max, cfg, graphs, fix, kinds (clean fixes [B][N][5] / [B][N]), fix_jump (the same
    with EFFECT_JUMP m added to every EFFECT_JUMP_EVERY-th fix of an instance), jumped [B][N])."""
    if "effect" not in _CASES:
        from live_ekf_slam_amd.config import default_config
        from oracle import oracle as O
        N, KP, L_max = EFFECT_N, 8, 12
        cfg = default_config()
        st = R.make_streams(N, EFFECT_MS, 8, 77, window=6, quiet=((11, 23),))
        st = dict(st)
        st["cmds"] = (st["cmds"].astype(np.float64) * np.array([1.04, 1.0]) + np.array([0.0, 0.004])).astype(np.float32)
        rng = np.random.default_rng(99)
        B = len(EFFECT_MS)
        fix, kinds = np.zeros((B, N, 5)), np.zeros((B, N), dtype=np.int32)
        jumped = np.zeros((B, N), dtype=bool)
        for b in range(B):
            for i in range(1, N):
                fix[b, i] = (st["truth"][i, 0] + rng.uniform(-EFFECT_NOISE, EFFECT_NOISE), st["truth"][i, 1] + rng.uniform(-EFFECT_NOISE, EFFECT_NOISE),
                             0.0, EFFECT_SIGMA, 0.0)
                kinds[b, i] = POS
                jumped[b, i] = (i + b) % EFFECT_JUMP_EVERY == 0
        fix_jump = fix.copy()
        ang = rng.uniform(-math.pi, math.pi, (B, N))
        fix_jump[..., 0] += np.where(jumped, EFFECT_JUMP * np.cos(ang), 0.0)
        fix_jump[..., 1] += np.where(jumped, EFFECT_JUMP * np.sin(ang), 0.0)
        _CASES["effect"] = dict(st=st, N=N, KP=KP, L_max=L_max, cfg=cfg, graphs=R.build_oracle_graphs(O, cfg, st, N, L_max, KP), Ms=list(EFFECT_MS),
                                fix=fix, kinds=kinds, fix_jump=fix_jump, jumped=jumped)
    return _CASES["effect"]


def position_error(poses, truth):
    """Mean distance of the poses' (x, y) from the truth's."""
    return float(np.mean(np.hypot(poses[:, 0] - truth[:, 0], poses[:, 1] - truth[:, 1])))
