"""Extended-precision reference for ONE Levenberg-Marquardt step of the pose-graph solver, shared by tests/test_pgs_step_reference.py
(CPU: the reference itself) and tests/test_pgs_step_gpu.py (every device solve path against it).

A step solves the damped normal equations A delta = b, A = J^T J + lam I, b = -J^T e, of the whitened sparse Jacobian J and residual e
the oracle exports (OraclePoseGraph.jacobian).  The reference solves once with a double Cholesky of A and refines with residuals
b - A delta accumulated in np.longdouble, A applied as J^T (J delta) + lam delta - A is never formed in double for a residual.  A step is
judged by its normwise backward error

    eta(delta) = |b - A delta|_inf / (|A|_inf |delta|_inf + |b|_inf),

which does not grow with the condition of A: a backward-stable solve (Cholesky in any elimination order) gives eta of a few n u whatever
kappa(A) is, so the bound stays tight on ill-conditioned graphs.  The forward error is then bounded by about eta kappa(A).

The device returns x1 = x0 (+) delta, not delta: recover_step() inverts the oracle's retraction and says how much rounding that adds.
make_streams() builds the host measurement streams of a ragged batch with every instance's landmark count and detections chosen exactly.
This is a plain helper module (no fixtures)."""
import math

import numpy as np

U = 2.0 ** -53                      # unit roundoff of float64
TWO_PI = 6.283185307179586          # slam::kTwoPi, the constant of the oracle's and the device's remainder()
BOUND_C = 8                         # eta <= BOUND_C n u: see test_pgs_step_reference.py for the calibration


class StepSystem:
    """A = J^T J + lam I and b = -J^T e of one graph at given values, with J kept sparse (sorted by row and by column for the two
    products).  Dense A in double exists only for the factorisation and the norms."""

    def __init__(self, rows, cols, vals, e, n, lam):
        self.n, self.lam = int(n), float(lam)
        self.m = len(e)
        self.rows, self.cols, self.vals, self.e = rows, cols, vals, e
        self._rstart = np.flatnonzero(np.r_[True, rows[1:] != rows[:-1]]) if len(rows) else np.zeros(0, dtype=np.int64)
        self._rid = rows[self._rstart] if len(rows) else rows
        order = np.argsort(cols, kind="stable")
        self._corder = order
        cs = cols[order]
        self._cstart = np.flatnonzero(np.r_[True, cs[1:] != cs[:-1]]) if len(cs) else np.zeros(0, dtype=np.int64)
        self._cid = cs[self._cstart] if len(cs) else cs
        self.vals_ld = vals.astype(np.longdouble)
        self.b_ld = -self.JT(e.astype(np.longdouble))
        self.b = self.b_ld.astype(np.float64)
        from scipy.sparse import csr_matrix
        Js = csr_matrix((vals, (rows, cols)), shape=(self.m, self.n))
        self.A = (Js.T @ Js).toarray()
        self.A[np.diag_indices(self.n)] += self.lam
        self.normA = float(np.abs(self.A).sum(axis=1).max()) if self.n else 0.0   # |A|_inf = |A|_1 (symmetric)

    def J(self, x):          # J x, x longdouble [n] -> [m]
        out = np.zeros(self.m, dtype=np.longdouble)
        if len(self.rows):
            out[self._rid] = np.add.reduceat(self.vals_ld * x[self.cols], self._rstart)
        return out

    def JT(self, y):         # J^T y, y [m] -> [n] (longdouble)
        out = np.zeros(self.n, dtype=np.longdouble)
        if len(self.cols):
            prod = (self.vals.astype(np.longdouble) * y[self.rows])[self._corder]
            out[self._cid] = np.add.reduceat(prod, self._cstart)
        return out

    def residual(self, delta):
        """b - A delta in np.longdouble, A applied as J^T (J delta) + lam delta."""
        d = np.asarray(delta).astype(np.longdouble)
        return self.b_ld - (self.JT(self.J(d)) + np.longdouble(self.lam) * d)

    def eta(self, delta):
        """Normwise backward error of delta (residual in np.longdouble)."""
        r = float(np.abs(self.residual(delta)).max()) if self.n else 0.0
        den = self.normA * float(np.abs(np.asarray(delta, dtype=np.float64)).max(initial=0.0)) + float(np.abs(self.b).max(initial=0.0))
        return r / den if den > 0 else 0.0

    def eta_of_error(self, eps, delta):
        """An error eps (componentwise bound) on delta pushed through the same norm: |A eps|_inf <= |A|_inf |eps|_inf."""
        den = self.normA * float(np.abs(np.asarray(delta, dtype=np.float64)).max(initial=0.0)) + float(np.abs(self.b).max(initial=0.0))
        return self.normA * float(np.max(eps, initial=0.0)) / den if den > 0 else 0.0


def reference_step(sys_, max_rounds=5):
    """delta_ref (np.longdouble) of A delta = b: a double Cholesky solve, refined with longdouble residuals.  Returns (delta_ref,
    kappa_1(A) from LAPACK dpocon on the double factor, rounds).

    Accuracy: the residuals carry a 64-bit mantissa, so the refinement converges to about kappa 2^-64 |delta| (forward), not to a few u:
    the correction cannot fall below 1e-3 u |delta| once kappa exceeds ~2e3, which is every graph here.  The loop therefore stops at that
    level OR once a correction no longer halves (the long-double limit is reached), at the latest after max_rounds rounds.  kappa 2^-64 is
    2^-11 of the forward tolerance the GPU test allows (BOUND_C n u kappa |delta|) and its backward error is ~1e-20: the reference is
    exact for every comparison made with it (test_pgs_step_reference.test_refined_step_agrees_with_a_50_digit_solve)."""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.linalg.lapack import dpocon
    n = sys_.n
    if n == 0:
        return np.zeros(0, dtype=np.longdouble), 1.0, 0
    c, low = cho_factor(sys_.A, lower=True)
    delta = cho_solve((c, low), sys_.b).astype(np.longdouble)
    rounds, last = 0, np.inf
    for rounds in range(1, max_rounds + 1):
        d = cho_solve((c, low), sys_.residual(delta).astype(np.float64))
        delta = delta + d.astype(np.longdouble)
        dn = float(np.abs(d).max())
        if dn <= 1e-3 * U * float(np.abs(delta).max()) or dn > 0.5 * last:
            break
        last = dn
    rcond, info = dpocon(c, sys_.normA, uplo="L")
    assert info == 0
    return delta, (1.0 / rcond if rcond > 0 else np.inf), rounds


def system_of(g, poses, lms, lam):
    """StepSystem of the oracle graph g at (poses [N][3], lms [M][2])."""
    rows, cols, vals, e = g.jacobian(poses, lms)
    n = 3 * poses.shape[0] + 2 * np.asarray(lms).reshape(-1, 2).shape[0]
    return StepSystem(rows, cols, vals, e, n, lam)


def factor_pairs(g, poses, lms):
    """(pose, landmark) of every bearing-range factor of the oracle graph g, in the order of its residuals (from the Jacobian's rows)."""
    rows, cols, _, _ = g.jacobian(poses, lms)
    N = poses.shape[0]
    lm_entry = cols >= 3 * N
    pose_of_row = np.full(rows.max() + 1 if len(rows) else 0, N, dtype=np.int64)
    np.minimum.at(pose_of_row, rows[~lm_entry], cols[~lm_entry] // 3)
    r = rows[lm_entry][::4]                      # four landmark entries per bearing-range factor (2 rows x 2 columns)
    return pose_of_row[r], (cols[lm_entry][::4] - 3 * N) // 2


def predict_plan(pairs, N, start, max_lm=63, max_sep=128):
    """The segment length pgs_solve takes for a batch whose factors are `pairs` (one (pose, landmark) array pair per instance), starting
    from `start` poses per segment (0: the sequential chain): the longest of start, start / 2, ... (>= 8) whose every segment's interior
    poses see at most max_lm landmarks and whose separators number at most max_sep; 0 when none does (pgs_capi.cpp, pgs_seg_plan_kernel)."""
    SL = start
    while SL > 0:
        NS = (N - 2) // SL if N >= 2 else 0
        mx = 0
        if NS > max_sep:
            mx = 1 << 30
        else:
            for pose, lm in pairs:
                interior = (pose % SL != 0) | (pose == 0) | (pose > NS * SL)
                seg = np.where(pose == 0, 0, (pose - 1) // SL)
                seg = np.minimum(seg, NS)
                for p in np.unique(seg[interior]):
                    mx = max(mx, len(np.unique(lm[interior & (seg == p)])))
        if mx <= max_lm:
            return SL
        nxt = SL // 2
        if mx == 1 << 30 or nxt < 8 or (N - 2) // nxt > max_sep:
            return 0
        SL = nxt
    return 0


def pack(dp, dl):
    return np.concatenate([np.asarray(dp).reshape(-1), np.asarray(dl).reshape(-1)])


def recover_step(p0, l0, p1, l1):
    """Inverse of the oracle's retraction x1 = x0 (+) delta (pose: p0 + R(th0) (dp0, dp1), remainder(th0 + dp2, 2 pi); landmark: l0 + dl).
    Returns (delta packed as [poses..., landmarks...], eps_rec): eps_rec = 4 u (|x0| + |x1|) componentwise bounds the rounding of the
    retraction and of this inverse; for the two rotated components |x0| + |x1| sums both coordinates of the two poses (the rotation mixes
    them)."""
    p0, p1 = np.asarray(p0, dtype=np.float64), np.asarray(p1, dtype=np.float64)
    l0, l1 = np.asarray(l0, dtype=np.float64).reshape(-1, 2), np.asarray(l1, dtype=np.float64).reshape(-1, 2)
    c, s = np.cos(p0[:, 2]), np.sin(p0[:, 2])
    dx, dy = p1[:, 0] - p0[:, 0], p1[:, 1] - p0[:, 1]
    dp = np.empty_like(p0)
    dp[:, 0] = c * dx + s * dy
    dp[:, 1] = -s * dx + c * dy
    dp[:, 2] = [math.remainder(a - b, TWO_PI) for a, b in zip(p1[:, 2], p0[:, 2])]
    ep = np.empty_like(p0)
    ep[:, 0] = ep[:, 1] = 4 * U * (np.abs(p0[:, :2]).sum(axis=1) + np.abs(p1[:, :2]).sum(axis=1))
    ep[:, 2] = 4 * U * (np.abs(p0[:, 2]) + np.abs(p1[:, 2]))
    el = 4 * U * (np.abs(l0) + np.abs(l1))
    return pack(dp, l1 - l0), pack(ep, el)


# ----------------------------------------------------------------------------------------------------------------------------
# host measurement streams
# ----------------------------------------------------------------------------------------------------------------------------
def sep_last_landmark(M, at_last, sep_only):
    """Index of the landmark make_streams(sep_last=True) places at the last separator in an instance of M landmarks (None: the instance
    has no landmark left for it: at_last and sep_only took them, or M is too small)."""
    free = M - at_last
    if free <= sep_only:
        return None
    taken = {(q * 7 + 3) % free for q in range(sep_only)}
    j = (sep_only * 7 + 3) % free
    return None if j in taken else j


def make_streams(N, Ms, per_pose, seed, *, window=24, new_last=False, at_last=0, sep_only=0, SL=32, quiet=(), far_once=0,
                 empty_every=0, radius=3.0, sep_last=False):
    """Host streams of a batch of len(Ms) graphs of N poses (N - 1 updates after init(0, 0, 0)) in which instance b creates exactly
    Ms[b] landmarks.  The truth drives a circle of `radius` round (0, radius) with the shared commands (0.1 m, 0.1 / radius rad); the maps
    lie near it, so |x| stays small against |delta|.  Landmark j of an instance is in view on the poses [s_j, s_j + window) (s_j spread
    evenly over the chain); a pose's message lists up to per_pose landmarks in view, landmarks not yet seen first (new_last: LAST, so
    that in a message longer than the handle's k_per_pose their detections are dropped while their landmarks are created - the first
    factor comes later).  Measurements: range / bearing from the truth plus 0.02 m / 0.01 rad noise.  Secondary-filter poses: the truth
    moved 0.1 - 0.5 m in a random direction and 0.05 rad in yaw.
      at_last:     the last `at_last` landmarks are first seen at the last pose
      sep_only:    that many landmarks are seen only from separator poses (multiples of SL)
      quiet:       (lo, hi) pose ranges without detections
      far_once:    that many landmarks are seen exactly once, 9 - 10 m away
      empty_every: poses t with t % empty_every == 0 have no detections
      sep_last:    one more landmark (sep_last_landmark) is seen only from the LAST three separators, (NS - 2) SL, (NS - 1) SL and NS SL with
                   NS = (N - 2) / SL: pose NS SL and row NS - 1 of whatever is staged per separator carry a landmark no interior pose sees.
                   (Off, it draws nothing: every stream built without it keeps its bits.)
    Returns dict(cmds [N-1][2] f32, meas [B][N-1][K][3] f32, cnt [B][N-1] i32, sec [B][N-1][3], truth [N][3])."""
    rng = np.random.default_rng(seed)
    B, T = len(Ms), N - 1
    cmd = np.array([0.1, 0.1 / radius], dtype=np.float32)
    cmds = np.tile(cmd, (T, 1))
    truth = np.zeros((N, 3))
    for t in range(T):
        x, y, th = truth[t]
        truth[t + 1] = (x + float(cmd[0]) * math.cos(th), y + float(cmd[0]) * math.sin(th), th + float(cmd[1]))
    wrap = lambda a: (a + math.pi) % (2 * math.pi) - math.pi   # noqa: E731
    quiet_pose = np.zeros(N, dtype=bool)
    for lo, hi in quiet:
        quiet_pose[lo:hi] = True
    if empty_every:
        quiet_pose[::empty_every] = True
    per_inst = []
    for b in range(B):
        M = int(Ms[b])
        start = np.array([1 + (j * max(T - 1, 0)) // max(M, 1) for j in range(M)], dtype=np.int64)
        wlen = np.full(M, window, dtype=np.int64)
        only_sep = np.zeros(M, dtype=bool)
        far = np.zeros(M, dtype=bool)
        pos = np.zeros((M, 2))
        for j in range(M - at_last, M):                         # first seen at the last pose
            if j >= 0:
                start[j], wlen[j] = T, 1
        seps = np.arange(SL, T + 1, SL)
        for q in range(min(sep_only, max(M - at_last, 0))):    # seen only from separator poses
            if len(seps) == 0:
                break
            j = (q * 7 + 3) % max(M - at_last, 1)
            s0 = seps[q % len(seps)]
            start[j], wlen[j], only_sep[j] = s0, 2 * SL + 1, True
        j = sep_last_landmark(M, at_last, sep_only) if sep_last else None
        if j is not None and (N - 2) // SL >= 3:                # seen only from the last three separators
            start[j], wlen[j], only_sep[j] = ((N - 2) // SL - 2) * SL, 2 * SL + 1, True
        for q in range(min(far_once, M)):                      # seen once, near the far end of the range
            j = (q * 5 + 1) % M
            if only_sep[j] or start[j] == T:
                continue
            while quiet_pose[start[j]] and start[j] < T:
                start[j] += 1
            wlen[j], far[j] = 1, True
        for j in range(M):
            tv = int(min(start[j] + wlen[j] // 2, T))
            if far[j]:
                x, y, th = truth[int(start[j])]
                r, a = rng.uniform(9.0, 10.0), rng.uniform(-1.2, 1.2)
                pos[j] = (x + r * math.cos(th + a), y + r * math.sin(th + a))
            else:
                x, y, th = truth[tv]
                r, a = rng.uniform(0.5, 2.5), rng.uniform(-1.5, 1.5)
                pos[j] = (x + r * math.cos(th + a), y + r * math.sin(th + a))
        per_inst.append((start, wlen, only_sep, pos))
    msgs = [[[] for _ in range(T)] for _ in range(B)]
    for b in range(B):
        start, wlen, only_sep, pos = per_inst[b]
        M = len(start)
        seen = np.zeros(M, dtype=bool)
        for t in range(1, N):
            must = [j for j in range(M) if start[j] == t and not seen[j]]   # a landmark's first pose always lists it
            if quiet_pose[t] and not must:
                continue
            view = [j for j in range(M) if start[j] <= t < start[j] + wlen[j] and (not only_sep[j] or t % SL == 0)]
            new = [j for j in view if not seen[j]]
            old = [j for j in view if seen[j]]
            if old:
                rot = t % len(old)
                old = old[rot:] + old[:rot]
            room = max(per_pose - len(new), 0)
            chosen = (old[:room] + new) if new_last else (new + old[:room])
            if quiet_pose[t]:
                chosen = must
            for j in chosen:
                seen[j] = True
            x, y, th = truth[t]
            for j in chosen:
                dx, dy = pos[j, 0] - x, pos[j, 1] - y
                r = math.hypot(dx, dy) + rng.normal(0.0, 0.02)
                br = wrap(math.atan2(dy, dx) - th + rng.normal(0.0, 0.01))
                msgs[b][t - 1].append((100 + j, r, br))
        assert seen.all(), f"instance {b}: {int((~seen).sum())} landmark(s) never listed"
    K = max(1, max(len(m) for mb in msgs for m in mb))
    meas = np.zeros((B, T, K, 3), dtype=np.float32)
    cnt = np.zeros((B, T), dtype=np.int32)
    for b in range(B):
        for t in range(T):
            m = msgs[b][t]
            cnt[b, t] = len(m)
            if m:
                meas[b, t, :len(m)] = np.asarray(m, dtype=np.float32)
    sec = np.zeros((B, T, 3))
    for b in range(B):
        mag = rng.uniform(0.1, 0.5, T)
        ang = rng.uniform(-math.pi, math.pi, T)
        sec[b, :, 0] = truth[1:, 0] + mag * np.cos(ang)
        sec[b, :, 1] = truth[1:, 1] + mag * np.sin(ang)
        sec[b, :, 2] = np.array([wrap(a) for a in truth[1:, 2]]) + rng.choice([-1.0, 1.0], T) * rng.uniform(0.03, 0.05, T)
    return dict(cmds=cmds, meas=meas, cnt=cnt, sec=sec, truth=truth)


def build_oracle_graphs(O, cfg, st, N, L_max, KP):
    """One OraclePoseGraph per instance fed the streams of make_streams (init(0, 0, 0), then per update the secondary pose and the
    message, as pgs_update gets them)."""
    B, T = st["cnt"].shape
    gs = []
    for b in range(B):
        g = O.OraclePoseGraph(cfg, N_max=N, L_max=L_max, KP=KP)
        g.init(0.0, 0.0, 0.0)
        for t in range(T):
            g.updateNaiveVehPoseEstimate(st["sec"][b, t])
            g.update(st["cmds"][t, 0], st["cmds"][t, 1], st["meas"][b, t, :st["cnt"][b, t]])
        gs.append(g)
    return gs
