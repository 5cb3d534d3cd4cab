"""The reference's goal-pursuit controller for a batch of instances, on the host (numpy, no GPU needed).

`PurePursuitBatch.next_cmds(estimates)` is one tick of goal_pursuit_node.py:23-50 for every instance: PurePursuit.get_next_cmd with
pare_path / choose_lookahead_pt / cmd_loose / cmd_tight (nav_method "pp") or PurePursuit.direct_nav ("direct"), pure_pursuit.py:17-161.
It restates csrc/nav_kernel.h operation for operation - the device kernel behind slam_nav_run compiles that header - so that the host
route (poses -> next_cmds -> run_sim with per-instance commands) and the device route issue the same float32 commands, bit for bit:

  * arithmetic in fp64, one IEEE operation at a time (numpy never fuses a multiply with an add);
  * powers as multiplication chains: x^4 = (x x)(x x), x^12 = x^8 x^4 by squaring, the cube of direct_nav x x x; distances by sqrt;
  * atan2 = det_atan2 below, the library's deterministic atan2 (csrc/slam_math.h) ported operation for operation;
  * the heading error is the IEEE remainder(., 2 pi);
  * the estimate is the state message's wire value (float32 x_v, y_v, yaw_v), the command is rounded to float32 after the clamps.

The reference's goal_queue is always a suffix of the path it was given (pare_path deletes up to the FIRST queued waypoint within 0.15 m,
direct_nav pops the front), so the queue of instance b is path[head[b]:].  Guards the reference lacks: consecutive equal waypoints are
refused (it divides by zero there); a frozen instance or a non-finite estimate gets (0, 0) and keeps its controller state.
"""
import math

import numpy as np

PP, DIRECT = 0, 1
LOOSE, TIGHT = 0, 1
MAX_WAYPOINTS = 1024
MAX_RADII = 64
PARE_RADIUS = 0.15            # pure_pursuit.py:91,159
TAU = 2 * 3.14159265358979323846
PI = 3.141592653589793

_rem_any = np.frompyfunc(lambda v: math.remainder(v, TAU), 1, 1)


def rem2pi(x):
    """IEEE remainder(x, 2 pi), elementwise (slam_math.h rem2pi: exact subtractions for |x| <= 4 pi, math.remainder beyond)."""
    x = np.asarray(x, dtype=np.float64)
    ax = np.abs(x)
    d = ax - TAU
    r = np.where(ax > PI, np.where(d >= PI, d - TAU, d), ax)
    r = np.where(np.signbit(x), -r, r)
    far = ~(ax <= 2.0 * TAU)
    if np.any(far):
        r = r.copy()
        r[far] = _rem_any(x[far]).astype(np.float64)
    return r


def det_atan(x):
    """slam_math.h det_atan, operation for operation (fdlibm's argument reduction and degree-11 odd polynomial)."""
    hi = (4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00)
    lo = (2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17)
    a = (3.33333333333329318027e-01, -1.99999999998764832476e-01, 1.42857142725034663711e-01, -1.11111104054623557880e-01,
         9.09088713343650656196e-02, -7.69187620504482999495e-02, 6.66107313738753120669e-02, -5.83357013379057348645e-02,
         4.97687799461593236017e-02, -3.65315727442169155270e-02, 1.62858201153657823623e-02)
    x = np.asarray(x, dtype=np.float64)
    neg = x < 0.0
    ax0 = np.abs(x)
    with np.errstate(all="ignore"):
        r0 = (2.0 * ax0 - 1.0) / (2.0 + ax0)
        r1 = (ax0 - 1.0) / (ax0 + 1.0)
        r2 = (ax0 - 1.5) / (1.0 + 1.5 * ax0)
        r3 = -1.0 / ax0
        idn = np.where(ax0 < 0.4375, -1, np.where(ax0 < 0.6875, 0, np.where(ax0 < 1.1875, 1, np.where(ax0 < 2.4375, 2, 3))))
        ax = np.choose(idn + 1, [ax0, r0, r1, r2, r3])
        h = np.choose(idn + 1, [0.0, hi[0], hi[1], hi[2], hi[3]])
        l = np.choose(idn + 1, [0.0, lo[0], lo[1], lo[2], lo[3]])
        z = ax * ax
        w = z * z
        s1 = z * (a[0] + w * (a[2] + w * (a[4] + w * (a[6] + w * (a[8] + w * a[10])))))
        s2 = w * (a[1] + w * (a[3] + w * (a[5] + w * (a[7] + w * a[9]))))
        res = np.where(idn < 0, ax - ax * (s1 + s2), h - ((ax * (s1 + s2) - l) - ax))
    res = np.where(ax0 >= 73786976294838206464.0, hi[3] + lo[3], res)
    return np.where(neg, -res, res)


def det_atan2(y, x):
    """slam_math.h det_atan2 for finite arguments, operation for operation (NaN propagates)."""
    pi, pi_lo, pi_o_2 = 3.1415926535897931160E+00, 1.2246467991473531772E-16, 1.5707963267948965580E+00
    y, x = np.broadcast_arrays(np.asarray(y, dtype=np.float64), np.asarray(x, dtype=np.float64))
    xneg, yneg = np.signbit(x), np.signbit(y)
    with np.errstate(all="ignore"):
        z = det_atan(np.abs(y / x))
        res = np.where(~xneg, np.where(yneg, -z, z), np.where(yneg, (z - pi_lo) - pi, pi - (z - pi_lo)))
    res = np.where(x == 0.0, np.where(yneg, -pi_o_2, pi_o_2), res)
    res = np.where(y == 0.0, np.where(~xneg, y, np.where(yneg, -pi, pi)), res)
    return np.where((x != x) | (y != y), x + y, res)


def check_config(dt, lookahead_dist_init, lookahead_dist_max, method, control):
    """The checks of slam_nav_set_path on the controller configuration (ValueError instead of SLAM_ERR_ARG)."""
    if not (dt > 0.0 and math.isfinite(dt)):
        raise ValueError(f"dt = {dt} must be positive and finite")
    if not (lookahead_dist_init > 0.0 and math.isfinite(lookahead_dist_init) and lookahead_dist_max > 0.0 and math.isfinite(lookahead_dist_max)):
        raise ValueError(f"lookahead distances {lookahead_dist_init} .. {lookahead_dist_max} must be positive and finite")
    d, radii = lookahead_dist_init, 0
    while d <= lookahead_dist_max:
        radii += 1
        if radii > MAX_RADII:
            raise ValueError(f"more than {MAX_RADII} lookahead radii between {lookahead_dist_init} and {lookahead_dist_max}")
        d *= 1.25
    if method not in (PP, DIRECT) or control not in (LOOSE, TIGHT):
        raise ValueError(f"unknown method {method} or control {control}")


def check_path(pts):
    """One path [P][2]: 1 <= P <= 1024, finite, no two consecutive waypoints equal."""
    pts = np.asarray(pts, dtype=np.float64)
    if pts.ndim != 2 or pts.shape[1] != 2 or not 1 <= pts.shape[0] <= MAX_WAYPOINTS:
        raise ValueError(f"expected a path of shape (1 <= P <= {MAX_WAYPOINTS}, 2), got {pts.shape}")
    if not np.all(np.isfinite(pts)):
        raise ValueError("a waypoint is not finite")
    if np.any(np.all(pts[1:] == pts[:-1], axis=1)):
        raise ValueError("two consecutive waypoints are equal: the reference divides by zero there (pure_pursuit.py:124)")
    return pts


class PurePursuitBatch:
    """Controller state and tick for `batch` instances.

    paths: one (P, 2) path for all instances, or a list of `batch` paths, or a (batch, P_stride, 2) array with `counts`.
    d_max, th_max: constraints.commands of the filter's config (params.yaml:27-28)."""

    def __init__(self, batch, paths, counts=None, dt=0.05, lookahead_dist_init=0.2, lookahead_dist_max=2.0, method=PP, control=LOOSE,
                 d_max=0.1, th_max=0.0546):
        check_config(dt, lookahead_dist_init, lookahead_dist_max, method, control)
        self.batch = int(batch)
        self.dt, self.la_init, self.la_max = float(dt), float(lookahead_dist_init), float(lookahead_dist_max)
        self.method, self.control, self.d_max, self.th_max = int(method), int(control), float(d_max), float(th_max)
        if isinstance(paths, (list, tuple)) and len(paths) and np.ndim(paths[0]) == 2:
            plist = [check_path(p) for p in paths]
            if len(plist) != self.batch:
                raise ValueError(f"expected {self.batch} paths, got {len(plist)}")
            self.plen = np.array([p.shape[0] for p in plist], dtype=np.int32)
            self.pts = np.zeros((self.batch, int(self.plen.max()), 2))
            for b, p in enumerate(plist):
                self.pts[b, :p.shape[0]] = p
        else:
            arr = np.asarray(paths, dtype=np.float64)
            if arr.ndim == 2:
                arr = check_path(arr)
                self.pts = np.broadcast_to(arr, (self.batch,) + arr.shape)
                self.plen = np.full(self.batch, arr.shape[0], dtype=np.int32)
            else:
                if arr.ndim != 3 or arr.shape[0] != self.batch or arr.shape[2] != 2:
                    raise ValueError(f"expected per-instance paths of shape ({self.batch}, P_stride, 2), got {arr.shape}")
                self.plen = (np.full(self.batch, arr.shape[1], np.int32) if counts is None else np.asarray(counts, dtype=np.int32))
                if self.plen.shape != (self.batch,) or np.any(self.plen > arr.shape[1]):
                    raise ValueError("counts: expected one waypoint count per instance, at most P_stride")
                for b in range(self.batch):
                    check_path(arr[b, :max(int(self.plen[b]), 0)])
                self.pts = arr
        self._rows = np.arange(self.batch)
        self.reset()

    def reset(self):
        """What slam_init / setting a path do to the controller state."""
        self.head = np.zeros(self.batch, dtype=np.int32)
        self.integ = np.zeros(self.batch)
        self.err_prev = np.zeros(self.batch)
        self.finish_tick = np.full(self.batch, -1, dtype=np.int32)
        self.tick = 0

    @property
    def remaining(self):
        return (self.plen - self.head).astype(np.int32)

    def _pt(self, idx):
        """Waypoint idx[b] of instance b (idx clipped into the path: masked lanes only)."""
        i = np.clip(idx, 0, self.plen - 1)
        return self.pts[self._rows, i, 0], self.pts[self._rows, i, 1]

    def _clamp(self, fwd, ang):
        f = np.where(self.d_max < fwd, self.d_max, fwd)
        a = np.where(self.th_max < ang, self.th_max, ang)
        return np.where(f > 0.0, f, 0.0).astype(np.float32), np.where(a > -self.th_max, a, -self.th_max).astype(np.float32)

    def next_cmds(self, estimates, frozen=None):
        """estimates: (batch, 3) x_v, y_v, yaw_v (rounded to float32 here, as the state message does); frozen: optional (batch,) mask.
        Returns the (batch, 2) float32 commands (fwd, ang) and advances the controller state by one tick."""
        est = np.asarray(estimates, dtype=np.float32).astype(np.float64)
        if est.shape != (self.batch, 3):
            raise ValueError(f"estimates: expected shape ({self.batch}, 3), got {est.shape}")
        ex, ey, eyaw = est[:, 0], est[:, 1], est[:, 2]
        active = np.isfinite(ex) & np.isfinite(ey) & np.isfinite(eyaw)
        if frozen is not None:
            active &= ~np.asarray(frozen, dtype=bool)
        cmd = np.zeros((self.batch, 2), dtype=np.float32)
        tick = self.tick
        with np.errstate(all="ignore"):
            if self.method == DIRECT:
                self._direct(ex, ey, eyaw, active, tick, cmd)
            else:
                self._pp(ex, ey, eyaw, active, tick, cmd)
        self.tick += 1
        return cmd

    def _direct(self, ex, ey, eyaw, active, tick, cmd):          # direct_nav, pure_pursuit.py:135-161
        empty = active & (self.head >= self.plen)
        self.finish_tick[empty & (self.finish_tick < 0)] = tick
        live = active & ~empty
        gx, gy = self._pt(self.head)
        rx, ry = ex - gx, ey - gy
        r = np.sqrt(rx * rx + ry * ry)
        beta = rem2pi(det_atan2(gy - ey, gx - ex) - eyaw)
        y = 1.0 - np.abs(beta) / self.th_max
        fwd = np.where(r > 0.1, 1.0 * (y * y * y) + 0.05, 0.0)
        f, a = self._clamp(fwd, beta)
        cmd[live, 0] = f[live]; cmd[live, 1] = a[live]
        pop = live & (r < PARE_RADIUS)
        self.head[pop] += 1
        self.finish_tick[pop & (self.head >= self.plen) & (self.finish_tick < 0)] = tick + 1

    def _pp(self, ex, ey, eyaw, active, tick, cmd):              # get_next_cmd, pure_pursuit.py:40-81
        pmax = self.pts.shape[1]
        # pare_path (85-94): the FIRST queued waypoint within 0.15 m, whichever it is
        done = ~active
        head0 = self.head.copy()
        for i in range(int(head0[active].min()) if np.any(active) else pmax, pmax):
            cand = ~done & (i >= head0) & (i < self.plen)
            if not np.any(cand):
                continue
            dx, dy = ex - self.pts[:, i, 0], ey - self.pts[:, i, 1]
            hit = cand & (np.sqrt(dx * dx + dy * dy) < PARE_RADIUS)
            self.head[hit] = i + 1
            done |= hit
        empty = active & (self.head >= self.plen)                # 49-51
        self.finish_tick[empty & (self.finish_tick < 0)] = tick
        live = active & ~empty
        if not np.any(live):
            return
        # lookahead point (54-63, choose_lookahead_pt 98-131)
        head = self.head
        hx, hy = self._pt(head)
        lx, ly = hx.copy(), hy.copy()
        multi = live & (self.plen - head > 1)
        found = np.zeros(self.batch, dtype=bool)
        dist = self.la_init
        while dist <= self.la_max:
            search = multi & ~found
            if not np.any(search):
                break
            for i in range(int(head[search].min()) + 1, int(self.plen[search].max())):
                seg = search & (i > head) & (i < self.plen)
                if not np.any(seg):
                    continue
                px, py, qx, qy = self.pts[:, i - 1, 0], self.pts[:, i - 1, 1], self.pts[:, i, 0], self.pts[:, i, 1]
                dfx, dfy = qx - px, qy - py
                vx, vy = px - ex, py - ey
                a = dfx * dfx + dfy * dfy
                b = 2.0 * (vx * dfx + vy * dfy)
                c = vx * vx + vy * vy - dist * dist
                arg = b * b - 4.0 * a * c
                discr = np.sqrt(arg)
                q0, q1 = (-b - discr) / (2.0 * a), (-b + discr) / (2.0 * a)
                ok = seg & ~(arg < 0.0)
                v0 = ok & (q0 >= 0.0) & (q0 <= 1.0)
                v1 = ok & ~v0 & (q1 >= 0.0) & (q1 <= 1.0)
                lx = np.where(v0, px + q0 * dfx, np.where(v1, px + q1 * dfx, lx))
                ly = np.where(v0, py + q0 * dfy, np.where(v1, py + q1 * dfy, ly))
                found |= v0 | v1
            dist *= 1.25
        beta = rem2pi(det_atan2(ly - ey, lx - ex) - eyaw)
        integ = self.integ + beta * self.dt
        x = 1.0 - np.abs(beta / PI)
        x2 = x * x
        x4 = x2 * x2
        if self.control == TIGHT:                                # cmd_tight, 28-37
            ang = 0.5 * beta + 0.0 * integ + 0.0 * (beta - self.err_prev) / self.dt
            x8 = x4 * x4
            fwd = 0.02 * (x8 * x4) + 0.01
        else:                                                    # cmd_loose, 17-26
            ang = 0.9 * beta + 0.01 * integ + 0.4 * (beta - self.err_prev) / self.dt
            fwd = x4 + 0.05
        f, a = self._clamp(fwd, ang)
        cmd[live, 0] = f[live]; cmd[live, 1] = a[live]
        self.integ = np.where(live, integ, self.integ)
        self.err_prev = np.where(live, beta, self.err_prev)


def kinematic_step(pose, cmd):
    """The simulator's noise-free motion model (sim_node.py:222) for a closed-loop dry run on the host: pose (.., 3), cmd (.., 2)."""
    pose = np.asarray(pose, dtype=np.float64)
    cmd = np.asarray(cmd, dtype=np.float64)
    out = pose.copy()
    out[..., 0] = pose[..., 0] + cmd[..., 0] * np.cos(pose[..., 2])
    out[..., 1] = pose[..., 1] + cmd[..., 0] * np.sin(pose[..., 2])
    out[..., 2] = pose[..., 2] + cmd[..., 1]
    return out
