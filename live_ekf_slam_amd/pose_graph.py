"""Host-side mirror of the reference's `PoseGraph : Filter` (GTSAM implementation) for a batch of graphs.

The reference drives ONE PoseGraph through (localization_node.cpp:90-140, pose_graph.cpp)
    readParams(config) -> init(x_0, y_0, yaw_0) -> per tick: updateNaiveVehPoseEstimate(secondary state) ->
    update(cmdMsg, lmMeasMsg) [solves + publishes when timestep+1 >= num_iterations, or every tick] -> publishState()
`BatchedPoseGraph` keeps those names, the stop/solve logic of PoseGraph::update (pose_graph.cpp:199-267) and the
exception-on-error convention for B Monte-Carlo instances; everything numeric happens in libslam_hip.so behind
include/slam_pgs.h.  `NaiveFilter` is the reference's secondary filter of params.yaml:60 (filter.h:325-369).
"""
import ctypes as C
import math

import numpy as np

from . import _lib
from .config import SlamConfig, default_config, FixSensorConfig, default_fix_sensor_config, FIX_POS, FIX_YAW   # noqa: F401
from ._marshal import Handle, Command, _d, _f, _i, opt

FIX_ABSENT, FIX_STORED, FIX_INVALID = 0, 1, 4            # pgs_fix_verdict (slam_pgs.h)


def fix_factor_host(pose, row, kinds, loss_kind=0, loss_k=0.0):
    """TEST HOOK (pgs_fix_factor_host): one fix factor at `pose` (x, y, yaw), the kernels' source compiled for the host; no GPU.  Returns
    dict(e (3,), J (3, 3) - rows 0, 1 position, row 2 heading, without the loss -, rho (2,), w (2,), verdict)."""
    p = np.ascontiguousarray(pose, dtype=np.float64); r = np.ascontiguousarray(row, dtype=np.float64)
    if p.shape != (3,) or r.shape != (5,):
        raise ValueError("pose (3,) and row (5,) expected")
    e = np.zeros(3); J = np.zeros((3, 3)); rho = np.zeros(2); w = np.zeros(2); v = C.c_int32(0)
    _lib.check(_lib.lib().pgs_fix_factor_host(_d(p), _d(r), int(kinds), int(loss_kind), float(loss_k), _d(e), _d(J), _d(rho), _d(w), C.byref(v)))
    return dict(e=e, J=J, rho=rho, w=w, verdict=v.value)


LOSS_NONE, LOSS_HUBER, LOSS_GEMAN_MCCLURE = 0, 1, 2      # pgs_loss_kind (slam_pgs.h)
LOSS_KINDS = {"none": LOSS_NONE, "huber": LOSS_HUBER, "geman_mcclure": LOSS_GEMAN_MCCLURE}


def robust_loss_host(kind, k, r):
    """TEST HOOK (pgs_robust_loss_host): (rho, w, sqrt(w)) of the loss at residual norm r, the kernels' source compiled for the host; no GPU."""
    rho, w, sw = C.c_double(0.0), C.c_double(0.0), C.c_double(0.0)
    _lib.check(_lib.lib().pgs_robust_loss_host(int(kind), float(k), float(r), C.byref(rho), C.byref(w), C.byref(sw)))
    return rho.value, w.value, sw.value


class NaiveFilter:
    """NaiveFilter (filter.h:325-369): propagate the commands, ignore the measurements.  Identical for every
    instance of a batch (it never sees instance-specific data), so one copy serves the whole batch."""

    def __init__(self):
        self.x_t = np.zeros(3)
        self.timestep = 0
        self.isInit = False
        self.lm_IDs = []

    def readParams(self, config=None):
        return self

    def init(self, x_0=0.0, y_0=0.0, yaw_0=0.0):
        self.timestep = 0
        self.x_t = np.array([float(np.float32(x_0)), float(np.float32(y_0)), float(np.float32(yaw_0))])
        self.isInit = True

    def update(self, cmdMsg, lmMeasMsg=None):
        fwd, ang = (cmdMsg.fwd, cmdMsg.ang) if isinstance(cmdMsg, Command) else (float(np.float32(cmdMsg[0])), float(np.float32(cmdMsg[1])))
        self.timestep += 1
        x = self.x_t
        self.x_t = np.array([x[0] + fwd * math.cos(x[2]), x[1] + fwd * math.sin(x[2]),
                             math.remainder(x[2] + ang, 2 * 3.14159265358979323846)])

    def getStateVector(self):
        return self.x_t.copy()


class BatchedPoseGraph(Handle):
    """Pose-graph SLAM (reference: class PoseGraph, filter.h:232-322, pose_graph.cpp) for `batch` instances."""

    _INIT, _INIT_EACH, _DESTROY = "pgs_init", "pgs_init_each", "pgs_destroy"

    def __init__(self, batch, num_iterations=1000, L_max=20, k_per_pose=8, device=0):
        self.batch, self.L_max, self.k_per_pose, self.device = int(batch), int(L_max), int(k_per_pose), int(device)
        self.num_iterations_total = int(num_iterations)      # config["num_iterations"], pose_graph.cpp:40
        self.solve_graph_every_iteration = False             # params.yaml:64 (the reference's file says true)
        self.cfg = default_config()
        self.h = None
        self.isInit = False
        self.solved_pose_graph = False
        self.timestep = 0

    # -- PoseGraph::readParams (pose_graph.cpp:12-66) --
    def readParams(self, config=None, solve_graph_every_iteration=None):
        L = _lib.lib()
        if isinstance(config, SlamConfig):
            self.cfg = config.copy()
        elif isinstance(config, str):
            # a params.yaml path: the common keys through the C reader, plus the three keys PoseGraph::readParams itself takes
            # from the file (pose_graph.cpp:28-47): num_iterations, pose_graph.implementation, .solve_graph_every_iteration
            _lib.check(L.slam_config_load(C.byref(self.cfg), config.encode()))
            section = None
            with open(config) as fh:
                for line in fh:
                    body = line.split("#", 1)[0].rstrip()
                    if not body.strip():
                        continue
                    if not body[0].isspace():
                        section = body.split(":", 1)[0].strip()
                    key, _, val = body.strip().partition(":")
                    val = val.strip().strip('"').strip("'")
                    if not val:
                        continue
                    if section == "num_iterations" and key == "num_iterations":
                        self.num_iterations_total = int(val)
                    elif section == "pose_graph" and key == "implementation" and val != "gtsam":   # pose_graph.cpp:31-40
                        raise _lib.SlamError("pose_graph.implementation must be gtsam (the reference's sesync/custom are incomplete)")
                    elif section == "pose_graph" and key == "solve_graph_every_iteration":
                        self.solve_graph_every_iteration = val.lower() == "true"
        elif isinstance(config, dict):
            pg = config.get("pose_graph", {})
            if pg.get("implementation", "gtsam") != "gtsam":   # pose_graph.cpp:31-40: sesync / custom throw
                raise _lib.SlamError("pose_graph.implementation must be gtsam (the reference's sesync/custom are incomplete)")
            self.solve_graph_every_iteration = bool(pg.get("solve_graph_every_iteration", self.solve_graph_every_iteration))
            self.num_iterations_total = int(config.get("num_iterations", self.num_iterations_total))
        elif config is not None:
            raise TypeError("unsupported config type")
        if solve_graph_every_iteration is not None:
            self.solve_graph_every_iteration = bool(solve_graph_every_iteration)
        if self.h is not None:
            self.close()
        h = C.c_void_p()
        _lib.check(L.pgs_create(C.byref(self.cfg), self.batch, self.num_iterations_total, self.L_max, self.k_per_pose, self.device, C.byref(h)))
        self.h = h
        return self

    # -- PoseGraph::init (pose_graph.cpp:68-95) --
    def init(self, x_0=0.0, y_0=0.0, yaw_0=0.0, truth0=None):
        """Scalars: one start pose for the batch.  x_0 a (batch, 3) array of (x, y, yaw): one per instance (pgs_init_each; y_0 and
        yaw_0 are then ignored).  truth0: optional (batch, 3) true start poses of the simulator (default: the start poses)."""
        self._init(x_0, y_0, yaw_0, truth0)
        self.solved_pose_graph, self._sec = False, None

    def _cmds(self, cmds):
        """(T, 2) float32 for the batch (a flat list of 2 T numbers too), (T, batch, 2) per instance."""
        c = np.ascontiguousarray(cmds, dtype=np.float32)
        if c.ndim == 3:
            if c.shape[0] == 0 or c.shape[1:] != (self.batch, 2):
                raise ValueError(f"per-instance commands: expected shape (T > 0, {self.batch}, 2), got {c.shape}")
            return c
        if c.size == 0 or c.ndim > 2 or (c.ndim == 2 and c.shape[1] != 2) or c.size % 2:
            raise ValueError(f"expected commands of shape (T, 2) or (T, {self.batch}, 2), got {c.shape}")
        return c.reshape(-1, 2)

    def set_stream(self, ptr):
        self._need(); _lib.check(_lib.lib().pgs_set_stream(self.h, C.c_void_p(ptr)))

    def set_seed(self, seed):
        self._need(); _lib.check(_lib.lib().pgs_set_seed(self.h, int(seed)))

    def set_instance_offset(self, first):
        self._need(); _lib.check(_lib.lib().pgs_set_instance_offset(self.h, int(first)))

    def set_map(self, map_xy, counts=None):
        """The simulator's true map [L][2] for every instance, or one per instance (pgs_set_maps): a (batch, L_stride, 2) array with
        `counts` [batch] landmarks each (default: all L_stride)."""
        self._need()
        m = np.ascontiguousarray(map_xy, dtype=np.float64)
        if m.ndim == 2 and counts is None:
            if m.shape[1] != 2 or m.shape[0] == 0:
                raise ValueError(f"expected a map of shape (L > 0, 2), got {m.shape}")
            _lib.check(_lib.lib().pgs_set_map(self.h, _d(m), m.shape[0]))
            return
        if m.ndim != 3 or m.shape[0] != self.batch or m.shape[2] != 2 or not 0 < m.shape[1] <= 255:
            raise ValueError(f"expected per-instance maps of shape ({self.batch}, 0 < L_stride <= 255, 2), got {m.shape}")
        cnt = np.full(self.batch, m.shape[1], np.int32) if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (self.batch,) or np.any(cnt <= 0) or np.any(cnt > m.shape[1]):
            raise ValueError(f"counts: expected {self.batch} landmark counts in [1, {m.shape[1]}]")
        _lib.check(_lib.lib().pgs_set_maps(self.h, _d(m), _i(cnt), m.shape[1]))

    # -- PoseGraph::updateNaiveVehPoseEstimate (pose_graph.cpp:97-119) --
    def updateNaiveVehPoseEstimate(self, state_vector, landmark_ids=None):
        """state_vector: [>=3] (one estimate for every instance, e.g. the NaiveFilter) or [B][>=3] (per instance, e.g.
        BatchedEKF.poses()); only (x, y, yaw) is used (update_landmarks_after_adding = false)."""
        sv = np.asarray(state_vector, dtype=np.float64)
        sv = np.broadcast_to(sv[:3], (self.batch, 3)) if sv.ndim == 1 else sv[:, :3]
        self._sec = np.ascontiguousarray(sv, dtype=np.float64)

    # -- PoseGraph::update (pose_graph.cpp:199-267) --
    def update(self, cmdMsg, lmMeasMsg, meas_count=None):
        """cmdMsg: Command or (fwd, ang) for the batch, or a (batch, 2) array with one command per instance (pgs_update_each)."""
        self._need()
        if not self.isInit:
            raise _lib.SlamError("init() must be called before update()")
        if self.solved_pose_graph and not self.solve_graph_every_iteration:
            return                                            # :201-205
        if self.timestep + 1 >= self.num_iterations_total:    # :208-214
            self.solvePoseGraph()
            return
        cmd = self._cmd(cmdMsg)
        meas = np.asarray(lmMeasMsg, dtype=np.float32)
        if meas.ndim <= 2 and meas_count is None:             # one message for all instances
            one = meas.reshape(-1, 3)
            k = one.shape[0]
            meas = np.broadcast_to(one, (self.batch, k, 3))
            meas_count = np.full(self.batch, k, dtype=np.int32)
        meas = np.ascontiguousarray(meas.reshape(self.batch, -1, 3), dtype=np.float32)
        cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
        if cnt.shape != (self.batch,):
            raise ValueError(f"meas_count: expected shape ({self.batch},), got {cnt.shape}")
        ks = meas.shape[1]
        step = _lib.lib().pgs_update_each if cmd.ndim == 2 else _lib.lib().pgs_update
        _lib.check(step(self.h, _f(cmd), opt(meas), _i(cnt) if ks else None, ks, opt(self._sec)))
        self.timestep += 1
        if self.solve_graph_every_iteration:                  # :258-264
            self.solvePoseGraph()
            _lib.check(_lib.lib().pgs_adopt_result(self.h))

    def run_sim(self, cmds):
        """All of `cmds` with the device-side measurement generator and the NaiveFilter as the secondary filter; cmds (T, 2) for the
        batch, or (T, batch, 2) per instance (pgs_run_sim_each)."""
        self._need()
        c = self._cmds(cmds)
        _lib.check((_lib.lib().pgs_run_sim_each if c.ndim == 3 else _lib.lib().pgs_run_sim)(self.h, _f(c), c.shape[0]))
        self.timestep += c.shape[0]

    def run_sim_every_iteration(self, cmds):
        """solve_graph_every_iteration (params.yaml:64; pose_graph.cpp:258-264) with the simulator on the device: per command one tick of
        run_sim, solvePoseGraph, initial_estimate = result.  cmds (T, 2), or (T, batch, 2) per instance.  Returns [batch][2]: LM
        iterations / lambda trials summed over the ticks."""
        self._need()
        c = self._cmds(cmds)
        counts = np.zeros((self.batch, 2), dtype=np.int32)
        run = _lib.lib().pgs_run_sim_every_iteration_each if c.ndim == 3 else _lib.lib().pgs_run_sim_every_iteration
        _lib.check(run(self.h, _f(c), c.shape[0], _i(counts)))
        self.timestep += c.shape[0]
        self.solved_pose_graph = True
        return counts

    def last_iter_phases(self):
        self._need(); o = np.zeros(6); _lib.check(_lib.lib().pgs_last_iter_phases(self.h, _d(o)))
        return dict(sim_append_ms=o[0], solve_ms=o[1], adopt_ms=o[2], trials_launched=int(o[3]), syrk_flop=o[4], chol_flop=o[5])

    # -- PoseGraph::solvePoseGraph (pose_graph.cpp:269-300) --
    def solvePoseGraph(self):
        self._need()
        _lib.check(_lib.lib().pgs_solve(self.h))
        self.solved_pose_graph = True

    def set_groups(self, groups):
        """Number of concurrently solved sub-batches (separate HIP streams); 0 = automatic."""
        self._need(); _lib.check(_lib.lib().pgs_set_groups(self.h, int(groups)))

    def set_slots(self, slots):
        """Streaming solve: at most `slots` graphs of the batch in flight, the others wait for a running slot (0 = lockstep)."""
        self._need(); _lib.check(_lib.lib().pgs_set_slots(self.h, int(slots)))

    def last_solve_timeline(self):
        """Running slots per trial of the last solve, one array per solve group."""
        self._need()
        out, g, ng = [], 0, C.c_int32(1)
        while g < ng.value:
            n = C.c_int32(0)
            _lib.check(_lib.lib().pgs_last_solve_timeline(self.h, g, None, 0, C.byref(n), C.byref(ng)))
            a = np.zeros(max(n.value, 1), dtype=np.int32)
            _lib.check(_lib.lib().pgs_last_solve_timeline(self.h, g, _i(a), n.value, C.byref(n), C.byref(ng)))
            out.append(a[:n.value].copy())
            g += 1
        return out

    def adopt_result(self):
        self._need(); _lib.check(_lib.lib().pgs_adopt_result(self.h))

    def get_graph(self, instance=0, which=None):
        self._need()
        which = int(self.solved_pose_graph) if which is None else int(which)
        N = self.timestep + 1
        poses = np.zeros((N, 3)); lms = np.zeros((self.L_max, 2)); ids = np.zeros(self.L_max, dtype=np.int32)
        ts = C.c_int32(0); M = C.c_int32(0)
        _lib.check(_lib.lib().pgs_get_graph(self.h, int(instance), which, _d(poses), _d(lms), C.byref(ts), C.byref(M), _i(ids)))
        return dict(poses=poses, landmarks=lms[:M.value].copy(), timestep=ts.value, M=M.value, ids=ids[:M.value].copy())

    def connections(self, instance=0):
        self._need()
        cap = (self.timestep + 1) * self.k_per_pose
        c = np.zeros((max(cap, 1), 2), dtype=np.int32); n = C.c_int32(0)
        _lib.check(_lib.lib().pgs_get_connections(self.h, int(instance), _i(c), cap, C.byref(n)))
        return c[:n.value].copy()

    # -- PoseGraph::publishState payload (pose_graph.cpp:302-387, PoseGraphState.msg) --
    def publishState(self, instance=0):
        g = self.get_graph(instance)
        ts = g["timestep"]
        p = g["poses"][:ts]                                   # the reference's loop is `i < timestep` (:325)
        return dict(timestep=ts, M=g["M"], x_v=p[:, 0].astype(np.float32), y_v=p[:, 1].astype(np.float32),
                    yaw_v=p[:, 2].astype(np.float32), landmarks=g["landmarks"].astype(np.float32).ravel(),
                    meas_connections=self.connections(instance).ravel(),
                    topic="/state/pose_graph/result" if self.solved_pose_graph else "/state/pose_graph/initial")

    def stats(self):
        self._need()
        B = self.batch
        it = np.zeros(B, dtype=np.int32); tr = np.zeros(B, dtype=np.int32); fl = np.zeros(B, dtype=np.int32)
        e0 = np.zeros(B); e1 = np.zeros(B); lam = np.zeros(B)
        _lib.check(_lib.lib().pgs_get_stats(self.h, _i(it), _i(tr), _i(fl), _d(e0), _d(e1), _d(lam)))
        return dict(iterations=it, trials=tr, flags=fl, err_init=e0, err_final=e1, lam=lam)

    # -- gtsam::Marginals(graph, values).marginalCovariance(key) (pose_graph.cpp:289-294) --
    def marginals(self, which=None):
        """Marginal covariances of every pose and landmark of every instance at initial_estimate (which = 0) / result (1; default as
        get_graph).  Read them with get_marginals / marginalCovariance; any update / solve / adopt_result invalidates them."""
        self._need()
        which = int(self.solved_pose_graph) if which is None else int(which)
        _lib.check(_lib.lib().pgs_marginals(self.h, which))

    def get_marginals(self, instance=0):
        """dict(pose_cov [N][3][3], lm_cov [M][2][2], status): pose blocks in the tangent coordinates of the pose (translation in its
        own frame, yaw), status 1 = singular graph (all blocks NaN)."""
        self._need()
        N = self.timestep + 1
        pc = np.zeros((N, 3, 3)); lc = np.zeros((self.L_max, 2, 2)); st = C.c_int32(0)
        _lib.check(_lib.lib().pgs_get_marginals(self.h, int(instance), _d(pc), _d(lc), C.byref(st)))
        ts = C.c_int32(0); M = C.c_int32(0)
        _lib.check(_lib.lib().pgs_get_graph(self.h, int(instance), 0, None, None, C.byref(ts), C.byref(M), None))
        return dict(pose_cov=pc, lm_cov=lc[:M.value].copy(), status=st.value)

    def marginalCovariance(self, instance, pose=None, landmark=None):
        """marginals.marginalCovariance(key) of one pose (3x3) or one landmark (2x2, by index) of `instance`."""
        if (pose is None) == (landmark is None):
            raise ValueError("give exactly one of pose= and landmark=")
        m = self.get_marginals(instance)
        blocks, k = (m["pose_cov"], pose) if pose is not None else (m["lm_cov"], landmark)
        if not 0 <= int(k) < blocks.shape[0]:
            raise IndexError(f"{'pose' if pose is not None else 'landmark'} {k} out of range ({blocks.shape[0]})")
        return blocks[int(k)].copy()

    def last_marginals_work(self):
        """(algorithmic FLOP of the last marginals() summed over the batch, its HIP-event milliseconds)."""
        return self._last_work("pgs_last_marginals_work", 2)

    # -- robust loss on the landmark factors (noiseModel::Robust; slam_pgs.h) --
    def set_robust(self, kind, k=0.0):
        """Loss of every bearing-range factor from the next solve / marginals / factor_weights on: kind LOSS_NONE | LOSS_HUBER |
        LOSS_GEMAN_MCCLURE (or "none" | "huber" | "geman_mcclure"), parameter k in whitened units (Huber: 1.345 is the usual choice)."""
        self._need()
        kind = LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)
        _lib.check(_lib.lib().pgs_set_robust(self.h, kind, float(k)))

    @property
    def robust(self):
        """(kind, k) as set."""
        self._need(); kind = C.c_int(0); k = C.c_double(0.0)
        _lib.check(_lib.lib().pgs_get_robust(self.h, C.byref(kind), C.byref(k)))
        return kind.value, k.value

    def factor_weights(self, which=None):
        """IRLS weight of every stored bearing-range factor at initial_estimate (which = 0) / result (1; default as get_graph):
        [batch][timestep + 1][k_per_pose] in slot order (the order of connections()), NaN where a pose stores no factor; all 1.0
        without a loss.  Which detections the solve did not believe."""
        self._need()
        which = int(self.solved_pose_graph) if which is None else int(which)
        _lib.check(_lib.lib().pgs_factor_weights(self.h, which))
        N = self.timestep + 1
        out = np.zeros((self.batch, N, self.k_per_pose))
        n = C.c_int32(0)
        for b in range(self.batch):
            _lib.check(_lib.lib().pgs_get_factor_weights(self.h, b, _d(out[b]), N * self.k_per_pose, C.byref(n)))
        return out

    # -- absolute fixes: unary pose factors (slam_pgs.h "absolute fixes") --
    def fix(self, fix, kinds, dev=False):
        """One fix per instance at the graph's newest pose: fix (batch, 5) rows {z_x, z_y, z_yaw, sigma_pos, sigma_yaw}, kinds [batch]
        (FIX_POS | FIX_YAW).  Returns the verdicts [batch] (position | heading << 4; 0 absent, 1 stored, 4 invalid).  dev=True: fix and
        kinds are DEVICE pointers read in stream order (pgs_fix_dev); returns None."""
        self._need()
        if dev:
            _lib.check(_lib.lib().pgs_fix_dev(self.h, C.c_void_p(fix), C.c_void_p(kinds), None))
            return None
        f = np.ascontiguousarray(self._rows(np.asarray(fix, dtype=np.float64), "fix", 5))
        k = np.ascontiguousarray(kinds, dtype=np.int32)
        if k.shape != (self.batch,):
            raise ValueError(f"kinds: expected shape ({self.batch},), got {k.shape}")
        verdict = np.zeros(self.batch, dtype=np.int32)
        _lib.check(_lib.lib().pgs_fix(self.h, _d(f), _i(k), _i(verdict)))
        return verdict

    def set_fix_robust(self, kind, k=0.0):
        """Loss of every fix part from the next solve / marginals / fix_weights on (kinds and parameter as set_robust)."""
        self._need()
        kind = LOSS_KINDS[kind] if isinstance(kind, str) else int(kind)
        _lib.check(_lib.lib().pgs_set_fix_robust(self.h, kind, float(k)))

    @property
    def fix_robust(self):
        """(kind, k) of the fix loss as set."""
        self._need(); kind = C.c_int(0); k = C.c_double(0.0)
        _lib.check(_lib.lib().pgs_get_fix_robust(self.h, C.byref(kind), C.byref(k)))
        return kind.value, k.value

    def fixes(self, instance=0):
        """The stored fixes of one instance: dict(fix (timestep + 1, 5), kinds [timestep + 1]); kinds 0 where a pose has none."""
        self._need()
        N = self.timestep + 1
        f = np.zeros((N, 5)); k = np.zeros(N, dtype=np.int32); n = C.c_int32(0)
        _lib.check(_lib.lib().pgs_get_fixes(self.h, int(instance), _d(f), _i(k), N, C.byref(n)))
        return dict(fix=f, kinds=k)

    def fix_weights(self, which=None):
        """IRLS weight of both parts of every fix at initial_estimate (which = 0) / result (1; default as get_graph):
        [batch][timestep + 1][2] (position, heading), NaN where a part is not stored; 1.0 without a fix loss."""
        self._need()
        which = int(self.solved_pose_graph) if which is None else int(which)
        _lib.check(_lib.lib().pgs_fix_weights(self.h, which))
        N = self.timestep + 1
        out = np.zeros((self.batch, N, 2))
        n = C.c_int32(0)
        for b in range(self.batch):
            _lib.check(_lib.lib().pgs_get_fix_weights(self.h, b, _d(out[b]), N, C.byref(n)))
        return out

    def set_fix_sensor(self, rows):
        """The simulated source of fix_sense() and run_sim_fix (pgs_set_fix_sensor_each): one FixSensorConfig (or a dict of its fields),
        replicated over the batch, or `batch` of them; None returns to the all-zero row, which emits nothing."""
        self._set_rows("pgs_set_fix_sensor_each", rows, FixSensorConfig, "fix sensor", one=default_fix_sensor_config)

    def fix_sense(self, dev=None):
        """One emission of the simulated source from the simulator's true poses: dict(fix (batch, 5), kinds [batch], jumped [batch]).
        dev = (d_fix, d_kinds, d_jumped or None): DEVICE pointers, written in stream order; returns None."""
        self._need()
        if dev is not None:
            _lib.check(_lib.lib().pgs_fix_sense_dev(self.h, C.c_void_p(dev[0]), C.c_void_p(dev[1]), C.c_void_p(dev[2]) if dev[2] else None))
            return None
        out = dict(fix=np.zeros((self.batch, 5)), kinds=np.zeros(self.batch, dtype=np.int32), jumped=np.zeros(self.batch, dtype=np.int32))
        _lib.check(_lib.lib().pgs_fix_sense(self.h, _d(out["fix"]), _i(out["kinds"]), _i(out["jumped"])))
        return out

    def run_sim_fix(self, cmds, fix_every):
        """run_sim with a fix of the simulated source attached after every fix_every-th tick of the call, all on the device."""
        self._need()
        c = self._cmds(cmds)
        _lib.check(_lib.lib().pgs_run_sim_fix(self.h, _f(c), c.shape[0], int(c.ndim == 3), int(fix_every)))
        self.timestep += c.shape[0]

    def error_stats(self, which=1):
        self._need(); out = np.zeros(self.batch); _lib.check(_lib.lib().pgs_error_stats(self.h, int(which), _d(out))); return out

    def last_solve_work(self):
        self._need(); f = C.c_double(0); t = C.c_int32(0)
        _lib.check(_lib.lib().pgs_last_solve_work(self.h, C.byref(f), C.byref(t)))
        return f.value, t.value

    def set_profiling(self, on=True):
        self._need(); _lib.check(_lib.lib().pgs_set_profiling(self.h, int(on)))

    def last_solve_kernel_ms(self):
        """{kernel: total ms in the last solve} from HIP events on the handle's stream (set_profiling(True))."""
        self._need(); ms = np.zeros(6); _lib.check(_lib.lib().pgs_last_solve_kernel_ms(self.h, _d(ms)))
        return dict(zip(("linearize", "chain", "syrk", "chol", "backsolve", "evaluate"), ms.tolist()))

    def last_solve_paths(self):
        """The last profiled solve by path: algorithmic SYRK FLOP and ms of the separate SYRK launches / of the fused chain + SYRK launches."""
        self._need(); o = np.zeros(8); _lib.check(_lib.lib().pgs_last_solve_paths_v2(self.h, _d(o), 8))
        return dict(flop_separate=o[0], flop_fused=o[1], ms_separate_syrk=o[2], ms_fused=o[3], flop_segmented=o[4], ms_segmented_syrk=o[5],
                    segmented=bool(o[6]), segment_length=int(o[7]))

    def sync(self):
        self._need(); _lib.check(_lib.lib().pgs_sync(self.h))
