"""Host-side mirror of the reference's `Filter` interface for the batched engine.

The reference drives ONE filter object through
    readParams(config) -> init(x_0, y_0, yaw_0) -> update(cmdMsg, lmMeasMsg) -> publishState()/getStateVector()
(ekf_ws/src/localization_pkg/include/localization_pkg/filter.h:54-77; caller: localization_node.cpp:33-47,
90-106,108-140).  `BatchedEKF` keeps those names, argument meanings and the exception-on-error convention, for a
batch of B instances that share map + commands (Monte-Carlo seeds) or get their own start pose, map and commands (several robots or
scenarios: the per-instance forms of init / set_map / update / run_sim); everything numeric happens in libslam_hip.so.
The C++ twin of this class (for a C++/ROS host) is include/slam_filter.hpp.  How arguments become pointers, structs and rows is in
_marshal.py; the *_instance_host test hooks are in _hooks.py and re-exported here.
"""
import ctypes as C
import numpy as np

from . import _lib
from ._marshal import Handle, Command, _d, _f, _i, ptr, opt, config_from   # noqa: F401
from ._marshal import MONITOR, NAV, INNOVATION, GATE, ASSOC, JOINT, MAP, MERGE, FIX
from ._hooks import (sense_instance_host, fix_instance_host, fix_sense_instance_host, merge_instance_host, map_instance_host,   # noqa: F401
                     innovation_instance_host, gate_instance_host, associate_instance_host, associate_joint_instance_host)
from .config import SlamConfig, NavConfig, default_config, default_nav_config, EKF_SLAM, UKF_LOC, UKF_SLAM, F64   # noqa: F401
from .config import MonitorConfig, default_monitor_config, MONITOR_SHARED, MONITOR_EACH, MONITOR_NAV   # noqa: F401
from .config import Noise
from .config import (InnovationConfig, default_innovation_config, INNOVATION_SHARED, INNOVATION_EACH, INNOVATION_NAV, INNOVATION_LOG,   # noqa: F401
                     INNOV_MAX_DET)
from .config import GateConfig, default_gate_config   # noqa: F401
from .config import AssocConfig, default_assoc_config   # noqa: F401
from .config import JointConfig, default_joint_config   # noqa: F401
from .config import MapConfig, default_map_config, MAP_CONFIG_FIELDS   # noqa: F401
from .config import MergeConfig, default_merge_config, MERGE_CONFIG_FIELDS   # noqa: F401
from .config import SensorConfig, SenseLog, default_sensor_config
from .config import FixConfig, FixSensorConfig, FixLog, default_fix_config, default_fix_sensor_config, FIX_CONFIG_FIELDS   # noqa: F401


class MonitorResult:
    """What monitor_run returns: `recs`, the (T, 16) records of the ticks (columns: the REC_* constants; slam_monitor_run in
    include/slam_batch.h defines them), and - with series=True, else None - `err_pos`, `err_yaw`, `nees_pose`, (T, batch) each."""

    (REC_N_OK, REC_N_FAILED, REC_N_NEES, REC_N_POSE_NOT_PD, REC_SUM_ERR_POS, REC_SUM_ERR_POS2, REC_MAX_ERR_POS, REC_SUM_ERR_YAW2,
     REC_MAX_ABS_ERR_YAW, REC_SUM_NEES_POSE, REC_N_BELOW, REC_N_ABOVE, REC_SUM_M, REC_N_FULL, REC_SUM_NEES_FULL, REC_SUM_DOF) = range(16)

    def __init__(self, recs, err_pos=None, err_yaw=None, nees_pose=None):
        self.recs, self.err_pos, self.err_yaw, self.nees_pose = recs, err_pos, err_yaw, nees_pose


class InnovationResult:
    """What innovation_run returns: `recs`, the (T, 16) records of the ticks (columns: the REC_* constants; slam_innovation in
    include/slam_batch.h defines them), and - with series=True, else None - `nis_sum`, `n_upd`, `flags`, (T, batch) each."""

    (REC_N_EVAL, REC_N_FROZEN, REC_N_TOO_LONG, REC_N_WOULD_FREEZE, REC_N_SINGULAR, REC_N_UPD, REC_N_NEW, REC_SUM_NIS, REC_MAX_NIS,
     REC_N_BELOW, REC_N_ABOVE, REC_SUM_NU_R, REC_SUM_NU_B, REC_SUM_NU_R2, REC_SUM_NU_B2, REC_RESERVED) = range(16)

    def __init__(self, recs, nis_sum=None, n_upd=None, flags=None):
        self.recs, self.nis_sum, self.n_upd, self.flags = recs, nis_sum, n_upd, flags


class GateResult(InnovationResult):
    """What gate_run returns: `recs` (T, 16) as InnovationResult, entries 5 and 7 - 14 over the accepted updates and REC_N_REJ = 15 the
    rejected detections, and - with series=True, else None - `nis_sum`, `n_upd`, `n_rej`, `flags`, (T, batch) each."""

    REC_N_REJ = 15

    def __init__(self, recs, nis_sum=None, n_upd=None, n_rej=None, flags=None):
        InnovationResult.__init__(self, recs, nis_sum, n_upd, flags)
        self.n_rej = n_rej


class AssocResult:
    """What associate_run returns: `recs`, the (T, 16) records of the ticks (columns: the REC_* constants; slam_associate in
    include/slam_batch.h defines them), and - with series=True, else None - `n_match`, `n_new`, `n_drop`, `flags`, (T, batch) each."""

    (REC_N_EVAL, REC_N_FROZEN, REC_N_TOO_LONG, REC_N_DET, REC_N_MATCHED, REC_N_NEW, REC_N_AMBIGUOUS, REC_SUM_D2, REC_MAX_D2, REC_N_CONFLICT,
     REC_N_NO_ROOM, REC_N_INVALID) = range(12)

    def __init__(self, recs, n_match=None, n_new=None, n_drop=None, flags=None):
        self.recs, self.n_match, self.n_new, self.n_drop, self.flags = recs, n_match, n_new, n_drop, flags


class JointResult:
    """What associate_joint_run returns: `recs`, the (T, 16) records of the ticks (columns: the REC_* constants; slam_associate_joint in
    include/slam_batch.h defines them), and - with series=True, else None - `n_match`, `n_new`, `n_drop`, `flags`, `nodes` and `d2_joint`,
    (T, batch) each."""

    (REC_N_EVAL, REC_N_FROZEN, REC_N_TOO_LONG, REC_N_DET, REC_N_MATCHED, REC_N_NEW, REC_N_AMBIGUOUS, REC_SUM_D2, REC_MAX_D2, REC_N_UNPAIRED,
     REC_N_NO_ROOM, REC_N_INVALID, REC_SUM_NODES, REC_N_BUDGET, REC_N_S_SINGULAR, REC_N_DIFFER) = range(16)

    def __init__(self, recs, n_match=None, n_new=None, n_drop=None, flags=None, nodes=None, d2_joint=None):
        self.recs, self.n_match, self.n_new, self.n_drop, self.flags, self.nodes, self.d2_joint = recs, n_match, n_new, n_drop, flags, nodes, d2_joint


def _joint_config(cfg):
    """A JointConfig from None (the defaults), a JointConfig or a dict of its fields (gate_joint: 16 values)."""
    return config_from(cfg, *JOINT)


class MapResult(AssocResult):
    """What manage_run returns: `recs` (T, 16) and - with series=True, else None - `n_match`, `n_new`, `n_drop`, `flags` as AssocResult, and
    `n_removed` (T, batch), the landmarks each prune took (0 on the ticks without one).  The REC_MAP_* constants index the (16,) record of
    remove_landmarks and map_prune."""

    REC_MAP_TOUCHED, REC_MAP_REMOVED, REC_MAP_MOVED = range(3)

    def __init__(self, recs, n_match=None, n_new=None, n_drop=None, flags=None, n_removed=None):
        AssocResult.__init__(self, recs, n_match, n_new, n_drop, flags)
        self.n_removed = n_removed


class MergeResult(MapResult):
    """What manage_merge_run returns: MapResult and - with series=True, else None - `n_merged` (T, batch), the landmarks each merge fused
    away (0 on the ticks without one).  The REC_MERGE_* constants index the (16,) record of merge_landmarks and map_merge."""

    REC_MERGE_TOUCHED, REC_MERGE_FUSED, REC_MERGE_NOT_MUTUAL, REC_MERGE_SINGULAR, REC_MERGE_UPDATED = range(5)
    REC_MERGE_SUM_D2, REC_MERGE_MAX_D2 = 7, 8

    def __init__(self, recs, n_match=None, n_new=None, n_drop=None, flags=None, n_removed=None, n_merged=None):
        MapResult.__init__(self, recs, n_match, n_new, n_drop, flags, n_removed)
        self.n_merged = n_merged


class FixResult:
    """The outcome of a fix_run: recs (T, 16), one record per tick (zeros on the ticks without a fix), indexed by the REC_FIX_* constants,
    and - series=True, else None - verdict (T, batch) int32 (position | heading << 4), nis (T, batch, 2), the emitted rows fix (T, batch, 5)
    and kinds (T, batch)."""
    REC_FIX_WRITTEN, REC_FIX_POS_PRESENT, REC_FIX_POS_APPLIED, REC_FIX_POS_REJECTED, REC_FIX_POS_SINGULAR, REC_FIX_POS_INVALID = 0, 1, 2, 3, 4, 5
    REC_FIX_YAW_PRESENT, REC_FIX_YAW_APPLIED, REC_FIX_YAW_REJECTED, REC_FIX_YAW_SINGULAR, REC_FIX_YAW_INVALID = 6, 7, 8, 9, 10
    REC_FIX_SUM_NIS_POS, REC_FIX_SUM_NIS_YAW, REC_FIX_SKIPPED = 11, 12, 13

    def __init__(self, recs, verdict=None, nis=None, fix=None, kinds=None):
        self.recs, self.verdict, self.nis, self.fix, self.kinds = recs, verdict, nis, fix, kinds


class BatchedFilter(Handle):
    """Common part of the batched filters (reference: class Filter, filter.h:54-145)."""

    kind = None
    _INIT, _INIT_EACH, _DESTROY = "slam_init", "slam_init_each", "slam_destroy"

    def __init__(self, batch, L_max, device=0, dtype=F64):
        self.batch, self.L_max, self.device, self.dtype = int(batch), int(L_max), int(device), dtype
        self.cfg = default_config()
        self.h = None
        self.isInit = False  # filter.h:68
        self.timestep = 0

    # -- Filter::readParams(YAML::Node) (filter.h:59, readCommonParams filter.h:105-121) --
    def readParams(self, config=None):
        """config: None (reference defaults), a SlamConfig, a params.yaml path, or a nested dict with the
        reference's YAML structure."""
        L = _lib.lib()
        if config is None:
            pass
        elif isinstance(config, SlamConfig):
            self.cfg = config.copy()
        elif isinstance(config, str):
            _lib.check(L.slam_config_load(C.byref(self.cfg), config.encode()))
        elif isinstance(config, dict):
            c = self.cfg
            pn, sn, cons = config.get("process_noise", {}), config.get("sensing_noise", {}), config.get("constraints", {})
            c.v_d = pn.get("mean", {}).get("v_d", c.v_d); c.v_th = pn.get("mean", {}).get("v_th", c.v_th)
            c.V_00 = pn.get("cov", {}).get("V_00", c.V_00); c.V_11 = pn.get("cov", {}).get("V_11", c.V_11)
            c.w_r = sn.get("mean", {}).get("w_r", c.w_r); c.w_b = sn.get("mean", {}).get("w_b", c.w_b)
            c.W_00 = sn.get("cov", {}).get("W_00", c.W_00); c.W_11 = sn.get("cov", {}).get("W_11", c.W_11)
            m = cons.get("measurements", {})
            c.landmark_id_is_known = int(m.get("landmark_id_is_known", c.landmark_id_is_known))
            c.min_landmark_separation = m.get("min_landmark_separation", c.min_landmark_separation)
            cm, v = cons.get("commands", {}), cons.get("vision", {})
            c.d_max = cm.get("d_max", c.d_max); c.th_max = cm.get("th_max", c.th_max)
            c.range_max = v.get("range_max", c.range_max); c.fov_min = v.get("fov_min", c.fov_min); c.fov_max = v.get("fov_max", c.fov_max)
            ip = config.get("init_pose", {})
            c.init_x = ip.get("x", c.init_x); c.init_y = ip.get("y", c.init_y); c.init_yaw = ip.get("yaw", c.init_yaw)
        else:
            raise TypeError("unsupported config type")
        if self.h is not None:
            self.close()
        h = C.c_void_p()
        _lib.check(L.slam_create(C.byref(self.cfg), self.kind, self.batch, self.L_max, self.dtype, self.device, C.byref(h)))
        self.h = h
        self.n_max = L.slam_state_dim_max(self.h)
        return self

    # -- Filter::init(float x_0, float y_0, float yaw_0) (filter.h:60) --
    def init(self, x_0=0.0, y_0=0.0, yaw_0=0.0, truth0=None):
        """Scalars: one start pose for the batch.  x_0 a (batch, 3) array of (x, y, yaw): one per instance (slam_init_each; y_0 and
        yaw_0 are then ignored).  truth0: optional (batch, 3) true start poses of the simulator (default: the config's init pose)."""
        self._init(x_0, y_0, yaw_0, truth0)

    # -- batch plumbing that has no counterpart in the single-instance reference --
    def set_stream(self, hip_stream_ptr):
        self._need(); _lib.check(_lib.lib().slam_set_stream(self.h, C.c_void_p(hip_stream_ptr)))

    def set_seed(self, seed):
        self._need(); _lib.check(_lib.lib().slam_set_seed(self.h, int(seed)))

    def set_instance_offset(self, first):
        self._need(); _lib.check(_lib.lib().slam_set_instance_offset(self.h, int(first)))

    def set_vision(self, range_max, fov_min, fov_max):
        self._need(); _lib.check(_lib.lib().slam_set_vision(self.h, range_max, fov_min, fov_max))

    def set_map(self, map_xy, counts=None):
        """True landmark map [L][2]; `filter->map` of localization_node.cpp:152-156 / sim landmarks.  One map per instance
        (slam_set_maps): a (batch, L_stride, 2) array with `counts` [batch] landmarks each (default: all L_stride), or a list of batch
        (L_b, 2) maps."""
        self._need()
        if isinstance(map_xy, (list, tuple)):
            if counts is not None:
                raise ValueError("counts go with a (batch, L_stride, 2) array; a list of maps carries its own")
            maps = [np.asarray(m, dtype=np.float64) for m in map_xy]
            if len(maps) != self.batch or any(m.ndim != 2 or m.shape[1] != 2 or m.shape[0] == 0 for m in maps):
                raise ValueError(f"expected a list of {self.batch} maps of shape (L_b > 0, 2)")
            counts = np.array([m.shape[0] for m in maps], dtype=np.int32)
            arr = np.zeros((self.batch, int(counts.max()), 2))
            for b, m in enumerate(maps):
                arr[b, :m.shape[0]] = m
            map_xy = arr
        m = np.ascontiguousarray(map_xy, dtype=np.float64)
        if m.ndim == 2 and counts is None:
            if m.shape[1] != 2 or m.shape[0] == 0:
                raise ValueError(f"expected a map of shape (L > 0, 2), got {m.shape}")
            _lib.check(_lib.lib().slam_set_map(self.h, _d(m), m.shape[0]))
            return
        if m.ndim != 3 or m.shape[0] != self.batch or m.shape[2] != 2 or m.shape[1] == 0:
            raise ValueError(f"expected per-instance maps of shape ({self.batch}, L_stride > 0, 2), got {m.shape}")
        cnt = np.full(self.batch, m.shape[1], np.int32) if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (self.batch,) or np.any(cnt <= 0) or np.any(cnt > m.shape[1]):
            raise ValueError(f"counts: expected {self.batch} landmark counts in [1, {m.shape[1]}]")
        _lib.check(_lib.lib().slam_set_maps(self.h, _d(m), _i(cnt), m.shape[1]))

    def set_noise(self, rows):
        """Per-instance noise parameters (slam_set_noise_each): `rows` = config.noise_rows(...) (a ctypes array of `batch` Noise rows,
        or a sequence of them); None returns to the config of readParams.  Inputs, not state: set them again after load_state."""
        self._set_rows("slam_set_noise_each", rows, Noise, "noise")

    # -- Filter::update(Command, Float32MultiArray) (filter.h:61) for every instance --
    def update(self, cmdMsg, lmMeasMsg, meas_count=None):
        """cmdMsg: Command or (fwd, ang).  lmMeasMsg: float32 array [B][k][3] of (id, range, bearing) padded to a
        common k, with meas_count[B] valid detections per instance; or a flat [3k] list (the reference's
        Float32MultiArray.data), which is then applied to EVERY instance."""
        self._need()
        if not self.isInit:
            raise _lib.SlamError("init() must be called before update()")  # localization_node.cpp:109
        cmd = self._cmd(cmdMsg)
        meas = np.asarray(lmMeasMsg, dtype=np.float32)
        if meas.ndim <= 2 and meas_count is None:  # one message for all instances
            one = meas.reshape(-1, 3)
            k = one.shape[0]
            meas = np.broadcast_to(one, (self.batch, k, 3)) if k else np.zeros((self.batch, 1, 3), np.float32)
            meas_count = np.full(self.batch, k, dtype=np.int32)
        meas = np.ascontiguousarray(meas.reshape(self.batch, -1, 3), dtype=np.float32)
        if meas.shape[1] == 0:
            meas = np.zeros((self.batch, 1, 3), np.float32)
        cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
        if cnt.shape != (self.batch,):
            raise ValueError(f"meas_count: expected shape ({self.batch},), got {cnt.shape}")
        step = _lib.lib().slam_step_each if cmd.ndim == 2 else _lib.lib().slam_step
        _lib.check(step(self.h, _f(cmd), _f(meas), _i(cnt), meas.shape[1]))
        self.timestep += 1

    def update_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride):
        """One timestep on DEVICE messages; cmdMsg is a Command / (fwd, ang) for the batch.  Per-instance commands already on the
        device: update_dev_each."""
        self._need()
        cmd = self._cmd(cmdMsg)
        if cmd.ndim != 1:
            raise ValueError("update_dev takes one command; per-instance commands on the device go to update_dev_each")
        _lib.check(_lib.lib().slam_step_dev(self.h, _f(cmd), C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), k_stride))
        self.timestep += 1

    def update_dev_each(self, d_cmds_ptr, d_meas_ptr, d_count_ptr, k_stride):
        """One timestep with per-instance commands, all DEVICE pointers: cmds [B][2] float32, meas [B][k_stride][3], count [B]."""
        self._need()
        _lib.check(_lib.lib().slam_step_each_dev(self.h, C.c_void_p(d_cmds_ptr), C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), k_stride))
        self.timestep += 1

    def update_sim(self, cmdMsg):
        """One step with the device-side generator (get_cmd, sim_node.py:209-250) feeding the filter; a (batch, 2) command array
        gives every instance its own command."""
        self._need()
        cmd = self._cmd(cmdMsg)
        if cmd.ndim == 2:
            _lib.check(_lib.lib().slam_run_sim_each(self.h, _f(cmd), 1))
        else:
            _lib.check(_lib.lib().slam_step_sim(self.h, _f(cmd)))
        self.timestep += 1

    def run_sim(self, cmds):
        """cmds: (T, 2) for the batch, or (T, batch, 2) per instance."""
        self._need()
        c = np.ascontiguousarray(cmds, dtype=np.float32)
        if c.ndim == 3:
            if c.shape[1:] != (self.batch, 2):
                raise ValueError(f"per-instance commands: expected shape (T, {self.batch}, 2), got {c.shape}")
            _lib.check(_lib.lib().slam_run_sim_each(self.h, _f(c), c.shape[0]))
        else:
            if c.ndim != 2 or c.shape[1] != 2:
                raise ValueError(f"expected commands of shape (T, 2) or (T, {self.batch}, 2), got {c.shape}")
            _lib.check(_lib.lib().slam_run_sim(self.h, _f(c), c.shape[0]))
        self.timestep += c.shape[0]

    # -- Filter::getStateVector() (filter.h:76; ekf.cpp:181-184) --
    def getStateVector(self, instance=0):
        return self.get_state(instance)["x"]

    def get_state(self, instance=0):
        self._need()
        x = np.zeros(self.n_max); P = np.zeros(self.n_max * self.n_max); ids = np.zeros(self.L_max, dtype=np.int32)
        M = C.c_int32(0); ts = C.c_int32(0)
        _lib.check(_lib.lib().slam_get_state(self.h, int(instance), _d(x), _d(P), C.byref(M), _i(ids), C.byref(ts)))
        n = self._n(M.value)
        return dict(x=x[:n].copy(), P=P[:n * n].reshape(n, n).copy(), M=M.value, ids=ids[:M.value].copy(), timestep=ts.value)

    def track_instance(self, instance):
        """publishState(instance) every tick without running the batch's queued steps (slam_track_instance); -1 = off."""
        self._need(); _lib.check(_lib.lib().slam_track_instance(self.h, int(instance)))

    def save_state(self, path):
        """Checkpoint of the whole batch (slam_save_state)."""
        self._need(); _lib.check(_lib.lib().slam_save_state(self.h, str(path).encode()))

    def load_state(self, path):
        """Resume from a checkpoint written by a handle of the same kind / batch / L_max / dtype (slam_load_state)."""
        self._need(); _lib.check(_lib.lib().slam_load_state(self.h, str(path).encode()))
        self.isInit = True

    def poses(self):
        self._need(); out = np.zeros((self.batch, 3)); _lib.check(_lib.lib().slam_get_poses(self.h, _d(out))); return out

    def landmark_counts(self):
        self._need(); out = np.zeros(self.batch, dtype=np.int32); _lib.check(_lib.lib().slam_get_landmark_counts(self.h, _i(out))); return out

    def truth(self):
        self._need(); out = np.zeros((self.batch, 3)); _lib.check(_lib.lib().slam_get_truth(self.h, _d(out))); return out

    def status(self):
        self._need(); out = np.zeros(self.batch, dtype=np.int32); _lib.check(_lib.lib().slam_status(self.h, _i(out))); return out

    def error_stats(self):
        """Per-instance average position error (compute_average_error, plotting_node.py:195-218)."""
        self._need(); out = np.zeros(self.batch); _lib.check(_lib.lib().slam_error_stats(self.h, _d(out))); return out

    def last_meas(self, k_stride):
        self._need()
        meas = np.zeros((self.batch, k_stride, 3), dtype=np.float32); cnt = np.zeros(self.batch, dtype=np.int32)
        _lib.check(_lib.lib().slam_get_last_meas(self.h, _f(meas), _i(cnt), k_stride))
        return meas, cnt

    def algorithmic_bytes(self):
        self._need(); v = C.c_double(0); _lib.check(_lib.lib().slam_algorithmic_bytes(self.h, C.byref(v))); return v.value

    def set_run_chunk(self, steps_per_launch):
        """Timesteps per kernel launch of run_sim (0 = the whole call)."""
        self._need(); _lib.check(_lib.lib().slam_set_run_chunk(self.h, int(steps_per_launch)))

    def set_debug_flags(self, flags):
        self._need(); _lib.check(_lib.lib().slam_set_debug_flags(self.h, int(flags)))

    def step_stamps(self, steps):
        """(wall-clock ticks at 100 MHz, detections) of every workgroup at the end of each of the first `steps` (<= 128)
        timesteps of the LAST multi-step launch (needs set_debug_flags(32) before that launch): two [batch][steps] arrays."""
        self._need()
        L = _lib.lib()
        L.slam_debug_read_prof_raw.argtypes = [C.c_void_p, C.c_void_p]
        L.slam_debug_read_prof_raw.restype = C.c_int
        buf = np.zeros((self.batch, 128), dtype=np.uint64)
        _lib.check(L.slam_debug_read_prof_raw(self.h, buf.ctypes.data_as(C.c_void_p)))
        return (buf[:, :steps] >> np.uint64(4)).astype(np.int64), (buf[:, :steps] & np.uint64(15)).astype(np.int64)

    def k_histogram(self, reset=False):
        """Instance-steps by detections per message (k = 0..6, >= 7) since creation / the last reset (EKF and UKF step kernels)."""
        self._need(); out = np.zeros(8, dtype=np.uint64)
        _lib.check(_lib.lib().slam_k_histogram(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset))))
        return out

    def sweep_stats(self, reset=False):
        """UKF: (Jacobi sweeps that rotated something, eigen-decompositions) since creation / the last reset."""
        self._need(); out = np.zeros(2, dtype=np.uint64)
        _lib.check(_lib.lib().slam_ukf_sweep_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset))))
        return out

    def reset_counters_async(self):
        """Zero the detection-count histogram and the traffic counters in stream order (no host synchronisation)."""
        _lib.check(_lib.lib().slam_reset_counters_async(self.h))

    def traffic_counters(self, reset=False):
        """EKF: device-counted (P-stream bytes read + written by passes, other global bytes, passes, updates applied by passes)
        since creation / the last reset (slam_traffic_counters)."""
        self._need(); out = np.zeros(4, dtype=np.uint64)
        _lib.check(_lib.lib().slam_traffic_counters(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset))))
        return out

    def kernel_info(self, multi_step=True):
        """EKF: the step-kernel instantiation this handle launches and what the runtime reports about it."""
        self._need(); name = C.create_string_buffer(128); out = np.zeros(5, dtype=np.int32)
        _lib.check(_lib.lib().slam_kernel_info(self.h, int(bool(multi_step)), name, 128, _i(out)))
        return dict(name=name.value.decode(), lds_bytes=int(out[0]), vgprs=int(out[1]), threads=int(out[2]),
                    workgroups_per_cu=int(out[3]), cus=int(out[4]))

    # -- no counterpart in the reference: is P believable?  (slam_consistency, include/slam_batch.h) --
    FULL_NOT_PD, POSE_NOT_PD, NO_TRUTH, INSTANCE_FAILED = 1, 2, 4, 8   # slam_consistency_flags

    def consistency(self):
        """NEES of every instance at the current state against the simulator's truth, computed on the GPU: dict of [batch] arrays
        nees_full (e^T S^-1 e, S = (P + P^T) / 2), nees_pose (vehicle marginal), map_rms, dof (3 + 2 M) and flags
        (FULL_NOT_PD, POSE_NOT_PD, NO_TRUTH, INSTANCE_FAILED).  Changes nothing in the handle.  Meaningful while the handle is stepped
        by the simulator (update_sim / run_sim) with a map set; consistency_summary() turns a batch into Bar-Shalom's test."""
        self._need()
        out = dict(nees_full=np.zeros(self.batch), nees_pose=np.zeros(self.batch), map_rms=np.zeros(self.batch),
                   dof=np.zeros(self.batch, dtype=np.int32), flags=np.zeros(self.batch, dtype=np.int32))
        _lib.check(_lib.lib().slam_consistency(self.h, _d(out["nees_full"]), _d(out["nees_pose"]), _d(out["map_rms"]), _i(out["dof"]),
                                               _i(out["flags"])))
        return out

    def last_consistency_work(self):
        """(bytes the model says the last consistency() had to read, its device time in ms)."""
        return self._last_work("slam_last_consistency_work", 2)

    # -- no counterpart in the reference: the error and the pose NEES at every tick of a run (slam_monitor_*, include/slam_batch.h) --
    def monitor_now(self, cfg=None):
        """One monitor evaluation at the current state, changing nothing: dict of rec (16,), err_pos, err_yaw, nees_pose, flags [batch]
        (flags: POSE_NOT_PD, INSTANCE_FAILED).  cfg: a MonitorConfig, a dict of its fields, or None for the defaults."""
        self._need()
        c = config_from(cfg, *MONITOR)
        out = dict(rec=np.zeros(16), err_pos=np.zeros(self.batch), err_yaw=np.zeros(self.batch), nees_pose=np.zeros(self.batch),
                   flags=np.zeros(self.batch, dtype=np.int32))
        _lib.check(_lib.lib().slam_monitor_now(self.h, C.byref(c), _d(out["rec"]), _d(out["err_pos"]), _d(out["err_yaw"]), _d(out["nees_pose"]),
                                               _i(out["flags"])))
        return out

    def _run_cmds(self, name, cmds, T, source=None):
        """The (cmds, T, source) arguments of a run the simulator feeds as (float32 commands or None, source, T).  The sources, numbered
        alike in slam_monitor_source and slam_innovation_source: (T, 2) SHARED, (T, batch, 2) EACH, no commands but T ticks NAV unless
        `source` says otherwise; with commands, a `source` must be the one their shape implies."""
        if cmds is None:
            if T is None:
                raise ValueError(f"{name} needs commands or, for the closed loop, a number of ticks T")
            return None, int(MONITOR_NAV if source is None else source), int(T)
        c32 = np.ascontiguousarray(cmds, dtype=np.float32)
        if c32.ndim == 3 and c32.shape[1:] == (self.batch, 2):
            want = MONITOR_EACH
        elif c32.ndim == 2 and c32.shape[1] == 2:
            want = MONITOR_SHARED
        else:
            raise ValueError(f"expected commands of shape (T, 2) or (T, {self.batch}, 2), got {c32.shape}")
        if T is not None and int(T) != c32.shape[0]:
            raise ValueError(f"T = {T} does not match the {c32.shape[0]} commands")
        if source is not None and source != want:
            raise ValueError(f"source {source} does not match commands of shape {c32.shape}")
        return c32, want, c32.shape[0]

    def monitor_run(self, cmds=None, T=None, source=None, series=False, cfg=None):
        """A monitored run: per tick one simulator timestep and one monitor evaluation, all on the device; the same bits as the
        unmonitored run of the same commands.  cmds (T, 2): shared commands; (T, batch, 2): per instance; None with T ticks: the
        controller of set_path / set_paths issues them (source MONITOR_NAV).  Returns a MonitorResult; series=True also records the
        per-instance err_pos, err_yaw and nees_pose of every tick."""
        self._need()
        c32, source, T = self._run_cmds("monitor_run", cmds, T, source)
        n = max(T, 0)
        res = MonitorResult(np.zeros((n, 16)))
        if series:
            res.err_pos, res.err_yaw, res.nees_pose = (np.zeros((n, self.batch)) for _ in range(3))
        c = config_from(cfg, *MONITOR)
        _lib.check(_lib.lib().slam_monitor_run(self.h, C.byref(c), source, ptr(c32), T,
                                               opt(res.recs), opt(res.err_pos), opt(res.err_yaw), opt(res.nees_pose)))
        self.timestep += n
        return res

    def last_monitor_work(self):
        """(device ms of what the monitor added to the last monitor_run, or -1 without set_nav_timing; device ms of the whole run)."""
        return self._last_work("slam_last_monitor_work", 2)

    # -- closed loop: goal_pursuit_node.py:23-50 on the device (slam_nav_*, include/slam_batch.h) --
    def set_path(self, pts, nav=None):
        """One path (P, 2) of waypoints for every instance; nav: a NavConfig, a dict of its fields, or None for the reference's
        defaults (pure pursuit, loose control).  Resets the controller state."""
        self._need()
        p = np.ascontiguousarray(pts, dtype=np.float64)
        if p.ndim != 2 or p.shape[1] != 2:
            raise ValueError(f"expected a path of shape (P, 2), got {p.shape}")
        c = config_from(nav, *NAV)
        _lib.check(_lib.lib().slam_nav_set_path(self.h, C.byref(c), _d(p), p.shape[0]))

    def set_paths(self, paths, counts=None, nav=None):
        """One path per instance: a list of batch (P_b, 2) arrays, or a (batch, P_stride, 2) array with `counts` [batch] waypoints
        each (default: all P_stride)."""
        self._need()
        if isinstance(paths, (list, tuple)):
            ps = [np.asarray(p, dtype=np.float64) for p in paths]
            if len(ps) != self.batch or any(p.ndim != 2 or p.shape[1] != 2 or p.shape[0] == 0 for p in ps):
                raise ValueError(f"expected a list of {self.batch} paths of shape (P_b > 0, 2)")
            counts = np.array([p.shape[0] for p in ps], dtype=np.int32)
            arr = np.zeros((self.batch, int(counts.max()), 2))
            for b, p in enumerate(ps):
                arr[b, :p.shape[0]] = p
            paths = arr
        a = np.ascontiguousarray(paths, dtype=np.float64)
        if a.ndim != 3 or a.shape[0] != self.batch or a.shape[2] != 2 or a.shape[1] == 0:
            raise ValueError(f"expected per-instance paths of shape ({self.batch}, P_stride > 0, 2), got {a.shape}")
        cnt = np.full(self.batch, a.shape[1], np.int32) if counts is None else np.ascontiguousarray(counts, dtype=np.int32)
        if cnt.shape != (self.batch,):
            raise ValueError(f"counts: expected {self.batch} waypoint counts")
        c = config_from(nav, *NAV)
        _lib.check(_lib.lib().slam_nav_set_paths(self.h, C.byref(c), _d(a), _i(cnt), a.shape[1]))

    def run_nav(self, T, return_cmds=False):
        """T ticks of {controller on every instance's own estimate, one simulator timestep}, all on the device.  return_cmds: the
        (T, batch, 2) float32 commands that were issued."""
        self._need()
        T = int(T)
        cmds = np.zeros((max(T, 0), self.batch, 2), dtype=np.float32) if return_cmds else None
        _lib.check(_lib.lib().slam_nav_run(self.h, T, opt(cmds)))
        self.timestep += max(T, 0)
        return cmds

    def nav_state(self):
        """Controller state of every instance: dict of [batch] arrays remaining (waypoints still queued), finish_tick (-1 until the
        queue is empty), integ, err_prev."""
        self._need()
        out = dict(remaining=np.zeros(self.batch, dtype=np.int32), finish_tick=np.zeros(self.batch, dtype=np.int32),
                   integ=np.zeros(self.batch), err_prev=np.zeros(self.batch))
        _lib.check(_lib.lib().slam_nav_state(self.h, _i(out["remaining"]), _i(out["finish_tick"]), _d(out["integ"]), _d(out["err_prev"])))
        return out

    def nav_estimates(self):
        """(batch, 3) float32 x_v, y_v, yaw_v: the state message's wire values, what the next controller tick reads."""
        self._need(); out = np.zeros((self.batch, 3), dtype=np.float32); _lib.check(_lib.lib().slam_nav_estimates(self.h, _f(out))); return out

    def set_nav_timing(self, per_tick=True):
        """Time every controller launch of the following run_nav calls with its own event pair (off by default)."""
        self._need(); _lib.check(_lib.lib().slam_nav_set_timing(self.h, int(bool(per_tick))))

    def last_nav_work(self):
        """(device ms of the controller kernels, or -1 without set_nav_timing; device ms of everything) of the last run_nav, by HIP events."""
        return self._last_work("slam_last_nav_work", 2)

    def set_lazy_steps(self, n):
        self._need(); _lib.check(_lib.lib().slam_set_lazy_steps(self.h, int(n)))

    def sync(self):
        self._need(); _lib.check(_lib.lib().slam_sync(self.h))


class BatchedEKF(BatchedFilter):
    """EKF-SLAM (reference: class EKF, filter.h:148-174, ekf.cpp)."""

    kind = EKF_SLAM

    def _n(self, M):
        return 3 + 2 * M

    # -- EKF::publishState payload (ekf.cpp:192-220, EKFState.msg) --
    def publishState(self, instance=0):
        s = self.get_state(instance)
        x, M = s["x"], s["M"]
        lm = np.empty(3 * M, dtype=np.float32)  # [id, x, y] triplets (ekf.cpp:203-208)
        lm[0::3] = s["ids"]; lm[1::3] = x[3::2]; lm[2::3] = x[4::2]
        return dict(timestep=s["timestep"], x_v=np.float32(x[0]), y_v=np.float32(x[1]), yaw_v=np.float32(x[2]),
                    M=M, landmarks=lm, P=s["P"].astype(np.float32).ravel())  # P row-major (ekf.cpp:211-217)

    # -- no counterpart in the reference: is the filter believable WITHOUT the truth?  (slam_innovation_*, include/slam_batch.h) --
    INNOVATION_FROZEN, INNOVATION_WOULD_FREEZE, INNOVATION_S_SINGULAR, INNOVATION_TOO_LONG = 1, 2, 4, 8   # slam_innovation_flags

    def innovation(self, cmdMsg, meas, meas_count, det=True, cfg=None):
        """What the next update(cmdMsg, meas, meas_count) will compute, from the state as it is and changing nothing: dict of rec (16,),
        nis_sum, n_upd, n_new, flags [batch], post (batch, 12) = the pose and its 3 x 3 covariance after the step, and - det=True -
        det (batch, INNOV_MAX_DET, 6) = (nis, nu_r, nu_b, S00, S01, S11) per detection slot, NaN where the slot is no update.  cmdMsg: one
        command or (batch, 2); meas (batch, k_stride, 3) float32 [id, range, bearing]; meas_count [batch]."""
        self._need()
        cmd = self._cmd(cmdMsg)
        m = np.ascontiguousarray(meas, dtype=np.float32)
        cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
        if m.ndim != 3 or m.shape[0] != self.batch or m.shape[2] != 3 or cnt.shape != (self.batch,):
            raise ValueError(f"expected meas of shape ({self.batch}, k_stride, 3) and meas_count of shape ({self.batch},)")
        B = self.batch
        out = dict(rec=np.zeros(16), nis_sum=np.zeros(B), n_upd=np.zeros(B, dtype=np.int32), n_new=np.zeros(B, dtype=np.int32),
                   flags=np.zeros(B, dtype=np.int32), post=np.zeros((B, 12)))
        if det:
            out["det"] = np.zeros((B, INNOV_MAX_DET, 6))
        c = config_from(cfg, *INNOVATION)
        _lib.check(_lib.lib().slam_innovation(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1], _d(out["rec"]),
                                              _d(out["nis_sum"]), _i(out["n_upd"]), _i(out["n_new"]), _i(out["flags"]), opt(out.get("det")),
                                              _d(out["post"])))
        return out

    def innovation_run(self, cmds=None, T=None, meas=None, meas_count=None, series=False, cfg=None):
        """A run with the innovation statistics of every tick: per tick the innovation launches and then the one-step launch, all on the
        device; the same bits as the plain run of the same inputs.  cmds (T, 2): shared commands, (T, batch, 2): per instance, None with
        T ticks: the controller of set_path / set_paths - the simulator generates the messages; cmds (T, 2) with meas
        (T, batch, k_stride, 3) and meas_count (T, batch): a recorded log (source INNOVATION_LOG).  Returns an InnovationResult;
        series=True also records nis_sum, n_upd and flags of every instance at every tick."""
        self._need()
        m = cnt = None
        if cmds is not None and meas is not None:   # a log: its shapes are checked as a whole, before T
            cmds = np.ascontiguousarray(cmds, dtype=np.float32)
            m = np.ascontiguousarray(meas, dtype=np.float32)
            cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
            if cmds.ndim != 2 or cmds.shape[1] != 2 or m.ndim != 4 or m.shape[:2] != (cmds.shape[0], self.batch) or m.shape[3] != 3 \
                    or cnt.shape != m.shape[:2]:
                raise ValueError(f"a log needs cmds (T, 2), meas (T, {self.batch}, k_stride, 3) and meas_count (T, {self.batch})")
        c32, source, T = self._run_cmds("innovation_run", cmds, T)
        if m is not None:
            source = INNOVATION_LOG
        n = max(T, 0)
        res = InnovationResult(np.zeros((n, 16)))
        if series:
            res.nis_sum = np.zeros((n, self.batch))
            res.n_upd, res.flags = np.zeros((n, self.batch), dtype=np.int32), np.zeros((n, self.batch), dtype=np.int32)
        c = config_from(cfg, *INNOVATION)
        _lib.check(_lib.lib().slam_innovation_run(self.h, C.byref(c), source, ptr(c32),
                                                  ptr(m), ptr(cnt),
                                                  0 if m is None else m.shape[2], T, opt(res.recs), opt(res.nis_sum), opt(res.n_upd),
                                                  opt(res.flags)))
        self.timestep += n
        return res

    def last_innovation_work(self):
        """(device ms of the innovation launches of the last innovation_run, or -1 without set_nav_timing; device ms of the whole run)."""
        return self._last_work("slam_last_innovation_work", 2)

    # -- what the gate, the association and the map calls share --
    def _message(self, meas, meas_count):
        m = np.ascontiguousarray(meas, dtype=np.float32)
        cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
        if m.ndim != 3 or m.shape[0] != self.batch or m.shape[1] == 0 or m.shape[2] != 3 or cnt.shape != (self.batch,):
            raise ValueError(f"expected meas of shape ({self.batch}, k_stride > 0, 3) and meas_count of shape ({self.batch},)")
        return m, cnt

    def _log(self, cmds, meas, meas_count):
        """A recorded log as (commands, each, meas, meas_count), float32 / int32 and their shapes checked against each other."""
        c32 = np.ascontiguousarray(cmds, dtype=np.float32)
        m = np.ascontiguousarray(meas, dtype=np.float32)
        cnt = np.ascontiguousarray(meas_count, dtype=np.int32)
        each = c32.ndim == 3
        if c32.shape[1:] != ((self.batch, 2) if each else (2,)) or m.ndim != 4 or m.shape[:2] != (c32.shape[0], self.batch) or m.shape[2] == 0 \
                or m.shape[3] != 3 or cnt.shape != m.shape[:2]:
            raise ValueError(f"a log needs cmds (T, 2) or (T, {self.batch}, 2), meas (T, {self.batch}, k_stride > 0, 3) and meas_count (T, {self.batch})")
        return c32, each, m, cnt

    def _stats(self, stats, key):
        """The outputs of a step or a map edit: (dict(rec (16,), `key` [batch] int32), their two pointers), all None without stats."""
        if not stats:
            return None, None, None
        out = {"rec": np.zeros(16), key: np.zeros(self.batch, dtype=np.int32)}
        return out, _d(out["rec"]), _i(out[key])

    def _filtered_run(self, run, cfgs, series, log=None, sim=None):
        """One of the ten runs that filter a message before the step, described by _RUNS[run].  log = (cmds, meas, meas_count): the
        recorded-log form; sim = (the caller's name, cmds, T, source, k_stride, log): the *_run_sim form, whose result gets `.sense`."""
        Result, symbol, symbol_sim, kinds, outs = _RUNS[run]
        self._need()
        if sim is None:
            c32, each, m, cnt = self._log(*log)
            T = c32.shape[0]
            head, tail = (_f(c32), int(each), _f(m), _i(cnt), m.shape[2], T), ()
        else:
            name, cmds, T, source, k_stride, want = sim
            c32, source, T = self._run_cmds(name, cmds, T, source)
            ks, symbol = int(k_stride), symbol_sim
            sense = SenseLogResult(max(T, 0), self.batch, max(ks, 1), want) if want else None
            head, tail = (source, ptr(c32), ks, T), (C.byref(sense.struct()) if want and T > 0 else None,)
        n = max(T, 0)
        res = Result(np.zeros((n, 16)))
        if series:
            for key, dtype in outs:
                setattr(res, key, np.zeros((n, self.batch), dtype=dtype))
        structs = [C.byref(config_from(cfg, *kind)) for cfg, kind in zip(cfgs, kinds)]
        _lib.check(getattr(_lib.lib(), symbol)(self.h, *structs, *head, opt(res.recs), *[opt(getattr(res, key)) for key, _ in outs], *tail))
        self.timestep += n
        if sim is not None:
            res.sense = sense
        return res

    # -- the chi-square gate on every detection (slam_gate_*, include/slam_batch.h) --
    def _gate_outputs(self, det):
        B = self.batch
        out = dict(rec=np.zeros(16), nis_sum=np.zeros(B), n_upd=np.zeros(B, dtype=np.int32), n_new=np.zeros(B, dtype=np.int32),
                   flags=np.zeros(B, dtype=np.int32), post=np.zeros((B, 12)), n_rej=np.zeros(B, dtype=np.int32),
                   verdict=np.zeros((B, INNOV_MAX_DET), dtype=np.int32))
        if det:
            out["det"] = np.zeros((B, INNOV_MAX_DET, 6))
        return out

    def gate(self, cmdMsg, meas, meas_count, det=True, cfg=None):
        """The chi-square gate on the message the next update(cmdMsg, meas, meas_count) would be given, changing nothing in the filter:
        the dict of innovation() - nis_sum, post and the record over the ACCEPTED updates - plus n_rej [batch], verdict
        (batch, INNOV_MAX_DET) (0 no update slot, 1 accepted, 2 rejected), and the filtered message meas_out (batch, k_stride, 3),
        count_out [batch]: update(cmdMsg, meas_out, count_out) is the gated step.  cfg: a GateConfig, a dict of its fields, or None."""
        self._need()
        cmd = self._cmd(cmdMsg)
        m, cnt = self._message(meas, meas_count)
        out = self._gate_outputs(det)
        out["meas_out"], out["count_out"] = np.zeros_like(m), np.zeros_like(cnt)
        c = config_from(cfg, *GATE)
        _lib.check(_lib.lib().slam_gate(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1],
                                        _d(out["rec"]), _d(out["nis_sum"]), _i(out["n_upd"]), _i(out["n_new"]), _i(out["flags"]),
                                        opt(out.get("det")), _d(out["post"]), _f(out["meas_out"]), _i(out["count_out"]),
                                        _i(out["n_rej"]), _i(out["verdict"])))
        return out

    def gate_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride, d_meas_out_ptr, d_count_out_ptr, det=True, cfg=None):
        """gate() on DEVICE messages: cmdMsg one command (host) or, as an int, the device pointer of (batch, 2) commands; the filtered
        message is written to d_meas_out_ptr / d_count_out_ptr, which may be the input pair itself (in place).  Returns the dict of gate()
        without meas_out and count_out."""
        self._need()
        cp, each = self._cmd_dev(cmdMsg, "gate_dev takes")
        out = self._gate_outputs(det)
        c = config_from(cfg, *GATE)
        _lib.check(_lib.lib().slam_gate_dev(self.h, C.byref(c), cp, each, C.c_void_p(d_meas_ptr),
                                            C.c_void_p(d_count_ptr), int(k_stride), _d(out["rec"]), _d(out["nis_sum"]), _i(out["n_upd"]),
                                            _i(out["n_new"]), _i(out["flags"]), opt(out.get("det")), _d(out["post"]),
                                            C.c_void_p(d_meas_out_ptr), C.c_void_p(d_count_out_ptr), _i(out["n_rej"]), _i(out["verdict"])))
        return out

    def step_gated(self, cmdMsg, meas, meas_count, stats=True, cfg=None):
        """One gated timestep: the gate, then the ordinary step on the filtered message, on the device.  cmdMsg one command or (batch, 2);
        host message as gate().  stats=True returns dict(rec (16,), n_rej [batch]) and synchronises; stats=False returns None."""
        self._need()
        cmd = self._cmd(cmdMsg)
        m, cnt = self._message(meas, meas_count)
        out, rec, nr = self._stats(stats, "n_rej")
        c = config_from(cfg, *GATE)
        fn = _lib.lib().slam_step_gated_each if cmd.ndim == 2 else _lib.lib().slam_step_gated
        _lib.check(fn(self.h, C.byref(c), _f(cmd), _f(m), _i(cnt), m.shape[1], rec, nr))
        self.timestep += 1
        return out

    def step_gated_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride, stats=True, cfg=None):
        """step_gated() on DEVICE messages; cmdMsg one command (host) or, as an int, the device pointer of (batch, 2) commands."""
        self._need()
        cp, each = self._cmd_dev(cmdMsg, "step_gated_dev takes")
        out, rec, nr = self._stats(stats, "n_rej")
        c = config_from(cfg, *GATE)
        if each:
            fn = _lib.lib().slam_step_gated_each_dev
        else:
            fn, cp = _lib.lib().slam_step_gated_dev, C.cast(cp, C.POINTER(C.c_float))   # this one symbol declares the host command as float *
        _lib.check(fn(self.h, C.byref(c), cp, C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), int(k_stride), rec, nr))
        self.timestep += 1
        return out

    def gate_run(self, cmds, meas, meas_count, series=False, cfg=None):
        """T gated ticks of a recorded log: cmds (T, 2) or (T, batch, 2), meas (T, batch, k_stride, 3), meas_count (T, batch); the same bits
        as T step_gated calls.  Returns a GateResult; series=True also records nis_sum, n_upd, n_rej and flags of every instance."""
        return self._filtered_run("gate", (cfg,), series, log=(cmds, meas, meas_count))

    def last_gate_work(self):
        """(device ms of the gate launches of the last gate_run, or -1 without set_nav_timing; device ms of the whole run)."""
        return self._last_work("slam_last_gate_work", 2)

    # -- detections without ids: nearest neighbour in Mahalanobis distance (slam_associate_*, include/slam_batch.h) --
    def _assoc_outputs(self, det):
        B = self.batch
        out = dict(rec=np.zeros(16), n_match=np.zeros(B, dtype=np.int32), n_new=np.zeros(B, dtype=np.int32), n_drop=np.zeros(B, dtype=np.int32),
                   flags=np.zeros(B, dtype=np.int32), verdict=np.zeros((B, INNOV_MAX_DET), dtype=np.int32),
                   slot=np.zeros((B, INNOV_MAX_DET), dtype=np.int32))
        if det:
            out["det"] = np.zeros((B, INNOV_MAX_DET, 4))
        return out

    @staticmethod
    def _assoc_pointers(out):
        """The outputs slam_associate* and slam_associate_joint* share, in C order up to det."""
        return (_d(out["rec"]), _i(out["n_match"]), _i(out["n_new"]), _i(out["n_drop"]), _i(out["flags"]), _i(out["verdict"]), _i(out["slot"]),
                opt(out.get("det")))

    def associate(self, cmdMsg, meas, meas_count, det=True, cfg=None):
        """Labels a message whose id column is not read with landmark ids, from the state as it is and changing nothing: dict of rec (16,),
        n_match, n_new, n_drop, flags [batch], verdict and slot (batch, INNOV_MAX_DET) (ASSOC_* verdicts; the best landmark slot or -1),
        - det=True - det (batch, INNOV_MAX_DET, 4) = (d2_best, d2_second, nu_r, nu_b of the best), and the labelled message meas_out
        (batch, k_stride, 3), count_out [batch]: update(cmdMsg, meas_out, count_out) is the associated step.  cfg: an AssocConfig, a dict of
        its fields, or None."""
        self._need()
        cmd = self._cmd(cmdMsg)
        m, cnt = self._message(meas, meas_count)
        out = self._assoc_outputs(det)
        out["meas_out"], out["count_out"] = np.zeros_like(m), np.zeros_like(cnt)
        c = config_from(cfg, *ASSOC)
        _lib.check(_lib.lib().slam_associate(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1],
                                             *self._assoc_pointers(out), _f(out["meas_out"]), _i(out["count_out"])))
        return out

    def associate_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride, d_meas_out_ptr, d_count_out_ptr, det=True, cfg=None):
        """associate() on DEVICE messages: cmdMsg one command (host) or, as an int, the device pointer of (batch, 2) commands; the labelled
        message is written to d_meas_out_ptr / d_count_out_ptr, which may be the input pair itself (in place).  Returns the dict of
        associate() without meas_out and count_out."""
        self._need()
        cp, each = self._cmd_dev(cmdMsg, "associate_dev takes")
        out = self._assoc_outputs(det)
        c = config_from(cfg, *ASSOC)
        _lib.check(_lib.lib().slam_associate_dev(self.h, C.byref(c), cp, each, C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), int(k_stride),
                                                 *self._assoc_pointers(out), C.c_void_p(d_meas_out_ptr), C.c_void_p(d_count_out_ptr)))
        return out

    def step_associated(self, cmdMsg, meas, meas_count, stats=True, cfg=None):
        """One associated timestep: the association, then the ordinary step on the labelled message, on the device.  cmdMsg one command or
        (batch, 2); host message as associate().  stats=True returns dict(rec (16,), n_drop [batch]) and synchronises; stats=False None."""
        self._need()
        cmd = self._cmd(cmdMsg)
        m, cnt = self._message(meas, meas_count)
        out, rec, nd = self._stats(stats, "n_drop")
        c = config_from(cfg, *ASSOC)
        _lib.check(_lib.lib().slam_step_associated(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1], rec, nd))
        self.timestep += 1
        return out

    def step_associated_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride, stats=True, cfg=None):
        """step_associated() on DEVICE messages; cmdMsg one command (host) or, as an int, the device pointer of (batch, 2) commands."""
        self._need()
        cp, each = self._cmd_dev(cmdMsg, "step_associated_dev takes")
        out, rec, nd = self._stats(stats, "n_drop")
        c = config_from(cfg, *ASSOC)
        _lib.check(_lib.lib().slam_step_associated_dev(self.h, C.byref(c), cp, each, C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr),
                                                       int(k_stride), rec, nd))
        self.timestep += 1
        return out

    def associate_run(self, cmds, meas, meas_count, series=False, cfg=None):
        """T associated ticks of a recorded log without ids: cmds (T, 2) or (T, batch, 2), meas (T, batch, k_stride, 3), meas_count
        (T, batch); the same bits as T step_associated calls.  Returns an AssocResult; series=True also records n_match, n_new, n_drop and
        flags of every instance."""
        return self._filtered_run("associate", (cfg,), series, log=(cmds, meas, meas_count))

    def last_associate_work(self):
        """(model bytes of the association launches of the last associate / associate_dev / associate_run, the same with the reads of P in
        128-byte lines, device ms of the association launches of the last associate_run or -1 without set_nav_timing, device ms of that
        whole run or -1)."""
        return self._last_work("slam_last_associate_work", 2, pair=True)

    # -- detections without ids, judged jointly: JCBB (slam_associate_joint_*, include/slam_batch.h) --
    def _joint_config(self, cfg):
        return _joint_config(cfg)

    def _joint_outputs(self, det):
        out = self._assoc_outputs(det)
        out.update(d2_joint=np.zeros(self.batch), nodes=np.zeros(self.batch, dtype=np.int32),
                   ncand=np.zeros((self.batch, INNOV_MAX_DET), dtype=np.int32))
        return out

    def associate_joint(self, cmdMsg, meas, meas_count, det=True, cfg=None, dev_out=None):
        """associate() with joint compatibility (JCBB): the dict of associate() - verdict may hold ASSOC_JOINT_UNPAIRED, slot and det are
        those of the paired slot where MATCHED - plus d2_joint [batch], nodes [batch] and ncand (batch, INNOV_MAX_DET).  cfg: a
        JointConfig, a dict of its fields, or None.  meas as an int: DEVICE pointers (meas_count = (pointer, k_stride), cmdMsg one command
        or a device pointer, dev_out = (d_meas_out, d_count_out), which may be the input pair); then no meas_out / count_out are returned."""
        self._need()
        out = self._joint_outputs(det)
        c = self._joint_config(cfg)
        tail = (_d(out["d2_joint"]), _i(out["nodes"]), _i(out["ncand"]))
        if isinstance(meas, int):
            cp, each = self._cmd_dev(cmdMsg, "device messages take")
            _lib.check(_lib.lib().slam_associate_joint_dev(self.h, C.byref(c), cp, each, C.c_void_p(meas), C.c_void_p(meas_count[0]),
                                                           int(meas_count[1]), *self._assoc_pointers(out), C.c_void_p(dev_out[0]),
                                                           C.c_void_p(dev_out[1]), *tail))
            return out
        cmd = self._cmd(cmdMsg)
        m, cnt = self._message(meas, meas_count)
        out["meas_out"], out["count_out"] = np.zeros_like(m), np.zeros_like(cnt)
        _lib.check(_lib.lib().slam_associate_joint(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1],
                                                   *self._assoc_pointers(out), _f(out["meas_out"]), _i(out["count_out"]), *tail))
        return out

    def step_associated_joint(self, cmdMsg, meas, meas_count, stats=True, cfg=None):
        """One jointly associated timestep, as step_associated().  meas as an int: DEVICE pointers as associate_joint()."""
        self._need()
        out, rec, nd = self._stats(stats, "n_drop")
        c = self._joint_config(cfg)
        if isinstance(meas, int):
            cp, each = self._cmd_dev(cmdMsg, "device messages take")
            _lib.check(_lib.lib().slam_step_associated_joint_dev(self.h, C.byref(c), cp, each, C.c_void_p(meas), C.c_void_p(meas_count[0]),
                                                                 int(meas_count[1]), rec, nd))
        else:
            cmd = self._cmd(cmdMsg)
            m, cnt = self._message(meas, meas_count)
            _lib.check(_lib.lib().slam_step_associated_joint(self.h, C.byref(c), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1], rec, nd))
        self.timestep += 1
        return out

    def associate_joint_run(self, cmds, meas, meas_count, series=False, cfg=None):
        """T jointly associated ticks of a recorded log without ids, layout and result as associate_run (the records' columns: JointResult's
        REC_* constants); series=True also records n_match, n_new, n_drop, flags, nodes and d2_joint of every instance."""
        return self._filtered_run("associate_joint", (cfg,), series, log=(cmds, meas, meas_count))

    def last_joint_work(self):
        """last_associate_work() for the joint association: (model bytes, the same with the reads of P in 128-byte lines, device ms of the
        joint launches of the last associate_joint_run or -1 without set_nav_timing, device ms of that whole run or -1)."""
        return self._last_work("slam_last_joint_work", 2, pair=True)

    # -- map management: landmarks leave the map again (slam_remove_landmarks, slam_map_*, include/slam_batch.h) --
    def _mask(self, a, what):
        m = np.ascontiguousarray(a, dtype=np.int32)
        if m.shape != (self.batch, self.L_max):
            raise ValueError(f"{what}: expected shape ({self.batch}, {self.L_max}), got {m.shape}")
        return m

    def remove_landmarks(self, remove, stats=True):
        """Drops the slots whose entry of remove (batch, L_max) is nonzero (entries at or above an instance's landmark count are ignored):
        exact marginalisation, x, P and ids compacted on the device bit for bit.  remove as an int: the DEVICE pointer of the mask.
        stats=True returns dict(rec (16,), n_removed [batch]) and synchronises; stats=False None."""
        self._need()
        out, rec, nr = self._stats(stats, "n_removed")
        if isinstance(remove, int):
            _lib.check(_lib.lib().slam_remove_landmarks_dev(self.h, C.c_void_p(remove), nr, rec))
        else:
            m = self._mask(remove, "remove")
            _lib.check(_lib.lib().slam_remove_landmarks(self.h, _i(m), nr, rec))
        return out

    def map_tally(self, meas, meas_count, assoc_flags=None, cfg=None):
        """Adds the evidence of one labelled message to the track counters, after the step that consumed it: host message as associate();
        assoc_flags [batch] or None.  meas as an int: DEVICE pointers (meas, meas_count = (pointer, k_stride), assoc_flags or None)."""
        self._need()
        c = config_from(cfg, *MAP)
        if isinstance(meas, int):
            d_count, k_stride = meas_count
            _lib.check(_lib.lib().slam_map_tally_dev(self.h, C.byref(c), C.c_void_p(meas), C.c_void_p(d_count), int(k_stride),
                                                     None if assoc_flags is None else C.c_void_p(assoc_flags)))
            return
        m, cnt = self._message(meas, meas_count)
        fl = None if assoc_flags is None else np.ascontiguousarray(assoc_flags, dtype=np.int32)
        if fl is not None and fl.shape != (self.batch,):
            raise ValueError(f"assoc_flags: expected shape ({self.batch},), got {fl.shape}")
        _lib.check(_lib.lib().slam_map_tally(self.h, C.byref(c), _f(m), _i(cnt), m.shape[1], ptr(fl)))

    def map_prune(self, stats=True, cfg=None):
        """Removes the slots the prune rule picks from the track counters, decided and compacted on the device.  Returns as remove_landmarks."""
        self._need()
        out, rec, nr = self._stats(stats, "n_removed")
        c = config_from(cfg, *MAP)
        _lib.check(_lib.lib().slam_map_prune(self.h, C.byref(c), rec, nr))
        return out

    def map_track(self):
        """(seen, expected), (batch, L_max) int32 each: the track counters."""
        self._need()
        seen = np.zeros((self.batch, self.L_max), dtype=np.int32); expected = np.zeros_like(seen)
        _lib.check(_lib.lib().slam_map_get_track(self.h, _i(seen), _i(expected)))
        return seen, expected

    def map_track_reset(self):
        self._need()
        _lib.check(_lib.lib().slam_map_track_reset(self.h))

    def step_managed(self, cmdMsg, meas, meas_count, stats=True, cfg=None, map_cfg=None):
        """step_associated(), then the tally of the labelled message with the association's flags, on the device.  meas as an int: DEVICE
        pointers as step_associated_dev (meas_count = (pointer, k_stride); cmdMsg one command or, as an int, a device pointer)."""
        self._need()
        ac, mc = config_from(cfg, *ASSOC), config_from(map_cfg, *MAP)
        out, rec, nd = self._stats(stats, "n_drop")
        if isinstance(meas, int):
            d_count, k_stride = meas_count
            cp, each = self._cmd_dev(cmdMsg, "a managed step on device messages takes")
            _lib.check(_lib.lib().slam_step_managed_dev(self.h, C.byref(ac), C.byref(mc), cp, each, C.c_void_p(meas), C.c_void_p(d_count),
                                                        int(k_stride), rec, nd))
        else:
            cmd = self._cmd(cmdMsg)
            m, cnt = self._message(meas, meas_count)
            _lib.check(_lib.lib().slam_step_managed(self.h, C.byref(ac), C.byref(mc), _f(cmd), int(cmd.ndim == 2), _f(m), _i(cnt), m.shape[1], rec, nd))
        self.timestep += 1
        return out

    def manage_run(self, cmds, meas, meas_count, series=False, cfg=None, map_cfg=None):
        """T managed ticks of a recorded log without ids, layout as associate_run: every tick a step_managed, and a map_prune after every
        prune_every-th tick; the same bits as that loop.  Returns a MapResult; series=True also records n_match, n_new, n_drop, flags and
        n_removed of every instance."""
        return self._filtered_run("manage", (cfg, map_cfg), series, log=(cmds, meas, meas_count))

    def last_map_work(self):
        """(model bytes the removals of the last remove_landmarks / map_prune / manage_run had to move, device ms of the prunes of the last
        manage_run or -1 without set_nav_timing, device ms of that whole run or -1)."""
        return self._last_work("slam_last_map_work", 3)

    # -- landmark merging: duplicate landmarks are found and fused (slam_map_duplicates, slam_merge_landmarks, slam_map_merge) --
    def map_duplicates(self, d2=True, cfg=None, dev=None):
        """The duplicate decision, no state change: (partner, d2), (batch, L_max) each: the slot's mutual nearest neighbour within gate_merge
        (-1: none) and - d2=True, else None - the d2 of its best candidate (NaN: none).  dev = (d_partner, d_d2 or None): DEVICE pointers,
        written in stream order; returns None."""
        self._need()
        c = config_from(cfg, *MERGE)
        if dev is not None:
            _lib.check(_lib.lib().slam_map_duplicates_dev(self.h, C.byref(c), C.c_void_p(dev[0]), None if dev[1] is None else C.c_void_p(dev[1])))
            return None
        partner = np.zeros((self.batch, self.L_max), dtype=np.int32)
        dd = np.zeros((self.batch, self.L_max)) if d2 else None
        _lib.check(_lib.lib().slam_map_duplicates(self.h, C.byref(c), _i(partner), opt(dd)))
        return partner, dd

    def merge_landmarks(self, partner, stats=True, cfg=None):
        """Fuses the pairs of partner (batch, L_max): an entry is honoured where it is mutual and both slots are mapped; the others are
        ignored and counted.  partner as an int: the DEVICE pointer of the array.  stats=True returns dict(rec (16,), n_merged [batch]) and
        synchronises; stats=False None."""
        self._need()
        c = config_from(cfg, *MERGE)
        out, rec, nm = self._stats(stats, "n_merged")
        if isinstance(partner, int):
            _lib.check(_lib.lib().slam_merge_landmarks_dev(self.h, C.byref(c), C.c_void_p(partner), nm, rec))
        else:
            m = self._mask(partner, "partner")
            _lib.check(_lib.lib().slam_merge_landmarks(self.h, C.byref(c), _i(m), nm, rec))
        return out

    def map_merge(self, stats=True, cfg=None):
        """Finds the duplicate pairs, fuses them and compacts the maps, all on the device.  Returns as merge_landmarks."""
        self._need()
        out, rec, nm = self._stats(stats, "n_merged")
        c = config_from(cfg, *MERGE)
        _lib.check(_lib.lib().slam_map_merge(self.h, C.byref(c), rec, nm))
        return out

    def manage_merge_run(self, cmds, meas, meas_count, series=False, cfg=None, map_cfg=None, merge_cfg=None):
        """manage_run with a map_merge after every merge_every-th tick, before that tick's prune; the same bits as that loop.  Returns a
        MergeResult; series=True also records n_match, n_new, n_drop, flags, n_removed and n_merged of every instance."""
        return self._filtered_run("manage_merge", (cfg, map_cfg, merge_cfg), series, log=(cmds, meas, meas_count))

    def last_merge_work(self):
        """(model bytes the last map_duplicates / merge_landmarks / map_merge / manage_merge_run had to move, device ms of the merges of the
        last manage_merge_run or -1 without set_nav_timing, device ms of that whole run or -1)."""
        return self._last_work("slam_last_merge_work", 3)

    # -- absolute position and heading fixes (slam_fix_*; include/slam_batch.h) --
    def fix(self, fix, kinds, stats=True, cfg=None):
        """One fix of every instance: fix (batch, 5) rows {z_x, z_y, z_yaw, sigma_pos, sigma_yaw}, kinds [batch] (FIX_POS | FIX_YAW).  Both as
        ints: the DEVICE pointers of the arrays, read in stream order (nothing is returned and nothing synchronises).  stats=True returns
        dict(verdict [batch] (position | heading << 4), nis (batch, 2), rec (16,)) and synchronises; stats=False None."""
        self._need()
        c = config_from(cfg, *FIX)
        if isinstance(fix, int) or isinstance(kinds, int):
            if not (isinstance(fix, int) and isinstance(kinds, int)):
                raise ValueError("fix and kinds are both device pointers or both arrays")
            _lib.check(_lib.lib().slam_fix_dev(self.h, C.byref(c), C.c_void_p(fix), C.c_void_p(kinds), None, None, None))
            return None
        f = np.ascontiguousarray(fix, dtype=np.float64)
        k = np.ascontiguousarray(kinds, dtype=np.int32)
        if f.shape != (self.batch, 5) or k.shape != (self.batch,):
            raise ValueError(f"expected fix ({self.batch}, 5) and kinds ({self.batch},), got {f.shape} and {k.shape}")
        out = dict(verdict=np.zeros(self.batch, dtype=np.int32), nis=np.zeros((self.batch, 2)), rec=np.zeros(16)) if stats else {}
        _lib.check(_lib.lib().slam_fix(self.h, C.byref(c), _d(f), _i(k), opt(out.get("verdict")), opt(out.get("nis")), opt(out.get("rec"))))
        return out or None

    def set_fix_sensor(self, rows):
        """The simulated source of fix_sense() and fix_run (slam_set_fix_sensor_each): one FixSensorConfig (or a dict of its fields),
        replicated over the batch, or `batch` of them; None returns to the all-zero row, which emits nothing.  Inputs, not state."""
        self._set_rows("slam_set_fix_sensor_each", rows, FixSensorConfig, "fix sensor", one=default_fix_sensor_config)

    def fix_sense(self, dev=None):
        """One emission of the simulated source from the true poses: dict(fix (batch, 5), kinds [batch], jumped [batch]).  dev = (d_fix,
        d_kinds, d_jumped or None): DEVICE pointers, written in stream order; returns None."""
        self._need()
        if dev is not None:
            _lib.check(_lib.lib().slam_fix_sense_dev(self.h, C.c_void_p(dev[0]), C.c_void_p(dev[1]), C.c_void_p(dev[2]) if dev[2] else None))
            return None
        out = dict(fix=np.zeros((self.batch, 5)), kinds=np.zeros(self.batch, dtype=np.int32), jumped=np.zeros(self.batch, dtype=np.int32))
        _lib.check(_lib.lib().slam_fix_sense(self.h, _d(out["fix"]), _i(out["kinds"]), _i(out["jumped"])))
        return out

    def fix_run(self, cmds=None, T=None, source=None, series=False, cfg=None):
        """Per tick one simulator timestep and, after every fix_every-th tick, one emission of the simulated source and its fix, all on the
        device; the same bits as that loop of single calls.  cmds (T, 2): shared commands; (T, batch, 2): per instance; None with T ticks:
        the controller of set_path / set_paths.  Returns a FixResult; series=True also records verdict, nis, fix and kinds of every tick."""
        self._need()
        c32, source, T = self._run_cmds("fix_run", cmds, T, source)
        n = max(T, 0)
        res = FixResult(np.zeros((n, 16)))
        log = None
        if series:
            res.verdict, res.kinds = np.zeros((n, self.batch), dtype=np.int32), np.zeros((n, self.batch), dtype=np.int32)
            res.nis, res.fix = np.zeros((n, self.batch, 2)), np.zeros((n, self.batch, 5))
            if n > 0:
                log = FixLog(_d(res.fix), _i(res.kinds))
        c = config_from(cfg, *FIX)
        _lib.check(_lib.lib().slam_fix_run(self.h, C.byref(c), source, ptr(c32), T, opt(res.recs),
                                           opt(res.verdict), opt(res.nis), None if log is None else C.byref(log)))
        self.timestep += n
        return res

    def last_fix_work(self):
        """(model bytes the last fix, or all the fixes of the last fix_run, had to move; device ms of the fix launches of the last fix_run
        or -1 without set_nav_timing; device ms of that whole run or -1)."""
        return self._last_work("slam_last_fix_work", 3)

    # -- the simulator source with a sensor fault model (slam_sense_*, the *_run_sim calls; include/slam_batch.h) --
    def set_sensor(self, rows):
        """The sensor fault model of sense() and the *_run_sim calls (slam_set_sensor_each): one SensorConfig (or a dict of its fields),
        replicated over the batch, or `batch` of them (a sequence or a ctypes array); None returns to the all-off row.  Inputs, not state:
        set them again after load_state."""
        self._set_rows("slam_set_sensor_each", rows, SensorConfig, "sensor", one=default_sensor_config)

    def sense(self, cmdMsg, k_stride, labels=True, stats=True):
        """One tick of the sensor model for the command the step will be given (one command or (batch, 2)): dict(meas (batch, k_stride, 3),
        count [batch], truth_next (batch, 3), and with labels origin and fault (batch, k_stride), with stats rec (16,)).  The truth is
        staged: step on the message (update_dev, step_gated_dev, ... or update) and then call sense_commit()."""
        self._need()
        cmd = self._cmd(cmdMsg)
        B, ks = self.batch, int(k_stride)
        out = dict(meas=np.zeros((B, max(ks, 0), 3), dtype=np.float32), count=np.zeros(B, dtype=np.int32), truth_next=np.zeros((B, 3)))
        if labels:
            out["origin"], out["fault"] = np.zeros((B, max(ks, 0)), dtype=np.int32), np.zeros((B, max(ks, 0)), dtype=np.int32)
        if stats:
            out["rec"] = np.zeros(16)
        _lib.check(_lib.lib().slam_sense(self.h, _f(cmd), int(cmd.ndim == 2), _f(out["meas"]), _i(out["count"]), ks,
                                         _i(out["origin"]) if labels else None, _i(out["fault"]) if labels else None, _d(out["truth_next"]),
                                         opt(out.get("rec"))))
        return out

    def sense_dev(self, cmdMsg, d_meas_ptr, d_count_ptr, k_stride, d_origin_ptr=None, d_fault_ptr=None):
        """sense() into DEVICE buffers, in the order of the handle's stream; cmdMsg one command (host) or, as an int, the device pointer
        of (batch, 2) commands.  Does not synchronise."""
        self._need()
        cp, each = self._cmd_dev(cmdMsg, "sense_dev takes")
        _lib.check(_lib.lib().slam_sense_dev(self.h, cp, each, C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), int(k_stride),
                                             C.c_void_p(d_origin_ptr) if d_origin_ptr else None, C.c_void_p(d_fault_ptr) if d_fault_ptr else None))

    def sense_commit(self, stats=True):
        """After the step on the sensed message: the staged truth becomes the truth of every instance that advanced by one timestep, and
        its position error is added.  stats=True returns the tick's record (16,) and synchronises; stats=False returns None."""
        self._need()
        rec = np.zeros(16) if stats else None
        _lib.check(_lib.lib().slam_sense_commit(self.h, opt(rec)))
        return rec

    def gate_run_sim(self, cmds=None, T=None, source=None, series=False, log=False, k_stride=16, cfg=None):
        """gate_run with the simulator and the sensor model of set_sensor as its source: cmds (T, 2) shared, (T, batch, 2) per instance,
        None with T ticks the controller of set_path (source INNOVATION_NAV).  Returns a GateResult whose `.sense` is None or, with
        log=True, a SenseLogResult (meas, count, origin, fault, truth, err_pos, cmds, recs of every tick); log may also name the wanted
        arrays, e.g. ("origin", "err_pos"): the others are not held on the device or copied."""
        return self._filtered_run("gate", (cfg,), series, sim=("gate_run_sim", cmds, T, source, k_stride, log))

    def associate_run_sim(self, cmds=None, T=None, source=None, series=False, log=False, k_stride=16, cfg=None):
        """associate_run with the simulator and the sensor model as its source (arguments and `.sense` as gate_run_sim)."""
        return self._filtered_run("associate", (cfg,), series, sim=("associate_run_sim", cmds, T, source, k_stride, log))

    def associate_joint_run_sim(self, cmds=None, T=None, source=None, series=False, log=False, k_stride=16, cfg=None):
        """associate_joint_run with the simulator and the sensor model as its source (arguments and `.sense` as gate_run_sim)."""
        return self._filtered_run("associate_joint", (cfg,), series, sim=("associate_joint_run_sim", cmds, T, source, k_stride, log))

    def manage_run_sim(self, cmds=None, T=None, source=None, series=False, log=False, k_stride=16, cfg=None, map_cfg=None):
        """manage_run with the simulator and the sensor model as its source (arguments and `.sense` as gate_run_sim)."""
        return self._filtered_run("manage", (cfg, map_cfg), series, sim=("manage_run_sim", cmds, T, source, k_stride, log))

    def manage_merge_run_sim(self, cmds=None, T=None, source=None, series=False, log=False, k_stride=16, cfg=None, map_cfg=None, merge_cfg=None):
        """manage_merge_run with the simulator and the sensor model as its source (arguments and `.sense` as gate_run_sim)."""
        return self._filtered_run("manage_merge", (cfg, map_cfg, merge_cfg), series,
                                  sim=("manage_merge_run_sim", cmds, T, source, k_stride, log))


_I32, _F64 = np.int32, np.float64
_ASSOC_SERIES = (("n_match", _I32), ("n_new", _I32), ("n_drop", _I32))
# the ten runs that filter a message before the step: the result class, the symbols of the recorded-log form and of the simulator
# form, the settings in C order, and - after recs - the (T, batch) series in C order (flags closes the manage runs; d2_joint and nodes
# follow it in the joint runs)
_RUNS = dict(
    gate=(GateResult, "slam_gate_run", "slam_gate_run_sim", (GATE,), (("nis_sum", _F64), ("n_upd", _I32), ("n_rej", _I32), ("flags", _I32))),
    associate=(AssocResult, "slam_associate_run", "slam_associate_run_sim", (ASSOC,), _ASSOC_SERIES + (("flags", _I32),)),
    associate_joint=(JointResult, "slam_associate_joint_run", "slam_associate_joint_run_sim", (JOINT,),
                     _ASSOC_SERIES + (("flags", _I32), ("d2_joint", _F64), ("nodes", _I32))),
    manage=(MapResult, "slam_manage_run", "slam_manage_run_sim", (ASSOC, MAP), _ASSOC_SERIES + (("n_removed", _I32), ("flags", _I32))),
    manage_merge=(MergeResult, "slam_manage_merge_run", "slam_manage_merge_run_sim", (ASSOC, MAP, MERGE),
                  _ASSOC_SERIES + (("n_removed", _I32), ("n_merged", _I32), ("flags", _I32))))


class SenseLogResult:
    """The `.sense` of a *_run_sim result with log=True: meas (T, batch, k_stride, 3) and count (T, batch), the messages as emitted, before
    the run's own filtering; origin and fault (T, batch, k_stride), the true map row (-1: clutter or no detection) and 1 where spiked; truth
    (T, batch, 3) after each tick's commit; err_pos (T, batch), the position error the commit added (NaN where not committed); cmds
    (T, batch, 2), what the step was given; recs (T, 16), the sense records (columns: the REC_* constants)."""

    (REC_N_SENSED, REC_N_FROZEN, REC_N_TOO_LONG, REC_N_CLEAN, REC_N_MISSED, REC_N_SPIKED, REC_N_CLUTTER, REC_SUM_OUT, REC_SUM_OVERFLOW,
     REC_SUM_SPIKE, REC_N_COMMITTED, REC_SUM_ERR_POS) = range(12)

    NAMES = ("meas", "count", "origin", "fault", "truth", "err_pos", "cmds", "recs")

    def __init__(self, T, batch, k_stride, names=True):
        """names: True for every array, or the names of the wanted ones (the others stay None and cost nothing)."""
        shapes = dict(meas=((T, batch, k_stride, 3), np.float32), count=((T, batch), np.int32), origin=((T, batch, k_stride), np.int32),
                      fault=((T, batch, k_stride), np.int32), truth=((T, batch, 3), np.float64), err_pos=((T, batch), np.float64),
                      cmds=((T, batch, 2), np.float32), recs=((T, 16), np.float64))
        want = self.NAMES if names is True else tuple(names)
        for n in want:
            if n not in shapes:
                raise ValueError(f"unknown log array {n!r}: expected some of {self.NAMES}")
        for n, (shape, dt) in shapes.items():
            setattr(self, n, np.zeros(shape, dtype=dt) if n in want else None)

    def struct(self):
        return SenseLog(*[opt(getattr(self, n)) for n in self.NAMES])


def innovation_summary(recs, alpha=0.05):
    """The curves of an innovation run from its (T, 16) records (one record: shape (16,)), per tick: dict of arrays mean_nis (sum nis /
    updates), nis_lower / nis_upper (the band for that MEAN: the chi-square quantiles of 2 n_upd degrees of freedom at alpha / 2 and
    1 - alpha / 2 divided by n_upd; NaN where 2 n_upd < 30), frac_outside, mean_nu_r, mean_nu_b, n_upd, n_eval.  Pure numpy (no GPU)."""
    r = np.atleast_2d(np.asarray(recs, dtype=np.float64))
    if r.ndim != 2 or r.shape[1] != 16:
        raise ValueError(f"expected records of shape (T, 16), got {np.shape(recs)}")
    R = InnovationResult
    with np.errstate(divide="ignore", invalid="ignore"):
        n = r[:, R.REC_N_UPD]
        out = dict(mean_nis=r[:, R.REC_SUM_NIS] / n, frac_outside=(r[:, R.REC_N_BELOW] + r[:, R.REC_N_ABOVE]) / n,
                   mean_nu_r=r[:, R.REC_SUM_NU_R] / n, mean_nu_b=r[:, R.REC_SUM_NU_B] / n, n_upd=n.astype(np.int64),
                   n_eval=r[:, R.REC_N_EVAL].astype(np.int64))
    lo, hi = np.full(r.shape[0], np.nan), np.full(r.shape[0], np.nan)
    for t, k in enumerate(out["n_upd"]):
        if 2 * k >= 30:
            lo[t], hi[t] = chi2_quantile(alpha / 2, 2 * int(k)) / k, chi2_quantile(1 - alpha / 2, 2 * int(k)) / k
    out["nis_lower"], out["nis_upper"] = lo, hi
    return out


def _normal_quantile(p):
    """Inverse of the standard normal distribution function (Acklam's rational approximation, relative error < 1.2e-9)."""
    import math
    a = (-3.969683028665376e+01, 2.209460984245205e+02, -2.759285104469687e+02, 1.383577518672690e+02, -3.066479806614716e+01,
         2.506628277459239e+00)
    b = (-5.447609879822406e+01, 1.615858368580409e+02, -1.556989798598866e+02, 6.680131188771972e+01, -1.328068155288572e+01)
    c = (-7.784894002430293e-03, -3.223964580411365e-01, -2.400758277161838e+00, -2.549732539343734e+00, 4.374664141464968e+00,
         2.938163982698783e+00)
    d = (7.784695709041462e-03, 3.224671290700398e-01, 2.445134137142996e+00, 3.754408661907416e+00)
    if not 0.0 < p < 1.0:
        raise ValueError("p must lie in (0, 1)")
    if p < 0.02425:
        q = math.sqrt(-2 * math.log(p))
        return (((((c[0] * q + c[1]) * q + c[2]) * q + c[3]) * q + c[4]) * q + c[5]) / ((((d[0] * q + d[1]) * q + d[2]) * q + d[3]) * q + 1)
    if p > 1 - 0.02425:
        return -_normal_quantile(1 - p)
    q = p - 0.5
    r = q * q
    return ((((((a[0] * r + a[1]) * r + a[2]) * r + a[3]) * r + a[4]) * r + a[5]) * q /
            (((((b[0] * r + b[1]) * r + b[2]) * r + b[3]) * r + b[4]) * r + 1))


def chi2_quantile(p, dof):
    """Quantile of the chi-square distribution by the Wilson-Hilferty cube approximation: within 0.31 % of the exact value for
    dof >= 30 and p in [0.005, 0.995] (0.036 % for dof >= 100; 6.5 % at dof 7, hence the refusal below 30).  scipy is not a
    dependency of this package."""
    if dof < 30:
        raise ValueError(f"the Wilson-Hilferty approximation is refused below 30 degrees of freedom (got {dof})")
    v = 2.0 / (9.0 * dof)
    return dof * (1.0 - v + _normal_quantile(p) * v ** 0.5) ** 3


def consistency_summary(nees, dof, flags, alpha=0.05):
    """Bar-Shalom's consistency test over the instances without a flag: {count, left_out, normalised = sum nees / sum dof, lower,
    upper}, the interval being the chi-square quantiles of sum dof at alpha / 2 and 1 - alpha / 2 divided by sum dof.  A consistent
    filter has `normalised` inside [lower, upper] with probability 1 - alpha; far below means an over-cautious covariance, above an
    over-confident one.  Pure numpy (no GPU); raises ValueError when sum dof < 30."""
    nees, dof, flags = np.asarray(nees, dtype=np.float64), np.asarray(dof, dtype=np.int64), np.asarray(flags)
    if not (nees.shape == dof.shape == flags.shape) or nees.ndim != 1:
        raise ValueError("nees, dof and flags must be one-dimensional arrays of one length")
    ok = flags == 0
    total = int(dof[ok].sum())
    lo, hi = chi2_quantile(alpha / 2, total), chi2_quantile(1 - alpha / 2, total)
    return dict(count=int(ok.sum()), left_out=int((~ok).sum()), normalised=float(nees[ok].sum() / total), lower=lo / total,
                upper=hi / total)


def monitor_summary(recs, alpha=0.05):
    """The curves of a monitored run from its (T, 16) records (one record: shape (16,)), per tick: dict of arrays
    mean_err_pos, std_err_pos (population standard deviation across the batch), rms_err_yaw, anees (mean nees_pose over the n_nees
    instances), anees_lower / anees_upper (Bar-Shalom's band for that MEAN: the chi-square quantiles of 3 n_nees degrees of freedom at
    alpha / 2 and 1 - alpha / 2, divided by n_nees; NaN where 3 n_nees < 30, which chi2_quantile refuses), frac_outside (the fraction of
    the n_nees instances below nees_lo or above nees_hi of the run's config), n_ok, n_nees.  Ticks without a counted instance give NaN.
    Pure numpy (no GPU)."""
    r = np.atleast_2d(np.asarray(recs, dtype=np.float64))
    if r.ndim != 2 or r.shape[1] != 16:
        raise ValueError(f"expected records of shape (T, 16), got {np.shape(recs)}")
    R = MonitorResult
    with np.errstate(divide="ignore", invalid="ignore"):
        n_ok, n_nees = r[:, R.REC_N_OK], r[:, R.REC_N_NEES]
        mean = r[:, R.REC_SUM_ERR_POS] / n_ok
        var = r[:, R.REC_SUM_ERR_POS2] / n_ok - mean * mean
        out = dict(mean_err_pos=mean, std_err_pos=np.sqrt(np.maximum(var, 0.0)), rms_err_yaw=np.sqrt(r[:, R.REC_SUM_ERR_YAW2] / n_ok),
                   anees=r[:, R.REC_SUM_NEES_POSE] / n_nees, frac_outside=(r[:, R.REC_N_BELOW] + r[:, R.REC_N_ABOVE]) / n_nees,
                   n_ok=n_ok.astype(np.int64), n_nees=n_nees.astype(np.int64))
    lo, hi = np.full(r.shape[0], np.nan), np.full(r.shape[0], np.nan)
    for t, n in enumerate(out["n_nees"]):
        if 3 * n >= 30:
            lo[t], hi[t] = chi2_quantile(alpha / 2, 3 * int(n)) / n, chi2_quantile(1 - alpha / 2, 3 * int(n)) / n
    out["anees_lower"], out["anees_upper"] = lo, hi
    return out


class BatchedUKF(BatchedFilter):
    """UKF-SLAM (reference: class UKF, filter.h:177-223, ukf.cpp).  State x = [x, y, cos(yaw), sin(yaw), landmarks]."""

    kind = UKF_SLAM

    def _n(self, M):
        return 4 + 2 * M

    # -- UKF::getStateVector (ukf.cpp:47-53; the reference's fixed-size Vector3d bug is not replicated) --
    def getStateVector(self, instance=0):
        x = self.get_state(instance)["x"]
        return np.concatenate([[x[0], x[1], np.remainder(np.arctan2(x[3], x[2]) + np.pi, 2 * np.pi) - np.pi], x[4:]])

    # -- UKF::predictionStage / UKF::updateStage (filter.h:187-188, ukf.cpp:197-291) --
    def predictionStage(self, cmdMsg):
        """cmdMsg: a Command / (fwd, ang) for the batch, or (batch, 2) per instance."""
        self._need()
        cmd = self._cmd(cmdMsg)
        _lib.check((_lib.lib().slam_predict_each if cmd.ndim == 2 else _lib.lib().slam_predict)(self.h, _f(cmd)))

    def updateStage(self, d_meas_ptr=None, d_count_ptr=None, k_stride=0):
        """Measurements as DEVICE pointers ([B][k_stride][3] float32, [B] int32); none = empty message."""
        self._need()
        _lib.check(_lib.lib().slam_update_dev(self.h, C.c_void_p(d_meas_ptr), C.c_void_p(d_count_ptr), int(k_stride)))
        self.timestep += 1

    SQRT_MODES = {"eigen": 0, "cholesky": 1}   # SLAM_UKF_SQRT_EIGEN / SLAM_UKF_SQRT_CHOLESKY (include/slam_batch.h)

    def set_sqrt_mode(self, mode):
        """Matrix square root of every following step: "eigen" (default; nearestSPD + sqrt of ukf.cpp:106-123,208, bit-identical to
        the reference) or "cholesky" (opt-in, NOT bit-identical: Y = L L^T, the columns of L as sigma-point offsets,
        eigen fallback for a pivot <= 1e-8).  It pays off only where P stays positive definite, which the reference's signed process
        noise rarely leaves: on the reference configuration it is slower than "eigen" (DESIGN.md 4.2a).  L_max <= 50 only; readParams()
        creates a new handle, which starts in "eigen"."""
        self._need()
        if mode not in self.SQRT_MODES:
            raise ValueError(f"unknown square-root mode {mode!r}: one of {sorted(self.SQRT_MODES)}")
        _lib.check(_lib.lib().slam_ukf_set_sqrt_mode(self.h, self.SQRT_MODES[mode]))

    def sqrt_stats(self, reset=False):
        """(Cholesky factorisations that succeeded, instance-steps that fell back to the eigen path) since creation / the last reset."""
        self._need(); out = np.zeros(2, dtype=np.uint64)
        _lib.check(_lib.lib().slam_ukf_sqrt_stats(self.h, out.ctypes.data_as(C.POINTER(C.c_uint64)), int(bool(reset))))
        return out

    def sigma_points(self, instance=0):
        """X of the last prediction stage, shape (n, 2n+1) (ukf.cpp:214-219)."""
        self._need()
        r = C.c_int32(0); c = C.c_int32(0)
        X = np.zeros(self.n_max * (2 * self.n_max + 1))
        _lib.check(_lib.lib().slam_get_sigma_points(self.h, int(instance), _d(X), C.byref(r), C.byref(c)))
        return X[:r.value * c.value].reshape(c.value, r.value).T.copy()

    # -- UKF::publishState payload (ukf.cpp:60-104, UKFState.msg); X column by column as the reference pushes it --
    def publishState(self, instance=0):
        import math
        s = self.get_state(instance)
        x, M = s["x"], s["M"]
        lm = np.empty(3 * M, dtype=np.float32)
        lm[0::3] = s["ids"]; lm[1::3] = x[4::2]; lm[2::3] = x[5::2]
        yaw = math.remainder(math.atan2(x[3], x[2]), 2 * 3.14159265358979323846)
        return dict(timestep=s["timestep"], x_v=np.float32(x[0]), y_v=np.float32(x[1]), yaw_v=np.float32(yaw),
                    M=M, landmarks=lm, P=s["P"].astype(np.float32).ravel(),
                    X=self.sigma_points(instance).T.astype(np.float32).ravel())


class BatchedUKFLoc(BatchedUKF):
    """UKF localisation against the known map (FilterChoice::UKF_LOC, localization_node.cpp:39-41, ukf.cpp:146-154):
    the state is the vehicle only; every detection updates against `set_map`'s landmark of the same id."""

    kind = UKF_LOC

    def __init__(self, batch, device=0):
        super().__init__(batch, 1, device)
