"""ctypes mirror of `slam_config` (include/slam_batch.h) + defaults from the reference's params.yaml.

Key names follow ekf_ws/src/base_pkg/config/params.yaml:25-52 (reference), the only config surface the hot
path reads (Filter::readCommonParams, filter.h:105-121; get_cmd, sim_node.py:209-250).
"""
import ctypes as C


def set_fields(c, fields, noun):
    """Sets fields of the ctypes struct c from a dict; a name c does not have is refused as an unknown `noun` setting.  An array field
    (JointConfig.gate_joint) takes a sequence of numbers."""
    types = dict(c._fields_)
    for k, v in dict(fields).items():
        if k not in types:
            raise ValueError(f"unknown {noun} setting {k!r}")
        setattr(c, k, types[k](*[float(g) for g in v]) if issubclass(types[k], C.Array) else v)
    return c


class SlamConfig(C.Structure):
    _fields_ = [
        ("v_d", C.c_float), ("v_th", C.c_float),
        ("V_00", C.c_double), ("V_11", C.c_double),
        ("w_r", C.c_float), ("w_b", C.c_float),
        ("W_00", C.c_double), ("W_11", C.c_double),
        ("landmark_id_is_known", C.c_int), ("min_landmark_separation", C.c_float),
        ("d_max", C.c_double), ("th_max", C.c_double),
        ("range_max", C.c_double), ("fov_min", C.c_double), ("fov_max", C.c_double),
        ("init_x", C.c_double), ("init_y", C.c_double), ("init_yaw", C.c_double),
        ("replicate_vw_quirk", C.c_int), ("ukf_float_trig", C.c_int),
        ("reserved", C.c_int * 2),
        # quirk switches of round 5 (include/slam_batch.h): 0 = the reference's behaviour as this build reads it
        ("ekf_abs_is_int", C.c_int), ("ekf_landmark_from_x_pred", C.c_int),
        ("ukf_accumulate_zest1", C.c_int), ("ukf_sensing_yaw_from_sigma", C.c_int),
    ]

    def copy(self):
        c = SlamConfig()
        C.memmove(C.byref(c), C.byref(self), C.sizeof(SlamConfig))
        return c


def default_config() -> SlamConfig:
    """Values committed in the reference's params.yaml (lines 19-52)."""
    c = SlamConfig()
    c.v_d, c.v_th, c.V_00, c.V_11 = 0.0, 0.0, 0.01, 0.001
    c.w_r, c.w_b, c.W_00, c.W_11 = 0.0, 0.0, 0.01, 0.01
    c.landmark_id_is_known, c.min_landmark_separation = 1, 0.1
    c.d_max, c.th_max = 0.1, 0.0546
    c.range_max, c.fov_min, c.fov_max = 3.0, -1.57, 1.57
    c.init_x, c.init_y, c.init_yaw = 0.0, 0.0, 0.0
    c.replicate_vw_quirk, c.ukf_float_trig = 1, 1
    return c


class Noise(C.Structure):
    """ctypes mirror of `slam_noise` (include/slam_batch.h): one instance's row of slam_set_noise_each.  Filter fields as the filter
    reads the YAML keys (the handle's replicate_vw_quirk maps them to the effective V / W), simulator fields = half-widths of the draws."""
    _fields_ = [("v_d", C.c_float), ("v_th", C.c_float), ("w_r", C.c_float), ("w_b", C.c_float),
                ("V_00", C.c_double), ("V_11", C.c_double), ("W_00", C.c_double), ("W_11", C.c_double),
                ("sim_V_00", C.c_double), ("sim_V_11", C.c_double), ("sim_W_00", C.c_double), ("sim_W_11", C.c_double)]


NOISE_FIELDS = tuple(name for name, _ in Noise._fields_)


def noise_from_config(cfg) -> Noise:
    """The row that reproduces a handle without rows (slam_noise_from_config): filter and simulator fields both from cfg."""
    return Noise(cfg.v_d, cfg.v_th, cfg.w_r, cfg.w_b, cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11, cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11)


def noise_rows(cfg, batch, **columns):
    """`batch` rows for BatchedFilter.set_noise: every row noise_from_config(cfg), with per-instance values overriding fields -
    noise_rows(cfg, 8, V_00=np.logspace(-6, -2, 8), sim_W_00=0.02); a column is a scalar or a [batch] array."""
    rows = (Noise * int(batch))()
    base = noise_from_config(cfg)
    for name in columns:
        if name not in NOISE_FIELDS:
            raise ValueError(f"unknown noise field {name!r}: expected one of {NOISE_FIELDS}")
    cols = {}
    for name, v in columns.items():
        a = [float(x) for x in (v if hasattr(v, "__len__") else [v] * int(batch))]
        if len(a) != int(batch):
            raise ValueError(f"{name}: expected a scalar or {int(batch)} values, got {len(a)}")
        cols[name] = a
    for b in range(int(batch)):
        for name in NOISE_FIELDS:
            setattr(rows[b], name, cols[name][b] if name in cols else getattr(base, name))
    return rows


class NavConfig(C.Structure):
    """ctypes mirror of `slam_nav_config` (include/slam_batch.h): params.yaml:14,81-84 plus the launch file's tight_control."""
    _fields_ = [("dt", C.c_double), ("lookahead_dist_init", C.c_double), ("lookahead_dist_max", C.c_double),
                ("method", C.c_int), ("control", C.c_int)]


NAV_PP, NAV_DIRECT = 0, 1
NAV_LOOSE, NAV_TIGHT = 0, 1


def default_nav_config() -> NavConfig:
    """dt 0.05, lookahead 0.2 .. 2 m, "pp" (params.yaml:14,81-84), loose control (sim_base.launch)."""
    return NavConfig(0.05, 0.2, 2.0, NAV_PP, NAV_LOOSE)


class MonitorConfig(C.Structure):
    """ctypes mirror of `slam_monitor_config` (include/slam_batch.h): the NEES band of the record and the stride of the full evaluation."""
    _fields_ = [("nees_lo", C.c_double), ("nees_hi", C.c_double), ("full_every", C.c_int)]


MONITOR_SHARED, MONITOR_EACH, MONITOR_NAV = 0, 1, 2


class InnovationConfig(C.Structure):
    """ctypes mirror of `slam_innovation_config` (include/slam_batch.h): the NIS band of the record."""
    _fields_ = [("nis_lo", C.c_double), ("nis_hi", C.c_double)]


INNOVATION_SHARED, INNOVATION_EACH, INNOVATION_NAV, INNOVATION_LOG = 0, 1, 2, 3
INNOV_MAX_DET, INNOV_MAX_LM = 64, 16   # SLAM_INNOV_MAX_DET, SLAM_INNOV_MAX_LM


def default_innovation_config() -> InnovationConfig:
    """The chi-square quantiles at 0.025 and 0.975 for 2 degrees of freedom: -2 ln 0.975 and -2 ln 0.025."""
    import math
    return InnovationConfig(-2.0 * math.log(0.975), -2.0 * math.log(0.025))


class GateConfig(C.Structure):
    """ctypes mirror of `slam_gate_config` (include/slam_batch.h): the chi-square gate on a detection's NIS and the band of the record."""
    _fields_ = [("gate", C.c_double), ("nis_lo", C.c_double), ("nis_hi", C.c_double)]


GATE_NOT_UPDATE, GATE_ACCEPTED, GATE_REJECTED = 0, 1, 2   # slam_gate_verdict


def default_gate_config() -> GateConfig:
    """gate = -2 ln 0.001, the 0.999 quantile of chi-square with 2 degrees of freedom; the band of default_innovation_config."""
    import math
    return GateConfig(-2.0 * math.log(0.001), -2.0 * math.log(0.975), -2.0 * math.log(0.025))


class AssocConfig(C.Structure):
    """ctypes mirror of `slam_assoc_config` (include/slam_batch.h): the match gate and the new-landmark gate on a detection's best cost."""
    _fields_ = [("gate_match", C.c_double), ("gate_new", C.c_double)]


ASSOC_NONE, ASSOC_MATCHED, ASSOC_NEW, ASSOC_AMBIGUOUS, ASSOC_CONFLICT, ASSOC_NO_ROOM, ASSOC_INVALID = range(7)   # slam_assoc_verdict


def default_assoc_config() -> AssocConfig:
    """gate_match = -2 ln 0.01 and gate_new = -2 ln 1e-6: the 0.99 and 1 - 1e-6 quantiles of chi-square with 2 degrees of freedom."""
    import math
    return AssocConfig(-2.0 * math.log(0.01), -2.0 * math.log(1e-6))


class JointConfig(C.Structure):
    """ctypes mirror of `slam_joint_config` (include/slam_batch.h): the individual gates of AssocConfig, the joint gates by pairing count
    and the node budget of the search."""
    _fields_ = [("gate_match", C.c_double), ("gate_new", C.c_double), ("gate_joint", C.c_double * 16), ("max_nodes", C.c_int32)]


ASSOC_JOINT_UNPAIRED = 7                                    # slam_assoc_verdict, slam_associate_joint only
JOINT_BUDGET, JOINT_S_SINGULAR, JOINT_LM_TABLE = 16, 32, 64   # slam_joint_flags
JOINT_MAX_CAND, JOINT_MAX_PAIR = 4, 16                      # SLAM_JOINT_MAX_CAND, SLAM_JOINT_MAX_PAIR
# the 0.99 quantiles of chi-square with 2, 4, ..., 32 degrees of freedom (mpmath, 50 digits, rounded to nearest)
JOINT_GATES_99 = (9.210340371976184, 13.276704135987625, 16.81189382977093, 20.090235029663233, 23.20925115895436, 26.21696730553585,
                  29.141237740672796, 31.99992690881518, 34.80530573470507, 37.56623478662505, 40.289360437593864, 42.97982013935164,
                  45.64168266628315, 48.2782357703155, 50.89218131151709, 53.485771836235365)


def default_joint_config() -> JointConfig:
    """The gates of default_assoc_config, gate_joint[m - 1] = the 0.99 quantile of chi-square with 2 m degrees of freedom (entry 0 is
    gate_match), max_nodes = 2048."""
    a = default_assoc_config()
    c = JointConfig(a.gate_match, a.gate_new, (C.c_double * 16)(*JOINT_GATES_99), 2048)
    c.gate_joint[0] = a.gate_match
    return c


class MapConfig(C.Structure):
    """ctypes mirror of `slam_map_config` (include/slam_batch.h): the shrunk view a landmark is expected in, the prune rule on its track
    counters and the stride of the prunes of manage_run."""
    _fields_ = [("range_shrink", C.c_double), ("fov_margin", C.c_double), ("min_expected", C.c_int32), ("min_ratio", C.c_double),
                ("prune_every", C.c_int32)]


MAP_CONFIG_FIELDS = tuple(name for name, _ in MapConfig._fields_)


def default_map_config() -> MapConfig:
    """range_shrink 0.9, fov_margin 0.1 rad, judged after 10 expectations, removed below a seen / expected ratio of 0.3, every 10 ticks."""
    return MapConfig(0.9, 0.1, 10, 0.3, 10)


class MergeConfig(C.Structure):
    """ctypes mirror of `slam_merge_config` (include/slam_batch.h): the gate on a pair's d2, the standard deviation of the pseudo-measurement
    l_i - l_j = 0 and the stride of the merges of manage_merge_run."""
    _fields_ = [("gate_merge", C.c_double), ("sigma", C.c_double), ("merge_every", C.c_int32)]


MERGE_CONFIG_FIELDS = tuple(name for name, _ in MergeConfig._fields_)


def default_merge_config() -> MergeConfig:
    """gate_merge = -2 ln 0.05, the 0.95 quantile of chi-square with 2 degrees of freedom; sigma 0: the copies are the same point; every 10 ticks."""
    import math
    return MergeConfig(-2.0 * math.log(0.05), 0.0, 10)


class SensorConfig(C.Structure):
    """ctypes mirror of `slam_sensor` (include/slam_batch.h): one row of the sensor fault model of sense() and the *_run_sim calls -
    dropout, range spikes, clutter, shuffled order, erased ids."""
    _fields_ = [("p_miss", C.c_double), ("p_spike", C.c_double), ("spike_lo", C.c_double), ("spike_hi", C.c_double), ("p_clutter", C.c_double),
                ("clutter_r_min", C.c_double), ("n_clutter", C.c_int32), ("shuffle", C.c_int32), ("erase_ids", C.c_int32)]


SENSOR_FIELDS = tuple(name for name, _ in SensorConfig._fields_)
SENSE_MAX_DET, SENSE_MAX_CLUTTER = 64, 8
SENSE_INSTANCE_FROZEN, SENSE_TOO_LONG = 1, 2


def default_sensor_config(**fields) -> SensorConfig:
    """The all-off row (every field 0): the message of the plain simulator step.  Keyword arguments set fields."""
    return set_fields(SensorConfig(), fields, "sensor")


class SenseLog(C.Structure):
    """ctypes mirror of `slam_sense_log`: the optional host arrays of a *_run_sim call."""
    _fields_ = [("meas", C.POINTER(C.c_float)), ("count", C.POINTER(C.c_int32)), ("origin", C.POINTER(C.c_int32)), ("fault", C.POINTER(C.c_int32)),
                ("truth", C.POINTER(C.c_double)), ("err_pos", C.POINTER(C.c_double)), ("cmds", C.POINTER(C.c_float)),
                ("recs", C.POINTER(C.c_double))]


class FixConfig(C.Structure):
    """ctypes mirror of `slam_fix_config` (include/slam_batch.h): the nis gates of the position and the heading part of a fix and the stride
    of the fixes of fix_run."""
    _fields_ = [("gate_pos", C.c_double), ("gate_yaw", C.c_double), ("fix_every", C.c_int32)]


FIX_CONFIG_FIELDS = tuple(name for name, _ in FixConfig._fields_)
FIX_POS, FIX_YAW = 1, 2
FIX_ABSENT, FIX_APPLIED, FIX_REJECTED, FIX_SINGULAR, FIX_INVALID = 0, 1, 2, 3, 4


def default_fix_config() -> FixConfig:
    """The 0.999 quantiles of chi-square with 2 and with 1 degrees of freedom; a fix every 10 ticks."""
    import math
    return FixConfig(-2.0 * math.log(0.001), 10.827566170662733, 10)


class FixSensorConfig(C.Structure):
    """ctypes mirror of `slam_fix_sensor` (include/slam_batch.h): one row of the simulated source of fixes - uniform noise, the sigmas the
    rows claim, misses and position jumps."""
    _fields_ = [("pos_halfwidth", C.c_double), ("yaw_halfwidth", C.c_double), ("sigma_pos", C.c_double), ("sigma_yaw", C.c_double),
                ("p_miss_pos", C.c_double), ("p_miss_yaw", C.c_double), ("p_jump", C.c_double), ("jump_lo", C.c_double), ("jump_hi", C.c_double),
                ("kinds", C.c_int32)]


FIX_SENSOR_FIELDS = tuple(name for name, _ in FixSensorConfig._fields_)


def default_fix_sensor_config(**fields) -> FixSensorConfig:
    """The all-zero row, which emits nothing.  Keyword arguments set fields."""
    return set_fields(FixSensorConfig(), fields, "fix sensor")


class FixLog(C.Structure):
    """ctypes mirror of `slam_fix_log`: the emitted rows and kinds of a fix_run."""
    _fields_ = [("fix", C.POINTER(C.c_double)), ("kinds", C.POINTER(C.c_int32))]


def default_monitor_config() -> MonitorConfig:
    """The chi-square quantiles at 0.025 and 0.975 for 3 degrees of freedom; no full evaluation."""
    return MonitorConfig(0.21579528262389785, 9.348403604496148, 0)


EKF_SLAM, UKF_LOC, UKF_SLAM = 1, 2, 3
F64, F32 = 0, 1
INST_NONFINITE, INST_S_SINGULAR, INST_INDEX_OOR, INST_CAPACITY, INST_SQRT_FAILED = 1, 2, 4, 8, 16
