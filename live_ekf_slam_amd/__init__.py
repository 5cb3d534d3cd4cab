"""MI355X-native batched EKF/UKF-SLAM predict–update engine (drop-in for the Filter::update path of
kevin-robb/live_ekf_slam).  Numerics live in the HIP extension libslam_hip.so behind include/slam_batch.h."""
from .config import SlamConfig, NavConfig, default_config, default_nav_config, EKF_SLAM, UKF_LOC, UKF_SLAM, F64, F32  # noqa: F401
from .config import NAV_PP, NAV_DIRECT, NAV_LOOSE, NAV_TIGHT  # noqa: F401
from .config import MonitorConfig, default_monitor_config, MONITOR_SHARED, MONITOR_EACH, MONITOR_NAV  # noqa: F401
from .config import InnovationConfig, default_innovation_config, INNOVATION_SHARED, INNOVATION_EACH, INNOVATION_NAV, INNOVATION_LOG  # noqa: F401
from .config import INNOV_MAX_DET, INNOV_MAX_LM  # noqa: F401
from .navigation import PurePursuitBatch  # noqa: F401
from .filters import BatchedEKF, BatchedUKF, BatchedUKFLoc, Command, MonitorResult, monitor_summary  # noqa: F401
from .filters import InnovationResult, innovation_summary, innovation_instance_host  # noqa: F401
from .config import GateConfig, default_gate_config, GATE_NOT_UPDATE, GATE_ACCEPTED, GATE_REJECTED  # noqa: F401
from .filters import GateResult, gate_instance_host  # noqa: F401
from .config import AssocConfig, default_assoc_config  # noqa: F401
from .config import ASSOC_NONE, ASSOC_MATCHED, ASSOC_NEW, ASSOC_AMBIGUOUS, ASSOC_CONFLICT, ASSOC_NO_ROOM, ASSOC_INVALID  # noqa: F401
from .filters import AssocResult, associate_instance_host  # noqa: F401
from .config import JointConfig, default_joint_config, ASSOC_JOINT_UNPAIRED, JOINT_BUDGET, JOINT_S_SINGULAR, JOINT_LM_TABLE  # noqa: F401
from .filters import JointResult, associate_joint_instance_host  # noqa: F401
from .config import MapConfig, default_map_config  # noqa: F401
from .filters import MapResult, map_instance_host  # noqa: F401
from .config import MergeConfig, default_merge_config  # noqa: F401
from .filters import MergeResult, merge_instance_host  # noqa: F401
from .config import SensorConfig, default_sensor_config, SENSE_MAX_DET, SENSE_MAX_CLUTTER, SENSE_INSTANCE_FROZEN, SENSE_TOO_LONG  # noqa: F401
from .filters import SenseLogResult, sense_instance_host  # noqa: F401
from .config import FixConfig, FixSensorConfig, default_fix_config, default_fix_sensor_config, FIX_POS, FIX_YAW  # noqa: F401
from .config import FIX_ABSENT, FIX_APPLIED, FIX_REJECTED, FIX_SINGULAR, FIX_INVALID  # noqa: F401
from .filters import FixResult, fix_instance_host, fix_sense_instance_host  # noqa: F401
from .pose_graph import BatchedPoseGraph, NaiveFilter  # noqa: F401
from ._lib import SlamError  # noqa: F401
