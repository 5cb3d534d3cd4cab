"""The marshalling layer between the Python mirrors (filters.py, pose_graph.py, _hooks.py) and the C ABI that _lib.SIGNATURES states:
numpy arrays to typed pointers, settings to config structs, rows to ctypes arrays, and `Handle`, what BatchedFilter and BatchedPoseGraph
share.  The library is fetched through _lib.lib() when a call is made, never at import, and every check of an argument comes before it.
"""
import ctypes as C

import numpy as np

from . import _lib
from .config import set_fields
from .config import (MonitorConfig, default_monitor_config, NavConfig, default_nav_config, InnovationConfig, default_innovation_config,
                     GateConfig, default_gate_config, AssocConfig, default_assoc_config, JointConfig, default_joint_config,
                     MapConfig, default_map_config, MergeConfig, default_merge_config, FixConfig, default_fix_config)


def _d(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _f(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _i(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


_CAST = {np.dtype(np.float64): _d, np.dtype(np.float32): _f, np.dtype(np.int32): _i}


def ptr(a):
    """The typed pointer of a float64, float32 or int32 array, NULL for None.  An empty array keeps its address: a run of T = 0 ticks
    still passes its commands."""
    return None if a is None else _CAST[a.dtype](a)


def opt(a):
    """The typed pointer of an optional output: NULL for None and for an empty array."""
    return None if a is None or a.size == 0 else ptr(a)


class Command:
    """base_pkg/Command (Command.msg:3-5): float32 fwd, ang."""

    def __init__(self, fwd=0.0, ang=0.0):
        self.fwd = float(np.float32(fwd))
        self.ang = float(np.float32(ang))


# the settings structs: (struct, its defaults, the noun of the refusal)
MONITOR = (MonitorConfig, default_monitor_config, "monitor")
NAV = (NavConfig, default_nav_config, "controller")
INNOVATION = (InnovationConfig, default_innovation_config, "innovation")
GATE = (GateConfig, default_gate_config, "gate")
ASSOC = (AssocConfig, default_assoc_config, "association")
JOINT = (JointConfig, default_joint_config, "joint association")
MAP = (MapConfig, default_map_config, "map")
MERGE = (MergeConfig, default_merge_config, "merge")
FIX = (FixConfig, default_fix_config, "fix")


def config_from(cfg, Type, default, noun):
    """A settings struct from None (the defaults), a struct (the same object) or a dict of its fields (the defaults with them set)."""
    if cfg is None:
        return default()
    if isinstance(cfg, Type):
        return cfg
    return set_fields(default(), cfg, noun)


def struct_rows(rows, Type, batch, what, one=None):
    """The argument of a *_each setter: None, or a ctypes array of `batch` rows of Type from a ctypes array or a sequence of rows.  With
    `one` (the row's default function) a dict of fields or a single row is replicated over the batch."""
    if rows is None:
        return None
    if one is not None:
        if isinstance(rows, dict):
            rows = one(**rows)
        if isinstance(rows, Type):
            rows = [rows] * batch
    if not (isinstance(rows, C.Array) and rows._type_ is Type):
        rows = (Type * len(rows))(*rows)
    if len(rows) != batch:
        raise ValueError(f"expected {batch} {what} rows, got {len(rows)}")
    return rows


class Handle:
    """What the batched filters and the batched pose graph share: the handle, its start poses, commands and per-instance rows."""

    _INIT = _INIT_EACH = _DESTROY = None     # the symbols of init(), set by the subclass

    def _need(self):
        if self.h is None:
            raise _lib.SlamError("readParams() must be called before using the filter")

    def _rows(self, a, what, width):
        if a.shape != (self.batch, width):
            raise ValueError(f"{what}: expected shape ({self.batch}, {width}), got {a.shape}")
        return a

    def _cmd(self, cmdMsg):
        """(2,) float32 for one command, (batch, 2) for one per instance."""
        if isinstance(cmdMsg, Command):
            return np.array([cmdMsg.fwd, cmdMsg.ang], dtype=np.float32)
        c = np.ascontiguousarray(cmdMsg, dtype=np.float32)
        if c.shape == (self.batch, 2):
            return c
        if c.size == 2:
            return c.reshape(2)
        raise ValueError(f"expected a command of shape (2,) or ({self.batch}, 2), got {c.shape}")

    def _cmd_dev(self, cmdMsg, who):
        """The command of an entry point on device messages as (void pointer, each): one host command, or - an int - the device pointer
        of per-instance commands.  `who` opens the refusal of (batch, 2) host commands."""
        if isinstance(cmdMsg, int):
            return C.c_void_p(cmdMsg), 1
        cmd = self._cmd(cmdMsg)
        if cmd.ndim != 1:
            raise ValueError(f"{who} one command, or the device pointer of per-instance commands")
        return C.cast(_f(cmd), C.c_void_p), 0

    def _init(self, x_0, y_0, yaw_0, truth0):
        self._need()
        if np.ndim(x_0) == 0 and truth0 is None:
            _lib.check(getattr(_lib.lib(), self._INIT)(self.h, x_0, y_0, yaw_0))
        else:
            pose = (np.asarray(x_0, dtype=np.float32) if np.ndim(x_0) else
                    np.broadcast_to(np.array([x_0, y_0, yaw_0], dtype=np.float32), (self.batch, 3)))
            pose = np.ascontiguousarray(self._rows(pose, "x_0", 3), dtype=np.float32)
            tr = None if truth0 is None else np.ascontiguousarray(self._rows(np.asarray(truth0, dtype=np.float64), "truth0", 3))
            _lib.check(getattr(_lib.lib(), self._INIT_EACH)(self.h, _f(pose), ptr(tr)))
        self.isInit, self.timestep = True, 0

    def _set_rows(self, symbol, rows, Type, what, one=None):
        self._need()
        rows = struct_rows(rows, Type, self.batch, what, one)
        _lib.check(getattr(_lib.lib(), symbol)(self.h, rows))

    def _last_work(self, symbol, n, pair=False):
        """What a *_last_*_work call reports: n doubles, after the two of a double[2] where the call has one."""
        self._need()
        by, vals = (C.c_double * 2)() if pair else (), [C.c_double(0) for _ in range(n)]
        _lib.check(getattr(_lib.lib(), symbol)(self.h, *([by] if pair else []), *[C.byref(v) for v in vals]))
        return (*by, *[v.value for v in vals])

    def close(self):
        if self.h is not None:
            getattr(_lib.lib(), self._DESTROY)(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
