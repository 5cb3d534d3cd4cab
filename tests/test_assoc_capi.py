"""Association of detections without ids (slam_associate_*, include/slam_batch.h) without a GPU: the entry points exist, are declared and
mirrored, the build lists the new files, the default gates are the 0.99 and 1 - 1e-6 quantiles of chi-square with 2 degrees of freedom,
and every SLAM_ERR_ARG path returns its code with a text before the handle is looked at."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import AssocConfig, Noise, default_assoc_config

ERR_ARG = -1
SYMBOLS = ("slam_assoc_config_default", "slam_associate", "slam_associate_dev", "slam_step_associated", "slam_step_associated_dev",
           "slam_associate_run", "slam_last_associate_work", "slam_associate_instance_host")
NOW = ("slam_associate", "slam_associate_dev")
STEPS = ("slam_step_associated", "slam_step_associated_dev")
ALL = NOW + STEPS + ("slam_associate_run",)


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    assert header.index("int slam_gate_instance_host(") < header.index("---- association of detections WITHOUT ids") < header.index("---- closed loop")
    doc = header.split("---- association of detections WITHOUT ids")[1].split("enum slam_assoc_verdict")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    for word in ("joint compatibility (JCBB)", "reassigning conflict losers", "ln det S", "simulator sources", "slam_multi_", "pose graph",
                 "slam_associate_dev and slam_step_gated_dev"):
        assert word in tail, word
    errors = " ".join(w for w in doc.split("Errors:")[1].split("Not covered:")[0].split() if w != "*")
    for word in ("before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "landmark_id_is_known = 0", "SLAM_ERR_STATE", "slam_track_instance"):
        assert word in errors, word
    assert "NOT READ" in doc and "ekf_landmark_from_x_pred cannot matter" in doc
    for i, name in enumerate(("NONE", "MATCHED", "NEW", "AMBIGUOUS", "CONFLICT", "NO_ROOM", "INVALID")):
        assert re.search(r"SLAM_ASSOC_%s = %d\b" % (name, i), header), name
    mirror = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    for name in ("stepAssociated", "slam_step_associated", "AssociatedStep"):
        assert name in mirror, name
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "assoc_kernel.hip" in build.SOURCES and "capi_assoc.cpp" in build.SOURCES and "assoc_kernel.h" in build.HEADERS
    for name in ("associate", "associate_dev", "step_associated", "step_associated_dev", "associate_run", "last_associate_work"):
        assert callable(getattr(filters.BatchedEKF, name))
    assert callable(S.associate_instance_host) and S.AssocConfig is AssocConfig and S.AssocResult.REC_MAX_D2 == 8
    assert (S.ASSOC_NONE, S.ASSOC_MATCHED, S.ASSOC_NEW, S.ASSOC_AMBIGUOUS, S.ASSOC_CONFLICT, S.ASSOC_NO_ROOM, S.ASSOC_INVALID) == tuple(range(7))


def test_default_config():
    L = _lib.lib()
    c = AssocConfig()
    assert L.slam_assoc_config_default(C.byref(c)) == 0
    assert c.gate_match == -2.0 * math.log(0.01) and abs(c.gate_match - 9.210340371976182) < 1e-14
    assert c.gate_new == -2.0 * math.log(1e-6) and abs(c.gate_new - 27.631021115928547) < 1e-13
    assert abs((1 - math.exp(-c.gate_match / 2)) - 0.99) < 1e-15     # chi-square with 2 degrees of freedom: F(x) = 1 - exp(-x / 2)
    assert abs(math.exp(-c.gate_new / 2) - 1e-6) < 1e-20
    assert bytes(default_assoc_config()) == bytes(c)
    assert L.slam_assoc_config_default(None) == ERR_ARG and "NULL" in _err()


def _call(fn, cfg=None, cmds=True, meas=True, count=True, k_stride=2, out="other", h=None, T=1):
    """One entry point on a NULL handle (or h) with tiny host arrays standing in for every pointer."""
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32)
    mo = np.zeros((1, 2, 3), np.float32); no = np.zeros(1, np.int32)
    dev = fn.endswith("_dev")
    ptr = (lambda a, t: C.c_void_p(a.ctypes.data) if dev else a.ctypes.data_as(t))
    cp = ptr(c, _lib._fp) if cmds else None
    mp = ptr(m, _lib._fp) if meas else None
    np_ = ptr(n, _lib._ip) if count else None
    cfgp = None if cfg is None else C.byref(cfg)
    if fn in NOW:
        outs = {"other": (mo, no), "in place": (m, n), "meas alone": (m, no), "count alone": (mo, n), "none": (None, None)}[out]
        mop = None if outs[0] is None else ptr(outs[0], _lib._fp)
        nop = None if outs[1] is None else ptr(outs[1], _lib._ip)
        return getattr(L, fn)(h, cfgp, cp, 0, mp, np_, k_stride, None, None, None, None, None, None, None, None, mop, nop)
    if fn == "slam_associate_run":
        return L.slam_associate_run(h, cfgp, cp, 0, mp, np_, k_stride, T, None, None, None, None, None)
    return getattr(L, fn)(h, cfgp, cp, 0, mp, np_, k_stride, None, None)


def _host(cfg=None, **over):
    n = 5
    a = dict(x=np.zeros(n), P=np.eye(n).ravel().copy(), ids=np.array([3], np.int32), M=1, L_max=4, status=0, cmd=np.zeros(2, np.float32),
             meas=np.array([[3.0, 1.0, 0.1]], np.float32), count=1, k_stride=1, noise=Noise(0, 0, 0, 0, 0.01, 0.001, 0.01, 0.01, 0, 0, 0, 0))
    a.update(over)
    d = (lambda v: None if v is None else v.ctypes.data_as(_lib._dp))
    return _lib.lib().slam_associate_instance_host(
        d(a["x"]), d(a["P"]), None if a["ids"] is None else a["ids"].ctypes.data_as(_lib._ip), a["M"], a["L_max"], a["status"],
        None if a["cmd"] is None else a["cmd"].ctypes.data_as(_lib._fp), None if a["meas"] is None else a["meas"].ctypes.data_as(_lib._fp),
        a["count"], a["k_stride"], None if a["noise"] is None else C.byref(a["noise"]), 0, 0, None if cfg is None else C.byref(cfg),
        None, None, None, None, None, None, None, None, None, None, None)


@pytest.mark.parametrize("gate_match,gate_new", [(float("nan"), 30.0), (9.0, float("nan")), (0.0, 30.0), (-1.0, 30.0), (-float("inf"), 30.0),
                                                 (30.0, 9.0), (float("inf"), 30.0)])
def test_config_checks_come_before_the_handle(gate_match, gate_new):
    cfg = AssocConfig(gate_match, gate_new)
    for fn in ALL:
        assert _call(fn, cfg=cfg) == ERR_ARG and "assoc config" in _err() and "gate_match" in _err(), fn
    assert _host(cfg=cfg) == ERR_ARG and "assoc config" in _err()


def test_an_infinite_new_gate_and_equal_gates_are_allowed():
    for cfg in (AssocConfig(9.0, float("inf")), AssocConfig(9.0, 9.0), AssocConfig(float("inf"), float("inf"))):
        for fn in ALL:
            assert _call(fn, cfg=cfg) == ERR_ARG and "NULL handle" in _err(), fn
        assert _host(cfg=cfg) == 0


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    for fn in ALL:
        assert _call(fn, cmds=False) == ERR_ARG and "cmds" in _err(), fn
        assert _call(fn, meas=False) == ERR_ARG and "meas" in _err(), fn
        assert _call(fn, count=False) == ERR_ARG and "meas" in _err(), fn
        assert _call(fn, k_stride=0) == ERR_ARG and "k_stride" in _err(), fn
        assert _call(fn, k_stride=-3) == ERR_ARG and "k_stride" in _err(), fn
        assert _call(fn) == ERR_ARG and "NULL handle" in _err(), fn
        assert _call(fn, cfg=default_assoc_config()) == ERR_ARG and "NULL handle" in _err(), fn
    for fn in NOW:     # a partial overlap of input and output: in place means both buffers
        assert _call(fn, out="meas alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="count alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="in place") == ERR_ARG and "NULL handle" in _err(), fn
    assert _call("slam_associate", out="none") == ERR_ARG and "NULL handle" in _err()          # host form: the message is optional
    assert _call("slam_associate_dev", out="none") == ERR_ARG and "d_meas_out" in _err()       # device form: it is where the result goes
    assert _call("slam_associate_run", T=-1) == ERR_ARG and "negative" in _err()
    assert L.slam_last_associate_work(None, None, None, None) == ERR_ARG and "NULL handle" in _err()


def test_argument_checks_of_the_host_hook():
    assert _host() == 0                                    # every output may be NULL
    for key in ("x", "P", "cmd", "noise", "ids", "meas"):
        assert _host(**{key: None}) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", -1), ("k_stride", 0)):
        assert _host(**{key: value}) == ERR_ARG, (key, value)
    assert _host(M=0, ids=None, x=np.zeros(3), P=np.eye(3).ravel().copy(), count=0, meas=None) == 0
    assert _host(count=-2) == 0                            # a negative count is an empty message, as the step reads it


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    m = np.zeros((3, 2, 3), np.float32); n = np.zeros(3, np.int32)
    calls = (lambda: f.associate((0.1, 0.0), m, n), lambda: f.step_associated((0.1, 0.0), m, n), f.last_associate_work,
             lambda: f.associate_run(np.zeros((2, 2)), np.zeros((2, 3, 2, 3)), np.zeros((2, 3))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
