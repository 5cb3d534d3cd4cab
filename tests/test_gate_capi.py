"""The chi-square gate (slam_gate_*, include/slam_batch.h) without a GPU: the entry points exist and are mirrored, the default gate is the
0.999 quantile of chi-square with 2 degrees of freedom, and every SLAM_ERR_ARG path returns its code with a text before the handle is
looked at."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import GateConfig, default_gate_config, default_innovation_config

ERR_ARG = -1
SYMBOLS = ("slam_gate_config_default", "slam_gate", "slam_gate_dev", "slam_step_gated", "slam_step_gated_dev", "slam_step_gated_each",
           "slam_step_gated_each_dev", "slam_gate_run", "slam_last_gate_work", "slam_gate_instance_host")
NOW = ("slam_gate", "slam_gate_dev")
STEPS = ("slam_step_gated", "slam_step_gated_dev", "slam_step_gated_each", "slam_step_gated_each_dev")


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    doc = header.split("---- innovation gating")[1].split("enum slam_gate_verdict")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    for word in ("simulator sources", "slam_multi_", "pose graph", "multi-step launches", "joint compatibility"):
        assert word in tail, word
    assert "NEVER rejected" in doc
    assert re.search(r"SLAM_GATE_NOT_UPDATE = 0,", header) and re.search(r"SLAM_GATE_ACCEPTED = 1,", header) and re.search(r"SLAM_GATE_REJECTED = 2\b", header)
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "gate_kernel.hip" in build.SOURCES and "gate_kernel.h" in build.HEADERS
    for name in ("gate", "gate_dev", "step_gated", "step_gated_dev", "gate_run", "last_gate_work"):
        assert callable(getattr(filters.BatchedEKF, name))
    assert callable(S.gate_instance_host) and S.GateResult.REC_N_REJ == 15 and S.GateConfig is GateConfig
    assert (S.GATE_NOT_UPDATE, S.GATE_ACCEPTED, S.GATE_REJECTED) == (0, 1, 2)


def test_default_config():
    L = _lib.lib()
    c = GateConfig()
    assert L.slam_gate_config_default(C.byref(c)) == 0
    assert c.gate == -2.0 * math.log(0.001) and abs(c.gate - 13.815510557964274) < 1e-14
    assert abs((1 - math.exp(-c.gate / 2)) - 0.999) < 1e-15       # chi-square with 2 degrees of freedom: F(x) = 1 - exp(-x / 2)
    band = default_innovation_config()
    assert (c.nis_lo, c.nis_hi) == (band.nis_lo, band.nis_hi)
    assert bytes(default_gate_config()) == bytes(c)
    assert L.slam_gate_config_default(None) == ERR_ARG and "NULL" in _err()


def _call(fn, cfg=None, cmds=True, meas=True, count=True, k_stride=2, out="other", h=None):
    """One gate entry point on a NULL handle (or h) with tiny host arrays standing in for every pointer."""
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32)
    mo = np.zeros((1, 2, 3), np.float32); no = np.zeros(1, np.int32)
    at = {"slam_gate": (_lib._fp, _lib._fp, _lib._ip), "slam_step_gated": (_lib._fp, _lib._fp, _lib._ip),
          "slam_step_gated_each": (_lib._fp, _lib._fp, _lib._ip), "slam_step_gated_dev": (_lib._fp, None, None)}.get(fn, (None, None, None))
    ptr = (lambda a, t: a.ctypes.data_as(t) if t is not None else C.c_void_p(a.ctypes.data))
    cp = ptr(c, at[0]) if cmds else None
    mp = ptr(m, at[1]) if meas else None
    np_ = ptr(n, at[2]) if count else None
    cfgp = None if cfg is None else C.byref(cfg)
    if fn in NOW:
        outs = {"other": (mo, no), "in place": (m, n), "meas alone": (m, no), "count alone": (mo, n), "none": (None, None)}[out]
        mop = None if outs[0] is None else ptr(outs[0], at[1])
        nop = None if outs[1] is None else ptr(outs[1], at[2])
        return getattr(L, fn)(h, cfgp, cp, 0, mp, np_, k_stride, None, None, None, None, None, None, None, mop, nop, None, None)
    if fn == "slam_gate_run":
        return L.slam_gate_run(h, cfgp, ptr(c, _lib._fp) if cmds else None, 0, ptr(m, _lib._fp) if meas else None,
                               ptr(n, _lib._ip) if count else None, k_stride, 1, None, None, None, None, None)
    return getattr(L, fn)(h, cfgp, cp, mp, np_, k_stride, None, None)


ALL = NOW + STEPS + ("slam_gate_run",)


@pytest.mark.parametrize("field,value,word", [("gate", float("nan"), "gate ="), ("gate", 0.0, "gate ="), ("gate", -1.0, "gate ="),
                                              ("gate", -float("inf"), "gate ="), ("nis_lo", float("nan"), "band"),
                                              ("nis_hi", float("inf"), "band"), ("nis_lo", 10.0, "band")])
def test_config_checks_come_before_the_handle(field, value, word):
    cfg = default_gate_config()
    setattr(cfg, field, value)
    for fn in ALL:
        assert _call(fn, cfg=cfg) == ERR_ARG and word in _err() and "gate config" in _err(), fn
    assert _host(cfg=cfg) == ERR_ARG and word in _err()


def test_an_infinite_gate_is_allowed():
    cfg = default_gate_config()
    cfg.gate = float("inf")
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
        assert _call(fn, cfg=default_gate_config()) == ERR_ARG and "NULL handle" in _err(), fn
    for fn in NOW:     # a partial overlap of input and output: in place means both buffers
        assert _call(fn, out="meas alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="count alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="in place") == ERR_ARG and "NULL handle" in _err(), fn
    assert _call("slam_gate", out="none") == ERR_ARG and "NULL handle" in _err()          # host form: the message is optional
    assert _call("slam_gate_dev", out="none") == ERR_ARG and "d_meas_out" in _err()       # device form: it is where the result goes
    assert L.slam_gate_run(None, None, np.zeros(2, np.float32).ctypes.data_as(_lib._fp), 0, np.zeros(6, np.float32).ctypes.data_as(_lib._fp),
                           np.zeros(1, np.int32).ctypes.data_as(_lib._ip), 2, -1, None, None, None, None, None) == ERR_ARG and "negative" in _err()
    assert L.slam_last_gate_work(None, None, None) == ERR_ARG and "NULL handle" in _err()


def _host(cfg=None, **over):
    from live_ekf_slam_amd.config import Noise
    n = 5
    a = dict(x=np.zeros(n), P=np.eye(n).ravel().copy(), ids=np.array([3], np.int32), M=1, L_max=4, status=0, cmd=np.zeros(2, np.float32),
             meas=np.array([[3.0, 1.0, 0.1]], np.float32), count=1, k_stride=1, noise=Noise(0, 0, 0, 0, 0.01, 0.001, 0.01, 0.01, 0, 0, 0, 0))
    a.update(over)
    d = (lambda v: None if v is None else v.ctypes.data_as(_lib._dp))
    return _lib.lib().slam_gate_instance_host(
        d(a["x"]), d(a["P"]), None if a["ids"] is None else a["ids"].ctypes.data_as(_lib._ip), a["M"], a["L_max"], a["status"],
        None if a["cmd"] is None else a["cmd"].ctypes.data_as(_lib._fp), None if a["meas"] is None else a["meas"].ctypes.data_as(_lib._fp),
        a["count"], a["k_stride"], None if a["noise"] is None else C.byref(a["noise"]), 0, 0, None if cfg is None else C.byref(cfg),
        None, None, None, None, None, None, None, None, None, None, None)


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
    calls = (lambda: f.gate((0.1, 0.0), m, n), lambda: f.step_gated((0.1, 0.0), m, n), f.last_gate_work,
             lambda: f.gate_run(np.zeros((2, 2)), np.zeros((2, 3, 2, 3)), np.zeros((2, 3))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
