"""Joint-compatibility association (slam_associate_joint_*, include/slam_batch.h) without a GPU: the entry points exist, are declared and
mirrored, the build lists the new files, the defaults are what the header states, every SLAM_ERR_ARG path returns its code with a text
before the handle is looked at, and without a GPU the mirror fails loudly."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import JointConfig, Noise, default_assoc_config, default_joint_config

ERR_ARG = -1
SYMBOLS = ("slam_joint_config_default", "slam_associate_joint", "slam_associate_joint_dev", "slam_step_associated_joint",
           "slam_step_associated_joint_dev", "slam_associate_joint_run", "slam_last_joint_work", "slam_associate_joint_instance_host")
NOW = ("slam_associate_joint", "slam_associate_joint_dev")
STEPS = ("slam_step_associated_joint", "slam_step_associated_joint_dev")
ALL = NOW + STEPS + ("slam_associate_joint_run",)


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    assert header.index("int slam_associate_instance_host(") < header.index("---- joint-compatibility association") < header.index("---- map management")
    doc = header.split("---- joint-compatibility association")[1].split("#define SLAM_JOINT_MAX_CAND")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    for word in ("UKF kinds", "simulator sources", "slam_multi_", "pose graph", "slam_manage_run", "ln det S", "more than 16 pairings"):
        assert word in tail, word
    errors = " ".join(w for w in doc.split("Errors:")[1].split("Not covered:")[0].split() if w != "*")
    for word in ("before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "landmark_id_is_known = 0", "SLAM_ERR_STATE", "slam_track_instance", "max_nodes"):
        assert word in errors, word
    assert re.search(r"SLAM_ASSOC_JOINT_UNPAIRED = 7\b", header) and re.search(r"SLAM_JOINT_BUDGET = 16\b", header)
    assert re.search(r"SLAM_JOINT_S_SINGULAR = 32\b", header) and re.search(r"#define SLAM_JOINT_MAX_PAIR 16\b", header)
    for section in ("---- innovation gating", "---- association of detections WITHOUT ids"):      # the two gaps point here now
        assert "slam_associate_joint" in header.split(section)[1].split("enum slam_")[0], section
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "joint_kernel.hip" in build.SOURCES and "capi_joint.cpp" in build.SOURCES and "joint_kernel.h" in build.HEADERS
    for name in ("associate_joint", "step_associated_joint", "associate_joint_run", "last_joint_work"):
        assert callable(getattr(filters.BatchedEKF, name))
    assert callable(S.associate_joint_instance_host) and S.JointConfig is JointConfig and S.JointResult.REC_MAX_D2 == 8
    assert (S.ASSOC_JOINT_UNPAIRED, S.JOINT_BUDGET, S.JOINT_S_SINGULAR) == (7, 16, 32)


def test_struct_layout_and_defaults(tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\n'
                   'int main(){printf("%zu %zu %zu\\n", sizeof(slam_joint_config), offsetof(slam_joint_config, gate_joint),'
                   ' offsetof(slam_joint_config, max_nodes));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(JointConfig), JointConfig.gate_joint.offset, JointConfig.max_nodes.offset]
    L = _lib.lib()
    c = JointConfig()
    assert L.slam_joint_config_default(C.byref(c)) == 0
    a = default_assoc_config()
    assert (c.gate_match, c.gate_new, c.max_nodes) == (a.gate_match, a.gate_new, 2048) and c.gate_joint[0] == a.gate_match
    assert abs(c.gate_joint[1] - 13.276704135987625) < 1e-14 and abs(c.gate_joint[15] - 53.485771836235365) < 1e-13
    assert bytes(default_joint_config()) == bytes(c)
    assert L.slam_joint_config_default(None) == ERR_ARG and "NULL" in _err()


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
        return getattr(L, fn)(h, cfgp, cp, 0, mp, np_, k_stride, None, None, None, None, None, None, None, None, mop, nop, None, None, None)
    if fn == "slam_associate_joint_run":
        return L.slam_associate_joint_run(h, cfgp, cp, 0, mp, np_, k_stride, T, None, None, None, None, None, None, None)
    return getattr(L, fn)(h, cfgp, cp, 0, mp, np_, k_stride, None, None)


def _host(cfg=None, **over):
    n = 5
    a = dict(x=np.zeros(n), P=np.eye(n).ravel().copy(), ids=np.array([3], np.int32), M=1, L_max=4, status=0, cmd=np.zeros(2, np.float32),
             meas=np.array([[3.0, 1.0, 0.1]], np.float32), count=1, k_stride=1, noise=Noise(0, 0, 0, 0, 0.01, 0.001, 0.01, 0.01, 0, 0, 0, 0))
    a.update(over)
    d = (lambda v: None if v is None else v.ctypes.data_as(_lib._dp))
    return _lib.lib().slam_associate_joint_instance_host(
        d(a["x"]), d(a["P"]), None if a["ids"] is None else a["ids"].ctypes.data_as(_lib._ip), a["M"], a["L_max"], a["status"],
        None if a["cmd"] is None else a["cmd"].ctypes.data_as(_lib._fp), None if a["meas"] is None else a["meas"].ctypes.data_as(_lib._fp),
        a["count"], a["k_stride"], None if a["noise"] is None else C.byref(a["noise"]), 0, 0, None if cfg is None else C.byref(cfg),
        None, None, None, None, None, None, None, None, None, None, None, None, None, None)


def _cfg(**kw):
    c = default_joint_config()
    for k, v in kw.items():
        if isinstance(k, str) and k.startswith("g") and k[1:].isdigit():
            c.gate_joint[int(k[1:])] = v
        else:
            setattr(c, k, v)
    return c


BAD = [dict(gate_match=float("nan")), dict(gate_new=float("nan")), dict(gate_match=0.0), dict(gate_match=-1.0), dict(gate_match=30.0, gate_new=9.0),
       dict(g0=float("nan")), dict(g0=0.0), dict(g3=-2.0), dict(g5=20.0), dict(g15=float("nan")), dict(max_nodes=0), dict(max_nodes=-4),
       dict(max_nodes=65537)]


@pytest.mark.parametrize("bad", BAD, ids=[",".join(f"{k}={v}" for k, v in b.items()) for b in BAD])
def test_config_checks_come_before_the_handle(bad):
    cfg = _cfg(**bad)
    word = "assoc config" if any(k.startswith("gate_") for k in bad) else "joint config"
    for fn in ALL:
        assert _call(fn, cfg=cfg) == ERR_ARG and word in _err(), fn
    assert _host(cfg=cfg) == ERR_ARG and word in _err()


def test_infinite_gates_equal_gates_and_the_largest_budget_are_allowed():
    inf = float("inf")
    flat = _cfg(**{f"g{i}": 9.5 for i in range(16)})
    for cfg in (_cfg(gate_new=inf), _cfg(**{f"g{i}": inf for i in range(8, 16)}), flat, _cfg(max_nodes=65536), _cfg(max_nodes=1)):
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
        assert _call(fn, cfg=default_joint_config()) == ERR_ARG and "NULL handle" in _err(), fn
    for fn in NOW:     # a partial overlap of input and output: in place means both buffers
        assert _call(fn, out="meas alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="count alone") == ERR_ARG and "in place" in _err(), fn
        assert _call(fn, out="in place") == ERR_ARG and "NULL handle" in _err(), fn
    assert _call("slam_associate_joint", out="none") == ERR_ARG and "NULL handle" in _err()          # host form: the message is optional
    assert _call("slam_associate_joint_dev", out="none") == ERR_ARG and "d_meas_out" in _err()       # device form: it is where the result goes
    assert _call("slam_associate_joint_run", T=-1) == ERR_ARG and "negative" in _err()
    assert L.slam_last_joint_work(None, None, None, None) == ERR_ARG and "NULL handle" in _err()


def test_argument_checks_of_the_host_hook():
    assert _host() == 0                                    # every output may be NULL
    for key in ("x", "P", "cmd", "noise", "ids", "meas"):
        assert _host(**{key: None}) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", -1), ("k_stride", 0)):
        assert _host(**{key: value}) == ERR_ARG, (key, value)
    assert _host(M=0, ids=None, x=np.zeros(3), P=np.eye(3).ravel().copy(), count=0, meas=None) == 0
    assert _host(count=-2) == 0                            # a negative count is an empty message, as the step reads it


def test_the_mirror_needs_a_handle_and_checks_its_settings():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    m = np.zeros((3, 2, 3), np.float32); n = np.zeros(3, np.int32)
    calls = (lambda: f.associate_joint((0.1, 0.0), m, n), lambda: f.step_associated_joint((0.1, 0.0), m, n), f.last_joint_work,
             lambda: f.associate_joint_run(np.zeros((2, 2)), np.zeros((2, 3, 2, 3)), np.zeros((2, 3))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
    with pytest.raises(ValueError, match="unknown joint association setting"):
        f._joint_config(dict(gate=3.0))
    assert f._joint_config(dict(max_nodes=7, gate_joint=[float(i + 1) for i in range(16)])).gate_joint[15] == 16.0
