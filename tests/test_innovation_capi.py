"""The innovation statistics (slam_innovation_*, include/slam_batch.h) without a GPU: the entry points exist and are mirrored, the
defaults are the chi-square quantiles for 2 degrees of freedom, every SLAM_ERR_ARG path returns its code with a text before the handle
is looked at, and without a device the mirror fails loudly."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import InnovationConfig, Noise, default_config, default_innovation_config, INNOV_MAX_DET, INNOV_MAX_LM

ERR_ARG = -1
SYMBOLS = ("slam_innovation_config_default", "slam_innovation", "slam_innovation_dev", "slam_innovation_run", "slam_last_innovation_work",
           "slam_innovation_instance_host")


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    doc = header.split("---- innovation (NIS) statistics")[1].split("enum slam_innovation_flags")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    for word in ("UKF", "unknown ids", "whiteness", "gating", "slam_multi_", "pose graph", "multi-step launches"):
        assert word in tail, word
    assert re.search(r"#define SLAM_INNOV_MAX_DET %d\b" % INNOV_MAX_DET, header) and re.search(r"#define SLAM_INNOV_MAX_LM %d\b" % INNOV_MAX_LM, header)
    assert re.search(r"SLAM_INNOVATION_INSTANCE_FROZEN = 1,", header) and re.search(r"SLAM_INNOVATION_WOULD_FREEZE = 2,", header)
    assert re.search(r"SLAM_INNOVATION_S_SINGULAR = 4,", header) and re.search(r"SLAM_INNOVATION_TOO_LONG = 8\b", header)
    assert "SLAM_INNOVATION_SHARED = 0, SLAM_INNOVATION_EACH = 1, SLAM_INNOVATION_NAV = 2, SLAM_INNOVATION_LOG = 3" in header
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    assert "Innovation innovation(" in hpp and "InnovationRun innovationRun(" in hpp and "lastInnovationWork(" in hpp
    from live_ekf_slam_amd import build, filters
    assert "innovation_kernel.hip" in build.SOURCES and "innovation_kernel.h" in build.HEADERS
    for name in ("innovation", "innovation_run", "last_innovation_work"):
        assert callable(getattr(filters.BatchedEKF, name))
    R = filters.InnovationResult
    assert (R.REC_N_EVAL, R.REC_N_UPD, R.REC_SUM_NIS, R.REC_MAX_NIS, R.REC_SUM_NU_B2, R.REC_RESERVED) == (0, 5, 7, 8, 14, 15)
    assert (filters.BatchedEKF.INNOVATION_FROZEN, filters.BatchedEKF.INNOVATION_WOULD_FREEZE, filters.BatchedEKF.INNOVATION_S_SINGULAR,
            filters.BatchedEKF.INNOVATION_TOO_LONG) == (1, 2, 4, 8)


def test_default_config():
    L = _lib.lib()
    c = InnovationConfig()
    assert L.slam_innovation_config_default(C.byref(c)) == 0
    assert (c.nis_lo, c.nis_hi) == (-2.0 * math.log(0.975), -2.0 * math.log(0.025))
    assert bytes(default_innovation_config()) == bytes(c)
    assert abs(c.nis_lo - 0.0506356) < 1e-7 and abs(c.nis_hi - 7.3777589) < 1e-7
    # chi-square with 2 degrees of freedom has the distribution function 1 - exp(-x / 2)
    assert abs((1 - math.exp(-c.nis_lo / 2)) - 0.025) < 1e-15 and abs((1 - math.exp(-c.nis_hi / 2)) - 0.975) < 1e-15
    assert L.slam_innovation_config_default(None) == ERR_ARG and "NULL" in _err()


def _now(fn="slam_innovation", cfg=None, cmds=True, meas=True, count=True, k_stride=2, h=None):
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32)
    host = fn == "slam_innovation"
    cp = (c.ctypes.data_as(_lib._fp) if host else C.c_void_p(c.ctypes.data)) if cmds else None
    mp = (m.ctypes.data_as(_lib._fp) if host else C.c_void_p(m.ctypes.data)) if meas else None
    np_ = (n.ctypes.data_as(_lib._ip) if host else C.c_void_p(n.ctypes.data)) if count else None
    return getattr(L, fn)(h, None if cfg is None else C.byref(cfg), cp, 0, mp, np_, k_stride, None, None, None, None, None, None, None)


def _run(cfg=None, source=0, cmds=True, meas=False, count=False, k_stride=0, T=1, h=None):
    L = _lib.lib()
    c = np.zeros((max(T, 1), 2), np.float32); m = np.zeros((max(T, 1), 1, 2, 3), np.float32); n = np.zeros((max(T, 1), 1), np.int32)
    return L.slam_innovation_run(h, None if cfg is None else C.byref(cfg), source, c.ctypes.data_as(_lib._fp) if cmds else None,
                                 m.ctypes.data_as(_lib._fp) if meas else None, n.ctypes.data_as(_lib._ip) if count else None, k_stride, T,
                                 None, None, None, None)


@pytest.mark.parametrize("field,value", [("nis_lo", float("nan")), ("nis_hi", float("inf")), ("nis_lo", 10.0), ("nis_hi", -float("inf"))])
def test_config_checks_come_before_the_handle(field, value):
    cfg = default_innovation_config()
    setattr(cfg, field, value)
    for rc in (_run(cfg), _now(cfg=cfg), _now("slam_innovation_dev", cfg=cfg)):
        assert rc == ERR_ARG and "band" in _err() and "innovation config" in _err()
    st = _host_args()
    st["cfg"] = cfg
    assert _host(**st) == ERR_ARG and "band" in _err()


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    for fn in ("slam_innovation", "slam_innovation_dev"):
        assert _now(fn, cmds=False) == ERR_ARG and "cmds" in _err()
        assert _now(fn, meas=False) == ERR_ARG and "meas" in _err()
        assert _now(fn, count=False) == ERR_ARG and "meas" in _err()
        assert _now(fn, k_stride=0) == ERR_ARG and "k_stride" in _err()
        assert _now(fn, k_stride=-3) == ERR_ARG and "k_stride" in _err()
        assert _now(fn) == ERR_ARG and "NULL handle" in _err()
        assert _now(fn, cfg=default_innovation_config()) == ERR_ARG and "NULL handle" in _err()
    assert _run(source=4) == ERR_ARG and "source" in _err()
    assert _run(source=-1) == ERR_ARG and "source" in _err()
    assert _run(T=-1) == ERR_ARG and "negative" in _err()
    for source in (0, 1, 3):
        assert _run(cmds=False, source=source) == ERR_ARG and "cmds" in _err()
    assert _run(cmds=False, source=2) == ERR_ARG and "NULL handle" in _err()      # NAV takes no commands: the next check is the handle
    assert _run(source=3, meas=False, count=True, k_stride=2) == ERR_ARG and "LOG" in _err()
    assert _run(source=3, meas=True, count=False, k_stride=2) == ERR_ARG and "LOG" in _err()
    assert _run(source=3, meas=True, count=True, k_stride=0) == ERR_ARG and "k_stride" in _err()
    assert _run(source=3, meas=True, count=True, k_stride=2) == ERR_ARG and "NULL handle" in _err()
    assert _run() == ERR_ARG and "NULL handle" in _err()                          # (the simulator sources do not read meas)
    assert L.slam_last_innovation_work(None, None, None) == ERR_ARG and "NULL handle" in _err()


def _host_args():
    n = 5
    return dict(x=np.zeros(n), P=np.eye(n).ravel().copy(), ids=np.array([3], np.int32), M=1, L_max=4, status=0, cmd=np.zeros(2, np.float32),
                meas=np.array([[3.0, 1.0, 0.1]], np.float32), k=1, noise=Noise(0, 0, 0, 0, 0.01, 0.001, 0.01, 0.01, 0, 0, 0, 0), cfg=None)


def _host(x, P, ids, M, L_max, status, cmd, meas, k, noise, cfg):
    L = _lib.lib()
    d = (lambda a: None if a is None else a.ctypes.data_as(_lib._dp))
    return L.slam_innovation_instance_host(d(x), d(P), None if ids is None else ids.ctypes.data_as(_lib._ip), M, L_max, status,
                                           None if cmd is None else cmd.ctypes.data_as(_lib._fp),
                                           None if meas is None else meas.ctypes.data_as(_lib._fp), k,
                                           None if noise is None else C.byref(noise), 0, 0, None if cfg is None else C.byref(cfg), None, None,
                                           None, None, None, None, None)


def test_argument_checks_of_the_host_hook():
    assert _host(**_host_args()) == 0                      # every output may be NULL
    for key in ("x", "P", "cmd", "noise", "ids", "meas"):
        a = _host_args(); a[key] = None
        assert _host(**a) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", -1), ("k", -1)):
        a = _host_args(); a[key] = value
        assert _host(**a) == ERR_ARG, (key, value)
    a = _host_args(); a["noise"].W_00 = float("nan")
    assert _host(**a) == ERR_ARG and "W_00" in _err()
    a = _host_args(); a.update(M=0, ids=None, x=np.zeros(3), P=np.eye(3).ravel().copy(), k=0, meas=None)
    assert _host(**a) == 0


def test_the_mirror_needs_a_handle_and_without_a_device_it_fails_loudly():
    from live_ekf_slam_amd.filters import BatchedEKF, BatchedUKF
    f = BatchedEKF(3, 4)
    m = np.zeros((3, 2, 3), np.float32); n = np.zeros(3, np.int32)
    calls = (lambda: f.innovation((0.1, 0.0), m, n), lambda: f.innovation_run(np.zeros((2, 2))), f.last_innovation_work)
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
    try:
        f.readParams(default_config())
    except _lib.SlamError as e:   # no HIP device: no handle, and the mirror refuses to compute without one
        assert "hip" in str(e).lower(), str(e)
        for call in calls:
            with pytest.raises(_lib.SlamError, match="readParams"):
                call()
        return
    with pytest.raises(_lib.SlamError, match="slam_init has not been called"):
        f.innovation((0.1, 0.0), m, n)
    with pytest.raises(_lib.SlamError, match="slam_init has not been called"):
        f.innovation_run(np.zeros((2, 2)))
    with pytest.raises(_lib.SlamError, match="has not run"):
        f.last_innovation_work()
    f.init(0.0, 0.0, 0.0)
    with pytest.raises(_lib.SlamError, match="slam_set_map"):
        f.innovation_run(np.zeros((2, 2)))
    r = f.innovation((0.1, 0.0), m, n)   # the start state, empty messages: the prediction alone
    assert r["flags"].tolist() == [0, 0, 0] and r["rec"][0] == 3 and np.all(r["nis_sum"] == 0) and np.isnan(r["det"]).all()
    f.close()
    u = BatchedUKF(2, 4).readParams(default_config())
    u.init(0.0, 0.0, 0.0)
    with pytest.raises(_lib.SlamError, match="sigma points"):
        _lib.check(_lib.lib().slam_innovation_run(u.h, None, 0, np.zeros((1, 2), np.float32).ctypes.data_as(_lib._fp), None, None, 0, 1, None,
                                                  None, None, None))
    u.close()
