"""Absolute position and heading fixes (slam_fix*, slam_fix_sense*, slam_fix_run; include/slam_batch.h) without a GPU: the entry points
exist, are declared and mirrored with matching argument counts, the build lists the new files, the struct layouts are the compiler's,
the defaults are the documented ones, and every SLAM_ERR_ARG path returns its code with a text before the handle is looked at."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import FixConfig, FixLog, FixSensorConfig, default_fix_config, default_fix_sensor_config

ERR_ARG = -1
SYMBOLS = ("slam_fix_config_default", "slam_fix", "slam_fix_dev", "slam_fix_sensor_default", "slam_set_fix_sensor_each", "slam_fix_sense",
           "slam_fix_sense_dev", "slam_fix_run", "slam_last_fix_work", "slam_fix_instance_host", "slam_fix_sense_instance_host")
BAD_CONFIGS = [("gate_pos", float("nan")), ("gate_pos", 0.0), ("gate_pos", -1.0), ("gate_yaw", float("nan")), ("gate_yaw", 0.0),
               ("gate_yaw", -float("inf")), ("fix_every", 0), ("fix_every", -3)]
BAD_ROWS = [("pos_halfwidth", -1e-9), ("pos_halfwidth", float("nan")), ("yaw_halfwidth", float("inf")), ("sigma_pos", -1.0),
            ("sigma_yaw", float("nan")), ("p_miss_pos", 1.5), ("p_miss_yaw", -0.1), ("p_jump", float("nan")), ("jump_lo", float("inf")),
            ("jump_hi", -1.0), ("kinds", 4), ("kinds", -1)]


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        m = re.search(r"\bint %s\(([^)]*)\)" % name, header)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert header.index("int slam_sense_instance_host(") < header.index("---- absolute position and heading fixes") < header.index("int slam_fix_config_default(")
    assert header.index("int slam_fix_sense_instance_host(") < header.index("---- closed loop")
    doc = " ".join(w for w in header.split("---- absolute position and heading fixes")[1].split("enum slam_fix_kinds")[0].split() if w != "*")
    for word in ("position first, then heading", "INVALID", "SINGULAR", "REJECTED", "a nis equal to the gate is accepted", "ONCE",
                 "after slam_sense_commit", "before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "Not covered:", "the UKF kinds", "slam_multi_",
                 "multi-step launches", "lever arms", "full 2 x 2 position covariances", "checkpoints of the sensor rows"):
        assert word in doc, word
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "fix_kernel.hip" in build.SOURCES and "capi_fix.cpp" in build.SOURCES and "fix_kernel.h" in build.HEADERS
    for name in ("fix", "set_fix_sensor", "fix_sense", "fix_run", "last_fix_work"):
        assert callable(getattr(filters.BatchedEKF, name)), name
        assert not hasattr(filters.BatchedUKF, name), name
    assert callable(S.fix_instance_host) and callable(S.fix_sense_instance_host) and S.FixConfig is FixConfig
    assert S.FixResult.REC_FIX_WRITTEN == 0 and S.FixResult.REC_FIX_POS_APPLIED == 2 and S.FixResult.REC_FIX_YAW_REJECTED == 8 and S.FixResult.REC_FIX_SKIPPED == 13
    assert (S.FIX_POS, S.FIX_YAW, S.FIX_APPLIED, S.FIX_REJECTED, S.FIX_SINGULAR, S.FIX_INVALID) == (1, 2, 1, 2, 3, 4)


def test_default_config_and_struct_layouts(tmp_path):
    mpmath = pytest.importorskip("mpmath")
    L = _lib.lib()
    c = FixConfig()
    assert L.slam_fix_config_default(C.byref(c)) == 0
    assert (c.gate_pos, c.gate_yaw, c.fix_every) == (-2.0 * math.log(0.001), 10.827566170662733, 10)
    # the literal is the 0.999 quantile of chi-square with 1 degree of freedom: P(chi2_1 <= q) = erf(sqrt(q / 2))
    mpmath.mp.dps = 30
    assert abs(mpmath.erf(mpmath.sqrt(mpmath.mpf(c.gate_yaw) / 2)) - mpmath.mpf("0.999")) < 1e-17
    assert abs((1 - mpmath.exp(-mpmath.mpf(c.gate_pos) / 2)) - mpmath.mpf("0.999")) < 1e-16
    d = default_fix_config()
    assert all(getattr(d, name) == getattr(c, name) for name, _ in FixConfig._fields_)
    assert L.slam_fix_config_default(None) == ERR_ARG and "NULL" in _err()
    row = FixSensorConfig(1, 2, 3, 4, 5, 6, 7, 8, 9, 3)
    assert L.slam_fix_sensor_default(C.byref(row)) == 0 and bytes(row) == bytes(C.sizeof(FixSensorConfig))
    assert L.slam_fix_sensor_default(None) == ERR_ARG and "NULL" in _err()
    fields = [("slam_fix_config", FixConfig), ("slam_fix_sensor", FixSensorConfig), ("slam_fix_log", FixLog)]
    body = "".join('printf("%%zu", sizeof(%s));' % s + "".join('printf(" %%zu", offsetof(%s, %s));' % (s, n) for n, _ in t._fields_) + 'printf("\\n");'
                   for s, t in fields)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\nint main(){%s return 0;}\n' % body)
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)]).decode().splitlines()
    for line, (_, t) in zip(lines, fields):
        assert [int(v) for v in line.split()] == [C.sizeof(t)] + [getattr(t, n).offset for n, _ in t._fields_], t


def _calls(cfg=None, fix=True, kinds=True, cmds=True, T=1, source=0):
    """Every entry point that takes a handle, on a NULL handle with tiny host arrays standing in for every pointer: name -> (code, text)."""
    L = _lib.lib()
    f = np.zeros((1, 5)); k = np.zeros(1, np.int32); c = np.zeros(2, np.float32)
    cfgp = None if cfg is None else C.byref(cfg)
    dp = (lambda a, on: a.ctypes.data_as(_lib._dp) if on else None)
    ip = (lambda a, on: a.ctypes.data_as(_lib._ip) if on else None)
    vp = (lambda a, on: C.c_void_p(a.ctypes.data) if on else None)
    out = {}
    out["slam_fix"] = (L.slam_fix(None, cfgp, dp(f, fix), ip(k, kinds), None, None, None), _err())
    out["slam_fix_dev"] = (L.slam_fix_dev(None, cfgp, vp(f, fix), vp(k, kinds), None, None, None), _err())
    out["slam_fix_run"] = (L.slam_fix_run(None, cfgp, source, c.ctypes.data_as(_lib._fp) if cmds else None, T, None, None, None, None), _err())
    if cfg is None:
        out["slam_fix_sense"] = (L.slam_fix_sense(None, dp(f, fix), ip(k, kinds), None), _err())
        out["slam_fix_sense_dev"] = (L.slam_fix_sense_dev(None, vp(f, fix), vp(k, kinds), None), _err())
    return out


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_config_checks_come_before_the_handle(field, value):
    cfg = default_fix_config()
    setattr(cfg, field, value)
    for fn, (rc, text) in _calls(cfg=cfg).items():
        assert rc == ERR_ARG and "fix config" in text and field in text, (fn, text)
    x = np.zeros(3); P = np.eye(3).ravel().copy(); row = np.zeros(5)
    d = lambda a: a.ctypes.data_as(_lib._dp)
    assert _lib.lib().slam_fix_instance_host(d(x), d(P), 0, 4, 0, 0, C.byref(cfg), d(row), 3, None, None, None) == ERR_ARG and "fix config" in _err()


def test_the_limits_of_the_config_are_allowed():
    for cfg in (FixConfig(1e-300, 1e-300, 1), FixConfig(math.inf, math.inf, 2 ** 31 - 1), FixConfig(13.8, 10.8, 7)):
        for fn, (rc, text) in _calls(cfg=cfg).items():
            assert rc == ERR_ARG and "NULL handle" in text, (fn, text)


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    for fn, (rc, text) in _calls().items():
        assert rc == ERR_ARG and "NULL handle" in text, (fn, text)
    for kw, word in ((dict(fix=False), "fix is NULL"), (dict(kinds=False), "kinds is NULL")):
        got = _calls(**kw)
        for fn in ("slam_fix", "slam_fix_dev", "slam_fix_sense", "slam_fix_sense_dev"):
            assert got[fn][0] == ERR_ARG and word in got[fn][1] and "NULL handle" not in got[fn][1], (fn, got[fn])
    for kw, word in ((dict(T=-1), "negative"), (dict(cmds=False), "cmds is NULL"), (dict(cmds=False, source=1), "cmds is NULL"), (dict(source=3), "LOG"),
                     (dict(source=9), "unknown source")):
        rc, text = _calls(**kw)["slam_fix_run"]
        assert rc == ERR_ARG and word in text and "NULL handle" not in text, (kw, text)
    assert _calls(cmds=False, source=2)["slam_fix_run"][1].count("NULL handle") == 1     # NAV reads no commands
    assert L.slam_last_fix_work(None, None, None, None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_set_fix_sensor_each(None, None) == ERR_ARG and "NULL handle" in _err()


@pytest.mark.parametrize("field,value", BAD_ROWS)
def test_sensor_rows_are_validated_by_field(field, value):
    row = default_fix_sensor_config(pos_halfwidth=0.1, jump_lo=0.0, jump_hi=1.0, kinds=3)
    setattr(row, field, value)
    fix = np.zeros(5); truth = np.zeros(3); kinds = C.c_int32(0)
    d = lambda a: a.ctypes.data_as(_lib._dp)
    rc = _lib.lib().slam_fix_sense_instance_host(1, 2, 3, d(truth), C.byref(row), d(fix), C.byref(kinds), None)
    assert rc == ERR_ARG and field in _err(), _err()


def test_argument_checks_of_the_host_hooks():
    L = _lib.lib()
    d = (lambda a: None if a is None else a.ctypes.data_as(_lib._dp))

    def call(**over):
        a = dict(x=np.zeros(5), P=np.eye(5).ravel().copy(), M=1, L_max=4, row=np.array([0.1, 0.1, 0.1, 0.5, 0.5]))
        a.update(over)
        return L.slam_fix_instance_host(d(a["x"]), d(a["P"]), a["M"], a["L_max"], 0, 0, None, d(a["row"]), 3, None, None, None)
    assert call() == 0                                     # every output may be NULL
    for key in ("x", "P", "row"):
        assert call(**{key: None}) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", 0), ("L_max", 1001)):
        assert call(**{key: value}) == ERR_ARG, (key, value)
    fix = np.zeros(5); truth = np.zeros(3); kinds = C.c_int32(7)
    assert L.slam_fix_sense_instance_host(1, 2, 3, d(truth), None, d(fix), C.byref(kinds), None) == 0 and kinds.value == 0
    assert L.slam_fix_sense_instance_host(1, 2, 3, None, None, d(fix), C.byref(kinds), None) == ERR_ARG
    assert L.slam_fix_sense_instance_host(1, 2, 3, d(truth), None, None, C.byref(kinds), None) == ERR_ARG


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    calls = (lambda: f.fix(np.zeros((3, 5)), np.zeros(3, np.int32)), lambda: f.set_fix_sensor(None), f.fix_sense, f.last_fix_work,
             lambda: f.fix_run(np.zeros((2, 2))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
