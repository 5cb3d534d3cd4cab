"""The simulator source with a sensor fault model (slam_sensor, slam_sense*, the *_run_sim calls; include/slam_batch.h) without a GPU: the
entry points exist, are declared and mirrored with matching argument counts, the build lists the new files, the struct layouts are the
compiler's, the default row round-trips, and every SLAM_ERR_ARG path returns its code with a text before the handle is looked at."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import (AssocConfig, GateConfig, MapConfig, MergeConfig, SenseLog, SensorConfig, default_config, default_joint_config,
                                      default_sensor_config)

ERR_ARG = -1
SHARED, EACH, NAV, LOG = 0, 1, 2, 3
RUNS = ("slam_gate_run_sim", "slam_associate_run_sim", "slam_associate_joint_run_sim", "slam_manage_run_sim", "slam_manage_merge_run_sim")
SYMBOLS = ("slam_sensor_default", "slam_set_sensor_each", "slam_sense", "slam_sense_dev", "slam_sense_commit", "slam_sense_instance_host") + RUNS


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
    assert header.index("int slam_merge_instance_host(") < header.index("---- simulator source with a sensor fault model") < header.index("---- closed loop")
    doc = " ".join(w for w in header.split("---- simulator source with a sensor fault model")[1].split("#define SLAM_SENSE_MAX_DET")[0].split() if w != "*")
    for word in ("F = 0x40000000", "missed iff a_v < p_miss", "spiked iff b_v < p_spike", "0x7FC00000", "timestep == (the timestep at the sense) + 1",
                 "before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "Not covered:", "the UKF kinds", "the pose graph", "slam_multi_",
                 "multi-step launches", "wrong-id", "bursty or correlated", "landmark part of slam_consistency"):
        assert word in doc, word
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "sense_kernel.hip" in build.SOURCES and "capi_sense.cpp" in build.SOURCES
    assert "sense_kernel.h" in build.HEADERS and "capi_sense.h" in build.HEADERS
    for name in ("set_sensor", "sense", "sense_dev", "sense_commit") + tuple(r[len("slam_"):] for r in RUNS):
        assert callable(getattr(filters.BatchedEKF, name)), name
        assert not hasattr(filters.BatchedUKF, name), name
    assert callable(S.sense_instance_host) and S.SensorConfig is SensorConfig and callable(S.default_sensor_config)
    assert (S.SENSE_MAX_DET, S.SENSE_MAX_CLUTTER, S.SENSE_INSTANCE_FROZEN, S.SENSE_TOO_LONG) == (64, 8, 1, 2)


def test_default_row_round_trip_and_struct_layouts(tmp_path):
    L = _lib.lib()
    row = SensorConfig(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 7, 1, 1)
    assert L.slam_sensor_default(C.byref(row)) == 0
    assert all(getattr(row, name) == 0 for name, _ in SensorConfig._fields_)
    assert bytes(row) == bytes(default_sensor_config()) == bytes(C.sizeof(SensorConfig))
    assert L.slam_sensor_default(None) == ERR_ARG and "NULL" in _err()
    fields = [n for n, _ in SensorConfig._fields_]; lfields = [n for n, _ in SenseLog._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\nint main(){printf("%zu %zu", sizeof(slam_sensor), sizeof(slam_sense_log));\n'
                   + "".join('printf(" %%zu", offsetof(slam_sensor, %s));\n' % f for f in fields)
                   + "".join('printf(" %%zu", offsetof(slam_sense_log, %s));\n' % f for f in lfields) + "return 0;}\n")
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(SensorConfig), C.sizeof(SenseLog)] + [getattr(SensorConfig, f).offset for f in fields] + [getattr(SenseLog, f).offset for f in lfields]


def _runs(source=SHARED, cmds=True, k_stride=4, T=1, gate=None, assoc=None, joint=None, mapc=None, merge=None):
    """Every *_run_sim call on a NULL handle: name -> (code, text)."""
    L = _lib.lib()
    c = np.zeros(2, np.float32)
    cp = c.ctypes.data_as(_lib._fp) if cmds else None
    by = (lambda v: None if v is None else C.byref(v))
    out = {}
    out["slam_gate_run_sim"] = (L.slam_gate_run_sim(None, by(gate), source, cp, k_stride, T, None, None, None, None, None, None), _err())
    out["slam_associate_run_sim"] = (L.slam_associate_run_sim(None, by(assoc), source, cp, k_stride, T, None, None, None, None, None, None), _err())
    out["slam_associate_joint_run_sim"] = (L.slam_associate_joint_run_sim(None, by(joint), source, cp, k_stride, T, None, None, None, None, None, None,
                                                                          None, None), _err())
    out["slam_manage_run_sim"] = (L.slam_manage_run_sim(None, by(assoc), by(mapc), source, cp, k_stride, T, None, None, None, None, None, None, None),
                                  _err())
    out["slam_manage_merge_run_sim"] = (L.slam_manage_merge_run_sim(None, by(assoc), by(mapc), by(merge), source, cp, k_stride, T, None, None, None, None,
                                                                    None, None, None, None), _err())
    return out


def test_argument_checks_of_the_runs_come_before_the_handle():
    for kw in (dict(), dict(source=EACH), dict(source=NAV, cmds=False), dict(T=0)):
        for fn, (rc, text) in _runs(**kw).items():
            assert rc == ERR_ARG and "NULL handle" in text, (fn, kw, text)
    for kw, word in ((dict(source=LOG), "LOG"), (dict(source=4), "unknown source"), (dict(source=-1), "unknown source"), (dict(cmds=False), "cmds is NULL"),
                     (dict(source=EACH, cmds=False), "cmds is NULL"), (dict(T=-1), "negative"), (dict(k_stride=0), "k_stride"), (dict(k_stride=-2), "k_stride")):
        for fn, (rc, text) in _runs(**kw).items():
            assert rc == ERR_ARG and word in text and "NULL handle" not in text, (fn, kw, text)
    # the configs of the LOG siblings are checked as there
    bad_joint = default_joint_config(); bad_joint.max_nodes = 0
    got = _runs(gate=GateConfig(-1.0, 1.0, 2.0), assoc=AssocConfig(30.0, 9.0), joint=bad_joint)
    assert got["slam_gate_run_sim"][0] == ERR_ARG and "gate config" in got["slam_gate_run_sim"][1]
    for fn in ("slam_associate_run_sim", "slam_manage_run_sim", "slam_manage_merge_run_sim"):
        assert got[fn][0] == ERR_ARG and "assoc config" in got[fn][1], got[fn]
    assert got["slam_associate_joint_run_sim"][0] == ERR_ARG and "NULL handle" not in got["slam_associate_joint_run_sim"][1]
    got = _runs(mapc=MapConfig(0.9, 0.1, 0, 0.3, 10), merge=MergeConfig(-1.0, 0.0, 10))
    assert "map config" in got["slam_manage_run_sim"][1] and "map config" in got["slam_manage_merge_run_sim"][1]
    got = _runs(merge=MergeConfig(-1.0, 0.0, 10))
    assert got["slam_manage_merge_run_sim"][0] == ERR_ARG and "merge config" in got["slam_manage_merge_run_sim"][1]


def test_argument_checks_of_sense_and_commit():
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32)
    fp, ip, vp = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip)), (lambda a: C.c_void_p(a.ctypes.data))
    assert L.slam_sense(None, fp(c), 0, fp(m), ip(n), 2, None, None, None, None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_sense_dev(None, vp(c), 0, vp(m), vp(n), 2, None, None) == ERR_ARG and "NULL handle" in _err()
    for args, word in (((None, 0, fp(m), ip(n), 2), "cmds is NULL"), ((fp(c), 0, None, ip(n), 2), "meas"), ((fp(c), 0, fp(m), None, 2), "meas"),
                       ((fp(c), 1, fp(m), ip(n), 0), "k_stride"), ((fp(c), 0, fp(m), ip(n), -1), "k_stride")):
        assert L.slam_sense(None, *args, None, None, None, None) == ERR_ARG and word in _err() and "NULL handle" not in _err(), (args, _err())
    for args, word in (((None, 0, vp(m), vp(n), 2), "cmds is NULL"), ((vp(c), 0, None, vp(n), 2), "meas"), ((vp(c), 0, vp(m), None, 2), "meas"),
                       ((vp(c), 0, vp(m), vp(n), 0), "k_stride")):
        assert L.slam_sense_dev(None, *args, None, None) == ERR_ARG and word in _err() and "NULL handle" not in _err(), (args, _err())
    assert L.slam_sense_commit(None, None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_set_sensor_each(None, None) == ERR_ARG and "NULL handle" in _err()
    rows = (SensorConfig * 1)(default_sensor_config())
    assert L.slam_set_sensor_each(None, rows) == ERR_ARG and "NULL handle" in _err()


BAD_ROWS = [("p_miss", dict(p_miss=-0.1)), ("p_miss", dict(p_miss=1.5)), ("p_miss", dict(p_miss=float("nan"))), ("p_spike", dict(p_spike=1.0001)),
            ("p_spike", dict(p_spike=float("inf"))), ("p_clutter", dict(p_clutter=-1e-9)), ("p_clutter", dict(p_clutter=float("nan"))),
            ("spike_lo", dict(spike_lo=float("nan"))), ("spike_lo", dict(spike_lo=float("-inf"))), ("spike_hi", dict(spike_lo=1.0, spike_hi=0.5)),
            ("spike_hi", dict(spike_hi=float("inf"))), ("n_clutter", dict(n_clutter=-1)), ("n_clutter", dict(n_clutter=9)),
            ("clutter_r_min", dict(clutter_r_min=-0.5)), ("clutter_r_min", dict(clutter_r_min=float("nan"))),
            ("clutter_r_min", dict(clutter_r_min=3.0001))]


@pytest.mark.parametrize("field,over", BAD_ROWS, ids=[f"{f}-{i}" for i, (f, _) in enumerate(BAD_ROWS)])
def test_the_value_checks_of_a_sensor_row_name_the_field(field, over):
    """The checker slam_set_sensor_each applies to every row, reached without a device through the host hook (range_max = 3)."""
    from live_ekf_slam_amd import sense_instance_host
    args = (1, 0, 0, np.zeros(3), (0.05, 0.0), np.array([[1.0, 0.0]]), default_config())
    with pytest.raises(_lib.SlamError, match="sensor field %s " % field):
        sense_instance_host(*args, row=default_sensor_config(**over))
    # the limits themselves are allowed
    ok = default_sensor_config(p_miss=1.0, p_spike=0.0, p_clutter=1.0, spike_lo=-2.0, spike_hi=-2.0, n_clutter=8, clutter_r_min=3.0)
    assert sense_instance_host(*args, row=ok)["count"] == 8


def test_argument_checks_of_the_host_hook():
    from live_ekf_slam_amd import sense_instance_host
    cfg = default_config()
    good = dict(seed=1, instance=0, step=0, truth=np.zeros(3), cmd=(0.05, 0.0), map_xy=np.array([[1.0, 0.0]]), cfg=cfg)
    assert sense_instance_host(**good)["count"] == 1
    with pytest.raises(_lib.SlamError, match="k_stride"):
        sense_instance_host(**good, k_stride=0)
    L = _lib.lib()
    t = np.zeros(3); c = np.zeros(2, np.float32); m = np.zeros((1, 2)); sn = np.zeros(4); meas = np.zeros((2, 3), np.float32); cnt = C.c_int32(0)
    d, f = (lambda a: a.ctypes.data_as(_lib._dp)), (lambda a: a.ctypes.data_as(_lib._fp))
    base = [1, 0, 0, d(t), f(c), 0, d(m), 1, 0.1, 0.05, 3.0, -1.57, 1.57, d(sn), None, 2, f(meas), C.cast(C.byref(cnt), _lib._ip), None, None, None, None, None]
    assert L.slam_sense_instance_host(*base) == 0
    for i in (3, 4, 6, 13, 16, 17):
        a = list(base); a[i] = None
        assert L.slam_sense_instance_host(*a) == ERR_ARG and "NULL" in _err(), i
    a = list(base); a[7] = 0
    assert L.slam_sense_instance_host(*a) == ERR_ARG and "L = 0" in _err()


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    calls = (lambda: f.set_sensor(None), lambda: f.sense((0.0, 0.0), 4), f.sense_commit, lambda: f.gate_run_sim(np.zeros((2, 2))),
             lambda: f.associate_run_sim(T=2), lambda: f.associate_joint_run_sim(np.zeros((2, 3, 2))), lambda: f.manage_run_sim(np.zeros((2, 2))),
             lambda: f.manage_merge_run_sim(np.zeros((2, 2))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
