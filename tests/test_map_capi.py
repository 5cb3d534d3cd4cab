"""Map management (slam_remove_landmarks, slam_map_*, slam_step_managed*, slam_manage_run; include/slam_batch.h) without a GPU: the entry
points exist, are declared and mirrored, the build lists the new files, the defaults are the documented ones, and every SLAM_ERR_ARG path
returns its code with a text before the handle is looked at."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import AssocConfig, MapConfig, default_map_config

ERR_ARG = -1
SYMBOLS = ("slam_map_config_default", "slam_remove_landmarks", "slam_remove_landmarks_dev", "slam_map_tally", "slam_map_tally_dev",
           "slam_map_prune", "slam_map_get_track", "slam_map_track_reset", "slam_step_managed", "slam_step_managed_dev", "slam_manage_run",
           "slam_last_map_work", "slam_map_instance_host")
BAD_CONFIGS = [("range_shrink", float("nan")), ("fov_margin", float("nan")), ("min_ratio", float("nan")), ("range_shrink", 0.0),
               ("range_shrink", -0.5), ("range_shrink", 1.0000001), ("fov_margin", -1e-9), ("min_expected", 0), ("min_expected", -4),
               ("min_ratio", -0.1), ("min_ratio", 1.5), ("prune_every", 0), ("prune_every", -1)]


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
    assert header.index("int slam_associate_instance_host(") < header.index("---- map management") < header.index("---- closed loop")
    doc = header.split("---- map management")[1].split("typedef struct slam_map_config")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    for word in ("merging duplicate landmarks", "the UKF", "slam_multi_", "simulator sources", "pose graph", "counters in checkpoints"):
        assert word in tail, word
    errors = " ".join(w for w in doc.split("Errors:")[1].split("Not covered:")[0].split() if w != "*")
    for word in ("before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "SLAM_ERR_STATE", "slam_track_instance", "prediction is pending"):
        assert word in errors, word
    for word in ("exact marginalisation", "inserted as NEW", "1 + max id", "OUTSIDE the checkpoint format"):
        assert word in " ".join(w for w in doc.split() if w != "*"), word
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "map_kernel.hip" in build.SOURCES and "capi_map.cpp" in build.SOURCES and "map_kernel.h" in build.HEADERS
    for name in ("remove_landmarks", "map_tally", "map_prune", "map_track", "step_managed", "manage_run", "last_map_work"):
        assert callable(getattr(filters.BatchedEKF, name)), name
        assert not hasattr(filters.BatchedUKF, name), name
    assert callable(S.map_instance_host) and S.MapConfig is MapConfig and S.MapResult.REC_MAP_MOVED == 2


def test_default_config_and_struct_layout(tmp_path):
    import subprocess
    L = _lib.lib()
    c = MapConfig()
    assert L.slam_map_config_default(C.byref(c)) == 0
    assert (c.range_shrink, c.fov_margin, c.min_expected, c.min_ratio, c.prune_every) == (0.9, 0.1, 10, 0.3, 10)
    d = default_map_config()
    assert all(getattr(d, name) == getattr(c, name) for name, _ in MapConfig._fields_)
    assert L.slam_map_config_default(None) == ERR_ARG and "NULL" in _err()
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(slam_map_config), offsetof(slam_map_config, fov_margin),'
                   ' offsetof(slam_map_config, min_expected), offsetof(slam_map_config, min_ratio), offsetof(slam_map_config, prune_every));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(MapConfig), MapConfig.fov_margin.offset, MapConfig.min_expected.offset, MapConfig.min_ratio.offset,
                   MapConfig.prune_every.offset]


def _calls(cfg=None, mask=True, meas=True, count=True, k_stride=2, cmds=True, T=1, acfg=None):
    """Every entry point that takes a handle, on a NULL handle with tiny host arrays standing in for every pointer: name -> return code."""
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32); r = np.zeros((1, 4), np.int32)
    cfgp = None if cfg is None else C.byref(cfg)
    ap = None if acfg is None else C.byref(acfg)
    fp = (lambda a, on: a.ctypes.data_as(_lib._fp) if on else None)
    ip = (lambda a, on: a.ctypes.data_as(_lib._ip) if on else None)
    vp = (lambda a, on: C.c_void_p(a.ctypes.data) if on else None)
    out = {}
    out["slam_remove_landmarks"] = (L.slam_remove_landmarks(None, ip(r, mask), None, None), _err())
    out["slam_remove_landmarks_dev"] = (L.slam_remove_landmarks_dev(None, vp(r, mask), None, None), _err())
    out["slam_map_tally"] = (L.slam_map_tally(None, cfgp, fp(m, meas), ip(n, count), k_stride, None), _err())
    out["slam_map_tally_dev"] = (L.slam_map_tally_dev(None, cfgp, vp(m, meas), vp(n, count), k_stride, None), _err())
    out["slam_map_prune"] = (L.slam_map_prune(None, cfgp, None, None), _err())
    out["slam_step_managed"] = (L.slam_step_managed(None, ap, cfgp, fp(c, cmds), 0, fp(m, meas), ip(n, count), k_stride, None, None), _err())
    out["slam_step_managed_dev"] = (L.slam_step_managed_dev(None, ap, cfgp, vp(c, cmds), 0, vp(m, meas), vp(n, count), k_stride, None, None), _err())
    out["slam_manage_run"] = (L.slam_manage_run(None, ap, cfgp, fp(c, cmds), 0, fp(m, meas), ip(n, count), k_stride, T, None, None, None, None,
                                                None, None), _err())
    return out


WITH_CONFIG = ("slam_map_tally", "slam_map_tally_dev", "slam_map_prune", "slam_step_managed", "slam_step_managed_dev", "slam_manage_run")
WITH_MESSAGE = ("slam_map_tally", "slam_map_tally_dev", "slam_step_managed", "slam_step_managed_dev", "slam_manage_run")
WITH_COMMANDS = ("slam_step_managed", "slam_step_managed_dev", "slam_manage_run")


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_config_checks_come_before_the_handle(field, value):
    cfg = default_map_config()
    setattr(cfg, field, value)
    got = _calls(cfg=cfg)
    for fn in WITH_CONFIG:
        assert got[fn][0] == ERR_ARG and "map config" in got[fn][1] and field in got[fn][1], (fn, got[fn])
    x = np.zeros(3); P = np.eye(3).ravel().copy(); ids = np.zeros(4, np.int32)
    rc = _lib.lib().slam_map_instance_host(x.ctypes.data_as(_lib._dp), P.ctypes.data_as(_lib._dp), ids.ctypes.data_as(_lib._ip), 0, 4, 0, None, 0, 1,
                                           0, 3.0, -1.57, 1.57, 0, C.byref(cfg), None, None, None, 0, None, None)
    assert rc == ERR_ARG and "map config" in _err()


def test_the_limits_of_the_config_are_allowed():
    for cfg in (MapConfig(1.0, 0.0, 1, 0.0, 1), MapConfig(1e-9, 5.0, 2 ** 31 - 1, 1.0, 2 ** 31 - 1), MapConfig(0.5, float("inf"), 3, 0.5, 7)):
        got = _calls(cfg=cfg)
        for fn in WITH_CONFIG:
            assert got[fn][0] == ERR_ARG and "NULL handle" in got[fn][1], (fn, got[fn])


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    got = _calls()
    for fn, (rc, text) in got.items():
        assert rc == ERR_ARG and "NULL handle" in text, (fn, text)
    got = _calls(mask=False)
    for fn in ("slam_remove_landmarks", "slam_remove_landmarks_dev"):
        assert got[fn][0] == ERR_ARG and "remove is NULL" in got[fn][1], (fn, got[fn])
    for kw, word in ((dict(meas=False), "meas"), (dict(count=False), "meas"), (dict(k_stride=0), "k_stride"), (dict(k_stride=-3), "k_stride")):
        got = _calls(**kw)
        for fn in WITH_MESSAGE:
            assert got[fn][0] == ERR_ARG and word in got[fn][1] and "NULL handle" not in got[fn][1], (fn, kw, got[fn])
    got = _calls(cmds=False)
    for fn in WITH_COMMANDS:
        assert got[fn][0] == ERR_ARG and "cmds" in got[fn][1], (fn, got[fn])
    got = _calls(acfg=AssocConfig(30.0, 9.0))
    for fn in WITH_COMMANDS:
        assert got[fn][0] == ERR_ARG and "assoc config" in got[fn][1], (fn, got[fn])
    assert _calls(T=-1)["slam_manage_run"][0] == ERR_ARG and "negative" in _err()
    assert L.slam_map_get_track(None, None, None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_map_track_reset(None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_last_map_work(None, None, None, None) == ERR_ARG and "NULL handle" in _err()


def test_argument_checks_of_the_host_hook():
    L = _lib.lib()
    d = (lambda a: None if a is None else a.ctypes.data_as(_lib._dp))
    i = (lambda a: None if a is None else a.ctypes.data_as(_lib._ip))

    def call(**over):
        a = dict(x=np.zeros(5), P=np.eye(5).ravel().copy(), ids=np.array([3, 0, 0, 0], np.int32), M=1, L_max=4, meas=None, k_stride=1,
                 seen=None, expected=None, remove=None, prune=0)
        a.update(over)
        return L.slam_map_instance_host(d(a["x"]), d(a["P"]), i(a["ids"]), a["M"], a["L_max"], 0,
                                        None if a["meas"] is None else a["meas"].ctypes.data_as(_lib._fp), 0, a["k_stride"], 0, 3.0, -1.57, 1.57,
                                        0, None, i(a["seen"]), i(a["expected"]), i(a["remove"]), a["prune"], None, None)
    z = np.zeros(4, np.int32)
    assert call() == 0                                     # nothing to do; every output may be NULL
    for key in ("x", "P", "ids"):
        assert call(**{key: None}) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", 0), ("L_max", 1001)):
        assert call(**{key: value}) == ERR_ARG, (key, value)
    m = np.zeros((1, 3), np.float32)
    assert call(meas=m) == ERR_ARG and "seen" in _err()     # a tally needs the counters
    assert call(prune=1) == ERR_ARG and "seen" in _err()    # and so does the prune rule
    assert call(seen=z.copy()) == ERR_ARG and "together" in _err()
    assert call(meas=m, seen=z.copy(), expected=z.copy(), k_stride=0) == ERR_ARG and "k_stride" in _err()
    assert call(meas=m, seen=z.copy(), expected=z.copy()) == 0
    assert call(remove=np.array([1], np.int32)) == 0        # a removal needs no counters


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    m = np.zeros((3, 2, 3), np.float32); n = np.zeros(3, np.int32)
    calls = (lambda: f.remove_landmarks(np.zeros((3, 4), np.int32)), lambda: f.map_tally(m, n), f.map_prune, f.map_track, f.last_map_work,
             lambda: f.step_managed((0.1, 0.0), m, n), lambda: f.manage_run(np.zeros((2, 2)), np.zeros((2, 3, 2, 3)), np.zeros((2, 3))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
