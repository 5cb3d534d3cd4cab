"""Landmark merging (slam_map_duplicates, slam_merge_landmarks, slam_map_merge, slam_manage_merge_run; include/slam_batch.h) without a
GPU: the entry points exist, are declared and mirrored with matching argument counts, the build lists the new files, the struct layout is
the compiler's, the defaults are the documented ones, and every SLAM_ERR_ARG path returns its code with a text before the handle is looked
at."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import AssocConfig, MapConfig, MergeConfig, default_merge_config

ERR_ARG = -1
SYMBOLS = ("slam_merge_config_default", "slam_map_duplicates", "slam_map_duplicates_dev", "slam_merge_landmarks", "slam_merge_landmarks_dev",
           "slam_map_merge", "slam_manage_merge_run", "slam_last_merge_work", "slam_merge_instance_host")
BAD_CONFIGS = [("gate_merge", float("nan")), ("gate_merge", float("inf")), ("gate_merge", 0.0), ("gate_merge", -1.0), ("sigma", float("nan")),
               ("sigma", float("inf")), ("sigma", -1e-9), ("merge_every", 0), ("merge_every", -3)]


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
    # the section order: after the map-management declarations, before the closed loop
    assert header.index("int slam_map_instance_host(") < header.index("---- landmark merging") < header.index("int slam_merge_config_default(")
    assert header.index("int slam_merge_instance_host(") < header.index("---- closed loop")
    # map management still says that it does not merge, and points here
    doc = header.split("---- map management")[1].split("typedef struct slam_map_config")[0]
    tail = " ".join(w for w in doc.split("Not covered:")[1].split() if w != "*")
    assert "merging duplicate landmarks" in tail and "landmark merging" in tail and "slam_map_merge" in tail
    doc = " ".join(w for w in header.split("---- landmark merging")[1].split("typedef struct slam_merge_config")[0].split() if w != "*")
    for word in ("l_i - l_j = 0", "exact marginalisation", "nn(i) == j && nn(j) == i", "ties to the lowest slot", "SINGULAR", "ascending i",
                 "before the handle is looked at", "SLAM_ERR_UNSUPPORTED", "Not covered:", "the UKF", "slam_multi_", "joint (multi-pair) updates",
                 "multi-step launches", "counters in checkpoints"):
        assert word in doc, word
    from live_ekf_slam_amd import build, filters
    import live_ekf_slam_amd as S
    assert "merge_kernel.hip" in build.SOURCES and "capi_merge.cpp" in build.SOURCES and "merge_kernel.h" in build.HEADERS
    for name in ("map_duplicates", "merge_landmarks", "map_merge", "manage_merge_run", "last_merge_work"):
        assert callable(getattr(filters.BatchedEKF, name)), name
        assert not hasattr(filters.BatchedUKF, name), name
    assert callable(S.merge_instance_host) and S.MergeConfig is MergeConfig and callable(S.default_merge_config)
    assert S.MergeResult.REC_MERGE_FUSED == 1 and S.MergeResult.REC_MERGE_MAX_D2 == 8


def test_default_config_and_struct_layout(tmp_path):
    L = _lib.lib()
    c = MergeConfig()
    assert L.slam_merge_config_default(C.byref(c)) == 0
    assert (c.gate_merge, c.sigma, c.merge_every) == (-2.0 * math.log(0.05), 0.0, 10)
    assert abs(c.gate_merge - 5.9915) < 1e-4
    d = default_merge_config()
    assert all(getattr(d, name) == getattr(c, name) for name, _ in MergeConfig._fields_)
    assert L.slam_merge_config_default(None) == ERR_ARG and "NULL" in _err()
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\n'
                   'int main(){printf("%zu %zu %zu %zu\\n", sizeof(slam_merge_config), offsetof(slam_merge_config, gate_merge),'
                   ' offsetof(slam_merge_config, sigma), offsetof(slam_merge_config, merge_every));return 0;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [C.sizeof(MergeConfig), MergeConfig.gate_merge.offset, MergeConfig.sigma.offset, MergeConfig.merge_every.offset]
    # slam_map_config is what it was
    assert [n for n, _ in MapConfig._fields_] == ["range_shrink", "fov_margin", "min_expected", "min_ratio", "prune_every"]


def _calls(cfg=None, partner=True, meas=True, count=True, k_stride=2, cmds=True, T=1, acfg=None, mcfg=None):
    """Every entry point that takes a handle, on a NULL handle with tiny host arrays standing in for every pointer: name -> (code, text)."""
    L = _lib.lib()
    c = np.zeros(2, np.float32); m = np.zeros((1, 2, 3), np.float32); n = np.zeros(1, np.int32); r = np.full((1, 4), -1, np.int32)
    cfgp = None if cfg is None else C.byref(cfg)
    ap = None if acfg is None else C.byref(acfg)
    mp = None if mcfg is None else C.byref(mcfg)
    fp = (lambda a, on: a.ctypes.data_as(_lib._fp) if on else None)
    ip = (lambda a, on: a.ctypes.data_as(_lib._ip) if on else None)
    vp = (lambda a, on: C.c_void_p(a.ctypes.data) if on else None)
    out = {}
    out["slam_map_duplicates"] = (L.slam_map_duplicates(None, cfgp, ip(r, partner), None), _err())
    out["slam_map_duplicates_dev"] = (L.slam_map_duplicates_dev(None, cfgp, vp(r, partner), None), _err())
    out["slam_merge_landmarks"] = (L.slam_merge_landmarks(None, cfgp, ip(r, partner), None, None), _err())
    out["slam_merge_landmarks_dev"] = (L.slam_merge_landmarks_dev(None, cfgp, vp(r, partner), None, None), _err())
    out["slam_map_merge"] = (L.slam_map_merge(None, cfgp, None, None), _err())
    out["slam_manage_merge_run"] = (L.slam_manage_merge_run(None, ap, mp, cfgp, fp(c, cmds), 0, fp(m, meas), ip(n, count), k_stride, T, None, None,
                                                            None, None, None, None, None), _err())
    return out


WITH_PARTNER = ("slam_map_duplicates", "slam_map_duplicates_dev", "slam_merge_landmarks", "slam_merge_landmarks_dev")


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_config_checks_come_before_the_handle(field, value):
    cfg = default_merge_config()
    setattr(cfg, field, value)
    for fn, (rc, text) in _calls(cfg=cfg).items():
        assert rc == ERR_ARG and "merge config" in text and field in text, (fn, text)
    x = np.zeros(3); P = np.eye(3).ravel().copy(); ids = np.zeros(4, np.int32)
    rc = _lib.lib().slam_merge_instance_host(x.ctypes.data_as(_lib._dp), P.ctypes.data_as(_lib._dp), ids.ctypes.data_as(_lib._ip), 0, 4, 0, 0,
                                             C.byref(cfg), None, None, None, 1, None, None, None, None)
    assert rc == ERR_ARG and "merge config" in _err()


def test_the_limits_of_the_config_are_allowed():
    for cfg in (MergeConfig(1e-300, 0.0, 1), MergeConfig(1e300, 1e300, 2 ** 31 - 1), MergeConfig(5.99, 0.5, 7)):
        for fn, (rc, text) in _calls(cfg=cfg).items():
            assert rc == ERR_ARG and "NULL handle" in text, (fn, text)


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    for fn, (rc, text) in _calls().items():
        assert rc == ERR_ARG and "NULL handle" in text, (fn, text)
    got = _calls(partner=False)
    for fn in WITH_PARTNER:
        assert got[fn][0] == ERR_ARG and "partner is NULL" in got[fn][1], (fn, got[fn])
    run = "slam_manage_merge_run"
    for kw, word in ((dict(meas=False), "meas"), (dict(count=False), "meas"), (dict(k_stride=0), "k_stride"), (dict(k_stride=-3), "k_stride"),
                     (dict(cmds=False), "cmds"), (dict(T=-1), "negative"), (dict(acfg=AssocConfig(30.0, 9.0)), "assoc config"),
                     (dict(mcfg=MapConfig(0.9, 0.1, 0, 0.3, 10)), "map config")):
        rc, text = _calls(**kw)[run]
        assert rc == ERR_ARG and word in text and "NULL handle" not in text, (kw, text)
    assert L.slam_last_merge_work(None, None, None, None) == ERR_ARG and "NULL handle" in _err()


def test_argument_checks_of_the_host_hook():
    L = _lib.lib()
    d = (lambda a: None if a is None else a.ctypes.data_as(_lib._dp))
    i = (lambda a: None if a is None else a.ctypes.data_as(_lib._ip))

    def call(**over):
        a = dict(x=np.zeros(5), P=np.eye(5).ravel().copy(), ids=np.array([3, 0, 0, 0], np.int32), M=1, L_max=4, seen=None, expected=None, partner=None)
        a.update(over)
        return L.slam_merge_instance_host(d(a["x"]), d(a["P"]), i(a["ids"]), a["M"], a["L_max"], 0, 0, None, i(a["seen"]), i(a["expected"]),
                                          i(a["partner"]), 1, None, None, None, None)
    z = np.zeros(4, np.int32)
    assert call() == 0                                     # nothing to do; every output may be NULL
    for key in ("x", "P", "ids"):
        assert call(**{key: None}) == ERR_ARG, key
    for key, value in (("M", -1), ("M", 5), ("L_max", 0), ("L_max", 1001)):
        assert call(**{key: value}) == ERR_ARG, (key, value)
    assert call(seen=z.copy()) == ERR_ARG and "together" in _err()
    assert call(seen=z.copy(), expected=z.copy()) == 0
    assert call(partner=np.array([7, -5, 0, 2], np.int32)) == 0   # entries out of range are ignored, not followed


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    calls = (f.map_duplicates, lambda: f.merge_landmarks(np.full((3, 4), -1, np.int32)), f.map_merge, f.last_merge_work,
             lambda: f.manage_merge_run(np.zeros((2, 2)), np.zeros((2, 3, 2, 3)), np.zeros((2, 3))))
    for call in calls:
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()
