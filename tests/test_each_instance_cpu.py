"""Heterogeneous batches (include/slam_batch.h, slam_*_each) without a GPU: the library exports the six entry points with the
bindings the header declares, NULL handles are refused, and the Python mirrors check shapes before anything reaches the library."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib

EACH = {"slam_init_each": 3, "slam_set_maps": 4, "slam_step_each": 5, "slam_step_each_dev": 5, "slam_run_sim_each": 3,
        "slam_predict_each": 2}


def test_each_entry_points_exported_and_bound():
    L = _lib.lib()
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "slam_batch.h")).read(), flags=re.S)
    for name, nargs in EACH.items():
        assert hasattr(L, name), name
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", txt)
        assert m, f"{name} is not declared in slam_batch.h"
        assert len(m.group(1).split(",")) == nargs == len(_lib.SIGNATURES[name][1]), name


def test_each_entry_points_refuse_null_handle():
    L = _lib.lib()
    f2 = (C.c_float * 2)()
    d = (C.c_double * 6)()
    i = (C.c_int32 * 2)(1, 1)
    assert L.slam_init_each(None, C.cast(f2, C.POINTER(C.c_float)), None) == -1
    assert L.slam_set_maps(None, C.cast(d, C.POINTER(C.c_double)), C.cast(i, C.POINTER(C.c_int32)), 1) == -1
    assert L.slam_step_each(None, C.cast(f2, C.POINTER(C.c_float)), C.cast(f2, C.POINTER(C.c_float)), C.cast(i, C.POINTER(C.c_int32)), 1) == -1
    assert L.slam_step_each_dev(None, None, None, None, 1) == -1
    assert L.slam_run_sim_each(None, C.cast(f2, C.POINTER(C.c_float)), 1) == -1
    assert L.slam_predict_each(None, C.cast(f2, C.POINTER(C.c_float))) == -1


class _NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"the library was called ({name}) although the arguments were malformed")


@pytest.fixture
def fake(monkeypatch):
    """A filter object with a (fake) handle whose library must not be reached."""
    import live_ekf_slam_amd as S
    monkeypatch.setattr(_lib, "lib", lambda: _NoLib())
    made = []

    def mk(cls, B=4):
        f = cls(B, 20) if cls is not S.BatchedUKFLoc else cls(B)
        f.h = C.c_void_p(1)
        f.isInit = True
        made.append(f)
        return f
    yield S, mk
    for f in made:
        f.h = None


def test_mirrors_reject_wrong_shapes(fake):
    S, mk = fake
    for cls in (S.BatchedEKF, S.BatchedUKF):
        f = mk(cls, 4)
        with pytest.raises(ValueError):
            f.init(np.zeros((3, 3)))                                  # one row short
        with pytest.raises(ValueError):
            f.init(np.zeros((4, 3)), truth0=np.zeros((4, 2)))
        with pytest.raises(ValueError):
            f.set_map(np.zeros((3, 10, 2)))                           # batch 4
        with pytest.raises(ValueError):
            f.set_map(np.zeros((4, 10, 2)), counts=[10, 10, 11, 10])  # a count above L_stride
        with pytest.raises(ValueError):
            f.set_map(np.zeros((4, 10, 2)), counts=[10, 0, 10, 10])   # an empty map
        with pytest.raises(ValueError):
            f.set_map([np.zeros((5, 2))] * 3)                         # three maps for four instances
        with pytest.raises(ValueError):
            f.set_map(np.zeros((10, 3)))
        with pytest.raises(ValueError):
            f.run_sim(np.zeros((7, 3, 2), np.float32))                # (T, batch, 2) with the wrong batch
        with pytest.raises(ValueError):
            f.run_sim(np.zeros((7, 3), np.float32))
        with pytest.raises(ValueError):
            f.update_sim(np.zeros((3, 2), np.float32))
        with pytest.raises(ValueError):
            f.update(np.zeros((5, 2), np.float32), np.zeros((4, 2, 3), np.float32), np.zeros(4, np.int32))
        with pytest.raises(ValueError):
            f.update(np.zeros((4, 2), np.float32), np.zeros((4, 2, 3), np.float32), np.zeros(3, np.int32))
        with pytest.raises(ValueError):
            f.update_dev(np.zeros((4, 2), np.float32), 0, 0, 1)     # per-instance device commands: update_dev_each
    u = mk(S.BatchedUKF, 4)
    with pytest.raises(ValueError):
        u.predictionStage(np.zeros((2, 2), np.float32))
