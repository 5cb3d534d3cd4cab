"""Heterogeneous pose-graph batches (pgs_*_each, include/slam_pgs.h) without a GPU: the library exports the entry points, the Python
mirror's shape dispatch rejects wrong shapes before any native call, and nothing falls back to a CPU path."""
import ctypes as C
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("pgs_init_each", "pgs_set_maps", "pgs_update_each", "pgs_update_each_dev", "pgs_run_sim_each", "pgs_run_sim_every_iteration_each")


def test_library_exports_the_entry_points():
    from live_ekf_slam_amd import _lib
    L = _lib.lib()
    for name in SYMBOLS:
        assert name in _lib.SIGNATURES and getattr(L, name) is not None, name
    header = open(os.path.join(ROOT, "include", "slam_pgs.h")).read()
    for name in SYMBOLS:
        assert f"int {name}(pgs_handle* h" in header, name


def test_null_handle_is_an_argument_error():
    from live_ekf_slam_amd import _lib
    L = _lib.lib()
    z = np.zeros(8, np.float32); d = np.zeros(8); i = np.ones(4, np.int32)
    fp, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    assert L.pgs_init_each(None, fp(z), None) == -1
    assert L.pgs_set_maps(None, dp(d), ip(i), 1) == -1
    assert L.pgs_update_each(None, fp(z), None, None, 0, None) == -1
    assert L.pgs_update_each_dev(None, None, None, None, 0, None) == -1
    assert L.pgs_run_sim_each(None, fp(z), 1) == -1
    assert L.pgs_run_sim_every_iteration_each(None, fp(z), 1, None) == -1
    assert b"NULL handle" in L.slam_last_error()


class _NoNativeCall:
    """Stands in for the loaded library: any attribute access is a native call that must not happen."""

    def __getattr__(self, name):
        raise AssertionError(f"native call {name} before the shapes were checked")


@pytest.fixture
def pg(monkeypatch):
    """A mirror object that believes it has a handle; its library raises on every use."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    g = S.BatchedPoseGraph(4, num_iterations=50, L_max=6, k_per_pose=4)
    g.h = C.c_void_p(1); g.isInit = True
    monkeypatch.setattr(_lib, "lib", lambda: _NoNativeCall())
    yield g
    g.h = None


def test_shape_dispatch_rejects_wrong_shapes_before_any_native_call(pg):
    B = pg.batch
    for bad in (np.zeros((B + 1, 3)), np.zeros((B, 2)), np.zeros(3), np.zeros((B, 3, 1))):
        with pytest.raises(ValueError):
            pg.init(bad)
    with pytest.raises(ValueError):
        pg.init(np.zeros((B, 3)), truth0=np.zeros((B, 2)))
    with pytest.raises(ValueError):
        pg.init(0.0, 0.0, 0.0, truth0=np.zeros((B + 1, 3)))
    for bad in (np.zeros((B + 1, 5, 2)), np.zeros((B, 5, 3)), np.zeros((B, 0, 2)), np.zeros((B, 256, 2)), np.zeros((0, 2)), np.zeros((5, 3))):
        with pytest.raises(ValueError):
            pg.set_map(bad)
    for counts in (np.ones(B + 1, np.int32), np.array([1, 2, 0, 1]), np.array([1, 2, 6, 1])):
        with pytest.raises(ValueError):
            pg.set_map(np.zeros((B, 5, 2)), counts)
    meas = np.zeros((B, 2, 3), np.float32); cnt = np.zeros(B, np.int32)
    for bad in (np.zeros((B + 1, 2)), np.zeros((B, 3)), np.zeros(3), np.zeros((1, B, 2))):
        with pytest.raises(ValueError):
            pg.update(bad, meas, cnt)
    with pytest.raises(ValueError):
        pg.update(np.zeros((B, 2)), meas, np.zeros(B + 1, np.int32))
    for run in (pg.run_sim, pg.run_sim_every_iteration):
        for bad in (np.zeros((5, B + 1, 2)), np.zeros((5, B, 3)), np.zeros((0, B, 2)), np.zeros((5, 3)), np.zeros((2, 5, B, 2)), np.zeros(0)):
            with pytest.raises(ValueError):
                run(bad)
    assert pg.timestep == 0


def test_the_new_calls_fail_loudly_without_a_device():
    """Without a HIP device there is no handle and every per-instance call raises; nothing computes on the CPU instead."""
    import torch
    import live_ekf_slam_amd as S
    B = 4
    g = S.BatchedPoseGraph(B, num_iterations=20, L_max=6, k_per_pose=4)
    if torch.cuda.is_available():
        g.readParams()          # a device: the handle exists and the same calls are tested in test_pgs_each_gpu.py
        assert g.h is not None
        g.close()
        return
    with pytest.raises(S.SlamError):
        g.readParams()
    assert g.h is None
    calls = (lambda: g.init(np.zeros((B, 3), np.float32)),
             lambda: g.set_map(np.zeros((B, 5, 2)), np.full(B, 5, np.int32)),
             lambda: g.update(np.zeros((B, 2), np.float32), np.zeros((B, 1, 3), np.float32), np.zeros(B, np.int32)),
             lambda: g.run_sim(np.zeros((3, B, 2), np.float32)),
             lambda: g.run_sim_every_iteration(np.zeros((3, B, 2), np.float32)))
    for call in calls:
        with pytest.raises(S.SlamError):
            call()
