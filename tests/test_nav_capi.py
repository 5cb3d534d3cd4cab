"""slam_nav_* argument checks and configuration through the C ABI that need no device."""
import ctypes as C

import numpy as np
import pytest

from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import NavConfig, default_nav_config, NAV_PP, NAV_DIRECT, NAV_LOOSE

ERR_ARG, ERR_IO = -1, -5
dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)


def _tick(cfg, pts, est=(0.0, 0.0, 0.0), head=0):
    L = _lib.lib()
    pts = np.ascontiguousarray(pts, dtype=np.float64)
    e = np.array(est, np.float32); cmd = np.zeros(2, np.float32)
    h, f, i, p = C.c_int32(head), C.c_int32(-1), C.c_double(0), C.c_double(0)
    rc = L.slam_nav_tick_host(C.byref(cfg), 0.1, 0.0546, pts.ctypes.data_as(dp), pts.shape[0], e.ctypes.data_as(fp), 0, 0,
                              C.byref(h), C.byref(f), C.byref(i), C.byref(p), cmd.ctypes.data_as(fp))
    return rc, cmd, h.value, f.value


def test_default_config_is_the_reference_yaml():
    L = _lib.lib()
    c = NavConfig()
    assert L.slam_nav_config_default(C.byref(c)) == 0
    assert (c.dt, c.lookahead_dist_init, c.lookahead_dist_max, c.method, c.control) == (0.05, 0.2, 2.0, NAV_PP, NAV_LOOSE)
    d = default_nav_config()
    assert bytes(d) == bytes(c)
    assert L.slam_nav_config_default(None) == ERR_ARG


def test_load_config(tmp_path):
    L = _lib.lib()
    p = tmp_path / "params.yaml"
    p.write_text("dt: 0.1 # period\nmap:\n  bound: 10.0\npath_planning:\n  local_planner_dist: 1.8\n  nav_method: \"direct\" # nav function\n"
                 "  lookahead_dist_init: 0.3 # meters\n  lookahead_dist_max: 4 # meters\n")
    c = default_nav_config()
    assert L.slam_nav_config_load(C.byref(c), str(p).encode()) == 0
    assert (c.dt, c.lookahead_dist_init, c.lookahead_dist_max, c.method, c.control) == (0.1, 0.3, 4.0, NAV_DIRECT, NAV_LOOSE)
    p.write_text("path_planning:\n  nav_method: simple\n")
    c = default_nav_config()
    assert L.slam_nav_config_load(C.byref(c), str(p).encode()) == 0 and c.method == NAV_DIRECT and c.dt == 0.05
    p.write_text("path_planning:\n  nav_method: \"teleport\"\n")
    assert L.slam_nav_config_load(C.byref(c), str(p).encode()) == ERR_IO
    assert L.slam_nav_config_load(C.byref(c), str(tmp_path / "missing.yaml").encode()) == ERR_IO
    assert L.slam_nav_config_load(None, str(p).encode()) == ERR_ARG


def test_path_checks():
    cfg = default_nav_config()
    assert _tick(cfg, [[1.0, 0.0], [2.0, 0.0]])[0] == 0
    assert _tick(cfg, [[1.0, 0.0], [1.0, 0.0], [2.0, 0.0]])[0] == ERR_ARG        # consecutive equal waypoints
    assert b"equal" in _lib.lib().slam_last_error()
    assert _tick(cfg, [[1.0, 0.0], [2.0, 0.0], [1.0, 0.0]])[0] == 0              # equal but not consecutive: a path may revisit a point
    big = np.stack([np.arange(1025.0), np.zeros(1025)], axis=1)
    assert _tick(cfg, big)[0] == ERR_ARG and _tick(cfg, big[:1024])[0] == 0      # P > 1024
    assert _tick(cfg, [[np.inf, 0.0]])[0] == ERR_ARG
    assert _tick(cfg, np.zeros((0, 2)))[0] == ERR_ARG


@pytest.mark.parametrize("field,value", [("dt", 0.0), ("dt", float("nan")), ("lookahead_dist_init", 0.0), ("lookahead_dist_init", 1e-30),
                                         ("lookahead_dist_max", float("inf")), ("method", 2), ("control", -1)])
def test_config_checks(field, value):
    cfg = default_nav_config()
    setattr(cfg, field, value)
    assert _tick(cfg, [[1.0, 0.0]])[0] == ERR_ARG


def test_empty_queue_and_nonfinite_estimate():
    cfg = default_nav_config()
    rc, cmd, head, fin = _tick(cfg, [[1.0, 0.0]], head=1)
    assert rc == 0 and not cmd.any() and fin == 0
    rc, cmd, head, fin = _tick(cfg, [[1.0, 0.0]], est=(float("nan"), 0.0, 0.0))
    assert rc == 0 and not cmd.any() and head == 0 and fin == -1
