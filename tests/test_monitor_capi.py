"""The run monitor (slam_monitor_*, include/slam_batch.h) without a GPU: the entry points exist and are mirrored, the argument checks that
need no device return their code with a text, the per-instance function compiled for the host (slam_monitor_instance_host: the kernel's own
source) agrees with tests/monitor_reference.py - err_pos and err_yaw bit for bit, flags and NaN patterns exactly, nees_pose by the
project's judging rule (consistency_reference.judge, n = 3: bar = min(10 G, 4)), every instance judged - and monitor_summary on hand-made
records."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import consistency_reference as R
import monitor_reference as MR
from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import MonitorConfig, default_monitor_config, EKF_SLAM, UKF_SLAM, UKF_LOC
from test_cholesky_highprec import cholesky_hp, spd_graded, spd_with_condition

ERR_ARG = -1
SYMBOLS = ("slam_monitor_config_default", "slam_monitor_now", "slam_monitor_run", "slam_last_monitor_work", "slam_monitor_instance_host")
TRUTH = np.array([0.5, -0.3, 0.2 + 2 * R.TWO_PI])   # (the simulator's heading is not wrapped)


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    doc = header.split("---- run monitor")[1].split("typedef struct slam_monitor_config")[0]
    assert "Not covered:" in doc and "UKF" in doc.split("Not covered:")[1] and "slam_multi_" in doc.split("Not covered:")[1]
    assert "depend on which instances share the batch" in " ".join(doc.split())
    cons = header.split("---- consistency")[1].split("enum slam_consistency_flags")[0]
    assert "inside the step kernels" not in cons and "run monitor" in cons
    assert re.search(r"SLAM_MONITOR_SHARED = 0, SLAM_MONITOR_EACH = 1, SLAM_MONITOR_NAV = 2", header)
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    assert "MonitorNow monitorNow(" in hpp and "MonitorRun monitorRun(" in hpp and "slam_monitor_run(h_" in hpp
    drv = open(os.path.join(ROOT, "live_ekf_slam_amd", "csrc", "host", "filter_driver.cpp")).read()
    assert 'mode == "monitor"' in drv
    from live_ekf_slam_amd import build, filters
    assert "monitor_kernel.hip" in build.SOURCES and "monitor_kernel.h" in build.HEADERS
    for name in ("monitor_now", "monitor_run", "last_monitor_work"):
        assert callable(getattr(filters.BatchedFilter, name))
    assert callable(filters.monitor_summary)
    assert filters.MonitorResult.REC_N_OK == 0 and filters.MonitorResult.REC_SUM_NEES_POSE == 9 and filters.MonitorResult.REC_SUM_DOF == 15


def _chi2_cdf_3(x):
    """The chi-square distribution function for 3 degrees of freedom in closed form."""
    return math.erf(math.sqrt(x / 2)) - math.sqrt(2 * x / math.pi) * math.exp(-x / 2)


def test_default_config():
    L = _lib.lib()
    c = MonitorConfig()
    assert L.slam_monitor_config_default(C.byref(c)) == 0
    assert (c.nees_lo, c.nees_hi, c.full_every) == (0.21579528262389785, 9.348403604496148, 0)
    assert bytes(default_monitor_config())[:20] == bytes(c)[:20]
    assert (MR.NEES_LO, MR.NEES_HI) == (c.nees_lo, c.nees_hi)
    assert L.slam_monitor_config_default(None) == ERR_ARG and "NULL" in _err()
    # the constants are the 0.025 and 0.975 quantiles for 3 degrees of freedom (closed-form distribution function)
    assert abs(_chi2_cdf_3(c.nees_lo) - 0.025) < 1e-13 and abs(_chi2_cdf_3(c.nees_hi) - 0.975) < 1e-13
    # filters.chi2_quantile states its accuracy from 30 degrees of freedom on and refuses below (6.5 % at 7), which is why the band of
    # ONE instance is a pair of constants; the band of the batch MEAN (monitor_summary) is where it serves.  Where it is defined it agrees
    # with the exact quantiles to the 0.31 % it states: the sum of ten instances' NEES has 30 degrees of freedom
    from live_ekf_slam_amd.filters import chi2_quantile
    with pytest.raises(ValueError, match="refused below 30"):
        chi2_quantile(0.025, 3)
    for p, exact in zip(R.CHI2_P, R.CHI2_TABLE[30]):
        assert abs(chi2_quantile(p, 30) - exact) <= 0.0031 * exact


def _run(cfg=None, source=0, cmds=True, T=1, h=None):
    L = _lib.lib()
    c = np.zeros((max(T, 1), 2), np.float32)
    return L.slam_monitor_run(h, None if cfg is None else C.byref(cfg), source, c.ctypes.data_as(_lib._fp) if cmds else None, T, None, None, None, None)


@pytest.mark.parametrize("field,value,text", [("nees_lo", float("nan"), "band"), ("nees_hi", float("inf"), "band"), ("nees_lo", 10.0, "band"),
                                              ("nees_hi", -float("inf"), "band"), ("full_every", -1, "full_every")])
def test_config_checks_come_before_the_handle(field, value, text):
    L = _lib.lib()
    cfg = default_monitor_config()
    setattr(cfg, field, value)
    assert _run(cfg) == ERR_ARG and text in _err() and "monitor config" in _err()
    assert L.slam_monitor_now(None, C.byref(cfg), None, None, None, None, None) == ERR_ARG and text in _err()


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    assert _run(source=3) == ERR_ARG and "source" in _err()
    assert _run(source=-1) == ERR_ARG and "source" in _err()
    assert _run(T=-1) == ERR_ARG and "negative" in _err()
    assert _run(cmds=False, source=0) == ERR_ARG and "cmds" in _err()
    assert _run(cmds=False, source=1) == ERR_ARG and "cmds" in _err()
    assert _run(cmds=False, source=2) == ERR_ARG and "NULL handle" in _err()      # NAV takes no commands: the next check is the handle
    assert _run() == ERR_ARG and "NULL handle" in _err()
    assert _run(default_monitor_config()) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_monitor_now(None, None, None, None, None, None, None) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_last_monitor_work(None, None, None) == ERR_ARG and "NULL handle" in _err()
    x = np.zeros(4); P = np.eye(3).ravel()
    dp = _lib._dp
    assert L.slam_monitor_instance_host(7, x.ctypes.data_as(dp), P.ctypes.data_as(dp), TRUTH.ctypes.data_as(dp), 0, None, None, None, None) == ERR_ARG
    assert "kind" in _err()
    assert L.slam_monitor_instance_host(EKF_SLAM, None, P.ctypes.data_as(dp), TRUTH.ctypes.data_as(dp), 0, None, None, None, None) == ERR_ARG
    assert L.slam_monitor_instance_host(EKF_SLAM, x.ctypes.data_as(dp), None, TRUTH.ctypes.data_as(dp), 0, None, None, None, None) == ERR_ARG
    assert L.slam_monitor_instance_host(UKF_SLAM, x.ctypes.data_as(dp), None, TRUTH.ctypes.data_as(dp), 0, None, None, None, None) == 0
    assert L.slam_monitor_instance_host(EKF_SLAM, x.ctypes.data_as(dp), P.ctypes.data_as(dp), TRUTH.ctypes.data_as(dp), 0, None, None, None, None) == 0


def test_the_mirror_needs_a_handle():
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    for call in (f.monitor_now, lambda: f.monitor_run(np.zeros((2, 2))), f.last_monitor_work):
        with pytest.raises(_lib.SlamError, match="readParams"):
            call()


def _host(kind, x, P3, truth, status=0):
    L = _lib.lib()
    x = np.ascontiguousarray(x, dtype=np.float64); truth = np.ascontiguousarray(truth, dtype=np.float64)
    P3 = None if P3 is None else np.ascontiguousarray(P3, dtype=np.float64)
    v = [C.c_double(0), C.c_double(0), C.c_double(0)]
    fl = C.c_int32(-1)
    rc = L.slam_monitor_instance_host(kind, x.ctypes.data_as(_lib._dp), None if P3 is None else P3.ctypes.data_as(_lib._dp),
                                      truth.ctypes.data_as(_lib._dp), status, C.byref(v[0]), C.byref(v[1]), C.byref(v[2]), C.byref(fl))
    assert rc == 0, _err()
    return v[0].value, v[1].value, v[2].value, fl.value


def _bits(v):
    return np.float64(v).tobytes()


def _check(kind, x, P3, truth, status, ukf):
    """host hook against the helper: err_pos, err_yaw bit for bit, flags and the NaN pattern exactly; returns (device value, reference)."""
    dev = _host(kind, x, P3, truth, status)
    ref = MR.instance(x, P3, truth, status, ukf)
    assert dev[3] == ref["flags"], (dev, ref["flags"])
    assert _bits(dev[0]) == _bits(ref["err_pos"]) and _bits(dev[1]) == _bits(ref["err_yaw"]), (dev, ref["err_pos"], ref["err_yaw"])
    assert math.isnan(dev[2]) == bool(np.isnan(ref["nees_pose"])), (dev, ref["nees_pose"])
    return dev, ref


def _draw(rng, S, truth=TRUTH, f32=False):
    e = rng.standard_normal(3) * np.sqrt(np.abs(np.diag(S)))
    x = truth + e
    P = S
    if f32:
        x = x.astype(np.float32).astype(np.float64)
        P = S.astype(np.float32).astype(np.float64)
        assert cholesky_hp(0.5 * (P + P.T))[0] is not None
    return x, P


def test_instance_function_against_the_reference():
    rng = np.random.default_rng(20261)
    pools = {}
    per = 48
    families = [("k1e1", lambda: spd_with_condition(rng, 3, 1e1), False), ("k1e4", lambda: spd_with_condition(rng, 3, 1e4), False),
                ("k1e8", lambda: spd_with_condition(rng, 3, 1e8), False), ("graded", lambda: spd_graded(rng, 3), False),
                ("small", lambda: spd_with_condition(rng, 3, 1e3, top=1e-4), False),
                ("f32 k1e1", lambda: spd_with_condition(rng, 3, 1e1), True), ("f32 k1e4", lambda: spd_with_condition(rng, 3, 1e4), True)]
    for name, make, f32 in families:
        for _ in range(per):
            x, P = _draw(rng, make(), f32=f32)
            dev, ref = _check(EKF_SLAM, x, P, TRUTH, 0, False)
            assert dev[3] == 0
            pools.setdefault(name, []).append((dev[2], ref["nees_pose"], ref["S"], ref["e"], ref["z"]))
    # P asymmetric by a skew part of relative size 1e-10: the value is that of (P + P^T) / 2
    for _ in range(per):
        Y = spd_with_condition(rng, 3, 1e3)
        K = np.triu(rng.standard_normal((3, 3)), 1) * 1e-10 * np.abs(Y)
        x, _ = _draw(rng, Y)
        P = Y + K - K.T
        assert not np.array_equal(P, P.T)
        dev, ref = _check(EKF_SLAM, x, P, TRUTH, 0, False)
        pools.setdefault("skew", []).append((dev[2], ref["nees_pose"], ref["S"], ref["e"], ref["z"]))
    # headings on both sides of the wrap, a truth many turns away
    for k in range(per):
        Y = spd_with_condition(rng, 3, 1e2)
        truth = np.array([rng.uniform(-9, 9), rng.uniform(-9, 9), rng.uniform(-math.pi, math.pi) + R.TWO_PI * int(rng.integers(-40, 40))])
        x, _ = _draw(rng, Y, truth=truth)
        x[2] = math.remainder(x[2] + (math.pi if k % 2 else 0.0), R.TWO_PI)
        dev, ref = _check(EKF_SLAM, x, Y, truth, 0, False)
        assert abs(dev[1]) <= math.pi
        pools.setdefault("wrap", []).append((dev[2], ref["nees_pose"], ref["S"], ref["e"], ref["z"]))
    bad = []
    for name in sorted(pools):
        pool = pools[name]
        assert len(pool) >= 30
        G, gd, bar, over = R.judge(pool)
        print(f"[monitor] host pool {name!r}: {len(pool)} instances, G = {G:.3g}, host-compiled kernel max g = {gd:.3g}, bar = {bar:.3g}")
        assert G <= R.CAP, (name, G)       # the pool keeps the three fp64 routes themselves under the cap
        if over:
            bad.append((name, len(over), gd, bar))
    assert not bad, f"pools above their bar (name, instances over, max g, bar): {bad}"


def test_instance_function_flags_and_nan_patterns():
    rng = np.random.default_rng(20262)
    Y = spd_with_condition(rng, 3, 1e2)
    x, _ = _draw(rng, Y)
    # an indefinite block at each pivot
    for k in range(3):
        for dk in (-1e-6, 0.0):
            S = R.not_pd_matrix(rng, 3, k, dk) if dk else None
            if S is None:
                S = Y.copy(); S[k, :] = 0.0; S[:, k] = 0.0
            dev, ref = _check(EKF_SLAM, x, S, TRUTH, 0, False)
            assert dev[3] == MR.POSE_NOT_PD and math.isnan(dev[2]) and math.isfinite(dev[0]) and math.isfinite(dev[1]), (k, dk, dev)
    # a non-finite entry of the block
    for idx in ((0, 0), (1, 0), (2, 1), (2, 2)):
        for bad in (np.nan, np.inf):
            S = Y.copy(); S[idx] = bad
            dev, _ = _check(EKF_SLAM, x, S, TRUTH, 0, False)
            assert dev[3] == MR.POSE_NOT_PD and math.isnan(dev[2]) and math.isfinite(dev[0])
    # a NaN or infinite state, a NaN truth: INSTANCE_FAILED, everything NaN
    for i in range(3):
        for bad in (np.nan, np.inf, -np.inf):
            xb = x.copy(); xb[i] = bad
            dev, _ = _check(EKF_SLAM, xb, Y, TRUTH, 0, False)
            assert dev[3] == MR.INSTANCE_FAILED and all(math.isnan(v) for v in dev[:3])
        tb = TRUTH.copy(); tb[i] = np.nan
        dev, _ = _check(EKF_SLAM, x, Y, tb, 0, False)
        assert dev[3] == MR.INSTANCE_FAILED and all(math.isnan(v) for v in dev[:3])
    # status: NONFINITE and WATCHDOG leave an undefined state; the other bits a valid one
    for status, failed in ((R.NONFINITE, True), (R.WATCHDOG, True), (R.NONFINITE | 4, True), (2, False), (4, False), (8, False), (16, False)):
        dev, _ = _check(EKF_SLAM, x, Y, TRUTH, status, False)
        assert (dev[3] == MR.INSTANCE_FAILED) == failed and math.isnan(dev[0]) == failed
    # the UKF kinds: errors from (x, y, cos yaw, sin yaw), no NEES
    for kind in (UKF_SLAM, UKF_LOC):
        for _ in range(64):
            yaw = rng.uniform(-math.pi, math.pi)
            r = rng.uniform(0.7, 1.3)                                   # (the UKF does not keep (cos, sin) on the unit circle)
            xu = np.array([rng.uniform(-9, 9), rng.uniform(-9, 9), r * math.cos(yaw), r * math.sin(yaw)])
            truth = np.array([xu[0] + rng.normal(0, 0.1), xu[1] + rng.normal(0, 0.1), yaw + rng.normal(0, 0.05) + R.TWO_PI * int(rng.integers(-3, 3))])
            dev, ref = _check(kind, xu, None, truth, 0, True)
            assert dev[3] == 0 and math.isnan(dev[2]) and abs(dev[1]) < 0.5
        dev, _ = _check(kind, np.array([0.0, 0.0, np.nan, 1.0]), None, TRUTH, 0, True)
        assert dev[3] == MR.INSTANCE_FAILED
        dev, _ = _check(kind, np.array([0.0, 0.0, 1.0, 0.0]), None, TRUTH, R.WATCHDOG, True)
        assert dev[3] == MR.INSTANCE_FAILED


def test_err_pos_is_the_wire_format_error():
    """err_pos is formed from the float32 wire values of x and y (the summand of the handle's error sum), e of the NEES from the fp64 state."""
    x = np.array([1.0 + 2.0 ** -30, -2.0 - 2.0 ** -29, 0.1])
    truth = np.array([1.0, -2.0, 0.1])
    P = np.diag([2.0 ** -50, 2.0 ** -50, 1.0])
    ep, ey, nees, fl = _host(EKF_SLAM, x, P, truth, 0)
    assert ep == 0.0 and ey == 0.0 and fl == 0           # float32(x) = truth exactly
    assert nees == (2.0 ** -30) ** 2 / 2.0 ** -50 + (2.0 ** -29) ** 2 / 2.0 ** -50


def test_monitor_summary_on_hand_made_records():
    from live_ekf_slam_amd.filters import MonitorResult as M, chi2_quantile, monitor_summary
    r = np.zeros((3, 16))
    # tick 0: 100 instances, all with a NEES
    r[0, M.REC_N_OK], r[0, M.REC_N_NEES] = 100, 100
    r[0, M.REC_SUM_ERR_POS], r[0, M.REC_SUM_ERR_POS2] = 100 * 0.5, 100 * (0.25 + 0.04)        # mean 0.5, standard deviation 0.2
    r[0, M.REC_SUM_ERR_YAW2] = 100 * 0.01
    r[0, M.REC_SUM_NEES_POSE], r[0, M.REC_N_BELOW], r[0, M.REC_N_ABOVE] = 100 * 3.6, 2, 5
    # tick 1: 8 counted instances of 10, 4 with a NEES (too few for the band of the mean)
    r[1, M.REC_N_OK], r[1, M.REC_N_FAILED], r[1, M.REC_N_NEES] = 8, 2, 4
    r[1, M.REC_SUM_ERR_POS], r[1, M.REC_SUM_ERR_POS2] = 8 * 1.0, 8 * 1.0
    r[1, M.REC_SUM_NEES_POSE], r[1, M.REC_N_ABOVE] = 4 * 2.0, 1
    # tick 2: nothing counted
    s = monitor_summary(r, alpha=0.05)
    assert np.allclose(s["mean_err_pos"][:2], [0.5, 1.0]) and np.isnan(s["mean_err_pos"][2])
    assert np.allclose(s["std_err_pos"][:2], [0.2, 0.0]) and np.allclose(s["rms_err_yaw"][0], 0.1)
    assert np.allclose(s["anees"][:2], [3.6, 2.0]) and np.isnan(s["anees"][2])
    assert np.allclose(s["frac_outside"][:2], [0.07, 0.25])
    assert s["n_ok"].tolist() == [100, 8, 0] and s["n_nees"].tolist() == [100, 4, 0]
    assert s["anees_lower"][0] == chi2_quantile(0.025, 300) / 100 and s["anees_upper"][0] == chi2_quantile(0.975, 300) / 100
    assert s["anees_lower"][0] < 3.0 < s["anees_upper"][0] < 3.6          # ANEES 3.6 over 100 instances is outside the 95 % band
    assert np.isnan(s["anees_lower"][1]) and np.isnan(s["anees_upper"][2])
    one = monitor_summary(r[0])
    assert one["anees"].shape == (1,) and one["anees"][0] == s["anees"][0]
    with pytest.raises(ValueError):
        monitor_summary(np.zeros((2, 15)))
