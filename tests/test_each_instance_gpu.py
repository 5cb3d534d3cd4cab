"""Heterogeneous batches on the GPU (include/slam_batch.h, slam_*_each): per-instance start poses, maps and commands.

Per-instance rows that are all equal give the bits of the shared calls; instances with their own scenario equal the oracle run of
that scenario; per-instance calls keep call order with the EKF step queue and the tracked instance's shadow."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_golden
from live_ekf_slam_amd.config import default_config
from live_ekf_slam_amd.scenario import make_scenario

pytestmark = pytest.mark.gpu
SEED = 31


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


@pytest.fixture(scope="module")
def hip():
    h = C.CDLL("libamdhip64.so")   # the runtime libslam_hip.so itself links (device buffers without torch)
    h.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    h.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    h.hipFree.argtypes = [C.c_void_p]
    return h


class _Dev:
    """Device copies of host arrays (freed at close)."""

    def __init__(self, hip):
        self.hip, self.ptrs = hip, {}

    def put(self, name, a):
        a = np.ascontiguousarray(a)
        if name not in self.ptrs:
            p = C.c_void_p()
            assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
            self.ptrs[name] = (p, a.nbytes)
        p, cap = self.ptrs[name]
        assert a.nbytes <= cap
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice
        return p.value

    def close(self):
        for p, _ in self.ptrs.values():
            self.hip.hipFree(p)


def _make(S, kind, B, L_max, dtype=0, chol=False):
    if kind == "ekf":
        f = S.BatchedEKF(B, L_max, dtype=dtype).readParams()
    elif kind == "ukf":
        f = S.BatchedUKF(B, L_max).readParams()
    else:
        f = S.BatchedUKFLoc(B).readParams()
    if chol:
        f.set_sqrt_mode("cholesky")
    f.set_seed(SEED)
    return f


def _snapshot(f):
    out = dict(truth=f.truth(), err=f.error_stats(), status=f.status(), M=f.landmark_counts())
    out["states"] = [f.get_state(b) for b in range(f.batch)]
    return out


def _assert_same(a, b):
    assert np.array_equal(a["status"], b["status"]) and np.array_equal(a["M"], b["M"])
    assert np.array_equal(a["truth"], b["truth"]) and np.array_equal(a["err"], b["err"])
    for sa, sb in zip(a["states"], b["states"]):
        assert sa["M"] == sb["M"] and sa["timestep"] == sb["timestep"] and np.array_equal(sa["ids"], sb["ids"])
        assert np.array_equal(sa["x"], sb["x"]) and np.array_equal(sa["P"], sb["P"])


def _assert_state(sg, so):
    assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
    assert np.array_equal(sg["x"], so["x"]), np.abs(sg["x"] - so["x"]).max()
    assert np.array_equal(sg["P"], so["P"]), np.abs(sg["P"] - so["P"]).max()


# ---- 1. broadcast identity ---------------------------------------------------------------------------------------------------------
SIM_CASES = [("ekf", 20, 0, False), ("ekf", 50, 0, False), ("ekf", 200, 0, False), ("ekf", 1000, 0, False),
             ("ekf", 20, 1, False), ("ekf", 50, 1, False),
             ("ukf", 20, 0, False), ("ukf", 50, 0, False), ("ukf", 200, 0, False), ("ukf", 20, 0, True)]


@pytest.mark.parametrize("kind,L_max,dtype,chol", SIM_CASES)
def test_broadcast_identity_sim(S, monkeypatch, kind, L_max, dtype, chol):
    """slam_set_maps / slam_init_each / slam_run_sim_each with equal rows == slam_set_map / slam_init / slam_run_sim, at run chunks 0, 1
    and 7 (chunk edges crossed), and the UKF's run split over streams (global instance index of the second part)."""
    monkeypatch.setenv("SLAM_UKF_SPLIT_MIN", "4")
    B = 6
    L = min(L_max, 60)
    T = 16 if L_max >= 200 else 24
    lm, cmds = make_scenario(400 + L_max, L, T)
    for chunk in ((0, 1, 7) if kind == "ekf" else (0,)):
        a = _make(S, kind, B, L_max, dtype, chol); b = _make(S, kind, B, L_max, dtype, chol)
        a.set_run_chunk(chunk); b.set_run_chunk(chunk)
        a.set_map(lm); a.init(0.0, 0.0, 0.0)
        b.set_map(np.broadcast_to(lm, (B, L, 2))); b.init(np.zeros((B, 3), np.float32))
        a.run_sim(cmds[:T // 2]); a.update_sim(cmds[T // 2]); a.run_sim(cmds[T // 2 + 1:])
        per = np.ascontiguousarray(np.broadcast_to(cmds[:, None, :], (T, B, 2)))
        b.run_sim(per[:T // 2]); b.update_sim(per[T // 2]); b.run_sim(per[T // 2 + 1:])
        _assert_same(_snapshot(a), _snapshot(b))
        assert np.all(a.status() == 0)
        a.close(); b.close()


@pytest.mark.parametrize("kind,L_max,dtype,chol", [c for c in SIM_CASES if c[2] == 0 and c[1] <= 200] + [("loc", 1, 0, False)])
def test_broadcast_identity_ext(S, hip, kind, L_max, dtype, chol):
    """slam_step_each and slam_step_each_dev (UKF: also slam_predict_each + slam_update_dev) with equal command rows == the shared
    calls, on the reference simulator's measurement stream."""
    g = load_golden("sim_seed2_L50_T1000.npz")
    B, T, ks = 5, 40, 6
    a = _make(S, kind, B, L_max, dtype, chol); b = _make(S, kind, B, L_max, dtype, chol)
    if kind == "loc":
        a.set_map(g["map"]); b.set_map(g["map"])
    a.init(0.0, 0.0, 0.0); b.init(np.zeros((B, 3), np.float32))
    dev = _Dev(hip)
    try:
        for t in range(T):
            k = min(int(g["meas_count"][t]), ks)
            meas = np.zeros((B, ks, 3), np.float32); meas[:, :k] = g["meas"][t, :k]
            cnt = np.full(B, k, np.int32)
            cmd = g["cmds"][t].astype(np.float32)
            per = np.ascontiguousarray(np.broadcast_to(cmd, (B, 2)))
            a.update(S.Command(cmd[0], cmd[1]), meas, cnt)
            dm, dc = dev.put("meas", meas), dev.put("cnt", cnt)
            if t % 3 == 0:
                b.update(per, meas, cnt)
            elif t % 3 == 1 or kind == "ekf":
                b.update_dev_each(dev.put("cmds", per), dm, dc, ks)
            else:
                b.predictionStage(per); b.updateStage(dm, dc, ks)
            b.sync()
        _assert_same(_snapshot(a), _snapshot(b))
    finally:
        a.close(); b.close(); dev.close()


# ---- 2. independent scenarios against the oracle -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_independent_scenarios_match_oracle(S, oracle, kind):
    """Instances [s*R, (s+1)*R) run make_scenario(100 + s, L_s, T) with maps of 20 and 50 landmarks in one L_max = 50 handle."""
    NS, R, L_max, T = 4, 16, 50, 120
    Ls = [20, 50, 20, 50]
    scen = [make_scenario(100 + s, Ls[s], T) for s in range(NS)]
    B = NS * R
    maps = np.zeros((B, L_max, 2)); counts = np.zeros(B, np.int32); cmds = np.zeros((T, B, 2), np.float32)
    for s, (lm, c) in enumerate(scen):
        maps[s * R:(s + 1) * R, :Ls[s]] = lm; counts[s * R:(s + 1) * R] = Ls[s]; cmds[:, s * R:(s + 1) * R] = c[:, None, :]
    f = _make(S, kind, B, L_max)
    f.set_map(maps, counts); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds)
    run = oracle.run_ekf_batch if kind == "ekf" else oracle.run_ukf_batch
    base = 3 if kind == "ekf" else 4
    M, truth, err = f.landmark_counts(), f.truth(), f.error_stats()
    for s, (lm, c) in enumerate(scen):
        r = run(lm, c, R, L_max, seed=SEED, inst0=s * R, nthreads=4)
        sl = slice(s * R, (s + 1) * R)
        assert np.array_equal(M[sl], r["M"]) and np.array_equal(truth[sl], r["truth"]) and np.array_equal(err[sl], r["avg_err"])
        for i in (0, R // 2, R - 1):
            st = f.get_state(s * R + i); n = base + 2 * r["M"][i]
            assert np.array_equal(st["x"], r["x"][i, :n]) and np.array_equal(st["P"].ravel(), r["P"][i, :n * n]), (s, i)
    assert np.all(f.status() == 0)
    f.close()


# ---- 3. per-instance commands and start poses on external messages ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_each_robot_its_own_stream_and_pose(S, oracle, kind):
    """Instance b follows golden stream b % 4 (its commands and detections) from its own start pose == an oracle filter started
    there and fed that stream."""
    names = ["sim_seed0_L20_T1000.npz", "sim_seed1_L20_T400.npz", "sim_seed2_L50_T1000.npz", "sim_seed1234_L50_T400.npz"]
    gs = [load_golden(n) for n in names]
    B, L_max, T = 8, 50, 400
    ks = max(g["meas"].shape[1] for g in gs)
    pose = np.array([[0.05 * b, -0.03 * b, 0.02 * b - 0.07] for b in range(B)], np.float32)
    f = _make(S, kind, B, L_max)
    f.init(pose)
    orc = []
    for b in range(B):
        o = oracle.OracleEKF(L_max=L_max) if kind == "ekf" else oracle.OracleUKF(L_max=L_max)
        o.init(float(pose[b, 0]), float(pose[b, 1]), float(pose[b, 2]))
        orc.append(o)
    for t in range(T):
        meas = np.zeros((B, ks, 3), np.float32); cnt = np.zeros(B, np.int32); cmds = np.zeros((B, 2), np.float32)
        for b in range(B):
            g = gs[b % 4]; k = int(g["meas_count"][t])
            meas[b, :k] = g["meas"][t, :k]; cnt[b] = k; cmds[b] = g["cmds"][t]
            orc[b].update(cmds[b, 0], cmds[b, 1], g["meas"][t, :k])
        f.update(cmds, meas, cnt)
        if t % 100 == 99:
            for b in range(B):
                _assert_state(f.get_state(b), orc[b].state())
    assert np.all(f.status() == 0)
    f.close()


# ---- 4. call order and the tracked instance ------------------------------------------------------------------------------------------
def _scenario_inputs(B, L_max, T):
    maps = np.zeros((B, L_max, 2)); counts = np.zeros(B, np.int32); cmds = np.zeros((T, B, 2), np.float32)
    for b in range(B):
        L = 20 if b % 2 == 0 else L_max
        lm, c = make_scenario(700 + b % 3, L, T)
        maps[b, :L] = lm; counts[b] = L; cmds[:, b] = c
    truth0 = np.array([[0.1 * b, 0.2, 0.05 * b] for b in range(B)])
    return maps, counts, cmds, truth0


def test_queued_shared_steps_mix_with_per_instance_runs(S):
    """Queued slam_step_sim calls, then slam_run_sim_each, then queued calls again == all per instance."""
    B, L_max, T = 8, 50, 60
    maps, counts, cmds, truth0 = _scenario_inputs(B, L_max, T)
    shared = make_scenario(9, 20, T)[1]
    cmds[:20] = shared[:20, None, :]; cmds[45:] = shared[45:, None, :]
    a = _make(S, "ekf", B, L_max); b = _make(S, "ekf", B, L_max)
    for f in (a, b):
        f.set_lazy_steps(32); f.set_map(maps, counts); f.init(np.zeros((B, 3), np.float32), truth0=truth0)
    for t in range(20):
        a.update_sim(shared[t])
    a.run_sim(cmds[20:45])
    for t in range(45, T):
        a.update_sim(shared[t])
    b.run_sim(cmds)
    _assert_same(_snapshot(a), _snapshot(b))
    a.close(); b.close()


def test_tracked_instance_gets_its_slice(S, hip):
    """slam_track_instance under per-instance maps, start poses and commands (SIM, host and device messages): the shadow's answer ==
    the batch's instance."""
    B, L_max, T, tr = 8, 50, 30, 5
    maps, counts, cmds, truth0 = _scenario_inputs(B, L_max, T)
    pose = np.array([[0.01 * b, 0.0, -0.02 * b] for b in range(B)], np.float32)
    a = _make(S, "ekf", B, L_max); b = _make(S, "ekf", B, L_max)
    a.track_instance(tr)
    for f in (a, b):
        f.set_map(maps, counts); f.init(pose, truth0=truth0)
        f.run_sim(cmds)
    assert a.get_state(tr)["timestep"] == T
    _assert_state(a.get_state(tr), b.get_state(tr))
    dev = _Dev(hip)
    try:
        g = load_golden("sim_seed1234_L50_T400.npz")
        for t in range(12):
            k = int(g["meas_count"][t]); ks = g["meas"].shape[1]
            meas = np.zeros((B, ks, 3), np.float32); meas[:, :k] = g["meas"][t, :k]; cnt = np.full(B, k, np.int32)
            c = cmds[t % T] * np.float32(0.5)
            for f in (a, b):
                if t % 2:
                    f.update(c, meas, cnt)
                else:
                    f.update_dev_each(dev.put("c", c), dev.put("m", meas), dev.put("n", cnt), ks)
                f.sync()   # (the device buffers are rewritten by the next step)
            _assert_state(a.get_state(tr), b.get_state(tr))
        a.track_instance(-1)
        _assert_same(_snapshot(a), _snapshot(b))
    finally:
        a.close(); b.close(); dev.close()


def test_argument_checks(S):
    from live_ekf_slam_amd import _lib
    L = _lib.lib()
    f = _make(S, "ekf", 4, 20); f.init(0.0, 0.0, 0.0)
    m = np.zeros((4, 10, 2))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    assert L.slam_set_maps(f.h, dp(m), ip(np.array([10, 11, 10, 10], np.int32)), 10) == -1    # L[b] > L_stride
    assert L.slam_set_maps(f.h, dp(m), ip(np.array([10, 0, 10, 10], np.int32)), 10) == -1     # L[b] <= 0
    assert L.slam_set_maps(f.h, None, ip(np.full(4, 10, np.int32)), 10) == -1
    assert L.slam_set_maps(f.h, dp(m), None, 10) == -1
    c = np.zeros((4, 2), np.float32)
    assert L.slam_run_sim_each(f.h, fp(c), -1) == -1
    assert L.slam_run_sim_each(f.h, None, 1) == -1
    assert L.slam_init_each(f.h, None, None) == -1
    assert L.slam_step_each(f.h, None, fp(np.zeros((4, 1, 3), np.float32)), ip(np.zeros(4, np.int32)), 1) == -1
    assert L.slam_run_sim_each(f.h, fp(c), 1) == -4          # no map yet
    assert L.slam_predict_each(f.h, fp(c)) == -3             # EKF: no separate prediction stage
    f.close()
    u = S.BatchedUKFLoc(4).readParams()
    assert L.slam_set_maps(u.h, dp(m), ip(np.full(4, 10, np.int32)), 10) == -3   # UKF_LOC: one known map
    u.close()


# ---- 5. the reference experiment in one handle ---------------------------------------------------------------------------------------
REF = json.load(open(os.path.join(GOLDEN, "ref_avg_error_runs.json")))
N_SCEN, B_PER = 10, 64


def _cfg(regime):
    c = default_config()
    r = REF["regimes"][regime]
    c.V_00, c.V_11, c.W_00, c.W_11 = r["V_00"], r["V_11"], r["W_00"], r["W_11"]
    return c


def _check(ours, ref_runs, what):
    ref = np.asarray(ref_runs)
    ours = np.asarray(ours)
    assert ref.min() <= ours.mean() <= ref.max(), (what, ours.mean(), ref.min(), ref.max())
    sem = math.sqrt(ref.var(ddof=1) / len(ref) + ours.var(ddof=1) / N_SCEN)   # instances of one map are correlated
    assert abs(ours.mean() - ref.mean()) < 2.0 * sem + 0.05 * ref.mean(), (what, ours.mean(), ref.mean(), sem)


@pytest.mark.parametrize("regime", ["low", "high"])
def test_reference_experiment_in_one_handle(S, regime):
    """10 random maps x 64 noise seeds (make_scenario(100 + s, 20, 1000)) as one handle of 640 instances; the per-instance mean errors
    pass the band check of tests/test_reference_statistics.py against the reference's published runs."""
    B, T = N_SCEN * B_PER, 1000
    maps = np.zeros((B, 20, 2)); cmds = np.zeros((T, B, 2), np.float32)
    for s in range(N_SCEN):
        lm, c = make_scenario(100 + s, 20, T)
        maps[s * B_PER:(s + 1) * B_PER] = lm; cmds[:, s * B_PER:(s + 1) * B_PER] = c[:, None, :]
    f = S.BatchedEKF(B, 20).readParams(_cfg(regime))
    f.set_seed(7); f.set_map(maps); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds)
    assert np.all(f.status() == 0)
    _check(f.error_stats(), REF["runs"][f"ekf_{regime}_noise_iter/ekf.csv"], f"GPU EKF {regime}, one handle")
    f.close()
