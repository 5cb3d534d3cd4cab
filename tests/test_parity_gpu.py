"""GPU parity tests: the HIP path (through the C ABI) against the CPU oracle.

Bar (north_star: "state/covariance trajectories match ... to a stated fp64 tolerance"): the tolerance is ZERO —
x, P, M, ids, truth poses, measurements and error statistics must be BIT-IDENTICAL to the oracle evaluated with
the same deterministic math policy (MATH_DET, MODE_FAST).  The oracle itself is tied to the reference by
tests/test_oracle.py (KATs, golden fixtures, libm-vs-deterministic-math bounds).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu

TOL = 0.0  # fp64 tolerance of the GPU-vs-oracle comparison: exact equality


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()  # raises if the HIP extension is missing: there is no fallback path to test instead
    return S


def _assert_state_equal(sg, so):
    assert sg["M"] == so["M"]
    assert np.array_equal(sg["ids"], so["ids"])
    assert np.array_equal(sg["x"], so["x"]), np.abs(sg["x"] - so["x"]).max()
    assert np.array_equal(sg["P"], so["P"]), np.abs(sg["P"] - so["P"]).max()


def _wpf(monkeypatch, w, L_max=50, dtype=0):
    """Force a tuning variant of the step kernel (code PIPE*1000 + W*100 + KG*10 + UNR).  The release library holds the
    defaults of every size class / storage type; the others exist in SLAM_SWEEP=1 builds only."""
    if w:
        from live_ekf_slam_amd import _lib
        # every variant a test names is part of the release build (build.py EKF_DEFAULT_VARIANTS); the sweep-only ones are
        # exercised by tools/gpu_variants.py in SLAM_SWEEP=1 builds, not by parametrisations that would skip here
        assert _lib.lib().slam_variant_available(L_max, dtype, w), f"kernel variant {w} is missing from the build"
        monkeypatch.setenv("SLAM_WAVES_PER_FILTER", str(w))
    else:
        monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)


def test_device_math_bit_exact(S, oracle):
    """sin/cos/atan2 (shared code), remainder, sqrt, division, double->float, Philox->u53: device == host bits."""
    from live_ekf_slam_amd import _lib
    rng = np.random.default_rng(1)
    n = 300000
    a = np.concatenate([rng.uniform(-8, 8, n // 3), rng.uniform(-300, 300, n // 3), rng.normal(0, 1e-3, n - 2 * (n // 3))])
    b = rng.uniform(-8, 8, n)
    out = np.zeros(8 * n)
    dp = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))
    _lib.check(_lib.lib().slam_math_probe(dp(a), dp(b), dp(out), n, 0))
    out = out.reshape(n, 8)
    L = oracle.lib()
    s, c, at, rem = (np.zeros(n) for _ in range(4))
    L.orc_det_sincos(dp(a), dp(s), dp(c), n); L.orc_det_atan2(dp(a), dp(b), dp(at), n); L.orc_libm_remainder2pi(dp(a), dp(rem), n)
    for i, ref in enumerate([s, c, at, rem, np.sqrt(np.abs(a)), a / b, a.astype(np.float32).astype(np.float64)]):
        assert np.array_equal(out[:, i], ref), i
    nz = np.zeros(2)
    for i in range(0, n, 1499):
        L.orc_noise_pair(12345, i, 7, 3, dp(nz))
        assert out[i, 7] == nz[0] + nz[1]


@pytest.mark.parametrize("fixture,L_max,wpf", [("sim_seed0_L20_T1000.npz", 20, 0), ("sim_seed1_L20_T400.npz", 20, 1124),
                                               ("sim_seed2_L50_T1000.npz", 50, 1444), ("sim_seed2_L50_T1000.npz", 50, 1454), ("sim_seed2_L50_T1000.npz", 50, 1464),
                                               ("sim_seed1_L20_T400.npz", 20, 1244),
                                               ("sim_seed0_L20_T1000.npz", 90, 0),
                                               ("sim_igvc1_seed5_T200.npz", 37, 0), ("sim_grid_seed5_T200.npz", 25, 0),
                                               ("sim_demo_seed5_T200.npz", 20, 0)])
def test_update_on_reference_measurement_stream(S, oracle, monkeypatch, fixture, L_max, wpf):
    """Filter::update fed with the measurement stream the REFERENCE simulator produced (golden fixture), the same
    message for every instance of the batch; x and P checked against the oracle every 20 steps."""
    _wpf(monkeypatch, wpf, L_max)
    g = load_golden(fixture)
    B = 5
    f = S.BatchedEKF(B, L_max).readParams(); f.init(0.0, 0.0, 0.0)
    e = oracle.OracleEKF(L_max=L_max); e.init(0, 0, 0)
    for t in range(int(g["T"])):
        k = int(g["meas_count"][t])
        f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())
        e.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
        if t % 20 == 19 or t == int(g["T"]) - 1:
            so = e.state()
            for b in (0, B - 1):
                _assert_state_equal(f.get_state(b), so)
    assert np.all(f.status() == 0)
    pub = f.publishState(0)   # EKFState payload: float32, P row-major, [id,x,y] triplets (ekf.cpp:192-220)
    so = e.state()
    assert pub["timestep"] == so["timestep"] == int(g["T"]) and pub["M"] == so["M"]
    assert np.array_equal(pub["P"], so["P"].astype(np.float32).ravel())
    assert np.array_equal(pub["landmarks"][0::3], so["ids"].astype(np.float32))
    f.close()


@pytest.mark.parametrize("L,T,B,wpf", [(20, 400, 192, 0), (50, 400, 96, 0), (50, 400, 96, 1444), (50, 400, 96, 1454), (20, 400, 96, 1124), (20, 300, 64, 1244)])
def test_sim_step_parity(S, oracle, monkeypatch, L, T, B, wpf):
    """Device-side generator + filter in one kernel vs oracle generator + oracle filter, per-instance noise
    streams keyed by global instance id; also the measurements themselves and the error statistic."""
    _wpf(monkeypatch, wpf, L)
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(77); f.set_instance_offset(5000); f.init(0, 0, 0)
    f.last_meas(8)  # switch the measurement dump on
    sims = [oracle.OracleSim(lm) for _ in range(3)]
    for t in range(T):
        f.update_sim(cmds[t])
        if t < 40:  # measurement-level check on three instances
            meas, cnt = f.last_meas(8)
            tr = f.truth()
            for j, b in enumerate((0, 1, B - 1)):
                truth, m = sims[j].step_philox(cmds[t, 0], cmds[t, 1], 77, 5000 + b, t)
                assert cnt[b] == len(m) and np.array_equal(meas[b, :cnt[b]], m) and np.array_equal(tr[b], truth)
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=77, inst0=5000, nthreads=8)
    assert np.array_equal(f.landmark_counts(), r["M"])
    assert np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"])
    assert np.array_equal(f.status(), r["flags"]) and np.all(r["flags"] == 0)
    for b in range(B):
        n = 3 + 2 * r["M"][b]
        sg = f.get_state(b)
        _assert_state_equal(sg, dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    assert 0.03 < f.error_stats().mean() < 0.6   # EKF-SLAM average error scale (0.15-0.5 m per run)
    f.close()


@pytest.mark.parametrize("L,T,B,chunk,dtype,idknown,wide", [
    (50, 301, 96, 0, "f64", 1, 0),      # the whole run in one launch (insertion steps switch buffers, the rest is in place)
    (50, 300, 64, 7, "f64", 1, 1),      # odd chunks + a wide-sensor step inside a chunk (k = 50 > KG: several groups)
    (20, 250, 64, 16, "f64", 0, 0),     # unknown-id association (over-provisioned leading dimension, re-pack)
    (50, 200, 48, 0, "f32", 1, 1),      # fp32 storage: resident thin rows must carry the storage rounding
    (20, 120, 64, 1, "f64", 1, 0),      # chunk 1 = one launch per step through the same entry point
])
def test_run_sim_multistep_launch_parity(S, oracle, monkeypatch, L, T, B, chunk, dtype, idknown, wide):
    """slam_run_sim runs many timesteps per launch (x_t, ids, true pose and the thin rows/cols of P stay on chip,
    P is updated in place except on insertion steps, which switch buffers): same bits as the oracle, whatever the chunking."""
    from live_ekf_slam_amd.scenario import make_scenario
    monkeypatch.setenv("SLAM_RUN_CHUNK", str(chunk))
    lm, cmds = make_scenario(4321, L, T)
    cfg = S.default_config(); cfg.landmark_id_is_known = idknown
    if wide:
        cfg.range_max = 1e9; cfg.fov_min = -4.0; cfg.fov_max = 4.0   # every landmark in view all the time
    f = S.BatchedEKF(B, L, dtype=S.F32 if dtype == "f32" else S.F64).readParams(cfg)
    f.set_map(lm); f.set_seed(99); f.set_instance_offset(123); f.init(0, 0, 0)
    f.run_sim(cmds[:T // 3]); f.run_sim(cmds[T // 3:])          # two calls: state carries over between launches
    mode = oracle.MODE_FAST | (oracle.STORAGE_F32 if dtype == "f32" else 0)
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=99, inst0=123, nthreads=8, cfg=cfg, mode=mode)
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * r["M"][b]
        sg = f.get_state(b)
        assert sg["timestep"] == T or r["flags"][b] != 0
        _assert_state_equal(sg, dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    assert r["M"].max() > 3
    f.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_steps_without_detections_skip_the_stream(S, oracle, dtype):
    """A blind sensor for 40 steps in the middle of a run: those steps change only what the prediction touches (rows and
    columns 0, 1 and (2,2) of P, ekf.cpp:61) and the kernel writes just the vehicle rows / columns in place; before and
    after, the ordinary stream.  Same bits as the oracle, which recomputes the full matrix every step."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 20, 40, 110
    lm, cmds = make_scenario(777, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1))
    vis[0] = [1e9, -4.0, 4.0]          # map everything at once
    vis[35:75] = [1e-6, -1.57, 1.57]   # nothing in range
    f = S.BatchedEKF(B, L, dtype=S.F32 if dtype == "f32" else S.F64).readParams()
    f.set_map(lm); f.set_seed(5); f.set_instance_offset(9); f.init(0, 0, 0)
    t = 0
    for t1, v in ((1, vis[0]), (35, vis[1]), (75, vis[35]), (T, vis[75])):
        f.set_vision(*v); f.run_sim(cmds[t:t1]); t = t1
    mode = oracle.MODE_FAST | (oracle.STORAGE_F32 if dtype == "f32" else 0)
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=5, inst0=9, nthreads=8, mode=mode, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * L
        _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()


def test_many_detections_in_one_step_and_groups(S, oracle):
    """A wide sensor shows every landmark at once (k = L = 50 > KG): insertion path, grouping, then updates of all."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B = 50, 16
    lm, cmds = make_scenario(7, L, 12)
    vis = np.tile([3.0, -1.57, 1.57], (12, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[5] = [1e9, -4.0, 4.0]
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(3); f.init(0, 0, 0)
    for t in range(12):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=3, nthreads=4, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"])
    for b in range(B):
        _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b], x=r["x"][b], P=r["P"][b].reshape(103, 103)))
    f.close()


def test_edge_cases_ragged_empty_duplicate_capacity(S, oracle):
    B, L_max = 6, 3
    f = S.BatchedEKF(B, L_max).readParams(); f.init(0.5, -0.25, 0.1)
    es = [oracle.OracleEKF(L_max=L_max) for _ in range(B)]
    for e in es:
        e.init(0.5, -0.25, 0.1)
    msgs = [
        [[], [], [], [], [], []],                                                        # empty for everybody
        [[[4, 1.0, 0.2]], [], [[4, 1.0, 0.2], [9, 2.0, -0.4]], [[9, 2.2, 0.0]], [], [[1, 0.7, 1.0], [2, 0.9, -1.0], [3, 1.1, 0.0], [5, 1.3, 0.5]]],  # ragged; inst 5 overflows capacity 3
        [[[4, 1.05, 0.15], [4, 1.04, 0.16]], [[8, 1.0, 0.0], [8, 1.0, 0.0]], [[9, 2.0, -0.45]], [], [[2, 1.0, 0.3]], [[3, 1.0, 0.0], [1, 0.8, 0.9]]],   # repeated known id (two updates); repeated NEW id (freeze inst 1)
        [[], [[8, 1.0, 0.0]], [[4, 0.9, 0.3], [9, 1.9, -0.5]], [[9, 2.1, 0.05]], [[2, 0.9, 0.35]], []],
    ]
    for step, per_inst in enumerate(msgs):
        kmax = max(1, max(len(m) for m in per_inst))
        meas = np.zeros((B, kmax, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b, m in enumerate(per_inst):
            cnt[b] = len(m)
            if m:
                meas[b, :len(m)] = m
        cmd = (0.1, 0.02 * (step - 1))
        f.update(cmd, meas, cnt)
        for b, m in enumerate(per_inst):
            es[b].update(cmd[0], cmd[1], m)
    flags = f.status()
    assert flags[1] & 4 and flags[5] & 8 and flags[0] == 0
    for b in range(B):
        so = es[b].state()
        sg = f.get_state(b)
        _assert_state_equal(sg, so)
        assert sg["timestep"] == so["timestep"]
    assert f.get_state(1)["timestep"] == 2   # frozen at the step of the duplicate
    f.close()


@pytest.mark.parametrize("quirk,idknown", [(0, 1), (1, 0), (0, 0)])
def test_config_switches(S, oracle, quirk, idknown):
    """V/W quirk off, and unknown-id association (ekf.cpp:82-98), on a reference measurement stream."""
    g = load_golden("sim_seed1_L20_T400.npz")
    cfg = S.default_config(); cfg.replicate_vw_quirk = quirk; cfg.landmark_id_is_known = idknown
    cfg.w_r = 0.01; cfg.v_d = 0.002   # non-zero noise means exercise the float adds of ekf.cpp:57,130
    f = S.BatchedEKF(3, 20).readParams(cfg); f.init(0, 0, 0)
    e = oracle.OracleEKF(cfg=cfg, L_max=20); e.init(0, 0, 0)
    for t in range(250):
        k = int(g["meas_count"][t])
        f.update(g["cmds"][t], g["meas"][t, :k].ravel()); e.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
        if t % 50 == 49:
            _assert_state_equal(f.get_state(2), e.state())
    assert f.get_state(0)["M"] > 3
    f.close()


@pytest.mark.parametrize("switch,idknown,L_max,fixture,T", [("ekf_abs_is_int", 0, 50, "sim_seed2_L50_T1000.npz", 400), ("ekf_abs_is_int", 0, 230, "sim_seed2_L50_T1000.npz", 120),
                                                            ("ekf_landmark_from_x_pred", 1, 20, "sim_seed1_L20_T400.npz", 160),
                                                            ("ekf_landmark_from_x_pred", 1, 230, "sim_seed1_L20_T400.npz", 160)])
def test_appendix_d_quirk_switches_ekf(S, oracle, switch, idknown, L_max, fixture, T):
    """SURVEY Appendix D asks for every quirk behind a named switch: `ekf_abs_is_int` (the unqualified abs of
    ekf.cpp:91-92 as ::abs(int): the association box becomes +-1) and `ekf_landmark_from_x_pred` (D-2: the landmark of an update read
    from x_pred instead of x_t).  Switched ON - i.e. NOT the reference's behaviour - kernel and oracle still agree bit for bit, and the
    trajectory differs from the default one (the switch is not vacuous); fast class and, for D-2, the HBM-streamed class (L_max 230)."""
    g = load_golden(fixture)
    res = {}
    for on in (0, 1):
        cfg = S.default_config(); cfg.landmark_id_is_known = idknown; cfg.w_r = 0.01; cfg.v_d = 0.002
        setattr(cfg, switch, on)
        f = S.BatchedEKF(2, L_max).readParams(cfg); f.init(0, 0, 0)
        e = oracle.OracleEKF(cfg=cfg, L_max=L_max); e.init(0, 0, 0)
        for t in range(T):
            k = int(g["meas_count"][t])
            f.update(g["cmds"][t], g["meas"][t, :k].ravel()); e.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
            if t % 40 == 39:
                _assert_state_equal(f.get_state(1), e.state())
        res[on] = f.get_state(0)
        f.close()
    assert res[0]["M"] != res[1]["M"] or not np.array_equal(res[0]["x"], res[1]["x"])


def test_call_order_errors(S):
    f = S.BatchedEKF(2, 20).readParams()
    with pytest.raises(S.SlamError):
        f.update((0.1, 0.0), [])          # before init (localization_node.cpp:109)
    f.init(0, 0, 0)
    with pytest.raises(S.SlamError):
        f.update_sim((0.1, 0.0))          # no map yet
    f.close()


def test_full_size_properties(S, oracle):
    """BASELINE size (L=50, batch=65536): determinism, shard invariance, invariants, and oracle spot checks."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 50, 65536, 24
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]

    def run(batch, offset):
        f = S.BatchedEKF(batch, L).readParams(); f.set_map(lm); f.set_seed(2025); f.set_instance_offset(offset); f.init(0, 0, 0)
        for t in range(T):
            f.set_vision(*vis[t]); f.update_sim(cmds[t])
        return f

    f = run(B, 0)
    M = f.landmark_counts(); poses = f.poses(); err = f.error_stats(); flags = f.status()
    assert np.all(M == L) and np.all(flags == 0)
    assert np.all(np.isfinite(poses)) and np.all(np.abs(poses[:, 2]) <= np.pi)
    assert 0.0 < err.mean() < 0.2
    assert abs(f.algorithmic_bytes() - B * 2 * (103 * 103 + 103) * 8) < 1
    picks = [0, 1, 4095, 32768, 65535]
    states = {b: f.get_state(b) for b in picks}
    for b in picks:   # oracle spot checks, bit-exact
        r = oracle.run_ekf_batch(lm, cmds, 1, L, seed=2025, inst0=b, vision=vis)
        _assert_state_equal(states[b], dict(M=L, ids=r["ids"][0], x=r["x"][0], P=r["P"][0].reshape(103, 103)))
        P = states[b]["P"]
        assert np.abs(P - P.T).max() < 1e-9 and np.linalg.eigvalsh((P + P.T) / 2).min() > -1e-10
    f.close()
    # shard invariance: a 4096-instance shard at offset 32768 reproduces the same instances
    g = run(4096, 32768)
    assert np.array_equal(g.poses(), poses[32768:32768 + 4096]) and np.array_equal(g.error_stats(), err[32768:32768 + 4096])
    _assert_state_equal(g.get_state(0), states[32768])
    g.close()
    # determinism: same run twice -> identical
    h = run(4096, 0)
    assert np.array_equal(h.poses(), poses[:4096])
    h.close()


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_run_sim_full_size_one_launch(S, oracle, dtype):
    """The BENCHMARKED path at its own size: BASELINE batch 65536, L = 50, slam_run_sim carrying K = 60 timesteps in ONE launch
    (deferred update groups, the decoupled control / streamer loop, the generator wavefront), fp64 and fp32 storage
    (configs[3]'s dtype): oracle spot checks on six instances bit for bit, shard invariance, determinism, no instance flagged."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 50, 65536, 61
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]
    dt = S.F32 if dtype == "f32" else S.F64
    mode = oracle.MODE_FAST | (oracle.STORAGE_F32 if dtype == "f32" else 0)

    def run(batch, offset):
        f = S.BatchedEKF(batch, L, dtype=dt).readParams(); f.set_map(lm); f.set_seed(2025); f.set_instance_offset(offset); f.init(0, 0, 0)
        f.set_vision(*vis[0]); f.update_sim(cmds[0]); f.set_vision(*vis[1])
        f.run_sim(cmds[1:T])                      # ONE multi-step launch, like bench.py's timed region
        return f

    f = run(B, 0)
    M = f.landmark_counts(); poses = f.poses(); err = f.error_stats(); flags = f.status(); truth = f.truth()
    assert np.all(M == L) and np.all(flags == 0)
    assert np.all(np.isfinite(poses)) and np.all(np.abs(poses[:, 2]) <= np.pi) and 0.0 < err.mean() < 0.3
    kh = f.k_histogram()
    assert kh.sum() == B * T and kh[3] > 0 and kh[1] > 0          # the window mixes detection counts
    picks = [0, 1, 4095, 32768, 36863, 65535]
    states = {b: f.get_state(b) for b in picks}
    for b in picks:
        r = oracle.run_ekf_batch(lm, cmds, 1, L, seed=2025, inst0=b, vision=vis, mode=mode)
        _assert_state_equal(states[b], dict(M=L, ids=r["ids"][0], x=r["x"][0], P=r["P"][0].reshape(103, 103)))
        assert err[b] == r["avg_err"][0] and np.array_equal(truth[b], r["truth"][0])
        assert states[b]["timestep"] == T
    f.close()
    g = run(8192, 32768)                          # configs[3]'s per-GPU shard (65536 / 8) at a global offset
    assert np.array_equal(g.poses(), poses[32768:32768 + 8192]) and np.array_equal(g.error_stats(), err[32768:32768 + 8192])
    _assert_state_equal(g.get_state(0), states[32768])
    _assert_state_equal(g.get_state(36863 - 32768), states[36863])
    g.close()
    h = run(4096, 0)                              # determinism
    assert np.array_equal(h.poses(), poses[:4096])
    _assert_state_equal(h.get_state(1), states[1])
    h.close()


@pytest.mark.parametrize("L,T,B", [(20, 300, 64), (50, 300, 48)])
def test_fp32_storage_variant(S, oracle, L, T, B):
    """SLAM_F32 (BASELINE configs[3]): x and P live in HBM as float, arithmetic stays fp64; the oracle rounds its
    stored state the same way -> still bit-identical.  Also: the fp32 run stays close to the fp64 run."""
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[3] = [1e9, -4.0, 4.0]   # one wide step: many insertions at once
    f = S.BatchedEKF(B, L, dtype=S.F32).readParams(); f.set_map(lm); f.set_seed(21); f.init(0, 0, 0)
    for t in range(T):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=21, nthreads=8, mode=oracle.MODE_FAST | oracle.STORAGE_F32, vision=vis)
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * r["M"][b]
        sg = f.get_state(b)
        _assert_state_equal(sg, dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
        assert np.array_equal(sg["P"], sg["P"].astype(np.float32).astype(np.float64))   # really stored as float
    r64 = oracle.run_ekf_batch(lm, cmds, B, L, seed=21, nthreads=8, vision=vis)
    assert np.abs(r64["x"] - r["x"]).max() < 5e-3 and abs(r64["avg_err"].mean() - r["avg_err"].mean()) < 1e-3
    assert abs(f.algorithmic_bytes() - sum(2 * ((3 + 2 * m) ** 2 + 3 + 2 * m) * 4 for m in r["M"])) < 1
    f.close()


@pytest.mark.parametrize("first_wide", [0, 1])
def test_large_state_100_landmarks(S, oracle, first_wide):
    """n = 203 (L = 100): the streaming kernel has no register-imposed limit on n; only the LDS arrays grow.  first_wide: the
    first message shows ALL 100 landmarks (the reference loops over any number of detections, ekf.cpp:65,73; until round 3 one
    wavefront associated at most 64 and flagged the rest SLAM_INST_CAPACITY), later wide looks carry 100 updates in one message."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 100, 120, 12
    lm, cmds = make_scenario(77, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1))
    for t in (2, 30, 60, 90, 110):
        vis[t] = [7.5, -3.2, 3.2]       # wide looks: many insertions / updates per step
    if first_wide:
        vis[0] = [1e9, -4.0, 4.0]
        vis[45] = [1e9, -4.0, 4.0]      # 100 updates in one message
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(4); f.init(0, 0, 0)
    for t in range(T):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
        if first_wide and t == 0:
            assert np.all(f.landmark_counts() == L) and not f.status().any()
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=4, nthreads=4, vision=vis)
    assert np.array_equal(f.landmark_counts(), r["M"]) and r["M"].max() > 50
    assert np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * r["M"][b]
        _assert_state_equal(f.get_state(b), dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()


@pytest.mark.parametrize("map_type,L,dtype,seed", [("grid", 50, "f64", 5), ("igvc1", 50, "f64", 6), ("demo", 20, "f32", 7), ("grid", 50, "f32", 8),
                                                   ("random", 50, "f64", 9)])
def test_long_runs_on_every_map_type(S, oracle, map_type, L, dtype, seed):
    """600 timesteps in multi-step launches on the reference's other map generators (regular grids put many landmarks at equal
    range: detection-heavy steps, landmarks entering and leaving the view all the time - the gather-without-drain, pre-flush and
    overflow paths of the decoupled loop), whole batch against the oracle, bit for bit."""
    from live_ekf_slam_amd.scenario import make_scenario
    T, B = 600, 192
    lm, cmds = make_scenario(seed, L, T, map_type=map_type)
    Lm = lm.shape[0]
    f = S.BatchedEKF(B, Lm, dtype=S.F32 if dtype == "f32" else S.F64).readParams()
    f.set_map(lm); f.set_seed(seed); f.set_instance_offset(1000 * seed); f.init(0, 0, 0)
    f.run_sim(cmds[:37]); f.run_sim(cmds[37:400]); f.run_sim(cmds[400:])
    mode = oracle.MODE_FAST | (oracle.STORAGE_F32 if dtype == "f32" else 0)
    r = oracle.run_ekf_batch(lm, cmds, B, Lm, seed=seed, inst0=1000 * seed, nthreads=8, mode=mode)
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * r["M"][b]
        _assert_state_equal(f.get_state(b), dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    kh = f.k_histogram()
    assert int(kh.sum()) == B * T
    print(f"{map_type} L={Lm} {dtype}: mean M {r['M'].mean():.1f}, k histogram {kh.tolist()}, oracle {r['seconds']:.2f} s")
    assert r["M"].mean() > 3 and kh[1:].sum() > B * T // 4
    f.close()


def test_step_dev_queued_equals_immediate(S):
    """slam_step_dev (device-resident messages) queues its calls like slam_step / slam_step_sim: each message is copied into a
    device-side queue at the call and a queue of them runs as one multi-step launch.  Same bits as one launch per call,
    from Filter::init through insertions and messages with eight detections (several update groups inside a multi-step launch)."""
    import ctypes as C
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, KS = 20, 64, 75, 8
    lm, cmds = make_scenario(11, L, T)
    def make():
        f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.set_instance_offset(900); f.init(0, 0, 0)
        return f
    hip = C.CDLL("libamdhip64.so")
    def to_device(a):
        a = np.ascontiguousarray(a); d = C.c_void_p()
        assert hip.hipMalloc(C.byref(d), a.nbytes) == 0 and hip.hipMemcpy(d, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
        return d
    rec = make()
    rec.last_meas(KS)   # measurement dump on
    msgs, kmax = [], 0
    for t in range(T):
        if t in (2, 30): rec.set_vision(1e9, -4.0, 4.0)      # two messages with every landmark in view (clipped to KS detections)
        if t in (3, 31): rec.set_vision(3.0, -1.57, 1.57)
        rec.update_sim(cmds[t])
        m, c = rec.last_meas(KS)
        kmax = max(kmax, int(c.max()))
        msgs.append((to_device(m), to_device(c)))
    assert kmax > 4
    Lc = _lib.lib()
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    outs = []
    for lazy in (32, 0, 5):
        f = make()
        _lib.check(Lc.slam_set_lazy_steps(f.h, lazy))
        for t in range(T):
            cm = np.ascontiguousarray(cmds[t], dtype=np.float32)
            _lib.check(Lc.slam_step_dev(f.h, fp(cm), msgs[t][0], msgs[t][1], KS))
            if t == 40:
                f.get_state(3)   # a getter in the middle of a queue flushes it
        outs.append(f)
    ref = outs[1]   # one launch per call (the wide messages were clipped to KS detections, so the generator's own filter saw more)
    assert ref.landmark_counts().min() >= 8 and not ref.status().any()
    for f in (outs[0], outs[2]):
        assert np.array_equal(f.landmark_counts(), ref.landmark_counts()) and np.array_equal(f.status(), ref.status())
        for b in range(B):
            _assert_state_equal(f.get_state(b), ref.get_state(b))
    # the three per-step entry points interleaved (generator / device message / host message): each flushes what the others
    # queued, so the order of the steps is the order of the calls
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    host = []
    mixed = []
    for lazy in (16, 0):
        f = make()
        _lib.check(Lc.slam_set_lazy_steps(f.h, lazy))
        for t in range(T):
            cm = np.ascontiguousarray(cmds[t], dtype=np.float32)
            if t % 3 == 0:
                _lib.check(Lc.slam_step_sim(f.h, fp(cm)))
            elif t % 3 == 1:
                _lib.check(Lc.slam_step_dev(f.h, fp(cm), msgs[t][0], msgs[t][1], KS))
            else:
                if len(host) <= t:
                    host.extend([None] * (t + 1 - len(host)))
                if host[t] is None:
                    m = np.zeros((B, KS, 3), dtype=np.float32); c = np.zeros(B, dtype=np.int32)
                    assert hip.hipMemcpy(m.ctypes.data_as(C.c_void_p), msgs[t][0], m.nbytes, 2) == 0
                    assert hip.hipMemcpy(c.ctypes.data_as(C.c_void_p), msgs[t][1], c.nbytes, 2) == 0
                    host[t] = (m, c)
                _lib.check(Lc.slam_step(f.h, fp(cm), fp(host[t][0]), ip(host[t][1]), KS))
        mixed.append(f)
    assert np.array_equal(mixed[0].landmark_counts(), mixed[1].landmark_counts()) and np.array_equal(mixed[0].status(), mixed[1].status())
    for b in range(B):
        _assert_state_equal(mixed[0].get_state(b), mixed[1].get_state(b))
    for f in outs + mixed + [rec]:
        f.close()
    for m, c in msgs:
        hip.hipFree(m); hip.hipFree(c)


def test_traffic_counters_count_what_the_kernel_streams(S):
    """slam_traffic_counters (bench.py's roofline.traffic) against what the algorithm must have moved.  Steady state (every
    landmark mapped, n = 3 + 2 L, ld = n + 1): with one launch per timestep every instance-step with a detection is exactly one
    in-place pass over P (2 n ld 8 bytes), a step without one writes only the vehicle rows / columns; in a multi-step launch the
    deferred groups take FEWER passes for the same number of rank-2 updates.  Updates applied = detections (k histogram)."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 20, 96, 81
    lm, cmds = make_scenario(31, L, T)
    n, ld = 3 + 2 * L, 4 + 2 * L
    res = {}
    for chunk in (1, 0):
        f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(3); f.set_instance_offset(40); f.init(0, 0, 0)
        f.set_vision(1e9, -4.0, 4.0); f.run_sim(cmds[:1]); f.set_vision(3.0, -1.57, 1.57)
        assert np.all(f.landmark_counts() == L)
        f.set_run_chunk(chunk)
        f.k_histogram(reset=True); f.traffic_counters(reset=True)
        f.run_sim(cmds[1:T])
        kh = f.k_histogram().astype(np.int64); tc = f.traffic_counters().astype(np.int64)
        assert kh.sum() == B * (T - 1) and kh[5:].sum() == 0          # this scenario never shows more than KG = 4 landmarks at once
        dets = int((kh * np.arange(8)).sum())
        assert tc[3] == dets                                           # every detection is one rank-2 update applied by some pass
        assert tc[0] == tc[2] * 2 * n * ld * 8                         # a pass reads and writes the n x ld matrix once
        assert tc[1] > 0
        if chunk == 1:
            assert tc[2] == kh[1:].sum()                               # one pass per instance-step that has a detection
        else:
            assert 0 < tc[2] < res[1][2] and tc[2] * 4 >= dets         # deferred groups: fewer passes, at most KG updates each
        res[chunk] = tc
        f.close()
    assert res[0][0] < res[1][0]


def test_step_dev_is_enqueued_at_the_call_unless_queueing_was_asked_for(S):
    """slam_step_dev takes caller-owned device buffers on a caller-owned stream, so by default the step is on the
    stream when the call returns (slam_queued_steps == 0: an event recorded after the call covers the kernel); its queue is
    opt-in (slam_set_lazy_steps).  slam_step_sim / slam_step queue by default; a getter runs what is queued."""
    import ctypes as C
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    L, B = 20, 512
    lm, cmds = make_scenario(11, L, 12)
    hip = C.CDLL("libamdhip64.so")
    dm, dc = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(dm), B * 4 * 3 * 4) == 0 and hip.hipMalloc(C.byref(dc), B * 4) == 0
    assert hip.hipMemset(dm, 0, B * 4 * 3 * 4) == 0 and hip.hipMemset(dc, 0, B * 4) == 0
    fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
    Lc = _lib.lib()
    for mode in ("default", "queued"):
        f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.init(0, 0, 0)
        if mode == "queued":
            f.set_lazy_steps(32)
        for t in range(8):
            cm = np.ascontiguousarray(cmds[t], dtype=np.float32)
            _lib.check(Lc.slam_step_dev(f.h, fp(cm), dm, dc, 4))
            assert Lc.slam_queued_steps(f.h) == (t + 1 if mode == "queued" else 0)
        f.update_sim(cmds[8])                                  # the generator-driven entry point queues by default
        assert Lc.slam_queued_steps(f.h) == 1
        assert f.get_state(0)["timestep"] == 9 and Lc.slam_queued_steps(f.h) == 0   # the getter ran the queue
        f.close()
    for q in (dm, dc):
        hip.hipFree(q)


def test_watchdog_turns_a_stuck_protocol_into_a_flag(S):
    """The polling loops of the step kernel's control / streamer protocol carry a budget: debug flag 128 makes the pass leader
    lose its `applied` update, so the control wavefront starves for a ring slot - the launch must END (about 0.1 s per resident
    round), with the instances flagged SLAM_INST_WATCHDOG and frozen, not hang the GPU.  Without the flag: no flags."""
    import time
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 50, 512, 60
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(1); f.init(0, 0, 0)
    f.set_vision(1e9, -4.0, 4.0); f.run_sim(cmds[:1]); f.set_vision(3.0, -1.57, 1.57)
    f.run_sim(cmds[1:20]); f.sync()
    assert not f.status().any()
    f.set_debug_flags(128)
    t0 = time.perf_counter()
    f.run_sim(cmds[20:T]); f.sync()
    dt = time.perf_counter() - t0
    st = f.status()
    assert dt < 20.0
    assert np.all(st & 32) and np.all(st & 4)          # SLAM_INST_WATCHDOG, frozen
    ts = np.array([f.get_state(b)["timestep"] for b in (0, B - 1)])
    f.set_debug_flags(0)
    f.run_sim(cmds[20:30]); f.sync()                   # frozen instances are skipped by later launches
    assert np.array_equal(np.array([f.get_state(b)["timestep"] for b in (0, B - 1)]), ts)
    f.close()


def test_state_of_200_landmarks(S, oracle):
    """n = 403 (L = 200, the pose-graph config's map size): the largest size class - thin rows / columns and update slots of one
    instance take 145 KB of the CU's 160 KB of LDS.  A first look at all 200 landmarks (200 insertions in one message), 200
    updates in one message, ordinary steps in between; bit-identical to the oracle."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 200, 40, 6
    lm, cmds = make_scenario(99, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1))
    vis[0] = [1e9, -4.0, 4.0]; vis[17] = [1e9, -4.0, 4.0]; vis[30] = [6.0, -3.2, 3.2]
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(8); f.init(0, 0, 0)
    t = 0
    for t1 in (1, 17, 18, 30, 31, T):
        f.set_vision(*vis[t]); f.run_sim(cmds[t:t1]); t = t1
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=8, nthreads=6, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 3 + 2 * L
        _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    assert f.kernel_info()["name"].startswith("ekf_step_kernel<403,")
    f.close()


def test_state_of_400_landmarks(S, oracle):
    """n = 803: beyond the LDS size classes (the reference's state grows without limit, ekf.cpp:144-146; up to round 3 slam_create
    answered SLAM_ERR_UNSUPPORTED above 200 landmarks).  The HBM-streamed class (ekf_big_kernel.hip): a first look at all 400
    landmarks in one message, a second full look (400 updates in one message), ordinary steps, single-step and multi-step calls;
    bit-identical to the oracle, error statistics and true poses included."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 400, 24, 3
    lm, cmds = make_scenario(77, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1))
    vis[0] = [1e9, -4.0, 4.0]; vis[9] = [1e9, -4.0, 4.0]; vis[15] = [6.0, -3.2, 3.2]
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.set_seed(8); f.init(0, 0, 0)
    assert f.kernel_info()["name"] == "ekf_big_step_kernel"
    t = 0
    for t1 in (1, 9, 10, 15, 16, T):
        f.set_vision(*vis[t])
        if t1 - t == 1: f.update_sim(cmds[t])
        else: f.run_sim(cmds[t:t1])
        t = t1
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=8, nthreads=3, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    for b in range(B):
        n = 3 + 2 * L
        _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()


def _capacity_script(B, L=1000):
    """Per-instance messages that fill a handle of L landmarks to the brim: ids 0 .. L - 3; 40 known ids and L - 2; 20 known ids and
    L - 1, L, L + 1 (the last two do not fit: SLAM_INST_CAPACITY at M = L); 30 known ids.  (msgs[b][t] [k][3] float32, cmds [4][2].)"""
    msgs = []
    for b in range(B):
        rng = np.random.default_rng(1000 + b)
        def msg(ids):
            m = np.zeros((len(ids), 3), dtype=np.float32)
            m[:, 0] = ids; m[:, 1] = rng.uniform(0.5, 6.0, len(ids)); m[:, 2] = rng.uniform(-3.1, 3.1, len(ids))
            return m
        msgs.append([msg(np.arange(L - 2)),
                     msg(np.append(rng.choice(L - 2, 40, replace=False), L - 2)),
                     msg(np.append(rng.choice(L - 1, 20, replace=False), [L - 1, L, L + 1])),
                     msg(rng.choice(L, 30, replace=False))])
    rng = np.random.default_rng(10)
    cmds = np.stack([rng.uniform(0.0, 0.1, 4), rng.uniform(-0.05, 0.05, 4)], axis=1).astype(np.float32)
    return msgs, cmds


def test_state_at_the_capacity_of_1000_landmarks(S, oracle):
    """n = 2003: the capacity of the HBM-streamed class (slam_create answers SLAM_ERR_UNSUPPORTED above 1000 landmarks), against the oracle
    and not only against another run on the GPU.  External messages, one oracle per instance: 998 insertions in one message, growth to 999
    and to 1000, two ids that no longer fit, updates at the full size."""
    L, B = 1000, 2
    msgs, cmds = _capacity_script(B, L)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0)
    assert f.kernel_info()["name"] == "ekf_big_step_kernel"
    es = [oracle.OracleEKF(L_max=L) for _ in range(B)]
    for e in es: e.init(0, 0, 0)
    def walk(b):
        fl = []
        for t in range(len(cmds)):
            fl.append(es[b].update(cmds[t][0], cmds[t][1], msgs[b][t]))
        return fl
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=B) as pool:
        flags = pool.map(walk, range(B))                       # (ctypes releases the GIL: the oracles run beside the device)
        counts = []
        for t in range(len(cmds)):
            ks = np.array([len(msgs[b][t]) for b in range(B)], dtype=np.int32)
            meas = np.zeros((B, int(ks.max()), 3), dtype=np.float32)
            for b in range(B): meas[b, :ks[b]] = msgs[b][t]
            f.update(cmds[t], meas, ks)
            counts.append(f.landmark_counts().tolist())
        flags = list(flags)
    print(f"[capacity 1000] counts after every message {counts}, oracle flags {flags}, device flags {f.status().tolist()}")
    assert counts == [[L - 2] * B, [L - 1] * B, [L] * B, [L] * B]
    assert flags == [[0, 0, 8, 8]] * B and f.status().tolist() == [8] * B       # SLAM_INST_CAPACITY, from the third message on
    for b in range(B):
        _assert_state_equal(f.get_state(b), es[b].state())
    f.close()


@pytest.mark.parametrize("idknown", [1, 0])
def test_streamed_class_walks_messages_of_any_length(S, oracle, idknown):
    """The HBM-streamed class follows the reference's loop detection by detection (ekf.cpp:73): per-instance external messages with
    repeated ids, ids beyond the capacity (SLAM_INST_CAPACITY), MORE detections than landmarks (no per-message limit here), a repeat
    of an id the message itself inserted (the reference dies: frozen in the pre-step state); known and unknown ids."""
    L, B, T = 230, 4, 10
    cfg = S.default_config(); cfg.landmark_id_is_known = idknown
    f = S.BatchedEKF(B, L).readParams(cfg); f.init(0.0, 0.0, 0.0)
    es = []
    for b in range(B):
        e = oracle.OracleEKF(cfg, L_max=L); e.init(0, 0, 0); es.append(e)
    rng = np.random.default_rng(5 + idknown)
    of = np.zeros(B, dtype=np.int64)
    for t in range(T):
        cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
        ks = rng.integers(0, 300, B)
        if t == 0: ks[:] = 250                      # a first look at more ids than the capacity
        if t == 3: ks[0] = 0
        K = max(1, int(ks.max()))
        meas = np.zeros((B, K, 3), dtype=np.float32)
        for b in range(B):
            k = int(ks[b])
            ids = rng.integers(0, 260, k)
            if t == 0: ids = rng.permutation(260)[:k]   # distinct at first (no freeze at the first step) ...
            if t == 6 and b == 1 and k > 3: ids[:3] = [900, 901, 900]   # ... later a repeat of a new id
            meas[b, :k, 0] = ids
            meas[b, :k, 1] = rng.uniform(0.5, 6.0, k)
            meas[b, :k, 2] = rng.uniform(-3.1, 3.1, k)
        f.update(cmd, meas, ks.astype(np.int32))
        for b in range(B):
            of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
    assert np.array_equal(f.status().astype(np.int64), of)
    for b in range(B):
        so, sg = es[b].state(), f.get_state(b)
        assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
        assert np.array_equal(sg["x"], so["x"]) and np.array_equal(sg["P"], so["P"]), b
    f.close()


@pytest.mark.parametrize("L,idknown", [(20, 1), (50, 1), (50, 0), (100, 1)])
def test_over_long_host_messages_walk_every_detection_in_the_lds_classes(S, oracle, L, idknown):
    """ekf.cpp:65,73 walk a message of any length; the LDS size classes hold L_class detections per message and drop
    the surplus with SLAM_INST_CAPACITY.  Round 5: slam_step sees the counts, so the instances whose message is beyond the class's capacity
    take that one timestep through the HBM-streamed kernel (same state layout, same arithmetic; the LDS kernel of the same launch pair skips
    them, EkfStepParams::long_mode): fp64 EKF handles now follow the oracle WITHOUT its per-message limit, interleaved with ordinary messages
    (fast kernel, queued and immediate) in the same batch and from step to step, bit for bit and flag for flag.  fp32 storage too: the
    streamed kernel reads and writes floats and runs the timestep in the handle's fp64 slab, which is the oracle's STORAGE_F32 (x_t and
    P_t rounded once per timestep).  The oracle has no per-message limit any more."""
    cap = 20 if L <= 20 else (50 if L <= 50 else 100)
    for f32 in (False, True):
        if f32 and L > 50:
            continue
        B, T = 4, 12
        cfg = S.default_config(); cfg.landmark_id_is_known = idknown
        f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams(cfg); f.init(0.0, 0.0, 0.0)
        es = []
        for b in range(B):
            e = oracle.OracleEKF(cfg, L_max=L, mode=oracle.MODE_FAST | (oracle.STORAGE_F32 if f32 else 0))
            e.init(0, 0, 0); es.append(e)
        rng = np.random.default_rng(11 + L + idknown)
        of = np.zeros(B, dtype=np.int64)
        for t in range(T):
            cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
            ks = rng.integers(0, 4, B)                        # ordinary messages ...
            if t in (2, 5, 6, 9): ks[rng.integers(0, B)] = cap + int(rng.integers(1, 40))   # ... and over-long ones, for one instance at a time
            if t == 7: ks[:] = cap + 5
            K = max(1, int(ks.max()))
            meas = np.zeros((B, K, 3), dtype=np.float32)
            for b in range(B):
                k = int(ks[b])
                meas[b, :k, 0] = rng.integers(0, L + 10, k)   # repeated ids and ids beyond the capacity included
                meas[b, :k, 1] = rng.uniform(0.5, 6.0, k)
                meas[b, :k, 2] = rng.uniform(-3.1, 3.1, k)
            f.update(cmd, meas, ks.astype(np.int32))
            for b in range(B):
                of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
        assert np.array_equal(f.status().astype(np.int64), of), (f32, f.status(), of)
        for b in range(B):
            if of[b] & 4:
                continue    # frozen in the pre-step state by a repeat of a freshly inserted id: compared through the flags
            so, sg = es[b].state(), f.get_state(b)
            assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
            assert np.array_equal(sg["x"], so["x"]) and np.array_equal(sg["P"], so["P"]), (f32, b)
        f.close()


@pytest.mark.parametrize("L", [60, 210])
def test_fp32_storage_beyond_the_lds_classes(S, oracle, L):
    """fp32 storage of x and P ended at 50 landmarks (the LDS classes instantiated for it; SLAM_ERR_UNSUPPORTED beyond).  Round 5: the HBM-streamed
    kernel reads and writes floats and runs the timestep in the handle's fp64 slab - the oracle's STORAGE_F32 (x_t, P_t rounded once per
    timestep) - so an fp32 handle takes any capacity the fp64 one does.  Device-generated messages with a first look at the whole map, and
    external messages with repeated ids and ids beyond the capacity; bit-identical to the oracle."""
    from live_ekf_slam_amd.scenario import make_scenario
    B, T = 3, 12
    lm, cmds = make_scenario(17, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[5] = [1e9, -4.0, 4.0]
    omode = oracle.MODE_FAST | oracle.STORAGE_F32
    f = S.BatchedEKF(B, L, dtype=S.F32).readParams(); f.set_map(lm); f.set_seed(6); f.init(0, 0, 0)
    for t in range(T):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=6, nthreads=3, mode=omode, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    n = 3 + 2 * L
    for b in range(B):
        _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()
    f = S.BatchedEKF(2, L, dtype=S.F32).readParams(); f.init(0.0, 0.0, 0.0)
    es = []
    for b in range(2):
        e = oracle.OracleEKF(S.default_config(), L_max=L, mode=omode); e.init(0, 0, 0); es.append(e)
    rng = np.random.default_rng(L)
    of = np.zeros(2, dtype=np.int64)
    for t in range(6):
        cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
        ks = np.array([L + 20 if t == 0 else int(rng.integers(0, 30)) for _ in range(2)])
        K = max(1, int(ks.max()))
        meas = np.zeros((2, K, 3), dtype=np.float32)
        for b in range(2):
            k = int(ks[b])
            meas[b, :k, 0] = rng.permutation(L + 30)[:k] if t == 0 else rng.integers(0, L + 30, k)
            meas[b, :k, 1] = rng.uniform(0.5, 6.0, k); meas[b, :k, 2] = rng.uniform(-3.1, 3.1, k)
        f.update(cmd, meas, ks.astype(np.int32))
        for b in range(2):
            of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
    assert np.array_equal(f.status().astype(np.int64), of)
    for b in range(2):
        if of[b] & 4:
            continue
        so, sg = es[b].state(), f.get_state(b)
        assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
        assert np.array_equal(sg["x"], so["x"]) and np.array_equal(sg["P"], so["P"]), b
    f.close()


@pytest.mark.parametrize("f32", [False, True])
def test_long_messages_from_device_buffers_and_from_the_generator(S, oracle, f32):
    """The other two entry points of the same limit.  slam_step_dev: the counts are on the device, so the caller's stride is the bound - a
    stride beyond the class's capacity runs the launch pair (LDS kernel for the instances whose message fits, streamed kernel for the others,
    EkfStepParams::long_mode), a stride within it the LDS kernel alone.  SIM mode: a map with more landmarks than a message of the class
    holds (30 on a 20-landmark handle: the state fills up and says so, but every detection of a KNOWN landmark is still an update,
    ekf.cpp:73) takes the streamed kernel.  Bit for bit and flag for flag against the oracle without a per-message limit."""
    import ctypes as C
    from live_ekf_slam_amd.scenario import make_scenario
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    L, B, T, KS = 20, 5, 10, 48
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), B * KS * 3 * 4) == 0 and hip.hipMalloc(C.byref(d_cnt), B * 4) == 0
    dt, omode = (S.F32, oracle.MODE_FAST | oracle.STORAGE_F32) if f32 else (S.F64, oracle.MODE_FAST)
    for lazy in (0, 8):
        f = S.BatchedEKF(B, L, dtype=dt).readParams(); f.init(0.0, 0.0, 0.0)
        if lazy: f.set_lazy_steps(lazy)
        es = []
        for b in range(B):
            e = oracle.OracleEKF(S.default_config(), L_max=L, mode=omode); e.init(0, 0, 0); es.append(e)
        rng = np.random.default_rng(77)
        of = np.zeros(B, dtype=np.int64)
        for t in range(T):
            cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
            ks = rng.integers(0, 4, B)
            if t in (1, 4, 5, 8): ks[rng.integers(0, B)] = 21 + int(rng.integers(0, 27))
            K = KS if t % 3 else 16                       # strides beyond and within the capacity alternate
            ks = np.minimum(ks, K)
            meas = np.zeros((B, K, 3), dtype=np.float32)
            for b in range(B):
                k = int(ks[b])
                meas[b, :k, 0] = rng.integers(0, L + 6, k)
                meas[b, :k, 1] = rng.uniform(0.5, 6.0, k)
                meas[b, :k, 2] = rng.uniform(-3.1, 3.1, k)
            cnt = ks.astype(np.int32)
            f.sync()                                       # (the buffers are re-used: the previous step has read them)
            assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0
            assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0
            f.update_dev(cmd, d_meas.value, d_cnt.value, K)
            for b in range(B):
                of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
        assert np.array_equal(f.status().astype(np.int64), of), (lazy, f.status(), of)
        for b in range(B):
            if of[b] & 4:
                continue
            so, sg = es[b].state(), f.get_state(b)
            assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
            assert np.array_equal(sg["x"], so["x"]) and np.array_equal(sg["P"], so["P"]), (lazy, b)
        f.close()
    Lm, T = 30, 40
    lm, cmds = make_scenario(9, Lm, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[7] = [1e9, -4.0, 4.0]; vis[8] = [1e9, -4.0, 4.0]
    for chunked in (False, True):
        f = S.BatchedEKF(6, L, dtype=dt).readParams(); f.set_map(lm); f.set_seed(4); f.init(0, 0, 0)
        if chunked:
            for t in range(T):
                f.set_vision(*vis[t]); f.update_sim(cmds[t])
        else:
            f.set_vision(1e9, -4.0, 4.0); f.run_sim(cmds)
        r = oracle.run_ekf_batch(lm, cmds, 6, L, seed=4, nthreads=3, mode=omode, vision=vis if chunked else np.tile([1e9, -4.0, 4.0], (T, 1)))
        assert np.all(r["M"] == L) and np.all(r["flags"] & 8) and np.array_equal(f.status(), r["flags"])
        assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
        n = 3 + 2 * L
        for b in range(6):
            _assert_state_equal(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
        f.close()


@pytest.mark.parametrize("kind", ["ekf", "ekf_f32", "ukf"])
def test_checkpoint_and_resume_are_bit_identical(S, tmp_path, kind):
    """slam_save_state / slam_load_state (the reference keeps the filter only in memory): a run continued from a checkpoint
    in a NEW handle equals the uninterrupted run bit for bit - state, counters, error statistics, true poses."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T1, T2 = 20, 48, 70, 60
    lm, cmds = make_scenario(5, L, T1 + T2)
    def make():
        if kind == "ukf":
            f = S.BatchedUKF(B, L).readParams()
        else:
            f = S.BatchedEKF(B, L, dtype=S.F32 if kind == "ekf_f32" else S.F64).readParams()
        f.set_map(lm); f.set_seed(21); f.set_instance_offset(300)
        return f
    a = make(); a.init(0, 0, 0); a.run_sim(cmds[:T1])
    path = tmp_path / "batch.ckpt"
    a.save_state(path)
    a.run_sim(cmds[T1:])
    b = make(); b.load_state(path); b.run_sim(cmds[T1:])
    assert np.array_equal(a.landmark_counts(), b.landmark_counts()) and np.array_equal(a.status(), b.status())
    assert np.array_equal(a.error_stats(), b.error_stats()) and np.array_equal(a.truth(), b.truth())
    for i in (0, 17, B - 1):
        sa, sb = a.get_state(i), b.get_state(i)
        assert sa["timestep"] == sb["timestep"] == T1 + T2 and sa["M"] == sb["M"] and np.array_equal(sa["ids"], sb["ids"])
        assert np.array_equal(sa["x"], sb["x"]) and np.array_equal(sa["P"], sb["P"])
    # a file of another shape is refused, a truncated one too
    c = S.BatchedEKF(B + 1, L).readParams()
    with pytest.raises(Exception):
        c.load_state(path)
    raw = open(path, "rb").read()
    open(tmp_path / "short.ckpt", "wb").write(raw[:len(raw) // 2])
    with pytest.raises(Exception):
        make().load_state(tmp_path / "short.ckpt")
    for f in (a, b, c):
        f.close()


@pytest.mark.parametrize("L,T,B,seed,scenario,inst0,f32,idknown,wide,chunk,split", [
    (50, 319, 7, 266407250, 165103127, 500196, True, 1, False, 3, 269),     # fp32: a timestep with more updates than ring slots (watchdog)
    (5, 398, 14, 904105935, 949266288, 153131, True, 1, True, 32, 281),      # fp32: five new landmarks in the first message (watchdog)
    (35, 180, 5, 836420149, 169661810, 226515, True, 0, True, 32, 90),       # unknown ids, wide sensor, full map: memory fault
    (35, 180, 5, 836420149, 169661810, 226515, False, 0, True, 32, 90),      # the same in fp64: neighbours' M / flags overwritten
    (150, 26, 6, 177541356, 1028310476, 83458, False, 0, True, 3, 14),
    (35, 393, 23, 409736089, 89432125, 553749, False, 0, True, 32, 164),
])
def test_configurations_the_random_soak_found(S, oracle, monkeypatch, L, T, B, seed, scenario, inst0, f32, idknown, wide, chunk, split):
    """tools/gpu_soak_ekf.py (random sizes / seeds / modes against the oracle) found two bugs in round 3: (1) unknown-id mode
    provisioned the step's matrix for k insertions even when the capacity had no room left - rows past the instance's slab; (2)
    the fp32 decoupled loop admitted timesteps with more updates than ring slots (its passes must end at a step end) - a
    deadlock the in-kernel watchdog turned into SLAM_INST_WATCHDOG.  These are the configurations it reported, replayed:
    flags equal the oracle's for every instance, state bit-exact for every unflagged one."""
    from live_ekf_slam_amd.scenario import make_scenario
    monkeypatch.setenv("SLAM_RUN_CHUNK", str(chunk))
    monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)
    lm, cmds = make_scenario(scenario, L, T)
    cfg = S.default_config(); cfg.landmark_id_is_known = idknown
    if wide:
        cfg.range_max = 1e9; cfg.fov_min = -4.0; cfg.fov_max = 4.0
    f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams(cfg)
    f.set_map(lm); f.set_seed(seed); f.set_instance_offset(inst0); f.init(0, 0, 0)
    f.run_sim(cmds[:split]); f.run_sim(cmds[split:])
    r = oracle.run_ekf_batch(lm, cmds, B, L, seed=seed, inst0=inst0, nthreads=8, cfg=cfg, mode=oracle.MODE_FAST | (oracle.STORAGE_F32 if f32 else 0))
    assert np.array_equal(f.status(), r["flags"]) and np.array_equal(f.truth(), r["truth"])
    clean = r["flags"] == 0
    assert np.array_equal(f.landmark_counts()[clean], r["M"][clean])
    for b in np.flatnonzero(clean):
        n = 3 + 2 * r["M"][b]
        _assert_state_equal(f.get_state(int(b)), dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()
