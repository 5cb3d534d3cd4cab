"""GPU parity tests for UKF-SLAM: the two HIP kernels per step (Jacobi eigen-sqrt; predict + update) against the
CPU oracle.  Tolerance: ZERO — x, P, M, ids, truth, error statistics and flags must be bit-identical (the oracle
runs the same parallel-order Jacobi schedule and the same sequential accumulation orders)."""
import numpy as np
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _eq(sg, so):
    assert sg["M"] == so["M"] and np.array_equal(sg["ids"], so["ids"])
    assert np.array_equal(sg["x"], so["x"]), np.abs(sg["x"] - so["x"]).max()
    assert np.array_equal(sg["P"], so["P"]), np.abs(sg["P"] - so["P"]).max()


@pytest.mark.parametrize("fixture,L_max,T", [("sim_seed0_L20_T1000.npz", 20, 400), ("sim_seed2_L50_T1000.npz", 50, 260),
                                             ("sim_seed1_L20_T400.npz", 50, 150)])
def test_ukf_update_on_reference_measurement_stream(S, oracle, fixture, L_max, T):
    g = load_golden(fixture)
    B = 3
    f = S.BatchedUKF(B, L_max).readParams(); f.init(0.0, 0.0, 0.0)
    u = oracle.OracleUKF(L_max=L_max); u.init(0, 0, 0)
    for t in range(T):
        k = int(g["meas_count"][t])
        f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())
        u.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
        if t % 10 == 9 or t == T - 1 or t < 4:
            so = u.state()
            for b in (0, B - 1):
                _eq(f.get_state(b), so)
    # workload counters of the two kernels (what bench.py prices the UKF step with): one histogram entry and one
    # eigen-decomposition per instance-step, the detection counts of the stream, the oracle's sweep counts (it also counts the
    # final sweep that only writes zeros, which the kernel skips: DESIGN.md 4.2)
    kh, sw = f.k_histogram(), f.sweep_stats()
    assert int(kh.sum()) == B * T and int(sw[1]) == B * T
    assert int((kh * np.arange(8)).sum()) == B * int(np.minimum(g["meas_count"][:T], 7).sum())
    assert 1.0 <= sw[0] / sw[1] <= 12.0
    assert np.all(f.status() == 0) and u.state()["M"] >= 2
    pub = f.publishState(1)
    assert pub["M"] == u.state()["M"] and pub["P"].dtype == np.float32
    f.close()


@pytest.mark.parametrize("L,T,B", [(20, 200, 48), (50, 120, 24)])
def test_ukf_sim_step_parity(S, oracle, L, T, B):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.set_instance_offset(300); f.init(0, 0, 0)
    f.run_sim(cmds)
    r = oracle.run_ukf_batch(lm, cmds, B, L, seed=5, inst0=300, nthreads=8)
    assert np.array_equal(f.landmark_counts(), r["M"])
    assert np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"])
    assert np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 4 + 2 * r["M"][b]
        _eq(f.get_state(b), dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()


@pytest.mark.parametrize("L", [20, 50])
def test_ukf_growing_state_walks_padded_sizes_bit_exact(S, oracle, L):
    """A map discovered landmark by landmark: the state passes through the sizes n = 2 (mod 4), which the sqrt kernels of the LDS classes
    (and the oracle) pad by two zero rows to walk the quadruple schedule - the pass table at L = 20, the generated passes at L = 50."""
    from live_ekf_slam_amd.scenario import make_scenario
    T, B = 90, 4
    lm, cmds = make_scenario(91, L, T)
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.set_instance_offset(3); f.init(0, 0, 0)
    seen = set()
    for t0 in range(0, T, 15):
        f.run_sim(cmds[t0:t0 + 15])
        seen.update(int(m) for m in f.landmark_counts())
    r = oracle.run_ukf_batch(lm, cmds, B, L, seed=5, inst0=3, nthreads=8)
    assert any(m % 2 == 1 for m in seen), seen          # odd landmark counts = sizes n = 2 (mod 4) were walked
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.error_stats(), r["avg_err"])
    for b in range(B):
        m = int(r["M"][b]); n = 4 + 2 * m
        _eq(f.get_state(b), dict(M=m, ids=r["ids"][b, :m], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))


@pytest.mark.parametrize("L,T,B", [(20, 70, 16), (50, 50, 8)])
def test_ukf_full_state_size_bit_exact(S, oracle, L, T, B):
    """A wide first step maps all L landmarks, so every later step runs both kernels of the size class at its full state size: n = 44
    (sqrt 256 threads with the pass table, step 128) and n = 104 (sqrt 1024 threads with generated passes, step 512)."""
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(77, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(3); f.set_instance_offset(11); f.init(0, 0, 0)
    f.set_vision(*vis[0]); f.run_sim(cmds[:1]); f.set_vision(*vis[1]); f.run_sim(cmds[1:])
    r = oracle.run_ukf_batch(lm, cmds, B, L, seed=3, inst0=11, nthreads=8, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.status(), r["flags"])
    for b in range(B):
        n = 4 + 2 * L
        _eq(f.get_state(b), dict(M=L, ids=r["ids"][b, :L], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
    f.close()


def test_ukf_many_detections_and_config_switches(S, oracle):
    """k = 20 detections at once (> the 8 updates held per pass), non-zero noise means, double-trig switch, V/W quirk off."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 20, 8, 10
    lm, cmds = make_scenario(3, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[4] = [1e9, -4.0, 4.0]; vis[5] = [1e9, -4.0, 4.0]
    for trig, quirk in ((1, 1), (0, 0)):
        cfg = S.default_config(); cfg.ukf_float_trig = trig; cfg.replicate_vw_quirk = quirk; cfg.w_r = 0.01; cfg.v_d = 0.002; cfg.w_b = 0.003
        f = S.BatchedUKF(B, L).readParams(cfg); f.set_map(lm); f.set_seed(9); f.init(0.2, -0.1, 0.3)
        for t in range(T):
            f.set_vision(*vis[t]); f.update_sim(cmds[t])
        r = oracle.run_ukf_batch(lm, cmds, B, L, seed=9, cfg=cfg, nthreads=4, vision=vis)
        # the oracle batch runner starts from cfg.init_*; run it from the same pose
        cfg2 = cfg.copy(); cfg2.init_x, cfg2.init_y, cfg2.init_yaw = 0.0, 0.0, 0.0
        assert np.all(r["M"] == L)
        g = S.BatchedUKF(B, L).readParams(cfg); g.set_map(lm); g.set_seed(9); g.init(0.0, 0.0, 0.0)
        for t in range(T):
            g.set_vision(*vis[t]); g.update_sim(cmds[t])
        for b in range(B):
            _eq(g.get_state(b), dict(M=L, ids=r["ids"][b], x=r["x"][b], P=r["P"][b].reshape(44, 44)))
        assert np.all(np.isfinite(f.poses()))
        f.close(); g.close()


@pytest.mark.parametrize("switch,L", [("ukf_accumulate_zest1", 20), ("ukf_sensing_yaw_from_sigma", 20), ("ukf_accumulate_zest1", 60), ("ukf_sensing_yaw_from_sigma", 60)])
def test_appendix_d_quirk_switches_ukf(S, oracle, switch, L):
    """`ukf_accumulate_zest1` (D-8: z_est(1) accumulated instead of left at 0, ukf.cpp:310-314) and `ukf_sensing_yaw_from_sigma` (D-9: the
    sensing model's yaw from its sigma-point argument instead of x_t, ukf.cpp:139).  Switched ON kernel and oracle agree bit for bit and the
    result differs from the default; LDS class (L = 20) and HBM-streamed class (L = 60)."""
    from live_ekf_slam_amd.scenario import make_scenario
    B, T = 4, 120 if L == 20 else 60
    lm, cmds = make_scenario(1234, L, T)
    res = {}
    for on in (0, 1):
        cfg = S.default_config(); cfg.w_r = 0.01; cfg.w_b = 0.003
        setattr(cfg, switch, on)
        f = S.BatchedUKF(B, L).readParams(cfg); f.set_map(lm); f.set_seed(9); f.init(0, 0, 0)
        f.run_sim(cmds)
        r = oracle.run_ukf_batch(lm, cmds, B, L, seed=9, cfg=cfg, nthreads=4)
        assert r["M"].max() >= 2
        for b in range(B):
            n = 4 + 2 * r["M"][b]
            _eq(f.get_state(b), dict(M=r["M"][b], ids=r["ids"][b, :r["M"][b]], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)))
        res[on] = f.get_state(0)["x"].copy()
        f.close()
    assert res[0].shape != res[1].shape or not np.array_equal(res[0], res[1])


def test_ukf_loc_mode(S, oracle):
    """FilterChoice::UKF_LOC (ukf.cpp:146-154, localization_node.cpp:39-41,152-156): vehicle-only state, every
    detection updates against the known (float32) map; host-fed reference stream and device-generated streams."""
    g = load_golden("sim_seed0_L20_T1000.npz")
    B = 3
    f = S.BatchedUKFLoc(B).readParams()
    with pytest.raises(S.SlamError):
        f.init(0, 0, 0); f.update((0.1, 0.0), [])        # no map yet (localization_node.cpp:113-116)
    f.set_map(g["map"]); f.init(0.0, 0.0, 0.0)
    u = oracle.OracleUKF(L_max=1); u.set_loc_map(g["map"]); u.init(0, 0, 0)
    for t in range(300):
        k = int(g["meas_count"][t])
        f.update(g["cmds"][t], g["meas"][t, :k].ravel()); u.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
        if t % 25 == 24:
            _eq(f.get_state(B - 1), u.state())
    so = u.state()
    assert so["M"] == 0 and so["x"].shape == (4,)
    assert np.hypot(*(so["x"][:2] - g["truth"][299][:2])) < 0.5
    f.close()
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, 20, 200)
    f = S.BatchedUKFLoc(32).readParams(); f.set_map(lm); f.set_seed(8); f.init(0, 0, 0); f.run_sim(cmds)
    r = oracle.run_ukf_batch(lm, cmds, 32, 1, seed=8, nthreads=4, loc=True)
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    for b in range(32):
        _eq(f.get_state(b), dict(M=0, ids=r["ids"][b, :0], x=r["x"][b, :4], P=r["P"][b, :16].reshape(4, 4)))
    f.close()


def test_prediction_and_update_stage_split_equals_fused_update(S):
    """UKF::predictionStage + UKF::updateStage (filter.h:187-188) as two calls == UKF::update, bit for bit; the state
    is untouched between the two calls (ukf.cpp:289-290), and UKFState.X holds the sigma points of that step."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")   # the runtime libslam_hip.so itself links (device buffers without torch)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    g = load_golden("sim_seed0_L20_T1000.npz")
    B, L, T = 4, 20, 120
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), B * 8 * 3 * 4) == 0 and hip.hipMalloc(C.byref(d_cnt), B * 4) == 0
    a = S.BatchedUKF(B, L).readParams(); a.init(0.0, 0.0, 0.0)
    b = S.BatchedUKF(B, L).readParams(); b.init(0.0, 0.0, 0.0)
    for t in range(T):
        k = int(g["meas_count"][t])
        cmd = S.Command(g["cmds"][t, 0], g["cmds"][t, 1])
        a.update(cmd, g["meas"][t, :k].ravel())
        before = b.get_state(1)
        b.predictionStage(cmd)
        mid = b.get_state(1)
        assert np.array_equal(mid["x"], before["x"]) and np.array_equal(mid["P"], before["P"])
        ks = 8
        meas = np.zeros((B, ks, 3), dtype=np.float32)
        meas[:, :k] = g["meas"][t, :k]
        cnt = np.full(B, k, dtype=np.int32)
        assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0   # hipMemcpyHostToDevice
        assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0
        b.updateStage(d_meas.value, d_cnt.value, ks)
        b.sync()
        if t % 20 == 19 or t < 3:
            for i in (0, B - 1):
                _eq(b.get_state(i), a.get_state(i))
            # sigma points of this step: X = [x, x + sqtP cols, x - sqtP cols] around the pre-step state, and
            # sqtP^2 == nearestSPD scaling of the pre-step covariance (ukf.cpp:106-123,208,214-219)
            X = b.sigma_points(1)
            n = len(before["x"])
            assert X.shape == (n, 2 * n + 1) and np.array_equal(X[:, 0], before["x"])
            Sq = X[:, 1:n + 1] - X[:, [0]]
            assert np.allclose(X[:, n + 1:] - X[:, [0]], -Sq, rtol=0, atol=1e-15)
            scale = float(np.float32(2 * before["M"] + 4) / (np.float32(1) - np.float32(0.2)))
            A = 0.5 * (before["P"] + before["P"].T) * scale
            w, V = np.linalg.eigh(A)                       # nearestSPD clamps the spectrum at 1e-8 (ukf.cpp:119)
            S_ref = (V * np.sqrt(np.maximum(w, 1e-8))) @ V.T
            assert np.abs(Sq - S_ref).max() < 1e-9 * max(1.0, np.abs(S_ref).max())
    pub = b.publishState(0)
    n_prev = b.sigma_points(0).shape[0]
    assert pub["X"].dtype == np.float32 and pub["X"].size == n_prev * (2 * n_prev + 1)
    with pytest.raises(S.SlamError):
        b.updateStage()                       # no prediction pending
    b.predictionStage(S.Command(0.1, 0.0))
    with pytest.raises(S.SlamError):
        b.update(S.Command(0.1, 0.0), [])     # a full step while a prediction stage is pending
    b.updateStage()
    e = S.BatchedEKF(2, 5).readParams(); e.init(0, 0, 0)
    with pytest.raises(S.SlamError):
        S._lib.check(S._lib.lib().slam_predict(e.h, (C.c_float * 2)(0.1, 0.0)))   # the EKF has no separate stages
    a.close(); b.close(); e.close()


def test_run_sim_two_stream_split_is_bit_identical(S, oracle, monkeypatch):
    """Batches >= 1024 run their halves on two streams in run_sim: same results as one stream, and as the oracle."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 20, 40, 1024
    lm, cmds = make_scenario(1234, L, T)
    outs = []
    for split_min in ("1000000", "1024"):
        monkeypatch.setenv("SLAM_UKF_SPLIT_MIN", split_min)
        f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.set_instance_offset(40); f.init(0, 0, 0)
        f.run_sim(cmds[:T // 2]); f.run_sim(cmds[T // 2:])
        outs.append((f.poses(), f.landmark_counts(), f.error_stats(), f.status(), [f.get_state(b) for b in (0, 511, 512, 1023)]))
        f.close()
    a, b = outs
    for i in range(4):
        assert np.array_equal(a[i], b[i])
    for sa, sb in zip(a[4], b[4]):
        _eq(sa, sb)
    for k, inst in enumerate((0, 511, 512, 1023)):
        r = oracle.run_ukf_batch(lm, cmds, 1, L, seed=5, inst0=40 + inst, nthreads=1)
        n = 4 + 2 * r["M"][0]
        _eq(b[4][k], dict(M=r["M"][0], ids=r["ids"][0, :r["M"][0]], x=r["x"][0, :n], P=r["P"][0, :n * n].reshape(n, n)))


@pytest.mark.parametrize("L", [20, 50])
def test_bench_scenario_raises_no_flags(S, L):
    """The secondary bench lines (bench.py --filter ukf, L=20 and L=50) on a small batch: no instance may flag (a Jacobi sign
    convention that cycled on equal eigenvalues went unnoticed by the parity tests, because the oracle cycled with it)."""
    from live_ekf_slam_amd.scenario import make_scenario
    T, B = 131, 64
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    f.set_vision(1e9, -4.0, 4.0); f.update_sim(cmds[0]); f.set_vision(3.0, -1.57, 1.57)
    f.run_sim(cmds[1:T])
    assert not f.status().any(), f.status()
    assert (f.landmark_counts() == L).all()
    sw = f.sweep_stats()
    assert int(sw[1]) == B * T and 2.0 <= sw[0] / sw[1] <= 8.0
    f.close()


def test_ukf_loc_on_a_map_larger_than_the_small_size_class(S, oracle):
    """UKF_LOC keeps a 4-state filter whatever the map: a map of 35 landmarks with the whole of it in view (35 detections per
    message) must use every detection (ukf.cpp:146-154).  The step kernel's small size class holds 20 detections per message; the
    launcher now takes the large one for maps of more than 20 landmarks (tools/gpu_soak_ekf.py found SLAM_INST_CAPACITY here)."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 35, 60, 9
    lm, cmds = make_scenario(31, L, T)
    cfg = S.default_config(); cfg.range_max = 1e9; cfg.fov_min = -4.0; cfg.fov_max = 4.0
    f = S.BatchedUKFLoc(B).readParams(cfg); f.set_map(lm); f.set_seed(3); f.set_instance_offset(17); f.init(0, 0, 0)
    f.run_sim(cmds[:25]); f.run_sim(cmds[25:])
    r = oracle.run_ukf_batch(lm, cmds, B, 1, seed=3, inst0=17, nthreads=4, cfg=cfg, loc=True)
    assert not f.status().any() and not r["flags"].any()
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    for b in range(B):
        _eq(f.get_state(b), dict(M=0, ids=r["ids"][b, :0], x=r["x"][b, :4], P=r["P"][b, :16].reshape(4, 4)))
    f.close()


def _hip_buffers(nbytes_meas, nbytes_cnt):
    import ctypes as C
    hip = C.CDLL("libamdhip64.so")   # the runtime libslam_hip.so itself links (device buffers without torch)
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), nbytes_meas) == 0 and hip.hipMalloc(C.byref(d_cnt), nbytes_cnt) == 0
    def put(meas, cnt):
        assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0   # hipMemcpyHostToDevice
        assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0
    return d_meas, d_cnt, put


@pytest.mark.parametrize("L,entry", [(20, "host"), (20, "stages"), (50, "host")])
def test_ukf_over_long_messages_walk_every_detection_in_the_lds_classes(S, oracle, L, entry):
    """VERDICT r04 item 5 for the UKF: ukf.cpp:249-287 walk a message of any length; the LDS size classes of the step kernel hold 20 / 50
    detections of one message.  A launch whose messages may be longer is now a PAIR of launches: the LDS kernel leaves the instances whose
    message it cannot hold untouched and the HBM-streamed step kernel takes exactly those (UkfStepParams::long_mode) - the sqrt kernel, and
    with it the Jacobi schedule, stays the class's own.  Ordinary and over-long messages side by side in one batch and from step to step,
    repeated ids and ids beyond the capacity, through slam_step (host buffers) and slam_predict + slam_update_dev (device buffers, the
    caller's stride as the bound): the oracle WITHOUT a per-message limit, bit for bit and flag for flag."""
    cap = 20 if L <= 20 else 50
    B, T = 4, 9 if L <= 20 else 6
    KS = cap + 45
    f = S.BatchedUKF(B, L).readParams(); f.init(0.0, 0.0, 0.0)
    es = [oracle.OracleUKF(L_max=L) for _ in range(B)]
    for e in es: e.init(0, 0, 0)
    if entry == "stages":
        d_meas, d_cnt, put = _hip_buffers(B * KS * 3 * 4, B * 4)
    rng = np.random.default_rng(3 + L)
    of = np.zeros(B, dtype=np.int64)
    for t in range(T):
        cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
        ks = rng.integers(0, 4, B)                                                        # ordinary messages ...
        if t in (1, 3, 4, 7): ks[rng.integers(0, B)] = cap + int(rng.integers(1, 40))   # ... and over-long ones, for one instance at a time
        if t == 5: ks[:] = cap + 5
        K = KS if entry == "stages" else max(1, int(ks.max()))
        meas = np.zeros((B, K, 3), dtype=np.float32)
        for b in range(B):
            k = int(ks[b])
            meas[b, :k, 0] = rng.integers(0, L + 10, k)
            meas[b, :k, 1] = rng.uniform(0.5, 6.0, k)
            meas[b, :k, 2] = rng.uniform(-3.1, 3.1, k)
        if entry == "stages":
            put(meas, ks.astype(np.int32))
            f.predictionStage(S.Command(cmd[0], cmd[1])); f.updateStage(d_meas.value, d_cnt.value, K); f.sync()
        else:
            f.update(cmd, meas, ks.astype(np.int32))
        for b in range(B):
            of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
    assert np.array_equal(f.status().astype(np.int64), of), (f.status(), of)
    for b in range(B):
        so = es[b].state()
        _eq(f.get_state(b), dict(M=so["M"], ids=so["ids"], x=so["x"], P=so["P"]))
    f.close()


def test_ukf_loc_messages_longer_than_the_size_class(S, oracle):
    """UKF_LOC sees a map of any size (ukf.cpp:146-154): 80 landmarks, all of them in view - 80 detections per message, the large size class
    holds 50.  Device-generated messages (the map is larger than a message of the class: the streamed step kernel takes the launch) and
    host-fed ones with an id outside the map; every detection is used, nothing is flagged but the foreign id."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 80, 24, 5
    lm, cmds = make_scenario(41, L, T)
    cfg = S.default_config(); cfg.range_max = 1e9; cfg.fov_min = -4.0; cfg.fov_max = 4.0
    f = S.BatchedUKFLoc(B).readParams(cfg); f.set_map(lm); f.set_seed(5); f.init(0, 0, 0)
    f.run_sim(cmds[:10]); f.run_sim(cmds[10:])
    r = oracle.run_ukf_batch(lm, cmds, B, 1, seed=5, nthreads=4, cfg=cfg, loc=True)
    assert not f.status().any() and not r["flags"].any()
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    for b in range(B):
        _eq(f.get_state(b), dict(M=0, ids=r["ids"][b, :0], x=r["x"][b, :4], P=r["P"][b, :16].reshape(4, 4)))
    f.close()
    f = S.BatchedUKFLoc(2).readParams(); f.set_map(lm); f.init(0.0, 0.0, 0.0)
    u = oracle.OracleUKF(L_max=1); u.set_loc_map(lm); u.init(0, 0, 0)
    rng = np.random.default_rng(6)
    fl = 0
    for t in range(8):
        k = 70 if t in (2, 5) else int(rng.integers(0, 6))
        meas = np.zeros((k, 3), dtype=np.float32)
        meas[:, 0] = rng.integers(0, L, k); meas[:, 1] = rng.uniform(0.5, 6.0, k); meas[:, 2] = rng.uniform(-3.1, 3.1, k)
        if t == 5: meas[60, 0] = L + 3
        f.update((0.05, 0.01), meas.ravel())
        fl |= u.update(0.05, 0.01, meas)
    assert fl != 0 and np.all(f.status() == fl)
    _eq(f.get_state(1), u.state())
    f.close()


def test_ukf_state_of_100_landmarks(S, oracle):
    """n = 204: beyond the LDS size classes of the UKF kernels (up to round 3: SLAM_ERR_UNSUPPORTED above 50 landmarks; the reference's
    state grows without a limit, ukf.cpp:357,371).  The HBM-streamed class (ukf_big_kernel.hip): a first look at all 100 landmarks
    (100 insertions in one message), a full second look (100 updates), ordinary steps with warm-started decompositions; device-generated
    messages (per-instance noise) and an external message with a repeated new id and more detections than landmarks.  Bit-identical
    to the oracle, error statistics and true poses included."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 100, 14, 3
    lm, cmds = make_scenario(31, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[6] = [1e9, -4.0, 4.0]
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(12); f.init(0, 0, 0)
    for t in range(T):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
    r = oracle.run_ukf_batch(lm, cmds, B, L, seed=12, nthreads=3, vision=vis)
    assert np.all(r["M"] == L) and np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    n = 4 + 2 * L
    for b in range(B):
        _eq(f.get_state(b), dict(M=L, ids=r["ids"][b], x=r["x"][b], P=r["P"][b].reshape(n, n)))
    f.close()
    # external messages, one oracle per instance: growth over several steps, a repeated NEW id (two insertions, ukf.cpp:279-287),
    # ids beyond the capacity, 130 detections in one message
    L2, B2 = 60, 2
    f = S.BatchedUKF(B2, L2).readParams(); f.init(0.0, 0.0, 0.0)
    es = [oracle.OracleUKF(L_max=L2) for _ in range(B2)]
    for e in es: e.init(0, 0, 0)
    rng = np.random.default_rng(4)
    of = np.zeros(B2, dtype=np.int64)
    for t in range(6):
        cmd = np.array([rng.uniform(0, 0.1), rng.uniform(-0.05, 0.05)], dtype=np.float32)
        ks = np.array([130 if t == 3 else int(rng.integers(0, 25)) for _ in range(B2)])
        K = max(1, int(ks.max()))
        meas = np.zeros((B2, K, 3), dtype=np.float32)
        for b in range(B2):
            kk = int(ks[b])
            ids = rng.integers(0, 70, kk)
            if t == 1 and kk > 2: ids[:3] = [500, 501, 500]
            meas[b, :kk, 0] = ids; meas[b, :kk, 1] = rng.uniform(0.5, 6.0, kk); meas[b, :kk, 2] = rng.uniform(-3.1, 3.1, kk)
        f.update(cmd, meas, ks.astype(np.int32))
        for b in range(B2):
            of[b] |= es[b].update(cmd[0], cmd[1], meas[b, :ks[b]])
    assert np.array_equal(f.status().astype(np.int64), of)
    for b in range(B2):
        so = es[b].state()
        _eq(f.get_state(b), dict(M=so["M"], ids=so["ids"], x=so["x"], P=so["P"]))
    f.close()


@pytest.mark.parametrize("kind", ["ukf", "ukf_loc"])
def test_ukf_checkpoint_round_trips_incl_the_cold_start_marker(S, kind, tmp_path):
    """slam_load_state refused every UKF checkpoint whose warm-start age column held -1 - the cold-start marker
    ukf_init_kernel writes and both sqrt kernels write after SLAM_INST_SQRT_FAILED.  (i) a checkpoint saved right after init
    (every age is -1) loads and continues bit-identically; (ii) so does one taken mid-run; (iii) a mid-run checkpoint in which one
    instance carries the marker (what a failed decomposition leaves behind) loads: that instance restarts its eigenvectors cold - the
    same factor to rounding - and the others continue bit-identically; (iv) an age outside [-1, 100] is still refused."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 20, 6, 40
    lm, cmds = make_scenario(17, L, T)
    def make():
        f = (S.BatchedUKF(B, L) if kind == "ukf" else S.BatchedUKFLoc(B)).readParams(); f.set_map(lm); f.set_seed(9); f.init(0, 0, 0)
        return f

    def states(f):
        return [f.get_state(b) for b in range(B)], f.status().copy(), f.error_stats().copy(), f.truth().copy()

    def same(a, b, skip=()):
        for i, (sa, sb) in enumerate(zip(a[0], b[0])):
            if i in skip:
                continue
            assert sa["M"] == sb["M"] and np.array_equal(sa["ids"], sb["ids"])
            assert np.array_equal(sa["x"], sb["x"]) and np.array_equal(sa["P"], sb["P"])
        keep = [i for i in range(B) if i not in skip]
        assert np.array_equal(a[1], b[1]) and np.array_equal(a[2][keep], b[2][keep]) and np.array_equal(a[3], b[3])

    # (i) save right after init: every age is -1
    a = make(); p0 = tmp_path / "init.ckpt"; a.save_state(p0)
    a.run_sim(cmds[:20])
    b = make(); b.load_state(p0); b.run_sim(cmds[:20])
    same(states(a), states(b))
    # (ii) mid-run
    p1 = tmp_path / "mid.ckpt"; a.save_state(p1)
    a.run_sim(cmds[20:])
    c = make(); c.load_state(p1); c.run_sim(cmds[20:])
    same(states(a), states(c))
    # (iii) instance 2 carries the cold-start marker (the age column is the file's last item)
    raw = bytearray(open(p1, "rb").read())
    ages = np.frombuffer(bytes(raw[-4 * B:]), dtype=np.int32)
    assert np.all(ages >= 0) and np.all(ages <= 100), ages    # 20 warm-started steps behind every instance
    cold = bytearray(raw); cold[-4 * B + 8:-4 * B + 12] = np.int32(-1).tobytes()
    pc = tmp_path / "cold.ckpt"; open(pc, "wb").write(cold)
    d = make(); d.load_state(pc); d.run_sim(cmds[20:])
    sa, sd = states(a), states(d)
    same(sa, sd, skip=(2,))
    assert sa[0][2]["M"] == sd[0][2]["M"] and np.abs(sa[0][2]["x"] - sd[0][2]["x"]).max() < 1e-5 and np.all(np.isfinite(sd[0][2]["P"]))
    # (iv) an impossible age is refused
    bad = bytearray(raw); bad[-4 * B:-4 * B + 4] = np.int32(101).tobytes()
    pb = tmp_path / "bad.ckpt"; open(pb, "wb").write(bad)
    e = make()
    with pytest.raises(S.SlamError, match="age of the warm-start"):
        e.load_state(pb)
    for f in (a, b, c, d, e):
        f.close()
