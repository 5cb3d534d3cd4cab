"""The Cholesky square-root mode of the UKF on the device (slam_ukf_set_sqrt_mode, SLAM_UKF_SQRT_CHOLESKY): ukf_chol_kernel
against the numpy reference of tests/test_ukf_chol_reference.py, the sqtP = L^T contract both consumers rely on, the eigen
fallback, every entry point, the setter's refusals, and that the default path is untouched."""
import ctypes as C

import numpy as np
import pytest

from batch_state import ckpt_layout
from conftest import load_golden
from test_ukf_chol_reference import NumpyUKF, cholesky_lower

pytestmark = pytest.mark.gpu

SLAM_ERR_ARG, SLAM_ERR_UNSUPPORTED = -1, -3


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _eq(sa, sb):
    assert sa["M"] == sb["M"] and np.array_equal(sa["ids"], sb["ids"])
    assert np.array_equal(sa["x"], sb["x"]), np.abs(sa["x"] - sb["x"]).max()
    assert np.array_equal(sa["P"], sb["P"]), np.abs(sa["P"] - sb["P"]).max()


def _scaled(P, M):
    return 0.5 * (P + P.T) * float(np.float32(2 * M + 4) / (np.float32(1) - np.float32(0.2)))


@pytest.mark.parametrize("fixture,L_max", [("sim_seed0_L20_T1000.npz", 20), ("sim_seed2_L50_T1000.npz", 50),
                                           ("sim_seed1_L20_T400.npz", 50)])
def test_cholesky_mode_matches_the_numpy_reference(S, fixture, L_max):
    """(a) x and P within 1e-8 of the numpy Cholesky UKF over 120 steps of a reference stream (the fixtures of
    test_ukf_update_on_reference_measurement_stream); the instances of the batch agree bit for bit; the device counts the same
    factorisations and fallbacks as the reference."""
    g = load_golden(fixture)
    B, T = 3, 120
    f = S.BatchedUKF(B, L_max).readParams(); f.init(0.0, 0.0, 0.0)
    f.set_sqrt_mode("cholesky")
    ref = NumpyUKF("cholesky"); ref.init(0, 0, 0)
    worst = 0.0
    for t in range(T):
        k = int(g["meas_count"][t])
        f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())
        ref.update(g["cmds"][t, 0], g["cmds"][t, 1], [tuple(r) for r in g["meas"][t, :k]])
        if t % 10 == 9 or t == T - 1 or t < 4:
            s0 = f.get_state(0)
            for b in range(1, B):
                _eq(f.get_state(b), s0)
            assert s0["M"] == ref.M and list(s0["ids"]) == ref.ids
            worst = max(worst, np.abs(s0["x"] - ref.x).max(), np.abs(s0["P"] - ref.P).max())
    assert worst < 1e-8, worst
    assert ref.factorisations > 0
    assert f.sqrt_stats().tolist() == [B * ref.factorisations, B * ref.fallbacks]
    assert np.all(f.status() == 0)
    f.close()


def test_factor_is_stored_as_L_transpose_row_major(S):
    """(b) After a Cholesky step the sigma-point offsets X[:, 1:n+1] - x are L itself: lower-triangular with explicit zeros above
    the diagonal and a positive diagonal, and L L^T = Y (the scaled pre-step P) to 1e-12 relative.  Pins the contract that
    sqtP holds L^T row-major, which ukf_step_kernel and slam_get_sigma_points read row by row as the factor's columns."""
    g = load_golden("sim_seed2_L50_T1000.npz")
    f = S.BatchedUKF(2, 50).readParams(); f.init(0.0, 0.0, 0.0)
    f.set_sqrt_mode("cholesky")
    checked = 0
    for t in range(80):
        before = f.get_state(1)
        Y = _scaled(before["P"], before["M"])
        k = int(g["meas_count"][t])
        f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())
        Lr = cholesky_lower(Y)
        if Lr is None or np.diag(Lr).min() < 1e-3:   # the fallback, or a pivot close to the floor: not a clean test of the layout
            continue
        X = f.sigma_points(1)
        n = len(before["x"])
        assert X.shape == (n, 2 * n + 1) and np.array_equal(X[:, 0], before["x"])
        L = X[:, 1:n + 1] - X[:, [0]]
        assert np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0)
        assert np.abs(L @ L.T - Y).max() <= 1e-12 * np.abs(Y).max()
        assert np.abs(L - Lr).max() < 1e-9 * max(1.0, np.abs(Lr).max())
        checked += 1
    assert checked >= 5, checked
    f.close()


def test_default_and_explicit_eigen_stay_bit_identical_to_the_oracle(S, oracle):
    """(c) A new handle, and one set to "eigen" before its first step, are the reference path, bit for bit."""
    g = load_golden("sim_seed0_L20_T1000.npz")
    B, L, T = 2, 20, 60
    a = S.BatchedUKF(B, L).readParams(); a.init(0.0, 0.0, 0.0)
    b = S.BatchedUKF(B, L).readParams(); b.set_sqrt_mode("eigen"); b.init(0.0, 0.0, 0.0)
    u = oracle.OracleUKF(L_max=L); u.init(0, 0, 0)
    for t in range(T):
        k = int(g["meas_count"][t])
        for f in (a, b):
            f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())
        u.update(g["cmds"][t, 0], g["cmds"][t, 1], g["meas"][t, :k])
    so = u.state()
    for f in (a, b):
        for i in range(B):
            _eq(f.get_state(i), so)
        assert f.sqrt_stats().tolist() == [0, 0] and int(f.sweep_stats()[1]) == B * T
        f.close()


def _ckpt_layout(f, path):
    """The checkpoint's bytes, the byte offset of the P slab, the P stride and the byte offset of the warm-start age column
    (tests/batch_state.py: ckpt_layout)."""
    head, off, hd = ckpt_layout(path)
    return bytearray(open(path, "rb").read()), head, hd["pstride"], off["age"][0]


def test_fallback_on_an_indefinite_P_is_the_cold_eigen_step(S, tmp_path):
    """(d) A checkpoint taken on a reference stream right before a step whose P factors (the reference's signed process noise
    leaves P indefinite on many steps, so the step is picked with the numpy reference).  One instance gets an indefinite P (a
    negative last diagonal entry: its last pivot is negative) and the cold-start marker.  A Cholesky handle then factors every other
    instance and sends exactly that one to the eigen path, counted, not flagged; its step is bit-identical to an eigen handle's on
    the same checkpoint (both start Jacobi cold)."""
    g = load_golden("sim_seed1_L20_T400.npz")
    B, L, bad = 4, 20, 2
    ref = NumpyUKF("eigh"); ref.init(0, 0, 0)
    t0 = None
    for t in range(120):
        Lr = cholesky_lower(ref.scaled())
        if t >= 10 and ref.M >= 2 and Lr is not None and np.diag(Lr).min() > 1e-3:
            t0 = t
            break
        k = int(g["meas_count"][t])
        ref.update(g["cmds"][t, 0], g["cmds"][t, 1], [tuple(r) for r in g["meas"][t, :k]])
    assert t0 is not None

    def make(mode):
        f = S.BatchedUKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode(mode)
        return f

    def step(f, t):
        k = int(g["meas_count"][t])
        f.update(S.Command(g["cmds"][t, 0], g["cmds"][t, 1]), g["meas"][t, :k].ravel())

    src = make("eigen")
    for t in range(t0):
        step(src, t)
    p0 = tmp_path / "plain.ckpt"; src.save_state(p0)
    M = int(src.landmark_counts()[bad]); n = 4 + 2 * M
    assert M == ref.M
    raw, head, ps, age_off = _ckpt_layout(src, p0)
    off = head + 8 * (bad * ps + (n - 1) * n + (n - 1))
    raw[off:off + 8] = np.float64(-1.0).tobytes()
    raw[age_off + 4 * bad:age_off + 4 * bad + 4] = np.int32(-1).tobytes()
    pc = tmp_path / "indefinite.ckpt"; open(pc, "wb").write(bytes(raw))
    e = make("eigen"); e.load_state(pc); step(e, t0)
    c = make("cholesky"); c.load_state(pc); step(c, t0)
    assert c.sqrt_stats().tolist() == [B - 1, 1]
    _eq(c.get_state(bad), e.get_state(bad))
    assert np.array_equal(c.sigma_points(bad), e.sigma_points(bad))
    assert c.status()[bad] == e.status()[bad]
    for b in range(B):
        if b != bad:
            X = c.sigma_points(b)
            assert np.all(np.triu(X[:, 1:n + 1] - X[:, [0]], 1) == 0)      # the others factored
    for f in (src, e, c):
        f.close()


def test_every_entry_point_honours_the_mode(S, monkeypatch):
    """(e) Cholesky mode through each launch site: predictionStage + updateStage == update (host messages); run_sim with the batch
    split over streams == update_sim step by step == update fed the messages update_sim generated."""
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    g = load_golden("sim_seed0_L20_T1000.npz")
    B, L, T = 4, 20, 80
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), B * 8 * 3 * 4) == 0 and hip.hipMalloc(C.byref(d_cnt), B * 4) == 0
    a = S.BatchedUKF(B, L).readParams(); a.init(0.0, 0.0, 0.0); a.set_sqrt_mode("cholesky")
    b = S.BatchedUKF(B, L).readParams(); b.init(0.0, 0.0, 0.0); b.set_sqrt_mode("cholesky")
    for t in range(T):
        k = int(g["meas_count"][t])
        cmd = S.Command(g["cmds"][t, 0], g["cmds"][t, 1])
        a.update(cmd, g["meas"][t, :k].ravel())
        b.predictionStage(cmd)
        meas = np.zeros((B, 8, 3), dtype=np.float32); meas[:, :k] = g["meas"][t, :k]
        cnt = np.full(B, k, dtype=np.int32)
        assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0
        assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0
        b.updateStage(d_meas.value, d_cnt.value, 8)
    for i in range(B):
        _eq(a.get_state(i), b.get_state(i))
    assert a.sqrt_stats().tolist() == b.sqrt_stats().tolist() and int(a.sqrt_stats()[0]) > 0
    assert np.array_equal(a.sigma_points(1), b.sigma_points(1))
    a.close(); b.close(); hip.hipFree(d_meas); hip.hipFree(d_cnt)

    from live_ekf_slam_amd.scenario import make_scenario
    B, T = 1024, 40
    lm, cmds = make_scenario(1234, L, T)
    monkeypatch.setenv("SLAM_UKF_SPLIT_MIN", "1024")
    KS = 24
    outs = []
    for entry in ("run_sim", "update_sim", "update"):
        f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(5); f.init(0, 0, 0); f.set_sqrt_mode("cholesky")
        if entry == "run_sim":            # the batch split over streams
            f.run_sim(cmds[:T // 2]); f.run_sim(cmds[T // 2:])
        elif entry == "update_sim":       # one step per call, the generated messages recorded
            f.last_meas(KS)
            msgs = []
            for t in range(T):
                f.update_sim(cmds[t])
                msgs.append(f.last_meas(KS))
        else:                             # the same messages as host measurements: UKF::update
            for t in range(T):
                meas, cnt = msgs[t]
                f.update(cmds[t], meas[:, :max(1, int(cnt.max()))], cnt)
        outs.append((f.landmark_counts(), f.status(), f.sqrt_stats(), [f.get_state(i) for i in (0, 511, 512, 1023)],
                     f.poses() if entry != "update" else None, f.error_stats() if entry != "update" else None))
        f.close()
    ra = outs[0]
    for rb in outs[1:]:
        for i in range(3):
            assert np.array_equal(ra[i], rb[i]), i
        for sa, sb in zip(ra[3], rb[3]):
            _eq(sa, sb)
    assert np.array_equal(ra[4], outs[1][4]) and np.array_equal(ra[5], outs[1][5])   # the simulator's own state (sim entry points)
    assert int(ra[2].sum()) == B * T and int(ra[2][0]) > 0


def test_setter_refuses_what_it_does_not_cover(S):
    """(f) EKF handles and unknown modes: SLAM_ERR_ARG; the HBM-streamed class (L_max > 50): SLAM_ERR_UNSUPPORTED."""
    lib = S._lib.lib()
    e = S.BatchedEKF(2, 5).readParams()
    assert lib.slam_ukf_set_sqrt_mode(e.h, 1) == SLAM_ERR_ARG
    assert lib.slam_ukf_set_sqrt_mode(e.h, 0) == SLAM_ERR_ARG
    big = S.BatchedUKF(2, 60).readParams()
    assert lib.slam_ukf_set_sqrt_mode(big.h, 1) == SLAM_ERR_UNSUPPORTED
    assert lib.slam_ukf_set_sqrt_mode(big.h, 0) == 0              # eigen stays available there
    u = S.BatchedUKF(2, 50).readParams()
    assert lib.slam_ukf_set_sqrt_mode(u.h, 2) == SLAM_ERR_ARG and lib.slam_ukf_set_sqrt_mode(u.h, -1) == SLAM_ERR_ARG
    assert lib.slam_ukf_set_sqrt_mode(u.h, 1) == 0
    with pytest.raises(ValueError):
        u.set_sqrt_mode("qr")
    with pytest.raises(S.SlamError):
        big.set_sqrt_mode("cholesky")
    loc = S.BatchedUKFLoc(2).readParams()
    loc.set_sqrt_mode("cholesky")                                  # n = 4: the small class
    assert lib.slam_ukf_sqrt_stats(e.h, (C.c_uint64 * 2)(), 0) == SLAM_ERR_ARG
    for f in (e, big, u, loc):
        f.close()


# (g) Cholesky vs eigen mode on the bench scenario.  Both filters see the same measurements (the generator does not depend on the
# filter), so the per-instance errors differ only through the square root.  The reference's signed process noise leaves P
# indefinite on most steps of this scenario (measured over the 400 steps of this test from init: 1 136 316 of 1 638 400 instance-steps
# fall back, 69 %; tools/gpu_ukf_sqrt_modes.py counts only its timed steps 21-140 at L = 20: 87 %), and on the others the Cholesky sigma
# points steer the quirk-laden filter elsewhere: the batch mean error measured 1.096 m against 0.912 m (+20 %).  Stated tolerance
# on the batch mean: 30 %.
STAT_MEAN_ERR_RTOL = 0.30


def test_cholesky_mode_statistics_at_bench_scale(S):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = 20, 4096, 400
    lm, cmds = make_scenario(1234, L, T)
    res = {}
    for mode in ("eigen", "cholesky"):
        f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode(mode)
        f.set_vision(1e9, -4.0, 4.0); f.update_sim(cmds[0]); f.set_vision(3.0, -1.57, 1.57)
        f.run_sim(cmds[1:])
        res[mode] = (f.error_stats().copy(), f.status().copy(), f.sqrt_stats().copy())
        f.close()
    (ee, fe, _), (ec, fc, sc) = res["eigen"], res["cholesky"]
    assert not fe.any() and not fc.any()
    assert int(sc.sum()) == B * T and int(sc[0]) > 0
    assert np.all(np.isfinite(ec))
    assert abs(ec.mean() - ee.mean()) <= STAT_MEAN_ERR_RTOL * ee.mean(), (ec.mean(), ee.mean(), sc.tolist())


def _hip_buffers(nbytes_meas, nbytes_cnt):
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), nbytes_meas) == 0 and hip.hipMalloc(C.byref(d_cnt), nbytes_cnt) == 0

    def put(meas, cnt):
        assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0   # hipMemcpyHostToDevice
        assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0

    def free():
        hip.hipFree(d_meas); hip.hipFree(d_cnt)
    return d_meas, d_cnt, put, free


def _close_to(sg, ref):
    assert sg["M"] == ref.M and list(sg["ids"]) == ref.ids
    return max(np.abs(sg["x"] - ref.x).max(), np.abs(sg["P"] - ref.P).max())


@pytest.mark.parametrize("entry", ["host", "stages"])
def test_cholesky_mode_over_long_messages(S, entry):
    """Cholesky mode on the long-message path of an LDS class: a message longer than the class holds (20 detections at L_max = 20)
    sends its instance to the HBM-streamed step kernel (ukf_big_kernel.hip), which must take the sigma-point offsets from the ROWS of
    sqtP like the LDS step kernel - the Cholesky kernel stores L^T.  Instances 0 and 1 get over-long messages of known ids every other
    step, 2 and 3 ordinary ones; each instance within 1e-8 of its own numpy Cholesky UKF, with the same factorisation / fallback counts,
    and Cholesky factors actually used on over-long steps."""
    L, cap, B, T = 20, 20, 4, 10
    KS = cap + 32
    f = S.BatchedUKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode("cholesky")
    refs = [NumpyUKF("cholesky") for _ in range(B)]
    for r in refs:
        r.init(0, 0, 0)
    if entry == "stages":
        d_meas, d_cnt, put, free = _hip_buffers(B * KS * 3 * 4, B * 4)
    rng = np.random.default_rng(5)
    long_factored = 0
    for t in range(T):
        cmd = np.array([rng.uniform(0.02, 0.1), rng.uniform(0.0, 0.04)], dtype=np.float32)   # heading stays in (0, pi/2): Q >= 0
        ks = rng.integers(0, 3, B)
        if t >= 4 and t % 2 == 0:
            ks[:2] = cap + rng.integers(3, 30, 2)
        meas = np.zeros((B, KS, 3), dtype=np.float32)
        for b in range(B):
            k = int(ks[b])
            known = refs[b].ids
            meas[b, :k, 0] = rng.choice(known, k) if (t >= 4 and known) else rng.integers(0, 6, k)
            meas[b, :k, 1] = rng.uniform(0.5, 6.0, k)
            meas[b, :k, 2] = rng.uniform(-1.0, 1.0, k)
        if entry == "stages":
            put(meas, ks.astype(np.int32))
            f.predictionStage(S.Command(cmd[0], cmd[1])); f.updateStage(d_meas.value, d_cnt.value, KS)
        else:
            f.update(cmd, meas[:, :max(1, int(ks.max()))], ks.astype(np.int32))
        for b in range(B):
            f0 = refs[b].factorisations
            refs[b].update(cmd[0], cmd[1], [tuple(r) for r in meas[b, :ks[b]]])
            long_factored += int(ks[b] > cap and refs[b].factorisations > f0)
    assert long_factored > 0
    assert not f.status().any(), f.status()
    worst = max(_close_to(f.get_state(b), refs[b]) for b in range(B))
    assert worst < 1e-8, worst
    assert f.sqrt_stats().tolist() == [sum(r.factorisations for r in refs), sum(r.fallbacks for r in refs)]
    f.close()
    if entry == "stages":
        free()


def test_cholesky_mode_in_sim_mode_on_a_map_larger_than_the_class(S):
    """SIM mode with a map of more landmarks than a message of the class holds (25 > 20): the streamed step kernel takes the whole launch
    after ukf_chol_kernel.  The generated messages (the measurement dump) fed to one numpy Cholesky UKF per instance: within 1e-8, the
    same factorisation / fallback counts, Cholesky factors used."""
    from live_ekf_slam_amd.scenario import make_scenario
    L_max, L, B, T, KS = 20, 25, 2, 30, 32
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedUKF(B, L_max).readParams(); f.set_map(lm); f.set_seed(7); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode("cholesky")
    f.last_meas(KS)   # measurement dump on
    refs = [NumpyUKF("cholesky") for _ in range(B)]
    for r in refs:
        r.init(0, 0, 0)
    longest = 0
    for t in range(T):
        f.update_sim(cmds[t])
        meas, cnt = f.last_meas(KS)
        longest = max(longest, int(cnt.max()))
        for b in range(B):
            refs[b].update(cmds[t][0], cmds[t][1], [tuple(r) for r in meas[b, :cnt[b]]])
    assert not f.status().any(), f.status()
    assert max(r.M for r in refs) <= L_max and longest >= 1
    assert sum(r.factorisations for r in refs) > 0
    worst = max(_close_to(f.get_state(b), refs[b]) for b in range(B))
    assert worst < 1e-8, worst
    assert f.sqrt_stats().tolist() == [sum(r.factorisations for r in refs), sum(r.fallbacks for r in refs)]
    f.close()
