"""Per-instance noise parameters on the GPU (include/slam_batch.h, slam_set_noise_each): one row of filter and simulator noise per
instance, in every step kernel and from every entry point.

Rows that all equal slam_noise_from_config give the bits of a handle without rows; an instance with its own row equals the oracle run
with that row's values (coupled: simulator = filter values, through oracle.run_*_batch; decoupled: OracleSim feeding OracleEKF /
OracleUKF, each with its own config) and, in the classes the oracle does not reach in seconds, a one-instance handle created from that
row's config at the same global instance index.  Every comparison is bit for bit."""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import load_golden
from live_ekf_slam_amd.config import default_config, noise_rows
from live_ekf_slam_amd.scenario import make_scenario
from test_each_instance_gpu import SIM_CASES, _Dev, _assert_same, _assert_state, _snapshot

pytestmark = pytest.mark.gpu
SEED = 31

# four settings of (v_d, v_th, w_r, w_b, V_00, V_11, W_00, W_11), all values distinct within a row so that a swapped field shows;
# instance b takes setting b % 4.  SIM_HALF: the simulator's half-widths of the decoupled test (filter != simulator).
SETTINGS = [(0.0005, -0.001, 0.0015, -0.0005, 0.01, 0.001, 0.011, 0.009),
            (0.004, -0.0015, -0.003, 0.002, 0.02, 0.002, 0.015, 0.025),
            (-0.002, 0.001, 0.005, -0.004, 0.004, 0.0005, 0.03, 0.005),
            (0.001, 0.0025, 0.002, 0.003, 0.05, 0.004, 0.006, 0.012)]
SIM_HALF = [(0.012, 0.0015, 0.008, 0.011), (0.006, 0.003, 0.02, 0.004), (0.02, 0.0008, 0.005, 0.016), (0.009, 0.0022, 0.013, 0.007)]
FIELDS = ("v_d", "v_th", "w_r", "w_b", "V_00", "V_11", "W_00", "W_11")


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


def _base_cfg(quirk=1):
    c = default_config()
    c.replicate_vw_quirk = quirk
    return c


def _cfg_of(setting, quirk=1):
    """The slam_config whose shared behaviour is the row of `setting` with the simulator coupled to the filter's keys."""
    c = _base_cfg(quirk)
    for name, v in zip(FIELDS, setting):
        setattr(c, name, v)
    return c


def _mixed_rows(cfg, B, first=0, decoupled=False):
    """Rows of instances first .. first + B - 1: setting (first + b) % 4; coupled (sim_* = the row's V_* / W_*) or with SIM_HALF."""
    cols = {name: [SETTINGS[(first + b) % 4][i] for b in range(B)] for i, name in enumerate(FIELDS)}
    for i, name in enumerate(("sim_V_00", "sim_V_11", "sim_W_00", "sim_W_11")):
        cols[name] = [SIM_HALF[(first + b) % 4][i] if decoupled else SETTINGS[(first + b) % 4][4 + i] for b in range(B)]
    return noise_rows(cfg, B, **cols)


def _make(S, kind, B, L_max, dtype=0, chol=False, cfg=None, offset=0):
    if kind == "ekf":
        f = S.BatchedEKF(B, L_max, dtype=dtype)
    elif kind == "ukf":
        f = S.BatchedUKF(B, L_max)
    else:
        f = S.BatchedUKFLoc(B)
    f.readParams(cfg)
    if chol:
        f.set_sqrt_mode("cholesky")
    f.set_seed(SEED)
    if offset:
        f.set_instance_offset(offset)
    return f


def _assert_instance(mixed_snap, b, one_snap, what=""):
    """instance b of a batch snapshot == instance 0 of a one-instance handle's snapshot"""
    assert mixed_snap["status"][b] == one_snap["status"][0] and mixed_snap["M"][b] == one_snap["M"][0], (what, b)
    assert np.array_equal(mixed_snap["truth"][b], one_snap["truth"][0]) and mixed_snap["err"][b] == one_snap["err"][0], (what, b)
    sa, sb = mixed_snap["states"][b], one_snap["states"][0]
    assert sa["M"] == sb["M"] and sa["timestep"] == sb["timestep"] and np.array_equal(sa["ids"], sb["ids"]), (what, b)
    assert np.array_equal(sa["x"], sb["x"]) and np.array_equal(sa["P"], sb["P"]), (what, b)


def _differs(a, b):
    return any(not np.array_equal(sa["x"], sb["x"]) for sa, sb in zip(a["states"], b["states"]))


# ---- 1. broadcast identity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L_max,dtype,chol", SIM_CASES + [("loc", 1, 0, False)])
def test_broadcast_identity_sim(S, monkeypatch, kind, L_max, dtype, chol):
    """Rows all equal to slam_noise_from_config(cfg) == a twin handle without rows: every size class, run chunks 0, 1 and 7, the UKF's
    run split over streams."""
    monkeypatch.setenv("SLAM_UKF_SPLIT_MIN", "4")
    B = 6
    L = 20 if kind == "loc" else min(L_max, 60)
    T = 16 if L_max >= 200 else 24
    lm, cmds = make_scenario(400 + L_max, L, T)
    for chunk in ((0, 1, 7) if kind == "ekf" else (0,)):
        a = _make(S, kind, B, L_max, dtype, chol); b = _make(S, kind, B, L_max, dtype, chol)
        b.set_noise(noise_rows(b.cfg, B))
        for f in (a, b):
            f.set_run_chunk(chunk); f.set_map(lm); f.init(0.0, 0.0, 0.0)
            f.run_sim(cmds[:T // 2]); f.update_sim(cmds[T // 2]); f.run_sim(cmds[T // 2 + 1:])
        _assert_same(_snapshot(a), _snapshot(b))
        assert np.all(a.status() == 0)
        a.close(); b.close()


@pytest.mark.parametrize("kind,L_max,dtype,chol", SIM_CASES + [("loc", 1, 0, False)])
def test_broadcast_identity_ext(S, hip, kind, L_max, dtype, chol):
    """The same on the reference simulator's measurement stream through slam_step, slam_step_each_dev and slam_predict + slam_update_dev,
    over every case of the SIM test: fp32 storage and the HBM-streamed EKF class (L_max = 1000) included."""
    g = load_golden("sim_seed2_L50_T1000.npz")
    B, T, ks = 5, 40, 6
    a = _make(S, kind, B, L_max, dtype, chol); b = _make(S, kind, B, L_max, dtype, chol)
    b.set_noise(noise_rows(b.cfg, B))
    dev = _Dev(hip)
    try:
        for f in (a, b):
            if kind == "loc":
                f.set_map(g["map"])
            f.init(0.0, 0.0, 0.0)
        for t in range(T):
            k = min(int(g["meas_count"][t]), ks)
            meas = np.zeros((B, ks, 3), np.float32); meas[:, :k] = g["meas"][t, :k]
            cnt = np.full(B, k, np.int32)
            cmd = g["cmds"][t].astype(np.float32)
            per = np.ascontiguousarray(np.broadcast_to(cmd, (B, 2)))
            dm, dc, dcm = dev.put("meas", meas), dev.put("cnt", cnt), dev.put("cmds", per)
            for f in (a, b):
                if t % 3 == 0:
                    f.update(S.Command(cmd[0], cmd[1]), meas, cnt)
                elif t % 3 == 1 or kind == "ekf":
                    f.update_dev_each(dcm, dm, dc, ks)
                else:
                    f.predictionStage(S.Command(cmd[0], cmd[1])); f.updateStage(dm, dc, ks)
                f.sync()
        _assert_same(_snapshot(a), _snapshot(b))
    finally:
        a.close(); b.close(); dev.close()


# ---- 2. mixed rows against the oracle, simulator coupled to the filter's keys ------------------------------------------------------
@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("kind,L_max", [("ekf", 20), ("ekf", 50), ("ukf", 20), ("loc", 1)])
def test_mixed_rows_match_oracle_coupled(S, oracle, kind, L_max, quirk):
    """B = 8, four distinct rows used twice each; instance b == the oracle's batch runner for one instance at inst0 = b with cfg_b."""
    B, T = 8, 24
    L = 20 if kind == "loc" else L_max
    lm, cmds = make_scenario(500 + L_max, L, T)
    f = _make(S, kind, B, L_max, cfg=_base_cfg(quirk))
    f.set_noise(_mixed_rows(f.cfg, B))
    f.set_map(lm); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds[:10]); f.update_sim(cmds[10]); f.run_sim(cmds[11:])
    M, truth, err, status = f.landmark_counts(), f.truth(), f.error_stats(), f.status()
    base = 3 if kind == "ekf" else 4
    for b in range(B):
        cfg_b = _cfg_of(SETTINGS[b % 4], quirk)
        if kind == "ekf":
            r = oracle.run_ekf_batch(lm, cmds, 1, L_max, seed=SEED, inst0=b, cfg=cfg_b)
        else:
            r = oracle.run_ukf_batch(lm, cmds, 1, L_max, seed=SEED, inst0=b, cfg=cfg_b, loc=(kind == "loc"))
        assert M[b] == r["M"][0] and status[b] == r["flags"][0], (b, M[b], r["M"][0], status[b], r["flags"][0])
        assert np.array_equal(truth[b], r["truth"][0]) and err[b] == r["avg_err"][0], b
        st = f.get_state(b); n = base + 2 * r["M"][0]
        assert np.array_equal(st["ids"], r["ids"][0, :r["M"][0]]), b
        assert np.array_equal(st["x"], r["x"][0, :n]), (b, np.abs(st["x"] - r["x"][0, :n]).max())
        assert np.array_equal(st["P"].ravel(), r["P"][0, :n * n]), (b, np.abs(st["P"].ravel() - r["P"][0, :n * n]).max())
    f.close()


# ---- 3. mixed rows against the oracle, filter != simulator ---------------------------------------------------------------------------
@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("kind", ["ekf", "ukf"])
def test_mixed_rows_match_oracle_decoupled(S, oracle, kind, quirk):
    """Instance b == OracleSim(map, cfg_sim_b).step_philox feeding OracleEKF / OracleUKF(cfg_filter_b): pins which field goes to the
    generator and which to the filter."""
    B, T, L_max = 8, 24, 20
    lm, cmds = make_scenario(520, L_max, T)
    f = _make(S, kind, B, L_max, cfg=_base_cfg(quirk))
    f.set_noise(_mixed_rows(f.cfg, B, decoupled=True))
    f.set_map(lm); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds[:9]); f.update_sim(cmds[9]); f.run_sim(cmds[10:])
    truth = f.truth()
    for b in range(B):
        cfg_sim = _base_cfg(quirk)
        cfg_sim.V_00, cfg_sim.V_11, cfg_sim.W_00, cfg_sim.W_11 = SIM_HALF[b % 4]
        sim = oracle.OracleSim(lm, cfg_sim)
        cfg_f = _cfg_of(SETTINGS[b % 4], quirk)
        filt = oracle.OracleEKF(cfg_f, L_max=L_max) if kind == "ekf" else oracle.OracleUKF(cfg_f, L_max=L_max)
        filt.init(0.0, 0.0, 0.0)
        tr = None
        for t in range(T):
            tr, meas = sim.step_philox(cmds[t, 0], cmds[t, 1], SEED, b, t)
            filt.update(cmds[t, 0], cmds[t, 1], meas)
        assert np.array_equal(truth[b], tr), b
        _assert_state(f.get_state(b), filt.state())
    assert np.all(f.status() == 0)
    f.close()


# ---- 4. partition invariance on the device ----------------------------------------------------------------------------------------------
def _drive_sim(f, cmds):
    T = len(cmds)
    f.run_sim(cmds[:T // 2]); f.update_sim(cmds[T // 2]); f.run_sim(cmds[T // 2 + 1:])


PARTITION_CASES = [("ekf", 20, 1, False), ("ekf", 50, 1, False), ("ekf", 200, 0, False), ("ekf", 1000, 0, False),
                   ("ukf", 50, 0, False), ("ukf", 200, 0, False), ("ukf", 20, 0, True)]


@pytest.mark.parametrize("kind,L_max,dtype,chol", PARTITION_CASES)
def test_partition_invariance_sim(S, monkeypatch, kind, L_max, dtype, chol):
    """Instance b of the mixed handle (coupled rows) == a one-instance handle created from cfg_b with set_instance_offset(b)."""
    monkeypatch.setenv("SLAM_UKF_SPLIT_MIN", "4")
    B = 6
    L = min(L_max, 60)
    T = 16 if L_max >= 200 else 24
    lm, cmds = make_scenario(540 + L_max, L, T)
    f = _make(S, kind, B, L_max, dtype, chol)
    f.set_noise(_mixed_rows(f.cfg, B))
    f.set_map(lm); f.init(0.0, 0.0, 0.0)
    _drive_sim(f, cmds)
    snap = _snapshot(f)
    f.close()
    ones = []
    for b in range(B):
        o = _make(S, kind, 1, L_max, dtype, chol, cfg=_cfg_of(SETTINGS[b % 4]), offset=b)
        o.set_map(lm); o.init(0.0, 0.0, 0.0)
        _drive_sim(o, cmds)
        ones.append(_snapshot(o))
        _assert_instance(snap, b, ones[-1], (kind, L_max))
        o.close()
    assert _differs(ones[0], ones[1])   # (the rows do change the result: the comparison above is not between equal runs)


@pytest.mark.parametrize("kind", ["ekf", "loc"])
def test_partition_invariance_long_messages_sim(S, kind):
    """SIM mode on a 30-landmark map wholly in view: every message exceeds the 20 detections of the size class, so the HBM-streamed
    kernels take the launches (EKF L_max = 20, UKF_LOC)."""
    B, T = 6, 12
    lm, cmds = make_scenario(571, 30, T)

    def run(f):
        f.set_vision(1e9, -4.0, 4.0); f.set_map(lm); f.init(0.0, 0.0, 0.0)
        _drive_sim(f, cmds)
        return _snapshot(f)

    f = _make(S, kind, B, 20)
    f.set_noise(_mixed_rows(f.cfg, B))
    snap = run(f)
    f.close()
    for b in range(B):
        o = _make(S, kind, 1, 20, cfg=_cfg_of(SETTINGS[b % 4]), offset=b)
        _assert_instance(snap, b, run(o), kind)
        o.close()


@pytest.mark.parametrize("kind,dtype", [("ekf", 0), ("ekf", 1), ("ukf", 0)])
def test_partition_invariance_long_messages_ext(S, kind, dtype):
    """EXT mode, messages of 25 detections for the even instances and 3 for the odd ones in an L_max = 20 handle: both launches of the
    pair run (the LDS kernel for the short messages, the streamed kernel for the long ones)."""
    B, T, ks = 6, 8, 25
    rng = np.random.default_rng(77)
    lm = np.stack([1.5 + rng.uniform(0.0, 1.0, ks), rng.uniform(-1.0, 1.0, ks)], axis=1)
    cmd = np.array([0.02, 0.004], np.float32)
    msgs = []
    for t in range(T):
        meas = np.zeros((B, ks, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b in range(B):
            k = ks if b % 2 == 0 else 3
            pick = np.arange(k) if k == ks else (np.arange(3) + t + b) % ks
            d = lm[pick] - np.array([0.02 * t, 0.0])
            meas[b, :k, 0] = pick
            meas[b, :k, 1] = np.hypot(d[:, 0], d[:, 1]) + rng.uniform(-0.01, 0.01, k)
            meas[b, :k, 2] = np.arctan2(d[:, 1], d[:, 0]) + rng.uniform(-0.01, 0.01, k)
            cnt[b] = k
        msgs.append((meas, cnt))

    def run(f, sl):
        f.init(0.0, 0.0, 0.0)
        for meas, cnt in msgs:
            f.update(S.Command(cmd[0], cmd[1]), meas[sl], cnt[sl])
        out = dict(status=f.status(), M=f.landmark_counts(), states=[f.get_state(i) for i in range(f.batch)])
        return out

    f = _make(S, kind, B, 20, dtype)
    f.set_noise(_mixed_rows(f.cfg, B))
    got = run(f, slice(0, B))
    f.close()
    xs = []
    for b in range(B):
        o = _make(S, kind, 1, 20, dtype, cfg=_cfg_of(SETTINGS[b % 4]), offset=b)
        one = run(o, slice(b, b + 1))
        o.close()
        assert got["status"][b] == one["status"][0] and got["M"][b] == one["M"][0], b
        _assert_state(got["states"][b], one["states"][0])
        assert got["states"][b]["timestep"] == T
        xs.append(one["states"][0]["x"])
    assert not np.array_equal(xs[0][:3], xs[2][:3])   # the long-message instances 0 and 2 have different rows, and it shows


# ---- 5. order and lifetime -------------------------------------------------------------------------------------------------------------
def test_set_noise_keeps_call_order_with_the_step_queue(S):
    """set_noise between queued update_sim calls: the steps before it use the old rows, the steps after it the new ones == a twin without
    a queue that synchronises around the call.  set_noise(None) returns to the shared bits."""
    B, L_max, T = 8, 20, 22
    lm, cmds = make_scenario(600, L_max, T)
    a = _make(S, "ekf", B, L_max); b = _make(S, "ekf", B, L_max); c = _make(S, "ekf", B, L_max)
    a.set_lazy_steps(8); b.set_lazy_steps(0); c.set_lazy_steps(8)
    rows1 = _mixed_rows(a.cfg, B); rows2 = _mixed_rows(a.cfg, B, first=1, decoupled=True)
    for f in (a, b, c):
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
    a.set_noise(rows1); b.set_noise(rows1)
    for t in range(5):
        a.update_sim(cmds[t]); b.update_sim(cmds[t]); c.update_sim(cmds[t])
    b.sync(); b.set_noise(rows2); b.sync()
    a.set_noise(rows2)
    for t in range(5, 16):
        a.update_sim(cmds[t]); b.update_sim(cmds[t]); c.update_sim(cmds[t])
    sa, sb, sc = _snapshot(a), _snapshot(b), _snapshot(c)
    _assert_same(sa, sb)
    assert _differs(sa, sc)
    # back to the config: from here on a steps like a handle that has the same state and no rows
    d = _make(S, "ekf", B, L_max); d.set_map(lm); d.init(0.0, 0.0, 0.0)
    d.set_noise(rows1); d.set_noise(None)
    for t in range(16):
        d.update_sim(cmds[t])
    _assert_same(_snapshot(d), sc)
    for f in (a, b, c, d):
        f.close()


def test_rows_are_inputs_not_state(S, tmp_path):
    """slam_save_state / slam_load_state keep their format; after a load the rows are set again."""
    B, L_max, T = 6, 20, 20
    lm, cmds = make_scenario(610, L_max, T)
    a = _make(S, "ekf", B, L_max); plain = _make(S, "ekf", B, L_max)
    rows = _mixed_rows(a.cfg, B)
    for f in (a, plain):
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
    a.set_noise(rows)
    a.run_sim(cmds[:10]); plain.run_sim(cmds[:10])
    pa, pp = str(tmp_path / "mixed.ckpt"), str(tmp_path / "plain.ckpt")
    a.save_state(pa); plain.save_state(pp)
    assert os.path.getsize(pa) == os.path.getsize(pp)
    a.run_sim(cmds[10:])
    c = _make(S, "ekf", B, L_max); c.set_map(lm); c.load_state(pa); c.set_noise(rows); c.run_sim(cmds[10:])
    _assert_same(_snapshot(a), _snapshot(c))
    d = _make(S, "ekf", B, L_max); d.set_map(lm); d.load_state(pa); d.run_sim(cmds[10:])   # without the rows: the config's values
    assert _differs(_snapshot(a), _snapshot(d))
    # slam_init does not clear the rows
    a.init(0.0, 0.0, 0.0); a.run_sim(cmds)
    e = _make(S, "ekf", B, L_max); e.set_map(lm); e.set_noise(rows); e.init(0.0, 0.0, 0.0); e.run_sim(cmds)
    _assert_same(_snapshot(a), _snapshot(e))
    for f in (a, plain, c, d, e):
        f.close()


def test_tracked_instance_gets_its_row(S):
    """slam_track_instance before and after set_noise: the shadow's answer == the batch's instance."""
    B, L_max, T, tr = 8, 20, 24, 5
    lm, cmds = make_scenario(620, L_max, T)
    a = _make(S, "ekf", B, L_max); b = _make(S, "ekf", B, L_max); c = _make(S, "ekf", B, L_max)
    rows1 = _mixed_rows(a.cfg, B); rows2 = _mixed_rows(a.cfg, B, first=2, decoupled=True)
    for f in (a, b, c):
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
    a.track_instance(tr); a.set_noise(rows1)      # tracked first, rows afterwards
    c.set_noise(rows1); c.track_instance(tr)      # rows first
    b.set_noise(rows1)
    for f in (a, b, c):
        f.run_sim(cmds[:8])
        for t in range(8, 12):
            f.update_sim(cmds[t])
    assert a.get_state(tr)["timestep"] == 12
    _assert_state(a.get_state(tr), b.get_state(tr)); _assert_state(c.get_state(tr), b.get_state(tr))
    for f in (a, b, c):
        f.set_noise(rows2); f.run_sim(cmds[12:])   # the rows change: the shadow gets its row again
    _assert_state(a.get_state(tr), b.get_state(tr)); _assert_state(c.get_state(tr), b.get_state(tr))
    a.track_instance(-1); c.track_instance(-1)
    _assert_same(_snapshot(a), _snapshot(b)); _assert_same(_snapshot(c), _snapshot(b))
    for f in (a, b, c):
        f.close()


def test_errors(S):
    from live_ekf_slam_amd import _lib
    L = _lib.lib()
    f = _make(S, "ukf", 4, 20); f.init(0.0, 0.0, 0.0)
    rows = _mixed_rows(f.cfg, 4)
    f.predictionStage(S.Command(0.05, 0.01))
    assert L.slam_set_noise_each(f.h, rows) == -4 and "prediction stage" in L.slam_last_error().decode()   # SLAM_ERR_STATE
    assert L.slam_set_noise_each(f.h, None) == -4
    f.updateStage()
    assert L.slam_set_noise_each(f.h, rows) == 0
    for field, bad in (("v_th", float("nan")), ("W_11", float("inf")), ("sim_V_00", -float("inf"))):
        r = _mixed_rows(f.cfg, 4)
        setattr(r[2], field, bad)
        assert L.slam_set_noise_each(f.h, r) == -1                                                          # SLAM_ERR_ARG
        text = L.slam_last_error().decode()
        assert "instance 2" in text and field in text, text
    neg = noise_rows(f.cfg, 4, V_00=-1.0, sim_W_11=0.0)     # no other value check: the reference has none
    assert L.slam_set_noise_each(f.h, neg) == 0
    assert L.slam_set_noise_each(None, rows) == -1 and "NULL handle" in L.slam_last_error().decode()
    with pytest.raises(ValueError):
        f.set_noise(_mixed_rows(f.cfg, 3))
    f.close()


# ---- 6. closed loop and monitor ------------------------------------------------------------------------------------------------------------
def test_closed_loop_and_monitor_per_instance(S):
    """run_nav(12) and monitor_run(T = 12, series = True) on a mixed EKF L = 20 handle: states, issued commands and the per-instance
    series of instance b == those of the one-instance handle of cfg_b at offset b.  (The batch records depend on who shares the batch.)"""
    B, L_max, T = 6, 20, 12
    lm = make_scenario(630, L_max, 2)[0]
    path = lm[:3].copy()

    def start(f):
        f.set_map(lm); f.init(0.0, 0.0, 0.0); f.set_path(path)

    f = _make(S, "ekf", B, L_max); f.set_noise(_mixed_rows(f.cfg, B)); start(f)
    cmds = f.run_nav(T, return_cmds=True)
    nav_snap = _snapshot(f)
    m = _make(S, "ekf", B, L_max); m.set_noise(_mixed_rows(m.cfg, B)); start(m)
    res = m.monitor_run(T=T, series=True)
    mon_snap = _snapshot(m)
    _assert_same(nav_snap, mon_snap)          # the monitored run gives the bits of the unmonitored one
    f.close(); m.close()
    for b in range(B):
        cfg_b = _cfg_of(SETTINGS[b % 4])
        o = _make(S, "ekf", 1, L_max, cfg=cfg_b, offset=b); start(o)
        c1 = o.run_nav(T, return_cmds=True)
        assert np.array_equal(c1[:, 0], cmds[:, b]), b
        _assert_instance(nav_snap, b, _snapshot(o), "nav")
        o.close()
        o = _make(S, "ekf", 1, L_max, cfg=cfg_b, offset=b); start(o)
        r1 = o.monitor_run(T=T, series=True)
        for name in ("err_pos", "err_yaw", "nees_pose"):
            assert np.array_equal(getattr(r1, name)[:, 0], getattr(res, name)[:, b], equal_nan=True), (name, b)
        _assert_instance(mon_snap, b, _snapshot(o), "monitor")
        o.close()
    assert not np.array_equal(cmds[:, 0], cmds[:, 1])


# ---- 7. nothing else moves ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L_max", [("ekf", 50), ("ukf", 20)])
def test_handles_without_rows_still_match_the_oracle(S, oracle, kind, L_max):
    """A handle that never calls slam_set_noise_each runs the same launches with noise_each == NULL."""
    B, T = 6, 24
    lm, cmds = make_scenario(640 + L_max, L_max, T)
    f = _make(S, kind, B, L_max)
    f.set_map(lm); f.init(0.0, 0.0, 0.0)
    _drive_sim(f, cmds)
    run = oracle.run_ekf_batch if kind == "ekf" else oracle.run_ukf_batch
    r = run(lm, cmds, B, L_max, seed=SEED, nthreads=2)
    base = 3 if kind == "ekf" else 4
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.truth(), r["truth"]) and np.array_equal(f.error_stats(), r["avg_err"])
    for b in range(B):
        st = f.get_state(b); n = base + 2 * r["M"][b]
        assert np.array_equal(st["x"], r["x"][b, :n]) and np.array_equal(st["P"].ravel(), r["P"][b, :n * n]), b
    f.close()
