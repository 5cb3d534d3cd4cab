"""The simulator source with a sensor fault model on the MI355X (slam_sense*, slam_sense_commit, the five *_run_sim calls).

Batch 257: one instance past a 256-instance reduction workgroup, and a four-instance workgroup partly filled.  A 12-landmark map,
k_stride = 16, T = 24; fp64 at L_max 20 and fp32 storage at L_max 50; per-instance noise rows, maps (3 to 12 landmarks) and commands, so
every instance differs; a few instances frozen beforehand by a message that repeats an id it inserts.

The default row is compared with slam_run_sim_each (checkpoint bytes, truth, error statistics, every tick's message); the faults with the
host hook - the kernel's own per-instance function compiled for the host - evaluated at the device's own truth, in bits; every *_run_sim
call with its LOG sibling fed the run's own log.  A host-fed handle's truth and error sum do not move, so there the checkpoint is compared
up to those two items (the last 32 bytes per instance), and the simulator handle's truth and error sum are compared with the log itself."""
import ctypes as C

import numpy as np
import pytest

from record_tree import ALL_SUMS, fixed_order_record
from test_gate_gpu import _Dev, _same_bits

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4
B, KS, T, L = 257, 16, 24, 12
PRE_FROZEN = list(range(5, B, 60))
CLASSES = [(20, False), (50, True)]
CLASS_IDS = ["L20_f64", "L50_f32"]
PATH = np.array([[0.6, 0.1], [1.4, 0.6], [2.2, 0.2], [3.0, 0.9], [3.8, 0.3]])


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


@pytest.fixture(scope="module")
def W(S):
    """The world every test shares: config, per-instance maps, noise rows and commands."""
    from live_ekf_slam_amd.config import noise_rows
    from live_ekf_slam_amd.scenario import make_scenario
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.W_00 = cfg.W_11 = 2.5e-3
    cfg.V_00 = cfg.V_11 = 1e-4
    lm, cmds = make_scenario(321 + L, L, T)
    rng = np.random.default_rng(2026)
    maps = lm[None] + rng.normal(0.0, 0.05, (B, L, 2))
    counts = (3 + np.arange(B) % 10).astype(np.int32)
    rows = noise_rows(cfg, B, sim_W_00=rng.uniform(0.005, 0.03, B), sim_W_11=rng.uniform(0.005, 0.03, B), sim_V_00=rng.uniform(0.002, 0.02, B),
                      W_00=rng.uniform(2e-3, 4e-3, B))
    each = (cmds[:, None, :] * rng.uniform(0.6, 1.0, (1, B, 1))).astype(np.float32)
    return dict(cfg=cfg, maps=maps, counts=counts, rows=rows, cmds=np.ascontiguousarray(cmds), each=np.ascontiguousarray(each))


def _handle(S, W, L_max, f32, freeze=True, warm=0):
    f = S.BatchedEKF(B, L_max, dtype=S.F32 if f32 else S.F64).readParams(W["cfg"])
    f.set_seed(11)
    f.set_map(W["maps"], W["counts"])
    f.init(0.0, 0.0, 0.0)
    f.set_noise(W["rows"])
    if warm:
        f.run_sim(W["each"][:warm])
    if freeze:
        meas = np.zeros((B, 2, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b in PRE_FROZEN:
            meas[b] = [[900.0, 2.0, 0.1], [900.0, 2.0, 0.1]]; cnt[b] = 2
        f.update((0.0, 0.0), meas, cnt)
    return f


def _saved(f, tmp_path):
    p = tmp_path / "s.ckpt"
    f.save_state(p)
    raw = open(p, "rb").read()
    p.unlink()
    return raw


def _filter_part(raw):
    """a checkpoint without its last two items, the true poses [B][3] and the error sums [B]"""
    return raw[:-32 * B]


def _timesteps(raw):
    return np.frombuffer(raw[-36 * B:-32 * B], dtype=np.int32)


def _sensor_rows(S, idless):
    """16 groups of rows over the instances (b % 16), the edge rows among them."""
    R = S.default_sensor_config
    e = dict(shuffle=1, erase_ids=1) if idless else dict()
    groups = [R(**e), R(p_miss=1.0, **e), R(p_spike=1.0, spike_lo=0.7, spike_hi=0.7, **e), R(p_clutter=1.0, n_clutter=8, **e),
              R(p_clutter=1.0, n_clutter=0, **e), R(p_clutter=0.0, n_clutter=8, **e), R(p_miss=1.0, p_clutter=1.0, n_clutter=8, clutter_r_min=3.0, **e),
              R(p_miss=0.3, p_spike=0.2, spike_lo=0.5, spike_hi=1.5, p_clutter=0.5, n_clutter=8, clutter_r_min=0.5, **e),
              R(p_spike=0.5, spike_lo=-0.5, spike_hi=1.0, shuffle=1), R(p_clutter=0.7, n_clutter=3, erase_ids=1 if idless else 0),
              R(p_miss=0.5, p_clutter=0.5, n_clutter=5, shuffle=1, erase_ids=1 if idless else 0), R(p_spike=0.1, spike_lo=1.0, spike_hi=2.0, **e),
              R(p_miss=0.1, p_clutter=0.2, n_clutter=2, **e), R(p_miss=0.2, p_spike=0.3, spike_lo=0.2, spike_hi=0.4, p_clutter=1.0, n_clutter=8, **e),
              R(p_clutter=0.3, n_clutter=8, clutter_r_min=1.5, shuffle=1), R(p_miss=0.05, p_spike=0.05, spike_lo=0.5, spike_hi=3.0, p_clutter=0.1, n_clutter=1, **e)]
    assert len(groups) == 16
    return [groups[b % 16] for b in range(B)]


# ---- 5. the default row against slam_run_sim_each ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", CLASSES, ids=CLASS_IDS)
def test_default_row_is_the_simulator_run(S, W, hip, tmp_path, L_max, f32):
    each = W["each"]
    dev = _Dev(hip)
    a = _handle(S, W, L_max, f32)
    d_meas, d_count, d_cmd = dev.put(np.zeros((B, KS, 3), np.float32)), dev.put(np.zeros(B, np.int32)), dev.put(each[0])
    msgs, cnts = [], []
    for t in range(T):
        assert hip.hipMemcpy(C.c_void_p(d_cmd), each[t].ctypes.data_as(C.c_void_p), each[t].nbytes, 1) == 0
        a.sense_dev(int(d_cmd), d_meas, d_count, KS)
        a.update_dev_each(d_cmd, d_meas, d_count, KS)
        a.sense_commit(stats=False)
        msgs.append(dev.get(d_meas, np.zeros((B, KS, 3), np.float32))); cnts.append(dev.get(d_count, np.zeros(B, np.int32)))
    one = _handle(S, W, L_max, f32)          # run chunk 1: a launch per tick, whose message is dumped
    one.set_run_chunk(1)
    one.last_meas(KS)
    for t in range(T):
        one.update_sim(each[t])
        m, c = one.last_meas(KS)
        assert np.array_equal(c, cnts[t]), t
        valid = np.arange(KS)[None, :] < np.minimum(c, KS)[:, None]
        assert msgs[t][valid].tobytes() == m[valid].tobytes(), t
        assert not msgs[t][~valid].any(), t
    whole = _handle(S, W, L_max, f32)        # the default chunk: one multi-step launch
    whole.run_sim(each)
    raw = _saved(a, tmp_path)
    assert raw == _saved(one, tmp_path) == _saved(whole, tmp_path)
    assert a.truth().tobytes() == whole.truth().tobytes() and a.error_stats().tobytes() == whole.error_stats().tobytes()
    assert sum(int(c.sum()) for c in cnts) > B and (a.error_stats() > 0).sum() >= B - len(PRE_FROZEN)
    assert (a.status()[PRE_FROZEN] & 4).all() and not a.error_stats()[PRE_FROZEN].any()
    for f in (a, one, whole):
        f.close()
    dev.close()


# ---- 6. faults on: every output against the host hook, the record against the fixed-order sum ----------------------------------------------
@pytest.mark.parametrize("L_max,f32", CLASSES, ids=CLASS_IDS)
def test_faults_against_the_host_hook(S, W, L_max, f32):
    import sense_reference as SR
    cfg, rows, maps, counts = W["cfg"], W["rows"], W["maps"], W["counts"]
    f = _handle(S, W, L_max, f32, warm=6)
    sensor = _sensor_rows(S, idless=True)
    f.set_sensor(sensor)
    seen = dict(short=0, spiked=0, clutter=0, missed=0)
    for tick in range(2):
        cmd = W["each"][6 + tick]
        truth, status = f.truth(), f.status()
        ks = KS if tick == 0 else 5               # a row shorter than many messages
        out = f.sense(cmd, ks)
        inst = np.zeros((B, 16))
        wrong = []
        for b in range(B):
            n = rows[b]
            h = S.sense_instance_host(11, b, 7 + tick, truth[b], cmd[b], maps[b, :counts[b]], cfg, sim_noise=(n.sim_V_00, n.sim_V_11, n.sim_W_00, n.sim_W_11),
                                      row=sensor[b], k_stride=ks, status=int(status[b]))
            got = dict(meas=out["meas"][b], count=int(out["count"][b]), origin=out["origin"][b], fault=out["fault"][b], truth_next=out["truth_next"][b],
                       flags=h["flags"], rec=h["rec"])
            if not SR.same(got, h):
                wrong.append((b, got["count"], h["count"]))
            inst[b] = h["rec"]
            seen["short"] += h["count"] > ks
        assert not wrong, f"tick {tick}: {len(wrong)} instance(s) differ from the host hook (b, count dev/host): {wrong[:10]}"
        want = fixed_order_record(inst, ALL_SUMS)
        assert _same_bits(want, out["rec"]), (tick, want, out["rec"])
        assert want[1] == len(PRE_FROZEN) and want[0] == B - len(PRE_FROZEN) and want[10] == 0 and want[11] == 0
        seen["spiked"] += want[5]; seen["clutter"] += want[6]; seen["missed"] += want[4]
        # the step on the message as a known-id step would be wrong for erased ids: the tick ends without one, nothing is committed
        before = f.truth()
        rec = f.sense_commit()
        assert rec[10] == 0 and rec[11] == 0 and _same_bits(rec[:10], want[:10]) and f.truth().tobytes() == before.tobytes()
    assert all(v > 0 for v in seen.values()), seen
    f.close()


# ---- 7. every *_run_sim call against its LOG sibling on its own log ------------------------------------------------------------------------
SERIES = dict(gate=("nis_sum", "n_upd", "n_rej", "flags"), associate=("n_match", "n_new", "n_drop", "flags"),
              associate_joint=("n_match", "n_new", "n_drop", "flags", "nodes", "d2_joint"), manage=("n_match", "n_new", "n_drop", "flags", "n_removed"),
              manage_merge=("n_match", "n_new", "n_drop", "flags", "n_removed", "n_merged"))
SERIES_BYTES = dict(gate=20, associate=20, associate_joint=36, manage=28, manage_merge=52)    # per instance and tick, on the device


def _check_against_the_log(f, res, raw, err0):
    log = res.sense
    assert f.truth().tobytes() == log.truth[-1].tobytes()
    acc = err0.copy()
    for t in range(log.err_pos.shape[0]):
        ok = ~np.isnan(log.err_pos[t])
        acc[ok] = acc[ok] + log.err_pos[t][ok]
    ts = _timesteps(raw)
    want = np.where(ts > 0, acc / np.maximum(ts, 1), 0.0)
    assert _same_bits(want, f.error_stats())
    assert np.array_equal(log.recs[:, 10], (~np.isnan(log.err_pos)).sum(axis=1))
    assert np.isnan(log.err_pos[:, PRE_FROZEN]).all()


@pytest.mark.parametrize("kind", list(SERIES))
@pytest.mark.parametrize("L_max,f32", CLASSES, ids=CLASS_IDS)
def test_run_sim_equals_the_log_sibling_on_its_own_log(S, W, tmp_path, monkeypatch, kind, L_max, f32):
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    each = W["each"]
    sensor = _sensor_rows(S, idless=kind != "gate")
    extra = dict(map_cfg=dict(prune_every=5)) if kind.startswith("manage") else dict()
    if kind == "manage_merge":
        extra["merge_cfg"] = dict(merge_every=4, sigma=0.05)

    def sim(budget=None, cmds=each, path=False):
        if budget is None:
            monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        else:
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        f = _handle(S, W, L_max, f32)
        f.set_sensor(sensor)
        if path:
            f.set_path(PATH)
        res = getattr(f, kind + "_run_sim")(cmds, T=T, series=True, log=True, k_stride=KS, **extra)
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        return f, res

    def same_results(r1, r2):
        return _same_bits(r1.recs, r2.recs) and all(_same_bits(getattr(r1, n), getattr(r2, n)) for n in SERIES[kind])

    a, res = sim()
    log = res.sense
    raw = _saved(a, tmp_path)
    assert a.timestep == T + 1 and log.meas.shape == (T, B, KS, 3) and log.cmds.tobytes() == each.tobytes()
    # (the labels cover the first k_stride detections of a message, the record all of them)
    assert log.recs[:, 7].sum() == log.count.sum() > B and log.recs[:, 5].sum() >= log.fault.sum() > 0
    assert log.recs[:, 6].sum() >= ((log.origin == -1) & (np.arange(KS) < log.count[:, :, None])).sum() > 0
    _check_against_the_log(a, res, raw, np.zeros(B))
    sib = _handle(S, W, L_max, f32)
    got = getattr(sib, kind + "_run")(log.cmds, log.meas, log.count, series=True, **extra)
    assert same_results(got, res), "the LOG sibling on the run's own log gives other records or series"
    assert _filter_part(_saved(sib, tmp_path)) == _filter_part(raw), "the LOG sibling on the run's own log ends in another filter state"
    sib.close()
    per_tick = (20 * KS + 36 + 8 + SERIES_BYTES[kind]) * B + 128      # the log's rows, the EACH commands, the series
    for budget in (1, int(9.5 * per_tick)):                # one tick per chunk; chunks of 9, 9 and 6 ticks
        k, kres = sim(budget)
        assert same_results(kres, res), budget
        assert _saved(k, tmp_path) == raw, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
        for n in ("meas", "count", "origin", "fault", "truth", "err_pos", "cmds", "recs"):
            assert getattr(kres.sense, n).tobytes() == getattr(log, n).tobytes(), (budget, n)
        k.close()
    a.close()
    if kind == "associate":                                 # the closed loop: the controller steers by the estimate the association gives
        n, nres = sim(cmds=None, path=True)
        nraw = _saved(n, tmp_path)
        assert np.abs(nres.sense.cmds).sum() > 0 and (nres.sense.cmds[:, PRE_FROZEN] == 0).all()
        _check_against_the_log(n, nres, nraw, np.zeros(B))
        sib = _handle(S, W, L_max, f32)
        got = sib.associate_run(nres.sense.cmds, nres.sense.meas, nres.sense.count, series=True)
        assert same_results(got, nres)
        assert _filter_part(_saved(sib, tmp_path)) == _filter_part(nraw)
        sib.close(); n.close()


# ---- 8. a freeze inside the tick -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", CLASSES, ids=CLASS_IDS)
def test_an_instance_that_freezes_in_the_tick_is_not_committed(S, W, hip, L_max, f32):
    cmd = W["cmds"][3]
    fresh = [7, 70, 128, 200, 256]
    twin = _handle(S, W, L_max, f32, warm=3)
    staged = twin.sense(cmd, KS)["truth_next"]
    twin.close()
    dev = _Dev(hip)
    a = _handle(S, W, L_max, f32, warm=3)
    truth0, err0, st0 = a.truth(), a.error_stats(), a.status()
    d_meas, d_count = dev.put(np.zeros((B, KS, 3), np.float32)), dev.put(np.zeros(B, np.int32))
    a.sense_dev(cmd, d_meas, d_count, KS)
    a.sync()
    bad = np.zeros((KS, 3), np.float32); bad[:2] = [[900.0, 2.0, 0.1], [900.0, 2.0, 0.1]]
    two = np.array([2], np.int32)
    for b in fresh:                                         # a message that repeats an id it inserts
        assert hip.hipMemcpy(C.c_void_p(d_meas + b * KS * 12), bad.ctypes.data_as(C.c_void_p), bad.nbytes, 1) == 0
        assert hip.hipMemcpy(C.c_void_p(d_count + b * 4), two.ctypes.data_as(C.c_void_p), 4, 1) == 0
    a.update_dev(cmd, d_meas, d_count, KS)
    rec = a.sense_commit()
    truth1, err1, st1 = a.truth(), a.error_stats(), a.status()
    out = PRE_FROZEN + fresh
    others = np.setdiff1d(np.arange(B), out)
    assert not (st0[fresh] & 4).any() and (st1[out] & 4).all() and not (st1[others] & 4).any()
    assert truth1[out].tobytes() == truth0[out].tobytes() and err1[out].tobytes() == err0[out].tobytes()
    assert rec[10] == B - len(fresh) - len(PRE_FROZEN) == len(others)
    assert truth1[others].tobytes() == staged[others].tobytes()
    assert (truth1[others] != truth0[others]).any(axis=1).all() and rec[11] > 0
    a.close()
    dev.close()


# ---- 9. the pending and scope rules ----------------------------------------------------------------------------------------------------------
def _sim_runs(Lb, h, source, cmd_ptr):
    """the five *_run_sim calls with default configs, one tick, no outputs: their return codes"""
    runs = [("slam_gate_run_sim", 1, 5), ("slam_associate_run_sim", 1, 5), ("slam_associate_joint_run_sim", 1, 7), ("slam_manage_run_sim", 2, 6),
            ("slam_manage_merge_run_sim", 3, 7)]
    return [getattr(Lb, name)(h, *([None] * ncfg), source, cmd_ptr, KS, 1, *([None] * nout), None) for name, ncfg, nout in runs]


def test_every_refusal_leaves_the_checkpoint_byte_identical(S, W, hip, tmp_path):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    err = (lambda: Lb.slam_last_error().decode())
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    cmd = np.array([0.05, 0.01], np.float32); cmds_each = np.ascontiguousarray(W["each"][0])
    meas, cnt = np.zeros((B, KS, 3), np.float32), np.zeros(B, np.int32)
    step_of = (lambda raw: int(np.frombuffer(raw[40:44], np.uint32)[0]))       # the RNG step of the checkpoint header

    def senses(h):
        return [Lb.slam_sense(h, fp(cmd), 0, fp(meas), ip(cnt), KS, None, None, None, None),
                Lb.slam_sense_dev(h, C.cast(fp(cmd), C.c_void_p), 0, C.c_void_p(meas.ctypes.data), C.c_void_p(cnt.ctypes.data), KS, None, None)]
    a = _handle(S, W, 20, False, warm=2)
    a.set_path(PATH)
    before = _saved(a, tmp_path)
    # a commit with nothing pending
    assert Lb.slam_sense_commit(a.h, None) == STATE and "no sense is pending" in err()
    assert _saved(a, tmp_path) == before
    # everything that is refused while a sense is pending, in a tick without a step: nothing but the RNG step may differ afterwards
    a.sense(cmd, KS)
    refused = senses(a.h) + [Lb.slam_step_sim(a.h, fp(cmd)), Lb.slam_run_sim(a.h, fp(cmd), 1), Lb.slam_run_sim_each(a.h, fp(cmds_each), 1),
                             Lb.slam_nav_run(a.h, 1, None), Lb.slam_monitor_run(a.h, None, 0, fp(cmd), 1, None, None, None, None),
                             Lb.slam_monitor_run(a.h, None, 2, None, 1, None, None, None, None),
                             Lb.slam_innovation_run(a.h, None, 0, fp(cmd), None, None, 0, 1, None, None, None, None),
                             Lb.slam_innovation_run(a.h, None, 2, None, None, None, 0, 1, None, None, None, None),
                             Lb.slam_save_state(a.h, str(tmp_path / "no.ckpt").encode())]
    refused += _sim_runs(Lb, a.h, 0, fp(cmd)) + _sim_runs(Lb, a.h, 1, fp(cmds_each)) + _sim_runs(Lb, a.h, 2, None)
    assert refused == [STATE] * len(refused) and len(refused) == 26, refused
    assert "a sense is pending" in err() and not (tmp_path / "no.ckpt").exists()
    assert a.sense_commit()[10] == 0
    after = _saved(a, tmp_path)
    assert after[:40] == before[:40] and after[44:] == before[44:], "a call refused while a sense was pending changed the state"
    assert step_of(after) == step_of(before) + 1
    # while slam_track_instance is on
    a.track_instance(3)
    on = _saved(a, tmp_path)
    refused = senses(a.h) + _sim_runs(Lb, a.h, 0, fp(cmd)) + _sim_runs(Lb, a.h, 2, None)
    assert refused == [STATE] * 12 and "slam_track_instance" in err(), refused
    assert _saved(a, tmp_path) == on == after
    a.track_instance(-1)
    # a host-fed step is no simulator source: allowed while pending, and the commit follows it
    out = a.sense(cmd, KS)
    a.update(cmd, out["meas"], out["count"])
    assert a.sense_commit()[10] == B - len(PRE_FROZEN)
    mid = _saved(a, tmp_path)
    assert step_of(mid) == step_of(after) + 1 and mid[44:] != after[44:]
    # load_state and init clear a pending sense
    p = tmp_path / "mid.ckpt"
    a.save_state(p)
    a.sense(cmd, KS)
    a.load_state(p)
    assert Lb.slam_sense_commit(a.h, None) == STATE and _saved(a, tmp_path) == mid
    a.sense(cmd, KS)
    a.init(0.0, 0.0, 0.0)
    assert Lb.slam_sense_commit(a.h, None) == STATE
    a.update_sim(cmd)
    a.close()
    # before slam_init, without a map, NAV without a path
    e = S.BatchedEKF(B, 20).readParams(W["cfg"])
    for word, prepare in (("slam_init", lambda: None), ("slam_set_map", lambda: e.init(0.0, 0.0, 0.0))):
        prepare()
        raw = _saved(e, tmp_path)
        refused = senses(e.h) + _sim_runs(Lb, e.h, 0, fp(cmd))
        assert refused == [STATE] * 7 and word in err(), (word, refused, err())
        assert _saved(e, tmp_path) == raw, word
    e.set_map(W["maps"], W["counts"])
    e.run_sim(W["cmds"][:2])
    raw = _saved(e, tmp_path)
    refused = _sim_runs(Lb, e.h, 2, None)
    assert refused == [STATE] * 5 and "path" in err(), refused
    bad = (S.SensorConfig * B)(*[S.default_sensor_config(clutter_r_min=3.5 if b == 200 else 0.0) for b in range(B)])
    assert Lb.slam_set_sensor_each(e.h, bad) == ARG and "instance 200" in err() and "clutter_r_min" in err()
    assert _saved(e, tmp_path) == raw
    e.close()


# ---- more than 64 landmarks in view on the device ---------------------------------------------------------------------------------------------
def test_too_long_on_the_device_against_the_host_hook(S, W):
    """Maps of 63, 64, 65 and 80 landmarks, all in view: the second pass of the generator over the map, the cap at 64 detections in LDS and
    SLAM_SENSE_TOO_LONG, every output against the host hook in bits."""
    import sense_reference as SR
    cfg = W["cfg"]
    counts = np.array([3, 63, 64, 65, 80, 80, 72, 12], np.int32)
    n = len(counts)
    ang = np.linspace(-1.2, 1.2, 80)
    rng = np.random.default_rng(9)
    maps = np.stack([np.stack([r * np.cos(ang), r * np.sin(ang)], axis=1) for r in rng.uniform(0.8, 2.5, (n, 80))])
    sensor = [S.default_sensor_config(), S.default_sensor_config(p_miss=0.3, p_spike=0.3, spike_lo=0.5, spike_hi=1.0, p_clutter=1.0, n_clutter=8, shuffle=1),
              S.default_sensor_config(p_clutter=1.0, n_clutter=8, erase_ids=1), S.default_sensor_config(shuffle=1, erase_ids=1),
              S.default_sensor_config(p_miss=0.5, p_clutter=0.5, n_clutter=8, shuffle=1), S.default_sensor_config(), S.default_sensor_config(p_spike=1.0, spike_lo=0.1, spike_hi=0.2),
              S.default_sensor_config(p_clutter=1.0, n_clutter=8)]
    f = S.BatchedEKF(n, 100).readParams(cfg)
    f.set_seed(11); f.set_map(maps, counts); f.init(0.0, 0.0, 0.0)
    f.set_sensor(sensor)
    cmd = np.array([0.05, 0.01], np.float32)
    for step, ks in enumerate((80, 16)):            # (a tick without a step still advances the RNG step)
        out = f.sense(cmd, ks)
        truth = f.truth()
        inst = np.zeros((n, 16))
        for b in range(n):
            h = S.sense_instance_host(11, b, step, truth[b], cmd, maps[b, :counts[b]], cfg, row=sensor[b], k_stride=ks)
            got = dict(meas=out["meas"][b], count=int(out["count"][b]), origin=out["origin"][b], fault=out["fault"][b], truth_next=out["truth_next"][b],
                       flags=h["flags"], rec=h["rec"])
            assert SR.same(got, h), (ks, b, got["count"], h["count"])
            assert h["flags"] == (SR.TOO_LONG if counts[b] > 64 else 0) and h["rec"][3] == min(counts[b], 64), (b, h["flags"], h["rec"][3])
            inst[b] = h["rec"]
        assert _same_bits(fixed_order_record(inst, ALL_SUMS), out["rec"]) and out["rec"][2] == 4
        assert f.sense_commit()[10] == 0
    f.close()


def test_the_ukf_is_refused_with_its_state_untouched(S, W, tmp_path):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    err = (lambda: Lb.slam_last_error().decode())
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    n = 8
    cmd = np.array([0.05, 0.01], np.float32); meas, cnt = np.zeros((n, KS, 3), np.float32), np.zeros(n, np.int32)
    cfg = S.default_config(); cfg.landmark_id_is_known = 0
    for f, word in ((S.BatchedUKF(n, 20).readParams(), "EKF_SLAM"), (S.BatchedEKF(n, 20).readParams(cfg), "landmark_id_is_known")):
        f.set_map(W["maps"][0]); f.init(0.0, 0.0, 0.0)
        f.run_sim(W["cmds"][:4])
        before = _saved(f, tmp_path)
        rows = (S.SensorConfig * n)()
        got = [Lb.slam_set_sensor_each(f.h, rows), Lb.slam_set_sensor_each(f.h, None),
               Lb.slam_sense(f.h, fp(cmd), 0, fp(meas), ip(cnt), KS, None, None, None, None),
               Lb.slam_sense_dev(f.h, C.cast(fp(cmd), C.c_void_p), 0, C.c_void_p(meas.ctypes.data), C.c_void_p(cnt.ctypes.data), KS, None, None),
               Lb.slam_sense_commit(f.h, None),
               Lb.slam_gate_run_sim(f.h, None, 0, fp(cmd), KS, 1, None, None, None, None, None, None),
               Lb.slam_associate_run_sim(f.h, None, 0, fp(cmd), KS, 1, None, None, None, None, None, None),
               Lb.slam_associate_joint_run_sim(f.h, None, 0, fp(cmd), KS, 1, None, None, None, None, None, None, None, None),
               Lb.slam_manage_run_sim(f.h, None, None, 0, fp(cmd), KS, 1, None, None, None, None, None, None, None),
               Lb.slam_manage_merge_run_sim(f.h, None, None, None, 0, fp(cmd), KS, 1, None, None, None, None, None, None, None, None)]
        assert got == [UNSUPPORTED] * len(got), (word, got)
        assert word in err()
        assert _saved(f, tmp_path) == before, word
        f.close()
