"""Absolute position and heading fixes on the MI355X (slam_fix*, slam_fix_sense*, slam_fix_run), batch 257, per-instance maps and noise
rows on, states grown by real steps, a few instances frozen and a few non-finite; L_max 20 and 50 in both storage types and one handle of
the class above 256 landmarks:
  (a) slam_get_state, verdict, nis, the record and the bytes of slam_last_fix_work equal the host hook - the two SEQUENTIAL passes of
      csrc/fix_kernel.h compiled for the host - in bits, for every combination of kinds and every verdict across the batch: this fails
      if the one-pass kernel is not bit-equal to the sequential definition;
  (b) checkpoints of instances without an applied part are byte-identical; M, ids, flags, timestep, truth and err_sum of every instance;
  (c) three further steps equal, bit for bit, the CPU oracle stepped from the hook's state;
  (d) the device-pointer variants equal the host-pointer calls;
  (e) slam_fix_run equals its loop of single calls under two chunk sizes, for SHARED, EACH and NAV;
  (f) slam_sense_dev -> slam_step_associated_dev -> slam_sense_commit -> slam_fix_sense_dev -> slam_fix_dev equals the host-side
      composition of the hooks;
  (g) a fix while a sense is pending is SLAM_ERR_STATE and UKF handles are refused, with the state untouched."""
import ctypes as C
import math

import numpy as np
import pytest

import assoc_reference as AR
import fix_reference as FR
import innovation_reference as IR
from record_tree import ALL_SUMS, fixed_order_record
from test_assoc_gpu import B, _config
from test_gate_gpu import _Dev, _same_bits
from test_map_gpu import S, hip, _each, _grown, _items, _raw, _same_state  # noqa: F401
from test_sense_gpu import PATH, W, _saved  # noqa: F401
from test_sense_gpu import _handle as _sim_handle

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, STATE = -1, -3, -4
SKIP = 1 | 4 | 32
CLASSES = [(20, 18, False), (20, 18, True), (50, 48, False), (50, 48, True)]
CLASS_IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32"]
HOWS = ("near", "far_pos", "far_yaw", "nan_sigma", "neg_sigma", "inf_z", "near")


def _fix_row(rng, x, how):
    """The fix row of one verdict scenario of HOWS, built from the estimate x (three draws of rng)."""
    row = np.array([x[0] + rng.normal(0, 0.01), x[1] + rng.normal(0, 0.01), x[2] + rng.normal(0, 0.005), 0.03, 0.01])
    if how == "far_pos":
        row[0] += 20.0
    elif how == "far_yaw":
        row[2] += 2.0
    elif how == "nan_sigma":
        row[3] = math.nan; row[4] = math.inf
    elif how == "neg_sigma":
        row[3] = -0.03; row[4] = -0.01
    elif how == "inf_z":
        row[1] = -math.inf; row[2] = math.nan
    return row


def _fix_rows(states, seed):
    """kinds b % 4 (every combination; some with bits that are ignored) and a verdict scenario (b // 4) % 7 per instance, built from
    the instance's own estimate."""
    rng = np.random.default_rng(seed)
    n = len(states)
    fix = np.zeros((n, 5)); kinds = np.zeros(n, np.int32)
    for b, st in enumerate(states):
        x = st["x"] if np.isfinite(st["x"][:3]).all() else np.zeros(3)
        fix[b] = _fix_row(rng, x, HOWS[(b // 4) % len(HOWS)])
        kinds[b] = (b % 4) | (16 if b % 5 == 0 else 0)
    return fix, kinds


def _hooks(S, states, status, L_max, f32, fix, kinds, cfg=None):
    return [S.fix_instance_host(st["x"], st["P"], L_max, fix[b], int(kinds[b]), status=int(status[b]), f32_storage=f32, cfg=cfg)
            for b, st in enumerate(states)]


def _check_fix(S, f, r, before, status, hooks, after, f32, what):
    n = len(before)
    hv = np.array([h["verdict"] for h in hooks], np.int32)
    assert np.array_equal(r["verdict"], hv), (what, np.nonzero(r["verdict"] != hv)[0][:10])
    assert _same_bits(r["nis"], np.stack([h["nis"] for h in hooks])), what
    wrong = [b for b in range(n) if not _same_state(after[b], dict(x=hooks[b]["x"], P=hooks[b]["P"], M=before[b]["M"], ids=before[b]["ids"]))]
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the hook's state: {wrong[:10]}"
    assert _same_bits(fixed_order_record(np.stack([h["rec"] for h in hooks]), ALL_SUMS), r["rec"]), (what, r["rec"])
    by, fix_ms, total_ms = f.last_fix_work()
    assert by == FR.model_bytes([st["M"] for st in before], hv, 4 if f32 else 8) and fix_ms == -1.0 and total_ms == -1.0, (what, by)
    return hv


# ---- (a), (b), (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,M,f32", CLASSES, ids=CLASS_IDS)
def test_the_fix_equals_the_host_hook_in_bits_and_the_steps_after_follow_the_oracle(S, oracle, tmp_path, L_max, M, f32):
    O = oracle
    cfg = _config(S)
    rows, maps = _each(S, cfg, 270 + L_max)
    f = _grown(S, L_max, M, f32, cfg, rows, maps)
    what = CLASS_IDS[CLASSES.index((L_max, M, f32))]
    status = f.status()
    assert (status & IR.INST_INDEX_OOR).any() and (status & IR.INST_NONFINITE).any() and (status == 0).sum() > B // 2
    before = [f.get_state(b) for b in range(B)]
    assert max(st["M"] for st in before) == M
    raw0 = _items(_raw(f, tmp_path))
    fix, kinds = _fix_rows(before, 31 + L_max)
    r = f.fix(fix, kinds)
    after = [f.get_state(b) for b in range(B)]
    raw1 = _items(_raw(f, tmp_path))
    hooks = _hooks(S, before, status, L_max, f32, fix, kinds)
    hv = _check_fix(S, f, r, before, status, hooks, after, f32, what)
    print(f"{what}: verdicts {dict(zip(*np.unique(hv, return_counts=True)))}")
    assert {0x00, 0x01, 0x10, 0x11, 0x02, 0x12, 0x20, 0x21, 0x04, 0x40, 0x44} <= set(hv.tolist())
    applied = ((hv & 15) == 1) | ((hv >> 4) == 1)
    assert r["rec"][0] == applied.sum() > B // 4 and r["rec"][13] == ((status & SKIP) != 0).sum() and not hv[(status & SKIP) != 0].any()
    assert r["rec"][2] == ((hv & 15) == 1).sum() and r["rec"][7] == ((hv >> 4) == 1).sum() and r["rec"][14] == r["rec"][15] == 0
    # (b)
    for b in range(B):
        for name in ("M", "ids", "flags", "ts", "truth", "err"):
            assert raw0[name][b] == raw1[name][b], (what, b, name, "a fix does not touch it")
        if not applied[b]:
            for name in ("P", "x"):
                assert raw0[name][b] == raw1[name][b], (what, b, name, "an instance without an applied part is not written")
        else:
            assert raw0["P"][b] != raw1["P"][b], (what, b)
    # a fix pulls the estimate onto the measurement
    # (x' - z = sigma^2 (P_pp + sigma^2 I)^-1 (x - z): a contraction) and shrinks the measured variance
    pos = np.nonzero(hv == 0x01)[0]
    d0 = np.array([np.hypot(*(before[b]["x"][:2] - fix[b, :2])) for b in pos]); d1 = np.array([np.hypot(*(after[b]["x"][:2] - fix[b, :2])) for b in pos])
    assert len(pos) > 8 and (d1 < d0).all() and all(after[b]["P"][2, 2] < before[b]["P"][2, 2] for b in np.nonzero(hv >> 4 == 1)[0])

    # (c) three more steps that re-observe two landmarks
    T = 3
    rng = np.random.default_rng(290 + L_max)
    meas = np.zeros((T, B, 2, 3), np.float32); cnt = np.zeros((T, B), np.int32)
    for b in range(B):
        st = after[b]
        if not np.isfinite(st["x"]).all():
            continue
        for t in range(T):
            m = [AR.clean(rng, st, int(j), float(st["ids"][j])) for j in rng.permutation(st["M"])[:2]]
            meas[t, b, :len(m)] = np.asarray(m, dtype=np.float32).reshape(-1, 3); cnt[t, b] = len(m)
    cmds = np.stack([rng.uniform(0.0, 0.02, (T, B)), rng.uniform(-0.01, 0.01, (T, B))], axis=2).astype(np.float32)
    for t in range(T):
        f.update(cmds[t], meas[t], cnt[t])
    final = [f.get_state(b) for b in range(B)]
    status1 = f.status()
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    wrong, compared = [], 0
    for b in range(B):
        if status[b] != 0:
            continue
        ekf = O.OracleEKF(IR.config_for(rows[b]), L_max=L_max, mode=mode)
        ekf.set_state(hooks[b]["x"], hooks[b]["P"], before[b]["ids"], timestep=int(after[b]["timestep"]))
        fl = 0
        for t in range(T):
            fl |= ekf.update(cmds[t, b, 0], cmds[t, b, 1], meas[t, b, :cnt[t, b]])
        twin = ekf.state()
        if fl != status1[b] or not _same_state(final[b], twin):
            wrong.append((b, int(status1[b]), int(fl), hex(hv[b])))
        compared += 1
    assert not wrong, f"{what}: {len(wrong)} of {compared} instance(s) differ from the oracle continued from the hook's state: {wrong[:10]}"
    assert compared > B // 2
    f.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_map_of_more_than_256_landmarks(S, f32):
    """L_max 300 holding 262 landmarks in 3 instances (n = 527: more rows than the workgroup has lanes, the workspace above 24 KB):
    position only, heading only and both, against the hook in bits."""
    nb, L_max, M0 = 3, 300, 262
    cfg = _config(S)
    f = S.BatchedEKF(nb, L_max, dtype=S.F32 if f32 else S.F64).readParams(cfg)
    f.set_seed(11); f.init(0.3, -0.2, 0.4)
    j = np.arange(M0)
    rr, bb, ids = 1.5 + 0.5 * (j // 10), -1.2 + 0.26 * (j % 10), 100.0 + j
    rng = np.random.default_rng(77)
    for rnd in range(3):                                             # insertions, then two rounds of updates
        for lo in range(0, M0, 40):
            hi = min(lo + 40, M0)
            m = np.zeros((nb, hi - lo, 3), np.float32)
            m[:, :, 0] = ids[lo:hi]
            m[:, :, 1] = rr[lo:hi] + min(rnd, 1) * 0.02 * rng.standard_normal((nb, hi - lo))
            m[:, :, 2] = bb[lo:hi] + min(rnd, 1) * 0.002 * rng.standard_normal((nb, hi - lo))
            f.update((0.02, 0.01), m, np.full(nb, hi - lo, np.int32))
    status = f.status()
    before = [f.get_state(b) for b in range(nb)]
    assert all(st["M"] == M0 for st in before) and not status.any()
    fix = np.array([[st["x"][0] + 0.01, st["x"][1] - 0.01, st["x"][2] + 0.004, 0.02, 0.01] for st in before])
    kinds = np.array([1, 2, 3], np.int32)
    r = f.fix(fix, kinds)
    after = [f.get_state(b) for b in range(nb)]
    hooks = _hooks(S, before, status, L_max, f32, fix, kinds)
    hv = _check_fix(S, f, r, before, status, hooks, after, f32, "L300")
    assert hv.tolist() == [0x01, 0x10, 0x11]
    f.close()


def test_a_batch_one_past_the_work_sums_launch(S):
    """B = 65 537, L_max = 1 with its landmark mapped, a position fix on every instance: the work sum (csrc/aux_device.h) launches
    256 x 256 lanes, so this is the smallest batch at which a lane - lane 0 - takes a second element of its grid-stride loop, and the
    record tree (csrc/record_kernel.h) joins 257 partial records.  Every instance is stepped alike into the same state, so the hook is
    evaluated once per kind of fix row (applied, rejected, invalid: b % 3; the last instance is a rejected one, whose traffic differs from
    its neighbours'); the bytes of slam_last_fix_work equal the model exactly and the record equals the restated tree in bits."""
    nb, L_max = 65537, 1
    f = S.BatchedEKF(nb, L_max).readParams(_config(S))
    f.set_seed(11); f.init(0.3, -0.2, 0.4)
    m = np.tile(np.array([[[100.0, 2.0, 0.1]]], np.float32), (nb, 1, 1))
    for _ in range(2):                                               # the insertion, then an update
        f.update((0.02, 0.01), m, np.ones(nb, np.int32))
    probe = (0, 1, 2, 255, 256, 65535, 65536)
    before = {b: f.get_state(b) for b in probe}
    st = before[0]
    assert not f.status().any() and all(s["M"] == 1 and _same_state(s, st) for s in before.values())
    rng = np.random.default_rng(5)
    rows3 = np.stack([_fix_row(rng, st["x"], how) for how in ("near", "far_pos", "nan_sigma")])
    which = np.arange(nb) % 3
    kinds = np.ones(nb, np.int32)
    r = f.fix(rows3[which], kinds)
    hooks3 = _hooks(S, [st] * 3, np.zeros(3, np.int32), L_max, False, rows3, kinds[:3])
    hv3 = np.array([h["verdict"] for h in hooks3], np.int32)
    assert hv3.tolist() == [0x01, 0x02, 0x04], hv3                      # applied, rejected, invalid
    assert np.array_equal(r["verdict"], hv3[which]) and _same_bits(r["nis"], np.stack([h["nis"] for h in hooks3])[which])
    want = fixed_order_record(np.stack([h["rec"] for h in hooks3])[which], ALL_SUMS)
    by = f.last_fix_work()[0]
    model = FR.model_bytes(np.ones(nb, np.int64), hv3[which], 8)
    print(f"B = {nb}: slam_last_fix_work bytes {by}, the model {model}; record {r['rec']}")
    assert by == model, (by, model)
    assert _same_bits(want, r["rec"]) and r["rec"][2] == (which == 0).sum() and r["rec"][3] == (which == 1).sum(), (want, r["rec"])
    for b in probe:
        h = hooks3[b % 3]
        assert _same_state(f.get_state(b), dict(x=h["x"], P=h["P"], M=1, ids=st["ids"])), b
    f.close()


# ---- (d) the device-pointer variants ------------------------------------------------------------------------------------------------------------
def test_device_pointer_variants_equal_the_host_pointer_calls(S, hip, W, tmp_path):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    dev = _Dev(hip)
    a = _sim_handle(S, W, 20, True, warm=6)
    d = _sim_handle(S, W, 20, True, warm=6)
    R = S.default_fix_sensor_config
    rows = [R(pos_halfwidth=0.03, yaw_halfwidth=0.01, sigma_pos=0.02, sigma_yaw=0.006, p_miss_pos=0.3, p_miss_yaw=0.3, p_jump=0.3, jump_lo=1.0, jump_hi=2.0, kinds=3)] * B
    a.set_fix_sensor(rows); d.set_fix_sensor(rows)
    s = a.fix_sense()
    dfix, dkinds, djump = dev.put(np.zeros((B, 5))), dev.put(np.zeros(B, np.int32)), dev.put(np.zeros(B, np.int32))
    assert d.fix_sense(dev=(dfix, dkinds, djump)) is None
    d.sync()
    assert _same_bits(dev.get(dfix, s["fix"]), s["fix"]) and np.array_equal(dev.get(dkinds, s["kinds"]), s["kinds"])
    assert np.array_equal(dev.get(djump, s["jumped"]), s["jumped"]) and s["jumped"].sum() > B // 8 and len(set(s["kinds"].tolist())) == 4
    ra = a.fix(s["fix"], s["kinds"])
    dv, dn, dr = dev.put(np.zeros(B, np.int32)), dev.put(np.zeros((B, 2))), dev.put(np.zeros(16))
    assert Lb.slam_fix_dev(d.h, None, C.c_void_p(dfix), C.c_void_p(dkinds), C.c_void_p(dv), C.c_void_p(dn), C.c_void_p(dr)) == 0
    d.sync()
    assert np.array_equal(dev.get(dv, ra["verdict"]), ra["verdict"]) and _same_bits(dev.get(dn, ra["nis"]), ra["nis"]) and _same_bits(dev.get(dr, ra["rec"]), ra["rec"])
    assert ra["rec"][3] > 0 and ra["rec"][2] > B // 4, "jumps are rejected, clean fixes applied"
    assert _saved(a, tmp_path) == _saved(d, tmp_path), "slam_fix_dev against slam_fix"
    assert a.last_fix_work() == d.last_fix_work()
    assert d.fix(int(dfix), int(dkinds)) is None and a.fix(s["fix"], s["kinds"], stats=False) is None     # outputs not wanted
    assert _saved(a, tmp_path) == _saved(d, tmp_path)
    a.close(); d.close(); dev.close()


# ---- (e) the run against its loop, and chunking -------------------------------------------------------------------------------------------------
def _sensor_rows(S):
    R = S.default_fix_sensor_config
    groups = [R(pos_halfwidth=0.03, sigma_pos=0.02, kinds=1), R(yaw_halfwidth=0.01, sigma_yaw=0.006, kinds=2),
              R(pos_halfwidth=0.03, yaw_halfwidth=0.01, sigma_pos=0.02, sigma_yaw=0.006, kinds=3), R(),
              R(pos_halfwidth=0.03, yaw_halfwidth=0.01, sigma_pos=0.02, sigma_yaw=0.006, p_jump=0.5, jump_lo=1.0, jump_hi=3.0, kinds=3),
              R(pos_halfwidth=0.03, yaw_halfwidth=0.01, sigma_pos=0.02, sigma_yaw=0.006, p_miss_pos=0.5, p_miss_yaw=0.5, kinds=3)]
    return [groups[b % len(groups)] for b in range(B)]


@pytest.mark.parametrize("source", ["shared", "each", "nav"])
def test_fix_run_equals_its_loop_whatever_the_chunking(S, W, tmp_path, monkeypatch, source):
    T, every = 12, 5
    cmds = {"shared": W["cmds"][:T], "each": W["each"][:T], "nav": None}[source]
    fc = S.FixConfig(S.default_fix_config().gate_pos, S.default_fix_config().gate_yaw, every)
    names = ("verdict", "kinds")

    def handle():
        f = _sim_handle(S, W, 20, False, warm=3)
        f.set_fix_sensor(_sensor_rows(S))
        if source == "nav":
            f.set_path(PATH)
        return f
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    a = handle()
    res = a.fix_run(cmds, T=T, series=True, cfg=fc)
    fix_ticks = [t for t in range(T) if (t + 1) % every == 0]
    assert fix_ticks == [4, 9] and res.recs.shape == (T, 16) and a.timestep == a.get_state(0)["timestep"]
    assert not np.delete(res.recs, fix_ticks, axis=0).any() and not np.delete(res.verdict, fix_ticks, axis=0).any()
    assert np.isnan(np.delete(res.nis, fix_ticks, axis=0)).all() and not np.delete(res.fix, fix_ticks, axis=0).any()
    assert (res.recs[fix_ticks, 0] > B // 4).all() and res.recs[fix_ticks, 3].sum() > 0
    loop = handle()
    for t in range(T):
        if source == "nav":
            loop.run_nav(1)
        else:
            loop.update_sim(cmds[t])
        if t in fix_ticks:
            s = loop.fix_sense()
            r = loop.fix(s["fix"], s["kinds"], cfg=fc)
            assert _same_bits(s["fix"], res.fix[t]) and np.array_equal(s["kinds"], res.kinds[t]), t
            assert np.array_equal(r["verdict"], res.verdict[t]) and _same_bits(r["nis"], res.nis[t]) and _same_bits(r["rec"], res.recs[t]), t
    final = _saved(a, tmp_path)
    assert _saved(loop, tmp_path) == final, "the checkpoint after slam_fix_run differs from the loop"
    loop.close()
    per_tick = 64 * B + 128 + (8 * B if source == "each" else 0)
    for budget in (1, 3 * per_tick + 7):                         # one tick per chunk, and chunks of three
        monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        k = handle()
        got = k.fix_run(cmds, T=T, series=True, cfg=fc)
        assert _same_bits(got.recs, res.recs) and _same_bits(got.nis, res.nis) and _same_bits(got.fix, res.fix), budget
        assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in names), budget
        assert _saved(k, tmp_path) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
        assert k.last_fix_work()[0] == a.last_fix_work()[0], budget
        k.close()
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    by, fix_ms, total_ms = a.last_fix_work()
    assert by > 0 and fix_ms == -1.0 and total_ms > 0.0
    plain = handle()                                             # without series the state is the same
    plain.fix_run(cmds, T=T, cfg=fc)
    assert _saved(plain, tmp_path) == final
    plain.set_nav_timing(True)
    plain.fix_run(cmds if cmds is None else cmds[:10], T=10, cfg=fc)
    by, fix_ms, total_ms = plain.last_fix_work()
    assert 0.0 < fix_ms < total_ms and by > 0
    plain.close(); a.close()


# ---- (f) a tick composed from the _dev calls ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", [(20, False), (50, True)], ids=["L20_f64", "L50_f32"])
def test_a_tick_composed_from_the_dev_calls_equals_the_composition_of_the_hooks(S, W, hip, L_max, f32):
    KS = 16
    dev = _Dev(hip)
    f = _sim_handle(S, W, L_max, f32, warm=2)
    rows = _sensor_rows(S)
    f.set_fix_sensor(rows)
    d_meas, d_count = dev.put(np.zeros((B, KS, 3), np.float32)), dev.put(np.zeros(B, np.int32))
    dfix, dkinds, djump = dev.put(np.zeros((B, 5))), dev.put(np.zeros(B, np.int32)), dev.put(np.zeros(B, np.int32))
    dv, dn = dev.put(np.zeros(B, np.int32)), dev.put(np.zeros((B, 2)))
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    applied = 0
    for t in range(4):
        cmd = W["cmds"][t]
        f.sense_dev(cmd, d_meas, d_count, KS)
        f.step_associated_dev(cmd, d_meas, d_count, KS, stats=False)
        f.sense_commit(stats=False)
        if t % 2 == 0:
            continue
        status, truth = f.status(), f.truth()
        before = [f.get_state(b) for b in range(B)]
        assert f.fix_sense(dev=(dfix, dkinds, djump)) is None
        assert Lb.slam_fix_dev(f.h, None, C.c_void_p(dfix), C.c_void_p(dkinds), C.c_void_p(dv), C.c_void_p(dn), None) == 0
        after = [f.get_state(b) for b in range(B)]
        sensed = [S.fix_sense_instance_host(11, b, f.timestep, truth[b], rows[b]) for b in range(B)]
        fix = np.stack([s["fix"] for s in sensed]); kinds = np.array([s["kinds"] for s in sensed], np.int32)
        assert _same_bits(dev.get(dfix, fix), fix) and np.array_equal(dev.get(dkinds, kinds), kinds), t
        assert np.array_equal(dev.get(djump, kinds), [s["jumped"] for s in sensed]), t
        hooks = _hooks(S, before, status, L_max, f32, fix, kinds)
        hv = np.array([h["verdict"] for h in hooks], np.int32)
        assert np.array_equal(dev.get(dv, hv), hv) and _same_bits(dev.get(dn, np.zeros((B, 2))), np.stack([h["nis"] for h in hooks])), t
        wrong = [b for b in range(B) if not _same_state(after[b], dict(x=hooks[b]["x"], P=hooks[b]["P"], M=before[b]["M"], ids=before[b]["ids"]))]
        assert not wrong, (t, wrong[:10])
        applied += int((((hv & 15) == 1) | ((hv >> 4) == 1)).sum())
    assert applied > B
    f.close(); dev.close()


# ---- (g) the states and the kinds the calls refuse -----------------------------------------------------------------------------------------------
def test_a_fix_while_a_sense_is_pending_is_refused_and_changes_nothing(S, W, hip, tmp_path):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    KS = 16
    dev = _Dev(hip)
    err = (lambda: Lb.slam_last_error().decode())
    dp, ip = (lambda a: a.ctypes.data_as(_lib._dp)), (lambda a: a.ctypes.data_as(_lib._ip))
    fix = np.tile(np.array([0.1, 0.1, 0.0, 0.05, 0.02]), (B, 1)); kinds = np.full(B, 3, np.int32)
    d_meas, d_count = dev.put(np.zeros((B, KS, 3), np.float32)), dev.put(np.zeros(B, np.int32))
    saved = []
    for attempt in (True, False):
        f = _sim_handle(S, W, 20, False, warm=2)
        cmd = W["cmds"][2]
        f.sense_dev(cmd, d_meas, d_count, KS)
        if attempt:
            assert Lb.slam_fix(f.h, None, dp(fix), ip(kinds), None, None, None) == STATE and "sense is pending" in err()
            assert Lb.slam_fix_dev(f.h, None, C.c_void_p(fix.ctypes.data), C.c_void_p(kinds.ctypes.data), None, None, None) == STATE
            assert Lb.slam_fix_sense(f.h, dp(fix.copy()), ip(kinds.copy()), None) == STATE
            assert Lb.slam_fix_run(f.h, None, 0, W["cmds"].ctypes.data_as(_lib._fp), 2, None, None, None, None) == STATE
        f.update_dev(cmd, d_meas, d_count, KS)
        f.sense_commit(stats=False)
        saved.append(_saved(f, tmp_path))
        if attempt:
            assert f.fix(fix, kinds)["rec"][1] > 0      # after the commit it runs
        f.close()
    assert saved[0] == saved[1], "a refused fix leaves the state untouched"
    dev.close()


def test_unsupported_kinds_and_states_are_refused_and_keep_their_state(S, tmp_path):
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    Lb = _lib.lib()
    L, T, n = 20, 10, 8
    lm, sim_cmds = make_scenario(341, L, T)
    fix = np.zeros((n, 5)); kinds = np.full(n, 3, np.int32)
    dp, ip, fp = (lambda a: a.ctypes.data_as(_lib._dp)), (lambda a: a.ctypes.data_as(_lib._ip)), (lambda a: a.ctypes.data_as(_lib._fp))
    err = (lambda: Lb.slam_last_error().decode())
    u = S.BatchedUKF(n, L).readParams()
    u.set_map(lm); u.init(0.0, 0.0, 0.0)
    u.run_sim(sim_cmds)
    before = _raw(u, tmp_path)
    assert Lb.slam_fix(u.h, None, dp(fix), ip(kinds), None, None, None) == UNSUPPORTED and "EKF_SLAM" in err()
    assert Lb.slam_fix_sense(u.h, dp(fix), ip(kinds), None) == UNSUPPORTED
    assert Lb.slam_fix_run(u.h, None, 0, fp(sim_cmds), 2, None, None, None, None) == UNSUPPORTED
    assert Lb.slam_set_fix_sensor_each(u.h, None) == UNSUPPORTED and Lb.slam_last_fix_work(u.h, None, None, None) == STATE
    assert _raw(u, tmp_path) == before
    u.close()
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_fix(e.h, None, dp(fix), ip(kinds), None, None, None) == STATE and "slam_init" in err()
    e.init(0.0, 0.0, 0.0)
    assert Lb.slam_fix_sense(e.h, dp(fix), ip(kinds), None) == STATE and "slam_set_map" in err()
    assert Lb.slam_fix_run(e.h, None, 0, fp(sim_cmds), 2, None, None, None, None) == STATE
    e.set_map(lm)
    assert Lb.slam_fix_run(e.h, None, 2, None, 2, None, None, None, None) == STATE and "path" in err()
    e.run_sim(sim_cmds)
    e.track_instance(2)
    assert Lb.slam_fix(e.h, None, dp(fix), ip(kinds), None, None, None) == STATE and "slam_track_instance" in err()
    e.track_instance(-1)
    before = _raw(e, tmp_path)
    s = e.fix_sense()                                                # no sensor rows: nothing is emitted, nothing is written
    assert not s["kinds"].any() and not s["fix"].any()
    r = e.fix(s["fix"], s["kinds"])
    assert not r["verdict"].any() and not r["rec"].any() and np.isnan(r["nis"]).all() and _raw(e, tmp_path) == before
    e.close()
