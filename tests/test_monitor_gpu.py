"""The run monitor on the MI355X (slam_monitor_now / slam_monitor_run): per-instance values against tests/monitor_reference.py evaluated at
the device's own state and against slam_consistency, records against the per-instance values, and the promises of the header - a
monitored run moves state, truth, error sums, RNG and controller exactly as the unmonitored run, slam_monitor_now moves nothing, and
records and series do not depend on the chunking.

err_pos and err_yaw are compared bit for bit, flags and NaN patterns exactly, nees_pose by consistency_reference.judge per pool of at
least 30 instances (bar = min(10 G, 4)), counts and maxima of a record exactly and each of its sums within B 2^-53 relative."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import consistency_reference as R
import monitor_reference as MR
from batch_state import describe, differing_instances
from conftest import ROOT
from test_cholesky_highprec import spd_with_condition
from test_consistency_gpu import _crafted_batch, _instance, _load

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _scenario(L, T, seed=321):
    from live_ekf_slam_amd.scenario import make_scenario
    return make_scenario(seed + L, L, T)


def _ekf(S, B, L, dt=None, seed=11, lm=None):
    f = S.BatchedEKF(B, L, dtype=S.F64 if dt is None else dt).readParams()
    f.set_seed(seed)
    if lm is not None:
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
    return f


def _same(fa, fb, what):
    d = differing_instances(fa, fb)
    assert not d, f"{what}: {describe(d)}"


def _bits_equal(a, b, what):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    diff = (a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))      # (a NaN is a NaN, whatever its payload)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} values differ in bits, first at {np.argwhere(diff)[0].tolist()}"


def _judge(pools, label):
    """every instance is judged: kinds with fewer than 30 instances share the pool 'other'"""
    merged = {}
    for name, pool in pools.items():
        merged.setdefault(name if len(pool) >= 30 else "other", []).extend(pool)
    bad = []
    for name in sorted(merged):
        pool = merged[name]
        G, gd, bar, over = R.judge(pool)
        print(f"[monitor] {label} pool {name!r}: {len(pool)} instances, G = {G:.3g}, device max g = {gd:.3g}, bar = {bar:.3g}")
        if over:
            bad.append((name, len(over), gd, bar))
    assert not bad, f"{label}: pools above their bar (name, instances over, device max g, bar): {bad}"


def _against_reference(f, m, kinds, pools, label):
    """per-instance outputs m of the monitor against the helper at the device's own state (get_state, truth, status)"""
    truth, status = f.truth(), f.status()
    wrong = []
    for b in range(f.batch):
        st = f.get_state(b)
        r = MR.instance(st["x"][:3], st["P"][:3, :3], truth[b], int(status[b]))
        same = (m["flags"][b] == r["flags"] and np.float64(m["err_pos"][b]).tobytes() == np.float64(r["err_pos"]).tobytes()
                and np.float64(m["err_yaw"][b]).tobytes() == np.float64(r["err_yaw"]).tobytes()
                and bool(np.isnan(m["nees_pose"][b])) == bool(np.isnan(r["nees_pose"])))
        if not same:
            wrong.append((b, kinds[b], int(m["flags"][b]), r["flags"], m["err_pos"][b], r["err_pos"], m["err_yaw"][b], r["err_yaw"]))
        elif r["z"] is not None:
            pools.setdefault(kinds[b], []).append((m["nees_pose"][b], r["nees_pose"], r["S"], r["e"], r["z"]))
    assert not wrong, f"{label}: {len(wrong)} instance(s) differ from the reference: {wrong[:10]}"


def _check_record(rec, m, M, L_max, B, what, flags=None, **full):
    fl = m["flags"] if flags is None else flags
    MR.assert_record(rec, MR.record(m["err_pos"], m["err_yaw"], m["nees_pose"], fl, np.clip(M, 0, L_max), **full), B, what)


# ---- 1. slam_monitor_now against slam_consistency and the reference, crafted states -------------------------------------------------------
@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", [20, 50])
def test_now_on_crafted_states(S, L_max, dtype32, tmp_path):
    B = 300
    # (two matrices per size and family at L_max = 20, so that a family's pool has 42 instances; 51 at L_max = 50)
    lm, insts, edges = _crafted_batch(L_max, dtype32, 9000 + L_max, range(L_max + 1), per=2 if L_max == 20 else 1)
    rng = np.random.default_rng(9100 + L_max)
    while len(insts) < B:      # fill up with plain matrices at random sizes
        M = int(rng.integers(0, L_max + 1))
        insts.append(_instance(rng, spd_with_condition(rng, 3 + 2 * M, 1e2), M, lm, dtype32, "k1e2"))
    insts = insts[:B]
    kinds = [it["kind"] for it in insts]
    f = _load(S, L_max, S.F32 if dtype32 else S.F64, insts, lm, tmp_path)
    m = f.monitor_now()
    c = f.consistency()
    keep = MR.POSE_NOT_PD | MR.INSTANCE_FAILED
    assert np.array_equal(m["flags"], c["flags"] & keep), np.flatnonzero(m["flags"] != (c["flags"] & keep))
    assert np.array_equal(np.isnan(m["nees_pose"]), np.isnan(c["nees_pose"]))
    _bits_equal(m["nees_pose"], c["nees_pose"], "nees_pose against slam_consistency's")   # the same operations in the same order
    assert (m["flags"] & MR.POSE_NOT_PD).any() and (m["flags"] & MR.INSTANCE_FAILED).any() and (m["flags"] == 0).sum() > B - 10
    pools = {}
    label = f"now, crafted L_max={L_max} {'f32' if dtype32 else 'f64'}"
    _against_reference(f, m, kinds, pools, label)
    _judge(pools, label)
    _check_record(m["rec"], m, f.landmark_counts(), L_max, B, label)
    assert m["rec"][MR.N_OK] + m["rec"][MR.N_FAILED] == B and not m["rec"][13:].any()
    f.close()


# ---- 2. slam_monitor_now changes nothing ------------------------------------------------------------------------------------------------
def test_now_moves_nothing(S, tmp_path):
    L, T, B = 20, 40, 37
    lm, cmds = _scenario(L, T)
    a, b = _ekf(S, B, L, lm=lm), _ekf(S, B, L, lm=lm)
    a.run_sim(cmds[:20]); b.run_sim(cmds[:20])
    before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
    a.save_state(before)
    m1 = a.monitor_now()
    m2 = a.monitor_now(dict(full_every=1))
    a.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_monitor_now"
    for k in ("err_pos", "err_yaw", "nees_pose"):
        _bits_equal(m1[k], m2[k], f"second call, {k}")
    assert np.array_equal(m1["flags"], m2["flags"])
    _bits_equal(m1["rec"][:13], m2["rec"][:13], "second call, record")
    assert m2["rec"][MR.N_FULL] == B and not m1["rec"][13:].any()
    _same(a, b, "after slam_monitor_now")
    # inside a queued stretch the call runs the queue first, and the steps after it are those of the twin
    a.set_lazy_steps(16); b.set_lazy_steps(16)
    for t in range(20, 30):
        a.update_sim(cmds[t]); b.update_sim(cmds[t])
    a.monitor_now()
    a.run_sim(cmds[30:]); b.run_sim(cmds[30:])
    _same(a, b, "steps after slam_monitor_now")
    assert np.array_equal(a.k_histogram(), b.k_histogram())
    a.close(); b.close()


# ---- 3. a monitored run against a twin stepped and read tick by tick --------------------------------------------------------------------
@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
def test_run_against_a_tick_wise_twin(S, dtype32):
    L, T, B = 20, 60, 300
    dt = S.F32 if dtype32 else S.F64
    lm, cmds = _scenario(L, T)
    a, b, u = (_ekf(S, B, L, dt, lm=lm) for _ in range(3))
    res = a.monitor_run(cmds, series=True)
    assert res.recs.shape == (T, 16) and res.err_pos.shape == (T, B) and a.timestep == T
    judged = (0, 1, 7, 29, 59)
    pools = {}
    label = f"run {'f32' if dtype32 else 'f64'}"
    for t in range(T):
        b.update_sim(cmds[t])
        c = b.consistency()
        pos, yaw = MR.errors(b.poses(), b.truth(), b.status())
        _bits_equal(res.err_pos[t], pos, f"{label} tick {t} err_pos")
        _bits_equal(res.err_yaw[t], yaw, f"{label} tick {t} err_yaw")
        _bits_equal(res.nees_pose[t], c["nees_pose"], f"{label} tick {t} nees_pose against the twin's slam_consistency")
        m = dict(err_pos=res.err_pos[t], err_yaw=res.err_yaw[t], nees_pose=res.nees_pose[t], flags=MR.flags_from(res.nees_pose[t], res.err_pos[t]))
        assert np.array_equal(m["flags"], c["flags"] & (MR.POSE_NOT_PD | MR.INSTANCE_FAILED))
        if t in judged:
            _against_reference(b, m, ["run"] * B, pools, f"{label} tick {t}")
        _check_record(res.recs[t], m, b.landmark_counts(), L, B, f"{label} tick {t}")
    assert len(pools["run"]) == len(judged) * B
    _judge(pools, label)
    assert not res.recs[:, 13:].any() and np.all(res.recs[:, MR.N_OK] == B)
    u.run_sim(cmds)
    _same(a, b, f"{label}: monitored run against the tick-wise twin")
    _same(a, u, f"{label}: monitored run against slam_run_sim")
    assert np.array_equal(a.k_histogram(), u.k_histogram())
    # the mean of an instance's err_pos series is its slam_error_stats
    mean, stats = res.err_pos.sum(axis=0) / T, a.error_stats()
    assert np.all(np.abs(mean - stats) <= (T + 2) * 2.0 ** -53 * stats), np.max(np.abs(mean - stats) / stats)
    mon_ms, total_ms = a.last_monitor_work()
    assert mon_ms == -1.0 and total_ms > 0.0
    for f in (a, b, u):
        f.close()


# ---- 4. the other command sources ---------------------------------------------------------------------------------------------------------
def test_source_each_against_run_sim_each(S):
    L, T, B = 20, 30, 64
    lm, cmds = _scenario(L, T)
    rng = np.random.default_rng(4)
    maps = lm[None] + rng.normal(0.0, 0.3, (B, L, 2))
    starts = rng.uniform(-0.05, 0.05, (B, 3)).astype(np.float32)
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)

    def handle():
        f = _ekf(S, B, L)
        f.set_map(maps); f.init(starts, truth0=starts.astype(np.float64))
        return f
    a, b = handle(), handle()
    res = a.monitor_run(each, series=True)
    b.run_sim(each)
    _same(a, b, "source EACH against slam_run_sim_each")
    m = b.monitor_now()
    for k in ("err_pos", "err_yaw", "nees_pose"):
        _bits_equal(getattr(res, k)[-1], m[k], f"last tick of the series against slam_monitor_now, {k}")
    _bits_equal(res.recs[-1], m["rec"], "last record against slam_monitor_now")
    pos, yaw = MR.errors(b.poses(), b.truth(), b.status())
    _bits_equal(m["err_pos"], pos, "err_pos"); _bits_equal(m["err_yaw"], yaw, "err_yaw")
    assert len({v.tobytes() for v in res.err_pos.T}) == B      # every instance runs its own scenario
    a.close(); b.close()


def test_source_nav_against_nav_run(S):
    L, T, B = 20, 40, 64
    lm, _ = _scenario(L, T)
    # half of the batch has its one waypoint 0.3 m ahead and finishes within a few ticks, the other half is under way to the end
    paths = [np.array([[0.3, 0.0]]) if b % 2 == 0 else np.array([[3.0, 0.5], [5.0, -1.0]]) for b in range(B)]
    a, b = _ekf(S, B, L, lm=lm), _ekf(S, B, L, lm=lm)
    a.set_paths(paths); b.set_paths(paths)
    res = a.monitor_run(T=T, series=True)
    cmds = b.run_nav(T, return_cmds=True)
    _same(a, b, "source NAV against slam_nav_run")
    sa, sb = a.nav_state(), b.nav_state()
    for k in sa:
        assert sa[k].tobytes() == sb[k].tobytes(), k
    assert (sa["finish_tick"] >= 0).any() and (sa["finish_tick"] < 0).any() and cmds.any()
    m = b.monitor_now()
    _bits_equal(res.err_pos[-1], m["err_pos"], "last tick of the series against slam_monitor_now")
    _bits_equal(res.recs[-1], m["rec"], "last record against slam_monitor_now")
    # a second call continues the run: the controller ticks go on counting
    a.monitor_run(T=5); b.run_nav(5)
    _same(a, b, "second NAV call")
    assert a.nav_state()["finish_tick"].tobytes() == b.nav_state()["finish_tick"].tobytes()
    a.close(); b.close()


# ---- 5. the UKF kinds --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["ukf_slam", "ukf_loc"])
def test_ukf_kinds(S, kind):
    L, T, B = 20, 30, 64
    lm, cmds = _scenario(L, T)

    def handle():
        f = (S.BatchedUKF(B, L) if kind == "ukf_slam" else S.BatchedUKFLoc(B)).readParams()
        f.set_seed(11); f.set_map(lm); f.init(0.0, 0.0, 0.0)
        return f
    a, b, u = handle(), handle(), handle()
    with pytest.raises(S.SlamError, match="full_every"):
        a.monitor_run(cmds, cfg=dict(full_every=1))
    with pytest.raises(S.SlamError, match="full_every"):
        a.monitor_now(dict(full_every=1))
    from live_ekf_slam_amd import _lib
    assert _lib.lib().slam_monitor_now(a.h, C.byref(S.MonitorConfig(0.1, 9.0, 1)), None, None, None, None, None) == UNSUPPORTED
    res = a.monitor_run(cmds, series=True)
    for t in range(T):
        b.update_sim(cmds[t])
        x = np.stack([b.get_state(i)["x"][:4] for i in range(B)])
        pos, yaw = MR.errors(x, b.truth(), b.status(), ukf=True)
        _bits_equal(res.err_pos[t], pos, f"{kind} tick {t} err_pos")
        _bits_equal(res.err_yaw[t], yaw, f"{kind} tick {t} err_yaw")
        m = dict(err_pos=res.err_pos[t], err_yaw=res.err_yaw[t], nees_pose=res.nees_pose[t], flags=MR.flags_from(res.nees_pose[t], res.err_pos[t], ukf=True))
        _check_record(res.recs[t], m, b.landmark_counts(), a.L_max, B, f"{kind} tick {t}")
    assert np.isnan(res.nees_pose).all() and not res.recs[:, MR.N_NEES].any() and not res.recs[:, MR.N_POSE_NOT_PD].any()
    assert not res.recs[:, MR.SUM_NEES].any() and np.all(res.recs[:, MR.N_OK] == B) and np.isfinite(res.err_pos).all()
    u.run_sim(cmds)
    _same(a, b, f"{kind}: monitored run against the tick-wise twin")
    _same(a, u, f"{kind}: monitored run against slam_run_sim")
    mean, stats = res.err_pos.sum(axis=0) / T, a.error_stats()
    assert np.all(np.abs(mean - stats) <= (T + 2) * 2.0 ** -53 * stats), np.max(np.abs(mean - stats) / stats)
    for f in (a, b, u):
        f.close()


# ---- 6. the full evaluation at a stride ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L,B", [(20, 300), (60, 40)], ids=["L20", "L60_workspace"])
def test_full_evaluation_every_7th_tick(S, L, B, monkeypatch):
    T = 30
    lm, cmds = _scenario(L, T)
    if L > 50:   # the workspace class, three instances per chunk
        monkeypatch.setenv("SLAM_CONSISTENCY_WS_BYTES", str(3 * 8 * (3 + 2 * L + 1) * (3 + 2 * L + 2) // 2))
    a, b = _ekf(S, B, L, lm=lm), _ekf(S, B, L, lm=lm)
    res = a.monitor_run(cmds, cfg=dict(full_every=7))
    assert res.err_pos is None
    full_ticks = [t for t in range(T) if (t + 1) % 7 == 0]
    assert full_ticks == [6, 13, 20, 27]
    for t in range(T):
        b.update_sim(cmds[t])
        if t not in full_ticks:
            assert not res.recs[t, 13:].any(), t
            continue
        c = b.consistency()
        fin = np.isfinite(c["nees_full"])
        assert fin.sum() > 0 and res.recs[t, MR.N_FULL] == fin.sum() and res.recs[t, MR.SUM_DOF] == c["dof"][fin].sum(), t
        ref = c["nees_full"][fin].sum()
        assert ref > 0 and abs(res.recs[t, MR.SUM_FULL] - ref) <= B * 2.0 ** -53 * ref, (t, res.recs[t, MR.SUM_FULL], ref)
        m = b.monitor_now(dict(full_every=7))
        _bits_equal(res.recs[t], m["rec"], f"tick {t}: the run's record against slam_monitor_now with the full evaluation")
    _same(a, b, "run with full evaluations against the twin")
    a.close(); b.close()


# ---- 7. the edges of the reduction --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_reduction_at_block_edges(S, B):
    L, T = 20, 12
    lm, cmds = _scenario(L, T)
    f = _ekf(S, B, L, lm=lm)
    res = f.monitor_run(cmds, series=True)
    m = f.monitor_now()
    _check_record(m["rec"], m, f.landmark_counts(), L, B, f"B={B}")
    _bits_equal(res.recs[-1], m["rec"], f"B={B}: run against now")
    assert m["rec"][MR.N_OK] == B and m["rec"][MR.N_NEES] == B and m["rec"][MR.MAX_POS] == m["err_pos"].max()
    f.close()


@pytest.mark.parametrize("case", ["first_block_failed", "nothing_countable"])
def test_reduction_with_failed_instances(S, case, tmp_path):
    L_max = 20
    B = 300 if case == "first_block_failed" else 257
    rng = np.random.default_rng(77)
    lm = rng.uniform(-8.0, 8.0, (L_max, 2))
    insts = []
    for b in range(B):
        failed = b < 256 or case == "nothing_countable"
        status = 0 if not failed else (R.NONFINITE if b % 2 else R.WATCHDOG)
        insts.append(_instance(rng, spd_with_condition(rng, 5, 1e2), 1, lm, False, "plain", status=status))
    f = _load(S, L_max, S.F64, insts, lm, tmp_path)
    m = f.monitor_now()
    n_failed = 256 if case == "first_block_failed" else B
    assert m["rec"][MR.N_FAILED] == n_failed and m["rec"][MR.N_OK] == B - n_failed
    assert np.isnan(m["err_pos"][:n_failed]).all() and np.all(m["flags"][:n_failed] == MR.INSTANCE_FAILED)
    _check_record(m["rec"], m, f.landmark_counts(), L_max, B, case)
    if case == "nothing_countable":
        assert not m["rec"][2:].any() and np.isfinite(m["rec"]).all(), m["rec"]      # maxima 0 and sums 0, not NaN
    else:
        assert m["rec"][MR.MAX_POS] == m["err_pos"][256:].max() > 0 and m["rec"][MR.N_NEES] == B - 256 and m["rec"][MR.SUM_M] == B - 256
    f.close()


# ---- 8. chunking ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("source", ["shared", "each"])
def test_chunking_changes_nothing(S, source, monkeypatch):
    L, T, B = 20, 10, 64
    lm, cmds = _scenario(L, T)
    if source == "each":
        cmds = (cmds[:, None, :] * np.linspace(0.5, 1.0, B)[None, :, None]).astype(np.float32)
    per_tick = 3 * 8 * B + (8 * B if source == "each" else 0)
    runs = {}
    for name, budget in (("unchunked", None), ("chunks", 3 * per_tick + 7), ("one_byte", 1)):
        if budget is None:
            monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        else:
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        f = _ekf(S, B, L, lm=lm)
        runs[name] = (f, f.monitor_run(cmds, series=True, cfg=dict(full_every=4)))
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    assert -(-T // 3) >= 3        # three ticks per chunk: four chunks
    ref = runs["unchunked"][1]
    assert ref.recs[3, MR.N_FULL] == B and ref.recs[7, MR.N_FULL] == B and not ref.recs[4, 13:].any()
    for name in ("chunks", "one_byte"):
        got = runs[name][1]
        for k in ("recs", "err_pos", "err_yaw", "nees_pose"):
            _bits_equal(getattr(got, k), getattr(ref, k), f"{source}/{name}: {k}")
        _same(runs[name][0], runs["unchunked"][0], f"{source}/{name}")
    # records alone, and a subset of the series
    g = _ekf(S, B, L, lm=lm)
    from live_ekf_slam_amd import _lib
    recs, yaw = np.zeros((T, 16)), np.zeros((T, B))
    c32 = np.ascontiguousarray(cmds, dtype=np.float32)
    assert _lib.lib().slam_monitor_run(g.h, C.byref(S.MonitorConfig(MR.NEES_LO, MR.NEES_HI, 4)), 1 if source == "each" else 0, c32.ctypes.data_as(_lib._fp), T,
                                       recs.ctypes.data_as(_lib._dp), None, yaw.ctypes.data_as(_lib._dp), None) == OK
    _bits_equal(recs, ref.recs, "records with one series"); _bits_equal(yaw, ref.err_yaw, "err_yaw alone")
    g.close()
    for f, _ in runs.values():
        f.close()


def test_chunking_changes_nothing_source_nav(S, monkeypatch):
    """The closed loop in chunks: the controller's commands stay on the device, so a tick holds its rows of the series alone."""
    L, T, B = 20, 7, 8
    lm, _ = _scenario(L, T)
    path = np.array([[3.0, 0.5], [5.0, -1.0]])
    runs = {}
    for name, budget in (("unchunked", None), ("chunks", 3 * (3 * 8 * B) + 7), ("one_byte", 1)):
        if budget is None:
            monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        else:
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        f = _ekf(S, B, L, lm=lm)
        f.set_path(path)
        runs[name] = (f, f.monitor_run(T=T, series=True))
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    plain = _ekf(S, B, L, lm=lm)
    plain.set_path(path)
    assert plain.run_nav(T, return_cmds=True).any()
    ref_f, ref = runs["unchunked"]
    _same(ref_f, plain, "monitored against plain closed loop")
    for name in ("chunks", "one_byte"):
        f, got = runs[name]
        for k in ("recs", "err_pos", "err_yaw", "nees_pose"):
            _bits_equal(getattr(got, k), getattr(ref, k), f"nav/{name}: {k}")
        _same(f, ref_f, f"nav/{name}")
        _same(f, plain, f"nav/{name} against slam_nav_run")
        sa, sb = f.nav_state(), ref_f.nav_state()
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes() == plain.nav_state()[k].tobytes(), (name, k)
    for f, _ in runs.values():
        f.close()
    plain.close()


# ---- 9. errors that need a device ---------------------------------------------------------------------------------------------------------
def test_error_codes(S):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    L, T = 20, 4
    lm, cmds = _scenario(L, T)
    c32 = np.ascontiguousarray(cmds, dtype=np.float32)

    def run(f, source=0, T=T, cfg=None, with_cmds=True):
        return Lb.slam_monitor_run(f.h, None if cfg is None else C.byref(cfg), source, c32.ctypes.data_as(_lib._fp) if with_cmds else None, T, None, None, None, None)

    def now(f, cfg=None):
        return Lb.slam_monitor_now(f.h, None if cfg is None else C.byref(cfg), None, None, None, None, None)

    f = S.BatchedEKF(8, L).readParams()
    assert run(f) == STATE and "slam_init" in Lb.slam_last_error().decode()          # before slam_init
    assert now(f) == STATE and Lb.slam_last_monitor_work(f.h, None, None) == STATE
    f.init(0.0, 0.0, 0.0)
    assert run(f) == STATE and "map" in Lb.slam_last_error().decode()                # without a map
    assert now(f) == STATE
    f.set_map(lm)
    assert run(f, source=2, with_cmds=False) == STATE and "path" in Lb.slam_last_error().decode()   # NAV without a path
    assert run(f, source=5) == ARG and run(f, T=-1) == ARG and run(f, with_cmds=False) == ARG
    assert run(f, cfg=S.MonitorConfig(2.0, 1.0, 0)) == ARG and now(f, S.MonitorConfig(0.1, 9.0, -1)) == ARG
    f.track_instance(2)
    assert run(f) == STATE and "slam_track_instance" in Lb.slam_last_error().decode()
    assert now(f) == OK                                                               # (a snapshot answers for the batch, as slam_consistency)
    f.track_instance(-1)
    assert run(f, T=0) == OK and f.get_state(0)["timestep"] == 0
    assert run(f) == OK and f.get_state(0)["timestep"] == T and now(f) == OK          # the handle is usable after every refusal
    g = _ekf(S, 8, L, seed=2025, lm=lm)
    g.run_sim(cmds)
    _same(f, g, "a handle that was refused five times")
    f.set_nav_timing(True)
    assert run(f) == OK
    mon_ms, total_ms = f.last_monitor_work()
    assert 0.0 < mon_ms < total_ms
    f.close(); g.close()
    # while a prediction stage is pending (UKF): refused before anything moves
    u = S.BatchedUKF(8, L).readParams(); u.set_map(lm); u.init(0.0, 0.0, 0.0)
    assert run(u) == OK
    before = u.get_state(3)
    u.predictionStage((0.05, 0.01))
    assert run(u) == STATE and "prediction stage" in Lb.slam_last_error().decode()
    u.updateStage()
    assert run(u) == OK and u.get_state(3)["timestep"] == before["timestep"] + 1 + T
    u.close()


# ---- 10. the mirrors ----------------------------------------------------------------------------------------------------------------------
def test_cpp_mirror_equals_the_python_mirror(S, tmp_path):
    from live_ekf_slam_amd.scenario import make_scenario
    B, L, T = 8, 10, 30
    dump = str(tmp_path / "monitor.bin")
    out = subprocess.run([os.path.join(ROOT, "live_ekf_slam_amd", "filter_driver"), "monitor", str(B), str(L), str(T), dump],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "driver ok: monitor" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    assert int(np.frombuffer(raw[:8], dtype=np.int64)[0]) == B and len(raw) == 8 + 8 * (16 * T + 3 * T * B) + 8 * (16 + 3 * B) + 4 * B
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_map(lm)
    res = f.monitor_run(cmds, series=True, cfg=dict(full_every=7))
    m = f.monitor_now()
    mine = b"".join(np.ascontiguousarray(a).tobytes() for a in (res.recs, res.err_pos, res.err_yaw, res.nees_pose, m["rec"], m["err_pos"], m["err_yaw"],
                                                               m["nees_pose"], m["flags"]))
    assert raw[8:] == mine and res.recs[6, MR.N_FULL] == B and np.isfinite(res.nees_pose).all()
    f.close()
