"""The innovation statistics on the MI355X (slam_innovation / slam_innovation_run): every output of every instance against the host hook
(the kernel's own per-instance function compiled for the host) evaluated at the device's own state IN BITS, `post` against what the step
itself leaves, and the promises of the header - slam_innovation changes nothing, a run moves state, truth, error sums, RNG and controller
exactly as the plain run, series equal a tick-wise twin's, chunking changes no bit, per-instance noise rows are honoured.

Records: counts and the maximum exactly, each non-negative sum within N 2^-53 relative (N its number of summands), each signed sum within
N 2^-53 sum |summand|."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import innovation_reference as IR
from batch_state import describe, differing_instances
from conftest import ROOT
from test_consistency_gpu import _write

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4
U = 2.0 ** -53


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _scenario(L, T, seed=321):
    from live_ekf_slam_amd.scenario import make_scenario
    return make_scenario(seed + L, L, T)


def _ekf(S, B, L, dt=None, seed=11, lm=None, cfg=None):
    f = S.BatchedEKF(B, L, dtype=S.F64 if dt is None else dt).readParams(cfg)
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


def _pack(msgs, k_stride):
    B = len(msgs)
    meas = np.zeros((B, k_stride, 3), dtype=np.float32); cnt = np.zeros(B, dtype=np.int32)
    for b, m in enumerate(msgs):
        m = np.asarray(m, dtype=np.float32).reshape(-1, 3)
        meas[b, :m.shape[0]] = m; cnt[b] = m.shape[0]
    return meas, cnt


def _against_hook(f, r, cmds, meas, cnt, cfg, rows, what):
    """every per-instance output of the device (dict r of innovation()) against the host hook at the device's own state"""
    status = f.status()
    wrong = []
    for b in range(f.batch):
        st = f.get_state(b)
        noise = IR.effective_noise(cfg) if rows is None else rows[b]
        cmd = cmds[b] if np.ndim(cmds) == 2 else cmds
        h = IR.hook(st, cmd, meas[b, :cnt[b]], cfg, f.L_max, status=int(status[b]), noise=noise)
        same = (h["flags"] == r["flags"][b] and h["n_upd"] == r["n_upd"][b] and h["n_new"] == r["n_new"][b])
        for k in ("nis_sum", "post", "det"):
            a, d = np.ascontiguousarray(h[k], dtype=np.float64).ravel(), np.ascontiguousarray(r[k][b], dtype=np.float64).ravel()
            same = same and not ((a.view(np.uint64) != d.view(np.uint64)) & ~(np.isnan(a) & np.isnan(d))).any()
        if not same:
            wrong.append((b, int(r["flags"][b]), h["flags"], int(r["n_upd"][b]), h["n_upd"], float(r["nis_sum"][b]), h["nis_sum"]))
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the host hook (b, flags dev/host, n_upd dev/host, nis_sum dev/host): {wrong[:10]}"


def _check_record(rec, r, cfg_band, what):
    """a record against the per-instance outputs it was reduced from"""
    flags, det = r["flags"], r["det"]
    ev = (flags & (IR.FROZEN | IR.TOO_LONG | IR.WOULD_FREEZE)) == 0
    nis = det[ev][:, :, 0]; fin = np.isfinite(nis)
    nu_r, nu_b = det[ev][:, :, 1][fin], det[ev][:, :, 2][fin]
    v = nis[fin]
    exact = {0: ev.sum(), 1: ((flags & IR.FROZEN) != 0).sum(), 2: ((flags & IR.TOO_LONG) != 0).sum(), 3: ((flags & IR.WOULD_FREEZE) != 0).sum(),
             4: (ev & ((flags & IR.S_SINGULAR) != 0)).sum(), 5: fin.sum(), 6: r["n_new"][ev].sum(), 8: v.max() if v.size else 0.0,
             9: (v < cfg_band[0]).sum(), 10: (v > cfg_band[1]).sum(), 15: 0.0}
    for i, want in exact.items():
        assert rec[i] == want, (what, i, rec[i], want)
    N = max(int(fin.sum()), 1)
    for i, terms in ((7, v), (13, nu_r * nu_r), (14, nu_b * nu_b)):
        ref = float(np.sum(terms.astype(np.longdouble)))
        assert abs(rec[i] - ref) <= N * U * ref, (what, i, rec[i], ref)
    for i, terms in ((11, nu_r), (12, nu_b)):
        ref = float(np.sum(terms.astype(np.longdouble)))
        assert abs(rec[i] - ref) <= N * U * float(np.abs(terms).sum()), (what, i, rec[i], ref)


def _post_against_the_step(S, f, r, cmds, meas, cnt, what):
    """after slam_innovation, the same handle is stepped with the same arguments: post rounded to storage = the pose and its block; the
    step raises SLAM_INST_S_SINGULAR for exactly the instances whose replay reported a singular S"""
    before = f.status()
    f.update(cmds, meas, cnt)
    status = f.status()
    f32 = f.dtype == S.F32
    n = 0
    for b in range(f.batch):
        fl = int(r["flags"][b])
        if fl & IR.WOULD_FREEZE:
            assert status[b] & IR.INST_INDEX_OOR, (what, b)
        if fl & (IR.WOULD_FREEZE | IR.FROZEN | IR.TOO_LONG):
            continue
        assert not status[b] & IR.INST_INDEX_OOR, (what, b)
        assert bool(status[b] & IR.INST_S_SINGULAR) == bool(fl & IR.S_SINGULAR or before[b] & IR.INST_S_SINGULAR), (what, b, int(status[b]), fl)
        st = f.get_state(b)
        _bits_equal(IR.post_as_stored(r["post"][b], f32), IR.oracle_post(st), f"{what}: post of instance {b} against the step")
        n += 1
    return n


def _random_message(rng, st, L_max):
    dets = []
    for _ in range(int(rng.integers(0, 5))):
        if st["M"] > 0 and rng.random() < 0.7:
            dets.append(IR.detection(rng, st, int(rng.integers(0, st["M"]))))
        else:
            dets.append(IR.detection(rng, st, new_id=int(rng.integers(0, 6))))
    return dets


# ---- 1. + 2. device against the host hook, and against the step itself, on loaded states ------------------------------------------------
@pytest.mark.parametrize("L_max,B,dtype32", [(20, 300, False), (20, 300, True), (50, 300, False), (50, 300, True), (201, 8, False)],
                         ids=["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L201_streamed"])
def test_device_equals_the_host_hook_and_the_step(S, L_max, B, dtype32, tmp_path):
    rng = np.random.default_rng(100 + L_max + dtype32)
    cases = IR.crafted_cases(5 + L_max, L_max, dtype32)
    if B < len(cases):
        cases = [c for c in cases if c["name"] in ("one update", "one landmark more", "insertion then a repeat of the new id", "singular S")]
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = S.config.noise_rows(cfg, B)
    insts, msgs = [], []
    where = {int(i * B / len(cases)): c for i, c in enumerate(cases)}     # the crafted messages spread over the batch
    for b in range(B):
        if b in where:
            c = where[b]
            st, m, status = c["st"], c["meas"], c["status"]
            if c["noise"] is not None:
                rows[b] = c["noise"]
        else:
            M = int(rng.integers(0, L_max + 1)) if b % 7 else L_max
            st = IR.synthetic_state(rng, M, dtype32); status = 0
            m = _random_message(rng, st, L_max)
        insts.append(dict(P=st["P"], x=st["x"], M=st["M"], ids=st["ids"], truth=np.zeros(3), status=status))
        msgs.append(m)
    dt = S.F32 if dtype32 else S.F64
    path = tmp_path / "crafted.ckpt"
    _write(S, L_max, dt, insts, path, tmp_path)
    f = S.BatchedEKF(B, L_max, dtype=dt).readParams(cfg)
    f.load_state(path); os.remove(path)
    f.set_noise(rows)
    meas, cnt = _pack(msgs, IR.MAX_DET + 2)
    band = (S.default_innovation_config().nis_lo, S.default_innovation_config().nis_hi)
    what = f"L_max={L_max} {'f32' if dtype32 else 'f64'}"
    each = np.stack([rng.uniform(0.0, 0.1, B), rng.uniform(-0.05, 0.05, B)], axis=1).astype(np.float32)
    for cmds in (each, np.array([0.08, -0.03], dtype=np.float32)):
        r = f.innovation(cmds, meas, cnt)
        _against_hook(f, r, cmds, meas, cnt, cfg, rows, f"{what}, {'cmd_each' if cmds.ndim == 2 else 'shared command'}")
        _check_record(r["rec"], r, band, what)
    seen = set(int(v) for v in r["flags"])
    assert {0, IR.WOULD_FREEZE, IR.TOO_LONG, IR.S_SINGULAR} <= seen and (B < 300 or IR.FROZEN in seen), seen
    assert r["rec"][5] > (B if B >= 300 else 0)
    n = _post_against_the_step(S, f, r, cmds, meas, cnt, what)
    assert n >= B // 2 - 1
    f.close()


def test_states_reached_by_run_sim_against_the_hook_and_the_step(S):
    L, B, T = 20, 300, 45
    lm, cmds = _scenario(L, T)
    cfg = S.default_config()
    f = _ekf(S, B, L, lm=lm)
    f.run_sim(cmds[:T - 1])
    rng = np.random.default_rng(8)
    msgs = []
    for b in range(B):
        st = f.get_state(b)
        msgs.append(_random_message(rng, st, L) + ([IR.detection(rng, st, st["M"] - 1)] if st["M"] else []))
    meas, cnt = _pack(msgs, 6)
    r = f.innovation(cmds[T - 1], meas, cnt)
    _against_hook(f, r, cmds[T - 1], meas, cnt, cfg, None, "after run_sim")
    assert r["rec"][0] + r["rec"][3] == B and r["rec"][0] > 0.8 * B and r["rec"][5] > B and np.all(r["det"][np.isfinite(r["det"][:, :, 0])][:, 0] > 0)
    assert _post_against_the_step(S, f, r, cmds[T - 1], meas, cnt, "after run_sim") == r["rec"][0]
    f.close()


# ---- 3. slam_innovation changes nothing ---------------------------------------------------------------------------------------------------
def test_innovation_moves_nothing(S, tmp_path):
    L, T, B = 20, 40, 37
    lm, cmds = _scenario(L, T)
    a, b = _ekf(S, B, L, lm=lm), _ekf(S, B, L, lm=lm)
    a.run_sim(cmds[:20]); b.run_sim(cmds[:20])
    rng = np.random.default_rng(3)
    meas, cnt = _pack([_random_message(rng, a.get_state(i), L) for i in range(B)], 4)
    before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
    a.save_state(before)
    r1 = a.innovation(cmds[20], meas, cnt)
    r2 = a.innovation(cmds[20], meas, cnt, det=False)
    a.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_innovation"
    for k in ("rec", "nis_sum", "post"):
        _bits_equal(r1[k], r2[k], f"second call, {k}")
    assert np.array_equal(r1["flags"], r2["flags"]) and np.array_equal(r1["n_upd"], r2["n_upd"])
    _same(a, b, "after slam_innovation")
    # inside a queued stretch the call runs the queue first, and the steps after it are those of the twin
    a.set_lazy_steps(16); b.set_lazy_steps(16)
    for t in range(20, 30):
        a.update_sim(cmds[t]); b.update_sim(cmds[t])
    a.innovation(cmds[30], meas, cnt)
    a.run_sim(cmds[30:]); b.run_sim(cmds[30:])
    _same(a, b, "steps after slam_innovation")
    assert np.array_equal(a.k_histogram(), b.k_histogram())
    a.close(); b.close()


# ---- 4. innovation_run SHARED against twins -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
def test_run_shared_against_twins(S, dtype32):
    L, T, B = 20, 60, 300
    dt = S.F32 if dtype32 else S.F64
    lm, cmds = _scenario(L, T)
    a, b, c, u = (_ekf(S, B, L, dt, lm=lm) for _ in range(4))
    b.last_meas(L)                                   # (switches the measurement dump on)
    res = a.innovation_run(cmds, series=True)
    assert res.recs.shape == (T, 16) and res.nis_sum.shape == (T, B) and a.timestep == T
    label = f"run {'f32' if dtype32 else 'f64'}"
    band = (S.default_innovation_config().nis_lo, S.default_innovation_config().nis_hi)
    for t in range(T):
        b.update_sim(cmds[t])
        meas, cnt = b.last_meas(L)
        r = c.innovation(cmds[t], meas, cnt)
        c.update(cmds[t], meas, cnt)
        _bits_equal(res.nis_sum[t], r["nis_sum"], f"{label} tick {t} nis_sum")
        assert np.array_equal(res.n_upd[t], r["n_upd"]) and np.array_equal(res.flags[t], r["flags"]), (label, t)
        _bits_equal(res.recs[t], r["rec"], f"{label} tick {t} record")
        if t in (0, 1, 29, 59):
            _check_record(res.recs[t], r, band, f"{label} tick {t}")
    assert np.all(res.recs[:, 0] == B) and res.recs[-1, 5] > B / 2 and not res.flags.any()
    u.run_sim(cmds)
    _same(a, b, f"{label}: innovation run against the update_sim twin")
    _same(a, u, f"{label}: innovation run against slam_run_sim")
    assert np.array_equal(a.k_histogram(), u.k_histogram())
    for k in ("x", "P"):                             # c saw the same messages through slam_step
        assert a.get_state(B - 1)[k].tobytes() == c.get_state(B - 1)[k].tobytes()
    inn_ms, total_ms = a.last_innovation_work()
    assert inn_ms == -1.0 and total_ms > 0.0
    for f in (a, b, c, u):
        f.close()


# ---- 5. EACH, NAV, LOG and chunking -------------------------------------------------------------------------------------------------------
def _series_equal(got, ref, what):
    _bits_equal(got.recs, ref.recs, f"{what}: recs"); _bits_equal(got.nis_sum, ref.nis_sum, f"{what}: nis_sum")
    assert np.array_equal(got.n_upd, ref.n_upd) and np.array_equal(got.flags, ref.flags), what


@pytest.mark.parametrize("source", ["each", "nav", "log"])
def test_the_other_sources_and_chunking(S, source, monkeypatch):
    L, T, B = 20, 40, 37
    lm, cmds = _scenario(L, T)
    rng = np.random.default_rng(4)
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)
    paths = [np.array([[0.3, 0.0]]) if i % 2 == 0 else np.array([[3.0, 0.5], [5.0, -1.0]]) for i in range(B)]

    def handle():
        f = _ekf(S, B, L, lm=lm)
        if source == "nav":
            f.set_paths(paths)
        return f
    log_meas = log_cnt = None
    if source == "log":                               # a recorded log: the messages of a simulated run
        g = handle(); g.last_meas(L)
        log_meas, log_cnt = np.zeros((T, B, L, 3), np.float32), np.zeros((T, B), np.int32)
        for t in range(T):
            g.update_sim(cmds[t]); log_meas[t], log_cnt[t] = g.last_meas(L)
        g.close()

    def run(f):
        if source == "each":
            return f.innovation_run(each, series=True)
        if source == "nav":
            return f.innovation_run(T=T, series=True)
        return f.innovation_run(cmds, meas=log_meas, meas_count=log_cnt, series=True)
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    a, p, tw = handle(), handle(), handle()
    res = run(a)
    # the plain run of the same inputs
    if source == "each":
        p.run_sim(each)
    elif source == "nav":
        issued = p.run_nav(T, return_cmds=True)
        sa, sp = a.nav_state(), p.nav_state()
        assert all(sa[k].tobytes() == sp[k].tobytes() for k in sa) and (sa["finish_tick"] >= 0).any() and (sa["finish_tick"] < 0).any()
    else:
        for t in range(T):
            p.update(cmds[t], log_meas[t], log_cnt[t])
    _same(a, p, f"source {source} against the plain run")
    # a tick-wise slam_innovation twin: for the simulator sources `tw` steps by update_sim and shows the message of the tick, and `lag`,
    # which starts equal, evaluates that message and is then stepped with it
    tw.last_meas(L)
    lag = None if source == "log" else handle()
    for t in range(T):
        if source == "log":
            cmd, meas, cnt = cmds[t], log_meas[t], log_cnt[t]
            r = tw.innovation(cmd, meas, cnt); tw.update(cmd, meas, cnt)
        else:
            cmd = each[t] if source == "each" else issued[t]
            tw.update_sim(cmd)
            meas, cnt = tw.last_meas(L)
            r = lag.innovation(cmd, meas, cnt); lag.update(cmd, meas, cnt)
        _bits_equal(res.nis_sum[t], r["nis_sum"], f"{source} tick {t} nis_sum")
        assert np.array_equal(res.n_upd[t], r["n_upd"]) and np.array_equal(res.flags[t], r["flags"]), (source, t)
        _bits_equal(res.recs[t], r["rec"], f"{source} tick {t} record")
    assert res.recs[:, 5].sum() > B
    if source != "log":
        lag.close()
    # chunking: one tick's worth, and a budget of one byte
    per_tick = 8 * B + 8 * B + (8 * B if source == "each" else 0) + (12 * L * B + 4 * B if source == "log" else 0)
    for budget in (per_tick, 1, 3 * per_tick + 7):
        monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        c = handle()
        _series_equal(run(c), res, f"{source}, SLAM_MONITOR_LOG_BYTES={budget}")
        _same(c, a, f"{source}, SLAM_MONITOR_LOG_BYTES={budget}")
        c.close()
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    for f in (a, p, tw):
        f.close()


# ---- 6. per-instance noise rows -----------------------------------------------------------------------------------------------------------
def test_noise_rows_against_one_row_handles(S):
    L, T, B, G = 20, 30, 64, 4
    lm, cmds = _scenario(L, T)
    cfg = S.default_config()
    W = np.repeat([0.002, 0.01, 0.05, 0.2], B // G); V = np.repeat([0.0005, 0.001, 0.01, 0.05], B // G)
    a = _ekf(S, B, L, lm=lm)
    a.set_noise(S.config.noise_rows(cfg, B, W_00=W, W_11=W, V_00=V, sim_W_00=0.5 * W))
    res = a.innovation_run(cmds, series=True)
    for g in range(G):
        n = B // G
        c = cfg.copy()
        one = _ekf(S, n, L, lm=lm)
        one.set_instance_offset(g * n)
        one.set_noise(S.config.noise_rows(c, n, W_00=W[g * n], W_11=W[g * n], V_00=V[g * n], sim_W_00=0.5 * W[g * n]))
        ref = one.innovation_run(cmds, series=True)
        sl = slice(g * n, (g + 1) * n)
        _bits_equal(res.nis_sum[:, sl], ref.nis_sum, f"group {g}: nis_sum")
        assert np.array_equal(res.n_upd[:, sl], ref.n_upd) and np.array_equal(res.flags[:, sl], ref.flags), g
        d = differing_instances(one, a, b_offset=g * n)
        assert not d, f"group {g}: {describe(d)}"
        one.close()
    means = [res.nis_sum[:, g * (B // G):(g + 1) * (B // G)].sum() / res.n_upd[:, g * (B // G):(g + 1) * (B // G)].sum() for g in range(G)]
    print("mean NIS per group:", means)
    assert len({round(m, 9) for m in means}) == G     # the rows are honoured: every group has its own statistics
    a.close()


# ---- 7. the edges of the reduction --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 255, 256, 257])
def test_reduction_at_block_edges(S, B):
    L, T = 20, 25
    lm, cmds = _scenario(L, T)
    f = _ekf(S, B, L, lm=lm)
    f.last_meas(L)
    res = f.innovation_run(cmds[:T - 1])
    g = _ekf(S, B, L, lm=lm); g.last_meas(L)
    g.run_sim(cmds[:T - 2]); g.update_sim(cmds[T - 2])
    g2 = _ekf(S, B, L, lm=lm); g2.run_sim(cmds[:T - 2])
    meas, cnt = g.last_meas(L)
    r = g2.innovation(cmds[T - 2], meas, cnt)
    band = (S.default_innovation_config().nis_lo, S.default_innovation_config().nis_hi)
    _check_record(r["rec"], r, band, f"B={B}")
    _bits_equal(res.recs[-1], r["rec"], f"B={B}: run against slam_innovation")
    v = r["det"][:, :, 0][np.isfinite(r["det"][:, :, 0])]
    assert r["rec"][0] == B and r["rec"][8] == (v.max() if v.size else 0.0)
    for h in (f, g, g2):
        h.close()


# ---- 8. errors that need a device, and the C++ mirror -----------------------------------------------------------------------------------
def test_error_codes(S):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    L, T = 20, 4
    lm, cmds = _scenario(L, T)
    c32 = np.ascontiguousarray(cmds, dtype=np.float32)
    meas = np.zeros((8, 2, 3), np.float32); cnt = np.zeros(8, np.int32)

    def run(f, source=0, T=T, cfg=None, with_cmds=True):
        return Lb.slam_innovation_run(f.h, None if cfg is None else C.byref(cfg), source, c32.ctypes.data_as(_lib._fp) if with_cmds else None, None, None,
                                      0, T, None, None, None, None)

    def now(f, cfg=None):
        return Lb.slam_innovation(f.h, None if cfg is None else C.byref(cfg), c32.ctypes.data_as(_lib._fp), 0, meas.ctypes.data_as(_lib._fp),
                                  cnt.ctypes.data_as(_lib._ip), 2, None, None, None, None, None, None, None)
    err = (lambda: Lb.slam_last_error().decode())
    f = S.BatchedEKF(8, L).readParams()
    assert run(f) == STATE and "slam_init" in err()
    assert now(f) == STATE and Lb.slam_last_innovation_work(f.h, None, None) == STATE
    f.init(0.0, 0.0, 0.0)
    assert run(f) == STATE and "map" in err()
    assert now(f) == OK                                                              # (a host-fed message needs no map)
    f.set_map(lm)
    assert run(f, source=2, with_cmds=False) == STATE and "path" in err()
    assert run(f, source=5) == ARG and run(f, T=-1) == ARG and run(f, with_cmds=False) == ARG and run(f, source=3) == ARG
    assert run(f, cfg=S.InnovationConfig(2.0, 1.0)) == ARG and now(f, S.InnovationConfig(float("nan"), 1.0)) == ARG
    f.track_instance(2)
    assert run(f) == STATE and "slam_track_instance" in err()
    assert now(f) == OK
    f.track_instance(-1)
    assert run(f, T=0) == OK and f.get_state(0)["timestep"] == 0
    assert run(f) == OK and f.get_state(0)["timestep"] == T and now(f) == OK          # the handle is usable after every refusal
    g = _ekf(S, 8, L, seed=2025, lm=lm)
    g.run_sim(cmds)
    _same(f, g, "a handle that was refused several times")
    f.set_nav_timing(True)
    assert run(f) == OK
    inn_ms, total_ms = f.last_innovation_work()
    assert 0.0 < inn_ms < total_ms
    f.close(); g.close()
    cfg = S.default_config(); cfg.landmark_id_is_known = 0
    h = _ekf(S, 8, L, lm=lm, cfg=cfg)
    assert run(h) == UNSUPPORTED and "landmark_id_is_known" in err() and now(h) == UNSUPPORTED
    h.close()
    for u in (S.BatchedUKF(8, L).readParams(), S.BatchedUKFLoc(8).readParams()):
        u.set_map(lm); u.init(0.0, 0.0, 0.0)
        assert run(u) == UNSUPPORTED and "sigma points" in err() and now(u) == UNSUPPORTED
        u.close()


@pytest.mark.parametrize("B,L,T,seed", [(8, 20, 45, 341), (8, 10, 30, 1234)], ids=["with_updates", "nothing_mapped"])
def test_cpp_mirror_equals_the_python_mirror(S, tmp_path, B, L, T, seed):
    from live_ekf_slam_amd.scenario import make_scenario
    dump = str(tmp_path / "innovation.bin")
    out = subprocess.run([os.path.join(ROOT, "live_ekf_slam_amd", "filter_driver"), "innovation", str(B), str(L), str(T), dump, str(seed)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "driver ok: innovation" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    lm, cmds = make_scenario(seed, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_map(lm)
    res = f.innovation_run(cmds, series=True)
    meas = np.zeros((B, 2, 3), np.float32); cnt = np.full(B, 2, np.int32)
    for b in range(B):
        st = f.get_state(b)
        meas[b, 0] = (st["ids"][0] if st["M"] else 998.0, 2.0, 0.1); meas[b, 1] = (999.0, 1.5, -0.2)
    r = f.innovation((0.05, 0.01), meas, cnt)
    parts = (("recs", res.recs), ("run nis_sum", res.nis_sum), ("run n_upd", res.n_upd), ("run flags", res.flags), ("rec", r["rec"]),
             ("nis_sum", r["nis_sum"]), ("post", r["post"]), ("det", r["det"]), ("n_upd", r["n_upd"]), ("n_new", r["n_new"]), ("flags", r["flags"]))
    assert int(np.frombuffer(raw[:8], dtype=np.int64)[0]) == B and len(raw) == 8 + sum(a.nbytes for _, a in parts)
    pos = 8
    for name, a in parts:
        theirs = np.frombuffer(raw[pos:pos + a.nbytes], dtype=a.dtype).reshape(a.shape)
        pos += a.nbytes
        if a.dtype == np.float64:
            _bits_equal(theirs, a, f"C++ mirror against the Python mirror: {name}")
        else:
            assert np.array_equal(theirs, a), (name, theirs, a)
    assert res.recs[-1, 0] == B and r["rec"][6] >= B
    if L == 20:
        assert res.recs[:, 5].sum() > B and r["rec"][5] == B
    f.close()
