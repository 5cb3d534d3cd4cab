"""The chi-square gate on the MI355X (slam_gate_dev, slam_step_gated*, slam_gate_run): every output of every instance against the host hook
(the kernel's own per-instance function compiled for the host) evaluated at the device's own state IN BITS, the record against the
fixed-order sum of the hook's per-instance records in bits, and the promises of the header: the gate changes nothing, a gated step is
byte for byte the plain step on the host-filtered message (also as slam_gate_dev + slam_step_each_dev, also in place), a gate run is its
tick-wise loop whatever the chunking, an infinite gate is the plain step, and the unsupported kinds are refused with the state untouched.

Batch 257: it crosses a 256-instance reduction block and leaves a workgroup of four instances partly filled."""
import ctypes as C

import numpy as np
import pytest

import gate_reference as GR
import innovation_reference as IR
from record_tree import MAX_ENTRY_8, fixed_order_record

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4
B = 257
KS = IR.MAX_DET + 2
SENTINEL = 7.0


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
        self.hip, self.ptrs = hip, []

    def put(self, a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert self.hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
        self.ptrs.append(p)
        assert self.hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0   # hipMemcpyHostToDevice
        return p.value

    def get(self, ptr, like):
        out = np.empty_like(like)
        assert self.hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), out.nbytes, 2) == 0   # hipMemcpyDeviceToHost
        return out

    def close(self):
        for p in self.ptrs:
            self.hip.hipFree(p)


def _config(S):
    """Filter noise at the scale of the crafted detections (gate_reference): with the reference configuration S >= 1 and no spike is seen."""
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.W_00 = cfg.W_11 = 2.5e-3
    cfg.V_00 = cfg.V_11 = 1e-4
    return cfg


def _scenario(L, T, seed=321):
    from live_ekf_slam_amd.scenario import make_scenario
    return make_scenario(seed + L, L, T)


def _handle(S, L_max, dt, cfg, lm, cmds, rows=None, maps=None, freeze=True):
    """A handle after a short simulated run, with a few instances frozen by a message that repeats an id it inserts."""
    f = S.BatchedEKF(B, L_max, dtype=dt).readParams(cfg)
    f.set_seed(11)
    if maps is not None:
        f.set_map(maps)
    else:
        f.set_map(lm)
    f.init(0.0, 0.0, 0.0)
    if rows is not None:
        f.set_noise(rows)
    f.run_sim(cmds)
    if freeze:
        meas = np.zeros((B, 2, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b in range(5, B, 60):
            meas[b] = [[900.0, 2.0, 0.1], [900.0, 2.0, 0.1]]; cnt[b] = 2
        f.update((0.0, 0.0), meas, cnt)
    return f


def _messages(f, L_max, seed):
    """The crafted shapes of the issue spread over the instances, built from each instance's own estimate."""
    rng = np.random.default_rng(seed)
    det, sp = IR.detection, GR.spiked
    msgs = []
    for b in range(f.batch):
        st = f.get_state(b)
        M = st["M"]
        lm = (lambda j: det(rng, st, j % M))
        shape = b % 14
        if M == 0 or shape == 0:
            m = [] if shape % 2 == 0 else [det(rng, st, new_id=700)]
        elif shape == 1:
            m = [lm(0)]
        elif shape == 2:
            m = [sp(lm(1))]
        elif shape == 3:
            m = [sp(lm(0)), lm(1), lm(2)]
        elif shape == 4:
            m = [lm(0), lm(1), sp(lm(2))]
        elif shape == 5:
            m = [sp(lm(2)), sp(lm(0)), sp(lm(1))]
        elif shape == 6:
            m = [sp(lm(1)), lm(1)]
        elif shape == 7:      # insertions, then capacity skips once the map is full, between updates (where the message has room for them)
            fill = min(L_max - M + 2, IR.MAX_DET - 4)
            m = [sp(lm(0)), lm(1)] + [det(rng, st, new_id=700 + i) for i in range(fill)] + [sp(lm(2)), lm(0)]
        elif shape == 8:
            m = [sp(lm(l % 8)) if l % 5 == 2 else lm(l % 8) for l in range(IR.MAX_DET)]
        elif shape == 9:
            m = [sp(lm(l % 8)) if l % 5 == 2 else lm(l % 8) for l in range(IR.MAX_DET + 1)]
        elif shape == 10:
            m = [sp(lm(0)), det(rng, st, new_id=800), det(rng, st, new_id=800)]
        elif shape == 11 and M > IR.MAX_LM:
            m = [sp(lm(j)) if j == 3 else lm(j) for j in range(IR.MAX_LM + 1)]
        else:
            m = [sp(lm(int(j))) if rng.random() < 0.4 else lm(int(j)) for j in rng.integers(0, M, int(rng.integers(1, 6)))]
        msgs.append(m)
    meas = np.full((f.batch, KS, 3), SENTINEL, dtype=np.float32); cnt = np.zeros(f.batch, dtype=np.int32)
    for b, m in enumerate(msgs):
        m = np.asarray(m, dtype=np.float32).reshape(-1, 3)
        meas[b, :m.shape[0]] = m; cnt[b] = m.shape[0]
    return meas, cnt


def _hooks(S, f, cmds, meas, cnt, cfg, rows, gate=GR.GATE):
    """The host hook on every instance at the device's own state."""
    status = f.status()
    f32 = f.dtype == S.F32
    out = []
    for b in range(f.batch):
        st = f.get_state(b)
        noise = IR.effective_noise(cfg) if rows is None else rows[b]
        out.append(S.gate_instance_host(st["x"], st["P"], st["ids"], f.L_max, int(status[b]), cmds[b], meas[b], noise,
                                        lm_from_pred=bool(cfg.ekf_landmark_from_x_pred), f32_storage=f32, cfg=GR.gate_cfg(gate),
                                        count=int(cnt[b]), k_stride=meas.shape[1]))
    return out


def _same_bits(a, b):
    a, b = np.ravel(np.asarray(a, dtype=np.float64)), np.ravel(np.asarray(b, dtype=np.float64))
    return not ((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))).any()


def _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, what):
    wrong = []
    for b, h in enumerate(hooks):
        cin = min(max(int(cnt[b]), 0), meas.shape[1])
        want = h["meas_out"].copy(); want[cin:] = meas_out[b, cin:]          # (from count_in up the kernel writes nothing)
        same = (h["flags"] == r["flags"][b] and h["n_upd"] == r["n_upd"][b] and h["n_new"] == r["n_new"][b] and h["n_rej"] == r["n_rej"][b]
                and h["count_out"] == count_out[b] and np.array_equal(h["verdict"], r["verdict"][b]) and want.tobytes() == meas_out[b].tobytes())
        for k in ("nis_sum", "post", "det"):
            same = same and _same_bits(h[k], r[k][b])
        if not same:
            wrong.append((b, int(r["flags"][b]), h["flags"], int(r["n_rej"][b]), h["n_rej"], int(count_out[b]), h["count_out"]))
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the host hook (b, flags dev/host, n_rej dev/host, count_out dev/host): {wrong[:10]}"
    rec = fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8)
    assert _same_bits(rec, r["rec"]), (what, "the record against the fixed-order sum of the hook's records", rec, r["rec"])


CLASSES = [(20, False, False), (20, True, False), (50, False, False), (50, True, False), (60, True, False), (20, False, True)]
CLASS_IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L60_f32_streamed", "L20_f64_noise_rows_and_maps"]


# ---- 1. - 4. the device against the host hook, nothing moves, and the gated step against the plain step on the filtered message ------------
@pytest.mark.parametrize("L_max,dtype32,each", CLASSES, ids=CLASS_IDS)
def test_gate_against_the_hook_and_the_gated_step_against_the_plain_step(S, hip, tmp_path, L_max, dtype32, each):
    L, T = min(L_max, 50), 30
    lm, sim_cmds = _scenario(L, T)
    cfg = _config(S)
    dt = S.F32 if dtype32 else S.F64
    rng = np.random.default_rng(50 + L_max)
    rows = maps = None
    if each:           # per-instance noise rows and per-instance maps
        W = rng.uniform(1.5e-3, 5e-3, B)
        rows = S.config.noise_rows(cfg, B, W_00=W, W_11=W[::-1].copy(), V_00=rng.uniform(5e-5, 2e-4, B))
        maps = np.repeat(lm[None], B, axis=0) + rng.uniform(-0.3, 0.3, (B, 1, 2))

    def handle():
        return _handle(S, L_max, dt, cfg, lm, sim_cmds, rows, maps)
    a = handle()
    what = CLASS_IDS[CLASSES.index((L_max, dtype32, each))]
    meas, cnt = _messages(a, L_max, 60 + L_max)
    cmds = np.stack([rng.uniform(0.0, 0.02, B), rng.uniform(-0.01, 0.01, B)], axis=1).astype(np.float32)
    hooks = _hooks(S, a, cmds, meas, cnt, cfg, rows)
    dev = _Dev(hip)
    d_cmds, d_meas, d_cnt = dev.put(cmds), dev.put(meas), dev.put(cnt)
    d_mo, d_co = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))

    # 1. every output against the hook; 2. nothing moves
    before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
    a.save_state(before)
    r = a.gate_dev(d_cmds, d_meas, d_cnt, KS, d_mo, d_co)
    a.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_gate_dev"
    meas_out, count_out = dev.get(d_mo, meas), dev.get(d_co, cnt)
    assert dev.get(d_meas, meas).tobytes() == meas.tobytes() and dev.get(d_cnt, cnt).tobytes() == cnt.tobytes(), "the input message was written"
    _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, what)
    seen = set(int(v) for v in r["flags"])
    assert {0, IR.FROZEN, IR.WOULD_FREEZE, IR.TOO_LONG} <= seen, seen
    assert r["rec"][15] == r["n_rej"].sum() > B // 4 and (r["verdict"] == GR.ACCEPTED).sum() > B // 2 and r["rec"][6] > 0
    # the host form gives the same
    rh = a.gate(cmds, meas, cnt)
    for k in ("rec", "nis_sum", "post", "det"):
        assert _same_bits(rh[k], r[k]), (what, "slam_gate against slam_gate_dev", k)
    assert np.array_equal(rh["verdict"], r["verdict"]) and np.array_equal(rh["count_out"], count_out)
    cin = np.clip(cnt, 0, KS)
    assert all(rh["meas_out"][b, :cin[b]].tobytes() == meas_out[b, :cin[b]].tobytes() and rh["meas_out"][b, cin[b]:].tobytes() == meas[b, cin[b]:].tobytes()
               for b in range(B)), (what, "the host form's output message")

    # 3. the gated step against twins stepped plainly
    host_meas = np.stack([h["meas_out"] for h in hooks]); host_cnt = np.array([h["count_out"] for h in hooks], dtype=np.int32)
    ckpt = {}

    def saved(f, name):
        p = tmp_path / f"{name}.ckpt"
        f.save_state(p)
        ckpt[name] = open(p, "rb").read()
        p.unlink()
    s = a.step_gated_dev(d_cmds, d_meas, d_cnt, KS)
    assert np.array_equal(s["n_rej"], r["n_rej"]) and _same_bits(s["rec"], r["rec"]), what
    saved(a, "gated"); a.close()
    t1 = handle()
    t1.update_dev_each(d_cmds, dev.put(host_meas), dev.put(host_cnt), KS)
    saved(t1, "plain on the host-filtered message"); t1.close()
    t2 = handle()
    d_mo2, d_co2 = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))
    t2.gate_dev(d_cmds, d_meas, d_cnt, KS, d_mo2, d_co2, det=False)
    t2.update_dev_each(d_cmds, d_mo2, d_co2, KS)
    saved(t2, "slam_gate_dev, then the plain step on its output"); t2.close()
    t3 = handle()
    d_mi, d_ci = dev.put(meas), dev.put(cnt)
    r3 = t3.gate_dev(d_cmds, d_mi, d_ci, KS, d_mi, d_ci, det=False)
    assert np.array_equal(r3["verdict"], r["verdict"]) and _same_bits(r3["rec"], r["rec"])
    inplace = dev.get(d_mi, meas)
    for b in range(B):                                                   # in place: the row beyond count_in keeps the input
        cin = min(max(int(cnt[b]), 0), KS)
        assert inplace[b, :cin].tobytes() == meas_out[b, :cin].tobytes() and inplace[b, cin:].tobytes() == meas[b, cin:].tobytes(), (what, b)
    assert np.array_equal(dev.get(d_ci, cnt), count_out)
    t3.update_dev_each(d_cmds, d_mi, d_ci, KS)
    saved(t3, "in place, then the plain step"); t3.close()
    t4 = handle()
    t4.step_gated(cmds, meas, cnt, stats=False)
    saved(t4, "slam_step_gated_each with host messages"); t4.close()
    for name, raw in ckpt.items():
        assert raw == ckpt["gated"], f"{what}: the checkpoint after `{name}` differs from the one after slam_step_gated_each_dev"
    dev.close()


# ---- 5. slam_gate_run against its tick-wise loop, and chunking ------------------------------------------------------------------------------
def test_gate_run_equals_the_loop_of_gated_steps_whatever_the_chunking(S, tmp_path, monkeypatch):
    L, T0, T = 20, 30, 6
    lm, sim_cmds = _scenario(L, T0 + T)
    cfg = _config(S)
    src = _handle(S, L, S.F64, cfg, lm, sim_cmds[:T0], freeze=False)
    src.last_meas(L)
    log_meas, log_cnt = np.zeros((T, B, L, 3), np.float32), np.zeros((T, B), np.int32)
    rng = np.random.default_rng(12)
    for t in range(T):                                # a recorded log: the messages of a simulated run, one detection in five spiked
        src.update_sim(sim_cmds[T0 + t]); log_meas[t], log_cnt[t] = src.last_meas(L)
    src.close()
    valid = np.arange(L)[None, None, :] < log_cnt[:, :, None]
    log_meas[~valid] = 0.0                            # (the dump leaves the slots beyond the count as they were)
    spikes = valid & (rng.random((T, B, L)) < 0.2)
    log_meas[:, :, :, 1] += np.where(spikes, np.float32(GR.SPIKE), np.float32(0.0))
    cmds = np.ascontiguousarray(sim_cmds[T0:], dtype=np.float32)
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)

    def saved(f):
        p = tmp_path / "run.ckpt"
        f.save_state(p)
        raw = open(p, "rb").read()
        p.unlink()
        return raw
    for c in (cmds, each):
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a = _handle(S, L, S.F64, cfg, lm, sim_cmds[:T0], freeze=False)
        res = a.gate_run(c, log_meas, log_cnt, series=True)
        assert res.recs.shape == (T, 16) and res.n_rej.shape == (T, B) and a.timestep == T0 + T
        assert res.recs[:, 15].sum() == res.n_rej.sum() > B // 4 and res.recs[:, 5].sum() > B
        loop = _handle(S, L, S.F64, cfg, lm, sim_cmds[:T0], freeze=False)
        for t in range(T):
            g = loop.gate(c[t], log_meas[t], log_cnt[t], det=False)
            s = loop.step_gated(c[t], log_meas[t], log_cnt[t])
            assert _same_bits(s["rec"], res.recs[t]) and np.array_equal(s["n_rej"], res.n_rej[t]), t
            assert _same_bits(g["rec"], res.recs[t]) and _same_bits(g["nis_sum"], res.nis_sum[t]), t
            assert np.array_equal(g["n_upd"], res.n_upd[t]) and np.array_equal(g["flags"], res.flags[t]), t
        final = saved(a)
        assert saved(loop) == final, "the checkpoint after slam_gate_run differs from the loop of slam_step_gated"
        loop.close()
        for budget in (1, 2 * (12 * L * B + 24 * B) + 7):           # one tick per chunk, and a chunk that does not divide T
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
            k = _handle(S, L, S.F64, cfg, lm, sim_cmds[:T0], freeze=False)
            got = k.gate_run(c, log_meas, log_cnt, series=True)
            assert _same_bits(got.recs, res.recs) and _same_bits(got.nis_sum, res.nis_sum), budget
            assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in ("n_upd", "n_rej", "flags")), budget
            assert saved(k) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
            k.close()
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a.set_nav_timing(True)
        a.gate_run(c[:2], log_meas[:2], log_cnt[:2])
        gate_ms, total_ms = a.last_gate_work()
        assert 0.0 < gate_ms < total_ms
        a.close()


def test_runs_of_every_kind_interleaved_on_one_handle(S):
    """monitor_run, gate_run, innovation_run (LOG), run_nav and monitor_run (NAV) one after the other on ONE handle - they share the
    driver of the per-tick runs, its event pool and the staging buffers of messages and commands - against a second handle that is given
    the same inputs through plain calls: run_sim, gate() + update on the filtered message, innovation() + update, and the host route of the
    closed loop.  Per-tick timing goes on before the third run, so the event pool grows between runs."""
    from batch_state import describe, differing_instances
    from test_nav_gpu import _host_controller, _same_nav_state
    L, Bn = 20, 8
    lm, cmds = _scenario(L, 9)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = _config(S)
    path = lm[:3].copy()

    def handle():
        f = S.BatchedEKF(Bn, L).readParams(cfg)
        f.set_seed(11); f.set_map(lm); f.init(0.0, 0.0, 0.0)
        return f
    src = handle()                                    # the log: the messages the simulator generates at ticks 3 .. 8, one in five spiked
    src.run_sim(cmds[:3]); src.last_meas(L)
    log_meas, log_cnt = np.zeros((6, Bn, L, 3), np.float32), np.zeros((6, Bn), np.int32)
    for t in range(6):
        src.update_sim(cmds[3 + t]); log_meas[t], log_cnt[t] = src.last_meas(L)
    src.close()
    valid = np.arange(L)[None, None, :] < log_cnt[:, :, None]
    log_meas[~valid] = 0.0
    log_meas[:, :, :, 1] += np.where(valid & (np.random.default_rng(3).random((6, Bn, L)) < 0.2), np.float32(GR.SPIKE), np.float32(0.0))

    a, b = handle(), handle()
    a.set_path(path)
    pp = _host_controller(b, path, dict(method=0, control=0))

    def same(what):
        d = differing_instances(a, b)
        assert not d, f"after {what}: {describe(d)}"
    # 1. a monitored run / run_sim
    mon = a.monitor_run(cmds[:3])
    b.run_sim(cmds[:3])
    assert _same_bits(mon.recs[-1], b.monitor_now()["rec"])
    same("monitor_run")
    # 2. a gated run of the log / gate() and update() on the message it returned
    gr = a.gate_run(cmds[3:6], log_meas[:3], log_cnt[:3], series=True)
    for t in range(3):
        g = b.gate(cmds[3 + t], log_meas[t], log_cnt[t], det=False)
        b.update(cmds[3 + t], g["meas_out"], g["count_out"])
        assert _same_bits(g["rec"], gr.recs[t]) and _same_bits(g["nis_sum"], gr.nis_sum[t]) and np.array_equal(g["n_rej"], gr.n_rej[t]), t
    assert gr.n_rej.sum() > 0 and gr.recs[:, 5].sum() > 0
    same("gate_run")
    gate_ms, total_ms = a.last_gate_work()
    assert gate_ms == -1.0 and total_ms > 0.0          # per-tick timing was off
    # 3. an innovation run of the log / innovation() and update()
    a.set_nav_timing(True)
    ir = a.innovation_run(cmds[6:9], meas=log_meas[3:], meas_count=log_cnt[3:], series=True)
    for t in range(3):
        r = b.innovation(cmds[6 + t], log_meas[3 + t], log_cnt[3 + t], det=False)
        b.update(cmds[6 + t], log_meas[3 + t], log_cnt[3 + t])
        assert _same_bits(r["rec"], ir.recs[t]) and _same_bits(r["nis_sum"], ir.nis_sum[t]) and np.array_equal(r["n_upd"], ir.n_upd[t]), t
    same("innovation_run")
    part, total = a.last_innovation_work()
    assert 0.0 < part < total
    assert a.last_gate_work() == (gate_ms, total_ms)   # every kind of run keeps its own times
    # 4. the closed loop / the host route
    nav_cmds = a.run_nav(3, return_cmds=True)
    for t in range(3):
        c = pp.next_cmds(b.nav_estimates(), (b.status() & 4) != 0)
        assert np.array_equal(c.view(np.uint32), nav_cmds[t].view(np.uint32)), t
        b.run_sim(c[None])
    same("run_nav")
    part, total = a.last_nav_work()
    assert 0.0 < part < total
    # 5. the monitored closed loop / the host route
    mon = a.monitor_run(T=2)
    for t in range(2):
        c = pp.next_cmds(b.nav_estimates(), (b.status() & 4) != 0)
        b.run_sim(c[None])
        assert _same_bits(mon.recs[t], b.monitor_now()["rec"]), t
    same("monitor_run, source NAV")
    part, total = a.last_monitor_work()
    assert 0.0 < part < total
    _same_nav_state(a.nav_state(), dict(remaining=pp.remaining, finish_tick=pp.finish_tick, integ=pp.integ, err_prev=pp.err_prev), "device vs host")
    assert a.timestep == 14 and a.get_state(0)["timestep"] == 14 and nav_cmds.any()
    a.close(); b.close()


# ---- 6. an infinite gate is the plain step ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
def test_an_infinite_gate_is_the_plain_step(S, tmp_path, dtype32):
    L, T = 20, 30
    lm, sim_cmds = _scenario(L, T)
    cfg = _config(S)
    dt = S.F32 if dtype32 else S.F64
    a, p = (_handle(S, L, dt, cfg, lm, sim_cmds) for _ in range(2))
    meas, cnt = _messages(a, L, 70)
    cmd = np.array([0.015, -0.004], dtype=np.float32)
    s = a.step_gated(cmd, meas, cnt, cfg=dict(gate=float("inf")))
    p.update(cmd, meas, cnt)
    assert not s["n_rej"].any() and s["rec"][15] == 0.0 and s["rec"][5] > B
    fa, fp = tmp_path / "a.ckpt", tmp_path / "p.ckpt"
    a.save_state(fa); p.save_state(fp)
    assert open(fa, "rb").read() == open(fp, "rb").read(), "a gated step with gate = +inf differs from the plain step"
    a.close(); p.close()


# ---- 7. the kinds the gate does not cover -------------------------------------------------------------------------------------------------
def test_unsupported_kinds_are_refused_and_keep_their_state(S, tmp_path):
    from live_ekf_slam_amd import _lib
    Lb = _lib.lib()
    L, T = 20, 10
    lm, sim_cmds = _scenario(L, T)
    n = 8
    cmd = np.array([0.05, 0.01], np.float32); meas = np.zeros((n, 2, 3), np.float32); cnt = np.zeros(n, np.int32)
    mo, co = np.zeros_like(meas), np.zeros_like(cnt)
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    err = (lambda: Lb.slam_last_error().decode())
    cfg = S.default_config(); cfg.landmark_id_is_known = 0
    unknown = S.BatchedEKF(n, L).readParams(cfg)
    handles = [(unknown, "landmark_id_is_known"), (S.BatchedUKF(n, L).readParams(), "sigma points"), (S.BatchedUKFLoc(n).readParams(), "sigma points")]
    for f, word in handles:
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
        f.run_sim(sim_cmds)
        before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
        f.save_state(before)
        assert Lb.slam_gate(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None, None, None, None, None, None, fp(mo), ip(co), None, None) == UNSUPPORTED
        assert word in err()
        assert Lb.slam_step_gated(f.h, None, fp(cmd), fp(meas), ip(cnt), 2, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_gate_run(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_last_gate_work(f.h, None, None) == STATE
        f.save_state(after)
        assert open(before, "rb").read() == open(after, "rb").read(), word
        f.close()
    # errors that need a handle: overlapping device buffers, the states a gated step refuses
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_step_gated(e.h, None, fp(cmd), fp(meas), ip(cnt), 2, None, None) == STATE and "slam_init" in err()
    e.set_map(lm); e.init(0.0, 0.0, 0.0)
    buf = np.zeros(n * 2 * 3 + 8, np.float32)          # (host memory: the call is refused before any of it is read)
    base = buf.ctypes.data
    rc = Lb.slam_gate_dev(e.h, None, C.c_void_p(cmd.ctypes.data), 0, C.c_void_p(base), C.c_void_p(cnt.ctypes.data), 2, None, None, None, None, None,
                          None, None, C.c_void_p(base + 16), C.c_void_p(co.ctypes.data), None, None)
    assert rc == ARG and "overlaps" in err()
    e.track_instance(2)
    assert Lb.slam_step_gated(e.h, None, fp(cmd), fp(meas), ip(cnt), 2, None, None) == STATE and "slam_track_instance" in err()
    e.track_instance(-1)
    assert Lb.slam_step_gated(e.h, None, fp(cmd), fp(meas), ip(cnt), 2, None, None) == OK and e.get_state(0)["timestep"] == 1
    e.close()
