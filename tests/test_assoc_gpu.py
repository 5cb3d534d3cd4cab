"""Association of detections without ids on the MI355X (slam_associate*, slam_step_associated*, slam_associate_run): every output of every
instance against the host hook (the kernel's own per-instance function compiled for the host) evaluated at the device's own state IN
BITS, the record against the fixed-order join of the hook's per-instance records, and the promises of the header: the association changes
nothing, an associated step is byte for byte the plain known-id step on the hook-labelled message, an associated run is its tick-wise
loop whatever the chunking, slam_associate_dev followed by slam_step_gated_dev on the same device buffers equals the host-side chain, and
the unsupported kinds are refused with their state untouched.

Batch 257: one instance past a 256-instance reduction workgroup, and a workgroup of four instances partly filled.  k_stride = 66 with
sentinels behind count_in.  The states are reached by stepping crafted messages WITH ids (insertions on the grid of assoc_reference, then
updates) and one step with per-instance commands and noise, so every instance differs."""
import ctypes as C

import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR
from record_tree import MAX_ENTRY_8, fixed_order_record
from test_gate_gpu import _Dev, _same_bits

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4
B = 257
KS = IR.MAX_DET + 2
SENTINEL = 7.0
POSE = (0.3, -0.2, 0.4)


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


def _config(S):
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.W_00 = cfg.W_11 = 2.5e-3
    cfg.V_00 = cfg.V_11 = 1e-4
    return cfg


def _grid(M):
    j = np.arange(M)
    return 1.5 + 1.0 * (j // 5), -1.0 + 0.5 * (j % 5)


def _handle(S, L_max, M, dt, cfg, rows=None, maps=None, freeze=True, seed=5):
    """M landmarks inserted on the grid under the ids 100 + j by messages with ids, four rounds of updates, the last with
    per-instance commands, all with per-instance detection noise; a few instances frozen by a message that repeats an id it inserts."""
    f = S.BatchedEKF(B, L_max, dtype=dt).readParams(cfg)
    f.set_seed(11)
    if maps is not None:
        f.set_map(maps)
    f.init(*POSE)
    if rows is not None:
        f.set_noise(rows)
    rng = np.random.default_rng(seed)
    rr, bb = _grid(M)
    ids = 100.0 + np.arange(M)
    for lo in range(0, M, 40):          # insertions
        hi = min(lo + 40, M)
        m = np.stack([ids[lo:hi], rr[lo:hi], bb[lo:hi]], axis=1).astype(np.float32)
        f.update((0.0, 0.0), np.repeat(m[None], B, axis=0), np.full(B, hi - lo, np.int32))
    for rnd in range(4):                # updates of every landmark, 40 at a time; the last round with per-instance commands
        for lo in range(0, M, 40):
            hi = min(lo + 40, M)
            m = np.zeros((B, hi - lo, 3), np.float32)
            m[:, :, 0] = ids[lo:hi]
            m[:, :, 1] = rr[lo:hi] + 0.02 * rng.standard_normal((B, hi - lo))
            m[:, :, 2] = bb[lo:hi] + 0.02 * rng.standard_normal((B, hi - lo))
            cmd = (0.0, 0.0)
            if rnd == 3 and lo == 0:
                cmd = np.stack([rng.uniform(0.0, 0.03, B), rng.uniform(-0.01, 0.01, B)], axis=1).astype(np.float32)
            f.update(cmd, m, np.full(B, hi - lo, np.int32))
    if freeze and M < L_max:
        meas = np.zeros((B, 2, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b in range(5, B, 60):
            meas[b] = [[900.0, 2.0, 0.1], [900.0, 2.0, 0.1]]; cnt[b] = 2
        f.update((0.0, 0.0), meas, cnt)
    return f


def _messages(f, seed):
    """The crafted shapes of the issue spread over the instances, built from each instance's own estimate; the id column holds garbage."""
    rng = np.random.default_rng(seed)
    garbage = [float("nan"), -7.0, 1e30, 3.5, float("inf")]
    msgs, counts = [], []
    for b in range(f.batch):
        st = f.get_state(b)
        M = st["M"]
        cl = (lambda j, dr=0.0: AR.clean(rng, st, int(j) % M, garbage[(b + int(j)) % 5], dr))
        shape = b % 12
        count = None
        if shape == 0:
            m = []
        elif shape == 1:
            m = [cl(j) for j in rng.permutation(M)[:IR.MAX_DET]]
        elif shape == 2:
            m = [cl(0), AR.fresh(2), cl(3), AR.fresh(M - 1), cl(1)]
        elif shape == 3:
            twice = cl(4)
            m = [cl(2), twice, cl(2), twice, cl(0)]
        elif shape == 4:
            m = [cl(0), [0.0, float("nan"), 0.1], cl(1)]
        elif shape == 5:
            m = [cl(l) for l in range(IR.MAX_DET + 1)]
        elif shape == 6:
            m = [cl(0), cl(4, 0.3), cl(7, -0.25), cl(2, 0.15)]
        elif shape == 7:
            m = [AR.fresh(c) for c in (1, 3, 6, 8, 11)] + [cl(1)]
        elif shape == 8:
            m = [cl(l) for l in range(3)]; count = KS + 4            # a count beyond the row: clamped to 66 > 64 detections
        elif shape == 9:
            m = [cl(1)]; count = -2
        else:
            m = [cl(j) if rng.random() < 0.6 else AR.fresh(int(j)) for j in rng.integers(0, M, int(rng.integers(1, 9)))]
        msgs.append(m); counts.append(len(m) if count is None else count)
    meas = np.full((f.batch, KS, 3), SENTINEL, dtype=np.float32)
    for b, m in enumerate(msgs):
        m = np.asarray(m, dtype=np.float32).reshape(-1, 3)
        meas[b, :m.shape[0]] = m
    return meas, np.asarray(counts, dtype=np.int32)


def _hooks(S, f, cmds, meas, cnt, cfg, rows, acfg=None):
    status = f.status()
    f32 = f.dtype == S.F32
    out = []
    for b in range(f.batch):
        st = f.get_state(b)
        noise = IR.effective_noise(cfg) if rows is None else rows[b]
        out.append(S.associate_instance_host(st["x"], st["P"], st["ids"], f.L_max, int(status[b]), cmds[b], meas[b], noise, f32_storage=f32,
                                             cfg=acfg, count=int(cnt[b]), k_stride=meas.shape[1]))
    return out


def _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, what):
    wrong = []
    for b, h in enumerate(hooks):
        cin = min(max(int(cnt[b]), 0), meas.shape[1])
        want = h["meas_out"].copy(); want[cin:] = meas_out[b, cin:]          # (from count_in up the kernel writes nothing)
        same = (h["flags"] == r["flags"][b] and h["n_match"] == r["n_match"][b] and h["n_new"] == r["n_new"][b] and h["n_drop"] == r["n_drop"][b]
                and h["count_out"] == count_out[b] and np.array_equal(h["verdict"], r["verdict"][b]) and np.array_equal(h["slot"], r["slot"][b])
                and want.tobytes() == meas_out[b].tobytes() and _same_bits(h["det"], r["det"][b]))
        if not same:
            wrong.append((b, int(r["flags"][b]), h["flags"], int(r["n_match"][b]), h["n_match"], int(count_out[b]), h["count_out"]))
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the host hook (b, flags dev/host, n_match dev/host, count_out dev/host): {wrong[:10]}"
    rec = fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8)
    assert _same_bits(rec, r["rec"]), (what, "the record against the fixed-order join of the hook's records", rec, r["rec"])


# (L_max, landmarks, fp32 storage, noise rows and per-instance maps)
CLASSES = [(20, 18, False, False), (20, 18, True, False), (50, 48, False, False), (50, 48, True, False), (70, 66, True, False),
           (70, 66, False, False), (20, 18, False, True)]
CLASS_IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L70_M66_f32_streamed", "L70_M66_f64_streamed", "L20_f64_noise_rows_and_maps"]


# ---- 1. - 3. and 5.: the device against the hook, nothing moves, the associated step against the plain step, the chain with the gate -------
@pytest.mark.parametrize("L_max,M,dtype32,each", CLASSES, ids=CLASS_IDS)
def test_associate_against_the_hook_and_the_associated_step_against_the_plain_step(S, hip, tmp_path, L_max, M, dtype32, each):
    cfg = _config(S)
    dt = S.F32 if dtype32 else S.F64
    rng = np.random.default_rng(50 + L_max)
    rows = maps = None
    if each:           # per-instance noise rows and per-instance maps
        W = rng.uniform(1.5e-3, 5e-3, B)
        rows = S.config.noise_rows(cfg, B, W_00=W, W_11=W[::-1].copy(), V_00=rng.uniform(5e-5, 2e-4, B))
        maps = rng.uniform(-3.0, 3.0, (B, 6, 2))

    def handle():
        return _handle(S, L_max, M, dt, cfg, rows, maps)
    a = handle()
    what = CLASS_IDS[CLASSES.index((L_max, M, dtype32, each))]
    assert a.get_state(0)["M"] == M and a.get_state(B - 1)["M"] == M
    meas, cnt = _messages(a, 60 + L_max)
    cmds = np.stack([rng.uniform(0.0, 0.02, B), rng.uniform(-0.01, 0.01, B)], axis=1).astype(np.float32)
    hooks = _hooks(S, a, cmds, meas, cnt, cfg, rows)
    dev = _Dev(hip)
    d_cmds, d_meas, d_cnt = dev.put(cmds), dev.put(meas), dev.put(cnt)
    d_mo, d_co = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))

    # 1. every output against the hook; 2. nothing moves
    before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
    a.save_state(before)
    r = a.associate_dev(d_cmds, d_meas, d_cnt, KS, d_mo, d_co)
    a.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_associate_dev"
    meas_out, count_out = dev.get(d_mo, meas), dev.get(d_co, cnt)
    assert dev.get(d_meas, meas).tobytes() == meas.tobytes() and dev.get(d_cnt, cnt).tobytes() == cnt.tobytes(), "the input message was written"
    _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, what)
    cin = np.clip(cnt, 0, KS)
    assert all((meas_out[b, cin[b]:] == SENTINEL).all() for b in range(B)), "something was written from count_in up"
    assert {0, IR.FROZEN, IR.TOO_LONG} <= set(int(v) for v in r["flags"])
    assert set(np.unique(r["verdict"]).tolist()) == set(range(7)), np.unique(r["verdict"])
    assert r["rec"][4] == r["n_match"].sum() > B and r["rec"][5] == r["n_new"].sum() > 0 and r["rec"][3] > 2 * B
    by, lines, _, _ = a.last_associate_work()
    model = AR.model_work([a.get_state(b)["M"] for b in range(B)], r["n_match"] + r["n_new"] + r["n_drop"], r["flags"], 4 if dtype32 else 8)
    print(f"{what}: slam_last_associate_work (bytes, lines) = {(by, lines)}, the model in Python integers = {model}")
    assert 0 < by and 0 < lines and (by, lines) == model, (what, "the traffic model summed on the device against its restatement", by, lines, model)
    # the host form gives the same, and changes nothing either
    rh = a.associate(cmds, meas, cnt)
    a.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_associate"
    for k in ("rec", "det"):
        assert _same_bits(rh[k], r[k]), (what, "slam_associate against slam_associate_dev", k)
    for k in ("verdict", "slot", "n_match", "n_new", "n_drop", "flags"):
        assert np.array_equal(rh[k], r[k]), (what, k)
    assert np.array_equal(rh["count_out"], count_out)
    assert all(rh["meas_out"][b, :cin[b]].tobytes() == meas_out[b, :cin[b]].tobytes() and rh["meas_out"][b, cin[b]:].tobytes() == meas[b, cin[b]:].tobytes()
               for b in range(B)), (what, "the host form's output message")

    # 3. the associated step against twins stepped plainly on the hook-labelled message
    host_meas = np.stack([h["meas_out"] for h in hooks]); host_cnt = np.array([h["count_out"] for h in hooks], dtype=np.int32)
    ckpt = {}

    def saved(f, name):
        p = tmp_path / f"{name}.ckpt"
        f.save_state(p)
        ckpt[name] = open(p, "rb").read()
        p.unlink()
    s = a.step_associated_dev(d_cmds, d_meas, d_cnt, KS)
    assert np.array_equal(s["n_drop"], r["n_drop"]) and _same_bits(s["rec"], r["rec"]), what
    assert dev.get(d_meas, meas).tobytes() == meas.tobytes(), "slam_step_associated_dev wrote the caller's message"
    saved(a, "associated"); a.close()
    t1 = handle()
    t1.update(cmds, host_meas, host_cnt)
    saved(t1, "slam_step_each on the hook-labelled message"); t1.close()
    t3 = handle()
    d_mi, d_ci = dev.put(meas), dev.put(cnt)
    r3 = t3.associate_dev(d_cmds, d_mi, d_ci, KS, d_mi, d_ci, det=False)
    assert np.array_equal(r3["verdict"], r["verdict"]) and _same_bits(r3["rec"], r["rec"])
    inplace = dev.get(d_mi, meas)
    for b in range(B):                                                   # in place: the row beyond count_in keeps the input
        assert inplace[b, :cin[b]].tobytes() == meas_out[b, :cin[b]].tobytes() and inplace[b, cin[b]:].tobytes() == meas[b, cin[b]:].tobytes(), (what, b)
    assert np.array_equal(dev.get(d_ci, cnt), count_out)
    t3.update_dev_each(d_cmds, d_mi, d_ci, KS)
    saved(t3, "in place, then the plain step"); t3.close()
    t4 = handle()
    t4.step_associated(cmds, meas, cnt, stats=False)
    saved(t4, "slam_step_associated with host messages"); t4.close()
    for name, raw in ckpt.items():
        assert raw == ckpt["associated"], f"{what}: the checkpoint after `{name}` differs from the one after slam_step_associated_dev"

    # 5. slam_associate_dev, then slam_step_gated_dev on the same device buffers, against the host-side chain
    cmd1 = np.array([0.012, -0.003], dtype=np.float32)
    t5 = handle()
    hooks1 = _hooks(S, t5, np.repeat(cmd1[None], B, axis=0), meas, cnt, cfg, rows)
    lab = np.stack([h["meas_out"] for h in hooks1]); lab_cnt = np.array([h["count_out"] for h in hooks1], dtype=np.int32)
    d_m5, d_c5 = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))
    t5.associate_dev(cmd1, d_meas, d_cnt, KS, d_m5, d_c5, det=False)
    g5 = t5.step_gated_dev(cmd1, d_m5, d_c5, KS)
    saved(t5, "chain on the device"); t5.close()
    t6 = handle()
    g6 = t6.gate(cmd1, lab, lab_cnt, det=False)
    t6.update(cmd1, g6["meas_out"], g6["count_out"])
    saved(t6, "chain on the host"); t6.close()
    assert ckpt["chain on the device"] == ckpt["chain on the host"], what
    assert _same_bits(g5["rec"], g6["rec"]) and np.array_equal(g5["n_rej"], g6["n_rej"]), what
    dev.close()


# ---- 4. slam_associate_run against its tick-wise loop, and chunking ---------------------------------------------------------------------
def test_associate_run_equals_the_loop_of_associated_steps_whatever_the_chunking(S, tmp_path, monkeypatch):
    L_max, M, T = 20, 12, 5
    cfg = _config(S)
    rng = np.random.default_rng(12)
    rr, bb = _grid(L_max)
    log_meas = np.full((T, B, KS, 3), SENTINEL, np.float32); log_cnt = np.zeros((T, B), np.int32)
    for t in range(T):                              # an id-less log: a random subset of the grid's 20 cells, so ticks insert and match
        for b in range(B):
            cells = rng.permutation(L_max)[:int(rng.integers(0, 9))]
            k = cells.shape[0]
            log_meas[t, b, :k, 0] = np.nan
            log_meas[t, b, :k, 1] = rr[cells] + 0.02 * rng.standard_normal(k)
            log_meas[t, b, :k, 2] = bb[cells] + 0.02 * rng.standard_normal(k)
            log_cnt[t, b] = k
    cmds = np.zeros((T, 2), np.float32); cmds[:, 0] = 0.002
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)

    def saved(f):
        p = tmp_path / "run.ckpt"
        f.save_state(p)
        raw = open(p, "rb").read()
        p.unlink()
        return raw
    for c in (cmds, each):
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        res = a.associate_run(c, log_meas, log_cnt, series=True)
        assert res.recs.shape == (T, 16) and res.n_drop.shape == (T, B) and a.timestep == a.get_state(0)["timestep"]
        assert res.recs[:, 4].sum() == res.n_match.sum() > B and res.recs[:, 5].sum() == res.n_new.sum() > B
        loop = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        for t in range(T):
            g = loop.associate(c[t], log_meas[t], log_cnt[t], det=False)
            s = loop.step_associated(c[t], log_meas[t], log_cnt[t])
            assert _same_bits(s["rec"], res.recs[t]) and np.array_equal(s["n_drop"], res.n_drop[t]), t
            assert _same_bits(g["rec"], res.recs[t]) and np.array_equal(g["n_match"], res.n_match[t]), t
            assert np.array_equal(g["n_new"], res.n_new[t]) and np.array_equal(g["flags"], res.flags[t]), t
        final = saved(a)
        assert saved(loop) == final, "the checkpoint after slam_associate_run differs from the loop of slam_step_associated"
        loop.close()
        for budget in (1, 2 * (12 * KS * B + 32 * B) + 7):           # one tick per chunk, and a chunk that does not divide T
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
            k = _handle(S, L_max, M, S.F64, cfg, freeze=False)
            got = k.associate_run(c, log_meas, log_cnt, series=True)
            assert _same_bits(got.recs, res.recs), budget
            assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in ("n_match", "n_new", "n_drop", "flags")), budget
            assert saved(k) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
            k.close()
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a.set_nav_timing(True)
        a.associate_run(c[:2], log_meas[:2], log_cnt[:2])
        by, lines, assoc_ms, total_ms = a.last_associate_work()
        assert 0.0 < assoc_ms < total_ms and 0 < by
        a.close()


# ---- 6. the kinds the association does not cover ----------------------------------------------------------------------------------------
def test_unsupported_kinds_are_refused_and_keep_their_state(S, tmp_path):
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    Lb = _lib.lib()
    L, T = 20, 10
    lm, sim_cmds = make_scenario(341, L, T)
    n = 8
    cmd = np.array([0.05, 0.01], np.float32); meas = np.zeros((n, 2, 3), np.float32); cnt = np.zeros(n, np.int32)
    mo, co = np.zeros_like(meas), np.zeros_like(cnt)
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    vp = (lambda a: C.c_void_p(a.ctypes.data))
    err = (lambda: Lb.slam_last_error().decode())
    cfg = S.default_config(); cfg.landmark_id_is_known = 0
    unknown = S.BatchedEKF(n, L).readParams(cfg)
    handles = [(unknown, "landmark_id_is_known"), (S.BatchedUKF(n, L).readParams(), "sigma points"), (S.BatchedUKFLoc(n).readParams(), "sigma points")]
    for f, word in handles:
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
        f.run_sim(sim_cmds)
        before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
        f.save_state(before)
        assert Lb.slam_associate(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None, None, None, None, None, None, None, fp(mo), ip(co)) == UNSUPPORTED
        assert word in err()
        assert Lb.slam_associate_dev(f.h, None, vp(cmd), 0, vp(meas), vp(cnt), 2, None, None, None, None, None, None, None, None, vp(mo), vp(co)) == UNSUPPORTED
        assert Lb.slam_step_associated(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_step_associated_dev(f.h, None, vp(cmd), 0, vp(meas), vp(cnt), 2, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_associate_run(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_last_associate_work(f.h, None, None, None) == STATE
        f.save_state(after)
        assert open(before, "rb").read() == open(after, "rb").read(), word
        f.close()
    # errors that need a handle: overlapping device buffers, the states an associated step refuses
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_step_associated(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == STATE and "slam_init" in err()
    e.set_map(lm); e.init(0.0, 0.0, 0.0)
    buf = np.zeros(n * 2 * 3 + 8, np.float32)          # (host memory: the call is refused before any of it is read)
    base = buf.ctypes.data
    rc = Lb.slam_associate_dev(e.h, None, vp(cmd), 0, C.c_void_p(base), vp(cnt), 2, None, None, None, None, None, None, None, None,
                               C.c_void_p(base + 16), vp(co))
    assert rc == ARG and "overlaps" in err()
    e.track_instance(2)
    assert Lb.slam_step_associated(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == STATE and "slam_track_instance" in err()
    assert Lb.slam_associate_run(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None) == STATE
    e.track_instance(-1)
    assert Lb.slam_step_associated(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == OK and e.get_state(0)["timestep"] == 1
    e.close()
