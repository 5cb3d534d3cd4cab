"""Joint-compatibility association on the MI355X (slam_associate_joint*, slam_step_associated_joint*, slam_associate_joint_run): every
output of every instance against the host hook (the kernel's own per-instance function compiled for the host) evaluated at the device's
own state IN BITS, the record against the fixed-order join of the hook's records, and the promises of the header: the evaluation changes
nothing, a jointly associated step is byte for byte the plain known-id step on the hook-labelled message, a run is its tick-wise loop
whatever the chunking, slam_associate_joint_dev followed by slam_step_gated_dev on the same device buffers equals the host-side chain, and
the unsupported kinds are refused with their state untouched.

The shape of test_assoc_gpu.py, whose handles are used: batch 257, k_stride 66 with sentinels, L_max 20 and 50 in both storage types, the
streamed class with 66 landmarks in both, per-instance noise rows and maps, states reached by real steps.  The messages spread the
crafted cases over the instances (b % 12), each built from the instance's OWN estimate; the pose uncertainty of cases (b) - (d) is widened
through the instance's noise row (V_11 = 0.25: the predicted yaw variance, with W_11 = 1e-4), so the neighbours 0.5 rad apart on the grid's
first ring are inside every individual gate while two innovations that differ by 0.5 rad are jointly impossible:
  0  (a) separated: one candidate per detection, one node per detection      6  AMBIGUOUS (a range offset under the default row)
  1  (f) every landmark, up to 64 detections: 16 matched                      7  new detections beyond the room of the map: NO_ROOM
  2  (b) nearest neighbour takes the neighbour, a second detection pins it    8  a NaN range: INVALID
  3  (c) two detections with the same best slot, both paired                  9  65 detections: TOO_LONG
  4  (d) two detections for one slot: one is left JOINT_UNPAIRED             10  a count beyond the row
  5  (g) V_11 = 2^100: the yaw swamps every bearing row, the joint S of      11  k = 0 / a negative count
         two pairings is exactly singular: JOINT_S_SINGULAR                  (frozen instances: b = 5, 65, ...)
Case (e): every class is evaluated a second time with max_nodes = 3.  M = 0 and the in-place form of (h): test_joint_reference.py and
the in-place twin below."""
import ctypes as C

import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR
import joint_reference as JR
import test_assoc_gpu as TA
from test_assoc_gpu import S, hip  # noqa: F401  (fixtures)
from record_tree import MAX_ENTRY_8, fixed_order_record
from test_gate_gpu import _Dev, _same_bits

pytestmark = pytest.mark.gpu

OK, ARG, UNSUPPORTED, STATE = 0, -1, -3, -4
B, KS, SENTINEL = TA.B, TA.KS, TA.SENTINEL
WIDE_SHAPES, SINGULAR_SHAPE, SHIFT = (2, 3, 4), 5, 0.4


def _rows(S, cfg, rng, each):
    """The noise row of every instance: the class's own (random where `each`), widened yaw for (b) - (d), a yaw that swamps for (g)."""
    shape = np.arange(B) % 12
    W0, W1 = np.full(B, cfg.W_00), np.full(B, cfg.W_11)
    V0, V1 = np.full(B, cfg.V_00), np.full(B, cfg.V_11)
    if each:
        W0 = rng.uniform(1.5e-3, 5e-3, B); W1 = W0[::-1].copy(); V0 = rng.uniform(5e-5, 2e-4, B)
    wide = np.isin(shape, WIDE_SHAPES)
    V1[wide] = 0.25; W0[wide] = 1e-2; W1[wide] = 1e-4    # (a loose range: the estimates of one ring differ by centimetres)
    V1[shape == SINGULAR_SHAPE] = 2.0 ** 100
    return S.config.noise_rows(cfg, B, W_00=W0, W_11=W1, V_00=V0, V_11=V1)


def _messages(f, seed):
    """Cases (a) - (h) over the instances, from each instance's own estimate; the id column holds garbage."""
    rng = np.random.default_rng(seed)
    garbage = [float("nan"), -7.0, 1e30, 3.5, float("inf")]
    msgs, counts = [], []
    for b in range(f.batch):
        st = f.get_state(b)
        M = st["M"]
        cl = (lambda j, dr=0.0: TA.AR.clean(rng, st, int(j) % M, garbage[(b + int(j)) % 5], dr))
        at = (lambda j, shift=0.0: JR.seen(st, j, shift))
        shape, count = b % 12, None
        if shape == 0:
            m = [cl(j) for j in rng.permutation(M)[:int(rng.integers(1, 9))]]
        elif shape == 1:
            m = [cl(j) for j in rng.permutation(M)[:IR.MAX_DET]]
        elif shape == 2:
            m = [at(0, SHIFT), at(4, SHIFT)]
        elif shape == 3:
            m = [at(3, SHIFT), at(4, SHIFT)]
        elif shape == 4:
            m = [at(0, SHIFT), at(4, SHIFT), at(3, SHIFT), at(4, SHIFT - 0.5)]
        elif shape == 5:
            m = [at(1), at(7), at(3)]
        elif shape == 6:
            m = [cl(0), cl(4, 0.3), cl(7, -0.25), cl(2, 0.15)]
        elif shape == 7:
            m = [TA.AR.fresh(c) for c in (1, 3, 6, 8, 11)] + [cl(1)]
        elif shape == 8:
            m = [cl(0), [0.0, float("nan"), 0.1], cl(1)]
        elif shape == 9:
            m = [cl(l) for l in range(IR.MAX_DET + 1)]
        elif shape == 10:
            m = [cl(l) for l in range(3)]; count = KS + 4            # a count beyond the row: clamped to 66 > 64 detections
        else:
            m = [cl(1)] if b % 24 == 11 else []; count = -2 if b % 24 == 11 else None
        msgs.append(m); counts.append(len(m) if count is None else count)
    meas = np.full((f.batch, KS, 3), SENTINEL, dtype=np.float32)
    for b, m in enumerate(msgs):
        m = np.asarray(m, dtype=np.float32).reshape(-1, 3)
        meas[b, :m.shape[0]] = m
    return meas, np.asarray(counts, dtype=np.int32)


def _hooks(S, f, cmds, meas, cnt, cfg, rows, jcfg):
    status = f.status()
    f32 = f.dtype == S.F32
    out = []
    for b in range(f.batch):
        st = f.get_state(b)
        noise = IR.effective_noise(cfg) if rows is None else rows[b]
        out.append(S.associate_joint_instance_host(st["x"], st["P"], st["ids"], f.L_max, int(status[b]), cmds[b], meas[b], noise, f32_storage=f32,
                                                   cfg=jcfg, count=int(cnt[b]), k_stride=meas.shape[1]))
    return out


def _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, what):
    wrong = []
    for b, h in enumerate(hooks):
        cin = min(max(int(cnt[b]), 0), meas.shape[1])
        want = h["meas_out"].copy(); want[cin:] = meas_out[b, cin:]          # (from count_in up the kernel writes nothing)
        same = (h["flags"] == r["flags"][b] and h["n_match"] == r["n_match"][b] and h["n_new"] == r["n_new"][b] and h["n_drop"] == r["n_drop"][b]
                and h["count_out"] == count_out[b] and np.array_equal(h["verdict"], r["verdict"][b]) and np.array_equal(h["slot"], r["slot"][b])
                and want.tobytes() == meas_out[b].tobytes() and _same_bits(h["det"], r["det"][b]) and h["nodes"] == r["nodes"][b]
                and np.array_equal(h["ncand"], r["ncand"][b]) and _same_bits(h["d2_joint"], r["d2_joint"][b]))
        if not same:
            wrong.append((b, int(r["flags"][b]), h["flags"], int(r["n_match"][b]), h["n_match"], int(r["nodes"][b]), h["nodes"],
                          float(r["d2_joint"][b]), h["d2_joint"]))
    assert not wrong, (f"{what}: {len(wrong)} instance(s) differ from the host hook (b, flags dev/host, n_match dev/host, nodes dev/host, "
                       f"d2_joint dev/host): {wrong[:8]}")
    rec = fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8)
    assert _same_bits(rec, r["rec"]), (what, "the record against the fixed-order join of the hook's records", rec, r["rec"])


@pytest.mark.parametrize("L_max,M,dtype32,each", TA.CLASSES, ids=TA.CLASS_IDS)
def test_joint_against_the_hook_and_the_joint_step_against_the_plain_step(S, hip, tmp_path, L_max, M, dtype32, each):  # noqa: F811
    cfg = TA._config(S)
    dt = S.F32 if dtype32 else S.F64
    rng = np.random.default_rng(70 + L_max)
    rows0 = maps = None
    if each:
        W = rng.uniform(1.5e-3, 5e-3, B)
        rows0 = S.config.noise_rows(cfg, B, W_00=W, W_11=W[::-1].copy(), V_00=rng.uniform(5e-5, 2e-4, B))
        maps = rng.uniform(-3.0, 3.0, (B, 6, 2))
    rows = _rows(S, cfg, np.random.default_rng(71 + L_max), each)

    def handle():
        f = TA._handle(S, L_max, M, dt, cfg, rows0, maps)       # the states are reached under the class's rows,
        f.set_noise(rows)                                       # the association and the step that follows run under the cases' rows
        return f
    a = handle()
    what = TA.CLASS_IDS[TA.CLASSES.index((L_max, M, dtype32, each))]
    meas, cnt = _messages(a, 80 + L_max)
    shape = np.arange(B) % 12
    live = a.status() == 0
    cmds = np.stack([rng.uniform(0.0, 0.02, B), rng.uniform(-0.01, 0.01, B)], axis=1).astype(np.float32)
    cmds[np.isin(shape, WIDE_SHAPES + (SINGULAR_SHAPE,))] = 0.0        # (the crafted innovations are those of the pose as it stands)
    dev = _Dev(hip)
    d_cmds, d_meas, d_cnt = dev.put(cmds), dev.put(meas), dev.put(cnt)
    before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
    a.save_state(before)
    cin = np.clip(cnt, 0, KS)
    seen_verdicts, seen_flags = set(), set()
    for name, jcfg in (("a budget of 3 nodes", JR.joint_cfg(max_nodes=3)), ("default", JR.joint_cfg())):
        hooks = _hooks(S, a, cmds, meas, cnt, cfg, rows, jcfg)
        d_mo, d_co = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))
        r = a.associate_joint(d_cmds, d_meas, (d_cnt, KS), cfg=jcfg, dev_out=(d_mo, d_co))
        a.save_state(after)
        assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_associate_joint_dev"
        meas_out, count_out = dev.get(d_mo, meas), dev.get(d_co, cnt)
        assert dev.get(d_meas, meas).tobytes() == meas.tobytes() and dev.get(d_cnt, cnt).tobytes() == cnt.tobytes(), "the input message was written"
        _check_against_hooks(r, hooks, meas_out, count_out, meas, cnt, f"{what}, {name}")
        assert all((meas_out[b, cin[b]:] == SENTINEL).all() for b in range(B)), "something was written from count_in up"
        assert r["rec"][4] == r["n_match"].sum() > B and r["rec"][12] == r["nodes"].sum() and r["n_match"].max() <= 16
        seen_verdicts |= set(np.unique(r["verdict"]).tolist()); seen_flags |= set(int(v) for v in r["flags"])
        # the traffic model: the association's, plus four elements of P and one 128-byte line per on-demand block; the block count is
        # not exposed, so both sums must leave the association's model by one and the same whole number of blocks
        by, lines, _, _ = a.last_joint_work()
        esz = 4 if dtype32 else 8
        m_by, m_lines = AR.model_work([a.get_state(b)["M"] for b in range(B)], r["n_match"] + r["n_new"] + r["n_drop"],
                                      r["flags"] & (IR.FROZEN | IR.TOO_LONG), esz)
        print(f"{what}, {name}: slam_last_joint_work (bytes, lines) = {(by, lines)}, the association's model = {(m_by, m_lines)}")
        n_blk = (int(by) - m_by) // (4 * esz)
        assert 0 < by and 0 < lines and by == int(by) and lines == int(lines) and n_blk >= 0, (what, name, by, lines, m_by, m_lines)
        assert int(by) - m_by == 4 * esz * n_blk and int(lines) - m_lines == 128 * n_blk, (what, name, by, lines, m_by, m_lines, n_blk)
        if name == "default":                       # the crafted cases on the device
            v, sl, fl = r["verdict"], r["slot"], r["flags"]
            with_cand = (r["ncand"] > 0).sum(axis=1)
            plain = (fl == 0) & (r["ncand"].max(axis=1) <= 1) & (with_cand <= 16)
            assert plain[shape == 0].all() and plain.sum() > B // 6
            assert np.array_equal(r["nodes"][plain], with_cand[plain]), (what, "separated detections: one node each")
            assert (r["n_match"][shape == 1] == 16).all(), (what, "(f)", r["n_match"][shape == 1])
            nn = a.associate(cmds, meas, cnt, det=False)
            for b in np.nonzero(live & (shape == 2))[0]:
                assert list(v[b, :2]) == [JR.MATCHED] * 2 and list(sl[b, :2]) == [0, 4] and nn["slot"][b, 0] == 1, (what, "(b)", b, sl[b, :2], nn["slot"][b, :2])
            for b in np.nonzero(live & (shape == 3))[0]:
                assert list(nn["slot"][b, :2]) == [4, 4] and JR.CONFLICT in nn["verdict"][b, :2], (what, "(c) nearest neighbour", b)
                assert list(v[b, :2]) == [JR.MATCHED] * 2 and list(sl[b, :2]) == [3, 4], (what, "(c)", b, sl[b, :2])
            for b in np.nonzero(live & (shape == 4))[0]:
                assert r["n_match"][b] == 3 and sorted(v[b, 2:4]) == [JR.MATCHED, JR.UNPAIRED] and list(sl[b, :2]) == [0, 4], (what, "(d)", b, v[b, :4])
            sing = live & (shape == SINGULAR_SHAPE)
            assert sing.sum() >= 10 and (fl[sing] & JR.S_SINGULAR).all() and (r["n_match"][sing] == 1).all(), (what, "(g)", fl[sing])
            assert r["rec"][14] >= sing.sum() and r["rec"][15] >= (live & (shape == 2)).sum() > 0 and r["rec"][9] > 0
            assert r["ncand"].max() == 4
        # the host form gives the same, and changes nothing either
        rh = a.associate_joint(cmds, meas, cnt, cfg=jcfg)
        a.save_state(after)
        assert open(before, "rb").read() == open(after, "rb").read(), "a checkpoint differs after slam_associate_joint"
        for k in ("rec", "det", "d2_joint"):
            assert _same_bits(rh[k], r[k]), (what, name, "slam_associate_joint against slam_associate_joint_dev", k)
        for k in ("verdict", "slot", "n_match", "n_new", "n_drop", "flags", "nodes", "ncand"):
            assert np.array_equal(rh[k], r[k]), (what, name, k)
        assert np.array_equal(rh["count_out"], count_out)
        assert all(rh["meas_out"][b, :cin[b]].tobytes() == meas_out[b, :cin[b]].tobytes() and rh["meas_out"][b, cin[b]:].tobytes() == meas[b, cin[b]:].tobytes()
                   for b in range(B)), (what, name, "the host form's output message")
    assert {0, IR.FROZEN, IR.TOO_LONG, JR.BUDGET, JR.S_SINGULAR} <= seen_flags, seen_flags
    assert seen_verdicts == {JR.NONE, JR.MATCHED, JR.NEW, JR.AMBIGUOUS, JR.NO_ROOM, JR.INVALID, JR.UNPAIRED}, seen_verdicts

    # the jointly associated step against twins stepped plainly on the hook-labelled message
    jcfg = JR.joint_cfg()
    host_meas = np.stack([h["meas_out"] for h in hooks]); host_cnt = np.array([h["count_out"] for h in hooks], dtype=np.int32)
    ckpt = {}

    def saved(f, name):
        p = tmp_path / f"{name}.ckpt"
        f.save_state(p)
        ckpt[name] = open(p, "rb").read()
        p.unlink()
    s = a.step_associated_joint(d_cmds, d_meas, (d_cnt, KS), cfg=jcfg)
    assert np.array_equal(s["n_drop"], r["n_drop"]) and _same_bits(s["rec"], r["rec"]), what
    assert dev.get(d_meas, meas).tobytes() == meas.tobytes(), "slam_step_associated_joint_dev wrote the caller's message"
    saved(a, "joint step"); a.close()
    t1 = handle()
    t1.update(cmds, host_meas, host_cnt)
    saved(t1, "slam_step_each on the hook-labelled message"); t1.close()
    t3 = handle()
    d_mi, d_ci = dev.put(meas), dev.put(cnt)
    r3 = t3.associate_joint(d_cmds, d_mi, (d_ci, KS), det=False, cfg=jcfg, dev_out=(d_mi, d_ci))
    assert np.array_equal(r3["verdict"], r["verdict"]) and _same_bits(r3["rec"], r["rec"])
    inplace = dev.get(d_mi, meas)
    for b in range(B):                                                   # in place: the row beyond count_in keeps the input
        assert inplace[b, :cin[b]].tobytes() == meas_out[b, :cin[b]].tobytes() and inplace[b, cin[b]:].tobytes() == meas[b, cin[b]:].tobytes(), (what, b)
    assert np.array_equal(dev.get(d_ci, cnt), count_out)
    t3.update_dev_each(d_cmds, d_mi, d_ci, KS)
    saved(t3, "in place, then the plain step"); t3.close()
    t4 = handle()
    t4.step_associated_joint(cmds, meas, cnt, stats=False, cfg=jcfg)
    saved(t4, "slam_step_associated_joint with host messages"); t4.close()
    for name, raw in ckpt.items():
        assert raw == ckpt["joint step"], f"{what}: the checkpoint after `{name}` differs from the one after slam_step_associated_joint_dev"

    # slam_associate_joint_dev, then slam_step_gated_dev on the same device buffers, against the host-side chain
    cmd1 = np.array([0.012, -0.003], dtype=np.float32)
    t5 = handle()
    hooks1 = _hooks(S, t5, np.repeat(cmd1[None], B, axis=0), meas, cnt, cfg, rows, jcfg)
    lab = np.stack([h["meas_out"] for h in hooks1]); lab_cnt = np.array([h["count_out"] for h in hooks1], dtype=np.int32)
    d_m5, d_c5 = dev.put(np.full_like(meas, SENTINEL)), dev.put(np.full_like(cnt, -1))
    t5.associate_joint(cmd1, d_meas, (d_cnt, KS), det=False, cfg=jcfg, dev_out=(d_m5, d_c5))
    g5 = t5.step_gated_dev(cmd1, d_m5, d_c5, KS)
    saved(t5, "chain on the device"); t5.close()
    t6 = handle()
    g6 = t6.gate(cmd1, lab, lab_cnt, det=False)
    t6.update(cmd1, g6["meas_out"], g6["count_out"])
    saved(t6, "chain on the host"); t6.close()
    assert ckpt["chain on the device"] == ckpt["chain on the host"], what
    assert _same_bits(g5["rec"], g6["rec"]) and np.array_equal(g5["n_rej"], g6["n_rej"]), what
    dev.close()


def test_joint_run_equals_the_loop_of_joint_steps_whatever_the_chunking(S, tmp_path, monkeypatch):  # noqa: F811
    L_max, M, T = 20, 12, 5
    cfg = TA._config(S)
    jcfg = JR.joint_cfg(gate_match=400.0, gate_new=1e4, max_nodes=96)   # (wide individual gates: several candidates on this log)
    rng = np.random.default_rng(13)
    rr, bb = TA._grid(L_max)
    log_meas = np.full((T, B, KS, 3), SENTINEL, np.float32); log_cnt = np.zeros((T, B), np.int32)
    for t in range(T):
        for b in range(B):
            cells = rng.permutation(L_max)[:int(rng.integers(0, 9))]
            k = cells.shape[0]
            log_meas[t, b, :k, 0] = np.nan
            log_meas[t, b, :k, 1] = rr[cells] + 0.02 * rng.standard_normal(k) + 0.3 * (rng.random(k) < 0.2)
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
        a = TA._handle(S, L_max, M, S.F64, cfg, freeze=False)
        res = a.associate_joint_run(c, log_meas, log_cnt, series=True, cfg=jcfg)
        assert res.recs.shape == (T, 16) and res.n_drop.shape == (T, B) and a.timestep == a.get_state(0)["timestep"]
        assert res.recs[:, 4].sum() == res.n_match.sum() > B and res.recs[:, 12].sum() == res.nodes.sum() > 0
        loop = TA._handle(S, L_max, M, S.F64, cfg, freeze=False)
        for t in range(T):
            g = loop.associate_joint(c[t], log_meas[t], log_cnt[t], det=False, cfg=jcfg)
            s = loop.step_associated_joint(c[t], log_meas[t], log_cnt[t], cfg=jcfg)
            assert _same_bits(s["rec"], res.recs[t]) and np.array_equal(s["n_drop"], res.n_drop[t]), t
            assert _same_bits(g["rec"], res.recs[t]) and np.array_equal(g["n_match"], res.n_match[t]), t
            assert np.array_equal(g["n_new"], res.n_new[t]) and np.array_equal(g["flags"], res.flags[t]), t
            assert np.array_equal(g["nodes"], res.nodes[t]) and _same_bits(g["d2_joint"], res.d2_joint[t]), t
        final = saved(a)
        assert saved(loop) == final, "the checkpoint after slam_associate_joint_run differs from the loop of slam_step_associated_joint"
        loop.close()
        for budget in (1, 2 * (12 * KS * B + 48 * B) + 7, 4 * (12 * KS * B + 48 * B) + 3):   # one tick per chunk, chunks that do not divide T
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
            k = TA._handle(S, L_max, M, S.F64, cfg, freeze=False)
            got = k.associate_joint_run(c, log_meas, log_cnt, series=True, cfg=jcfg)
            assert _same_bits(got.recs, res.recs) and _same_bits(got.d2_joint, res.d2_joint), budget
            assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in ("n_match", "n_new", "n_drop", "flags", "nodes")), budget
            assert saved(k) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
            k.close()
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a.set_nav_timing(True)
        a.associate_joint_run(c[:2], log_meas[:2], log_cnt[:2], cfg=jcfg)
        by, lines, joint_ms, total_ms = a.last_joint_work()
        assert 0.0 < joint_ms < total_ms and 0 < by
        a.close()


def test_unsupported_kinds_are_refused_and_keep_their_state(S, tmp_path):  # noqa: F811
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
    N3, N11 = (None,) * 3, (None,) * 8
    cfg = S.default_config(); cfg.landmark_id_is_known = 0
    unknown = S.BatchedEKF(n, L).readParams(cfg)
    handles = [(unknown, "landmark_id_is_known"), (S.BatchedUKF(n, L).readParams(), "sigma points"), (S.BatchedUKFLoc(n).readParams(), "sigma points")]
    for f, word in handles:
        f.set_map(lm); f.init(0.0, 0.0, 0.0)
        f.run_sim(sim_cmds)
        before, after = tmp_path / "before.ckpt", tmp_path / "after.ckpt"
        f.save_state(before)
        assert Lb.slam_associate_joint(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, *N11, fp(mo), ip(co), *N3) == UNSUPPORTED and word in err()
        assert Lb.slam_associate_joint_dev(f.h, None, vp(cmd), 0, vp(meas), vp(cnt), 2, *N11, vp(mo), vp(co), *N3) == UNSUPPORTED
        assert Lb.slam_step_associated_joint(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_step_associated_joint_dev(f.h, None, vp(cmd), 0, vp(meas), vp(cnt), 2, None, None) == UNSUPPORTED and word in err()
        assert Lb.slam_associate_joint_run(f.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, *((None,) * 7)) == UNSUPPORTED and word in err()
        assert Lb.slam_last_joint_work(f.h, None, None, None) == STATE
        f.save_state(after)
        assert open(before, "rb").read() == open(after, "rb").read(), word
        f.close()
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_step_associated_joint(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == STATE and "slam_init" in err()
    e.set_map(lm); e.init(0.0, 0.0, 0.0)
    buf = np.zeros(n * 2 * 3 + 8, np.float32)          # (host memory: the call is refused before any of it is read)
    base = buf.ctypes.data
    rc = Lb.slam_associate_joint_dev(e.h, None, vp(cmd), 0, C.c_void_p(base), vp(cnt), 2, *N11, C.c_void_p(base + 16), vp(co), *N3)
    assert rc == ARG and "overlaps" in err()
    e.track_instance(2)
    assert Lb.slam_step_associated_joint(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == STATE and "slam_track_instance" in err()
    assert Lb.slam_associate_joint_run(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, *((None,) * 7)) == STATE
    e.track_instance(-1)
    assert Lb.slam_step_associated_joint(e.h, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == OK and e.get_state(0)["timestep"] == 1
    e.close()
