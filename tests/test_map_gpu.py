"""Map management on the MI355X (slam_remove_landmarks*, slam_map_tally*, slam_map_prune, slam_step_managed*, slam_manage_run), batch 257,
k_stride 66, per-instance maps and noise rows on, states grown by real steps:
  (a) slam_get_state after a removal equals np.delete of slam_get_state before, in bits, for every instance (a different random mask per
      instance plus the crafted sets none / slot 0 / the last slot / all / alternating / a single survivor, frozen and non-finite
      instances among them); untouched instances are byte-identical in a checkpoint; record, n_removed and the bytes model add up;
  (b) five more steps on messages that re-observe kept landmarks, re-observe a removed id and insert new ones equal, bit for bit, the CPU
      oracle continued from set_state(np.delete(...)): a wrong leading dimension or a non-zero pad column would show here;
  (c) a full map answers NO_ROOM; after a removal the same message inserts;
  (d) counters and prune decisions equal the host hook (the kernels' own per-instance functions compiled for the host) over 30 ticks of
      a log with clutter;
  (e) slam_manage_run equals the loop of slam_step_managed and slam_map_prune under three chunkings;
  (f) the device-pointer variants equal the host-pointer calls.
Classes: L_max 20 and 50 in both storage types, and the streamed classes: fp32 with L_max 66, fp64 with L_max 201 holding 30 landmarks."""
import ctypes as C
import struct

import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR
import map_reference as MR
from test_assoc_gpu import B, KS, SENTINEL, _config, _grid, _handle
from record_tree import MAX_ENTRY_8, fixed_order_record
from test_gate_gpu import _Dev, _same_bits

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -3, -4
KINDS = MR.REMOVAL_SETS + ("random", "random", "random")
# (L_max, landmarks, fp32 storage)
CLASSES = [(20, 18, False), (20, 18, True), (50, 48, False), (50, 48, True), (66, 60, True), (201, 30, False)]
CLASS_IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L66_f32_streamed", "L201_M30_f64_streamed"]


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


def _each(S, cfg, seed):
    """Per-instance noise rows and per-instance maps, as test_assoc_gpu's last class."""
    rng = np.random.default_rng(seed)
    W = rng.uniform(1.5e-3, 5e-3, B)
    rows = S.config.noise_rows(cfg, B, W_00=W, W_11=W[::-1].copy(), V_00=rng.uniform(5e-5, 2e-4, B))
    return rows, rng.uniform(-3.0, 3.0, (B, 6, 2))


def _grown(S, L_max, M, f32, cfg, rows, maps, poison=True):
    """test_assoc_gpu's handle (M landmarks on the grid, updated, a few instances frozen), then a few instances made non-finite by a
    detection of a mapped landmark with a NaN range."""
    f = _handle(S, L_max, M, S.F32 if f32 else S.F64, cfg, rows, maps)
    if poison:
        meas = np.zeros((B, 1, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b in range(9, B, 70):
            meas[b, 0] = [101.0, np.nan, 0.1]; cnt[b] = 1
        f.update((0.0, 0.0), meas, cnt)
    return f


def _raw(f, tmp_path, name="state.ckpt"):
    p = tmp_path / name
    f.save_state(p)
    raw = open(p, "rb").read()
    p.unlink()
    return raw


def _items(raw):
    """The per-instance rows of a checkpoint: dict name -> [B] list of bytes."""
    kind, nb, L_max, dtype, n_max, pstride, xstride, esz = struct.unpack_from("<8i", raw, 8)
    assert nb == B
    sizes = [("P", esz * pstride), ("x", esz * xstride), ("M", 4), ("ids", 4 * L_max), ("flags", 4), ("ts", 4), ("truth", 24), ("err", 8)]
    off = 72
    out = {}
    for name, sz in sizes:
        out[name] = [raw[off + b * sz: off + (b + 1) * sz] for b in range(B)]
        off += B * sz
    assert off == len(raw)
    return out


def _masks(f, states, seed):
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 2, (B, f.L_max)).astype(np.int32)        # (entries at or above M are ignored)
    for b, st in enumerate(states):
        mask[b, :st["M"]] = MR.removal_mask(KINDS[b % len(KINDS)], st["M"], rng)
    return mask


def _deleted(st, row):
    M = st["M"]
    drop = [j for j in range(M) if row[j]]
    idx = [i for j in drop for i in (3 + 2 * j, 4 + 2 * j)]
    return dict(x=np.delete(st["x"], idx), P=np.delete(np.delete(st["P"], idx, 0), idx, 1), ids=np.delete(np.asarray(st["ids"], np.int32), drop),
                M=M - len(drop), dropped=[int(st["ids"][j]) for j in drop])


def _same_state(a, b):
    return (a["M"] == b["M"] and np.asarray(a["x"]).tobytes() == np.asarray(b["x"]).tobytes() and np.ascontiguousarray(a["P"]).tobytes() ==
            np.ascontiguousarray(b["P"]).tobytes() and np.asarray(a["ids"], np.int32).tolist() == np.asarray(b["ids"], np.int32).tolist())


def _model_bytes(M, removed, L_max, esz, from_counters, counters):
    total = 0
    for m, r in zip(M, removed):
        total += 4 + (8 if from_counters else 4) * int(m) + 4
        if r > 0:
            n2 = 3 + 2 * (int(m) - int(r))
            ld2 = (n2 + 1) & ~1 if esz == 8 else (n2 + 3) & ~3
            total += (2 * n2 * n2 + n2 * (ld2 - n2)) * esz + 2 * n2 * esz + (3 if counters else 1) * 4 * (int(m) - int(r) + L_max) + 4
    return float(total)


# ---- (a) and (b): the removal in bits, then stepping on against the oracle -------------------------------------------------------------------
@pytest.mark.parametrize("L_max,M,f32", CLASSES, ids=CLASS_IDS)
def test_removal_is_np_delete_in_bits_and_the_steps_after_it_follow_the_oracle(S, oracle, tmp_path, L_max, M, f32):
    O = oracle
    cfg = _config(S)
    rows, maps = _each(S, cfg, 70 + L_max)
    f = _grown(S, L_max, M, f32, cfg, rows, maps)
    what = CLASS_IDS[CLASSES.index((L_max, M, f32))]
    status = f.status()
    assert (status & IR.INST_INDEX_OOR).any() and (status & IR.INST_NONFINITE).any() and (status == 0).sum() > B // 2
    before = [f.get_state(b) for b in range(B)]
    assert before[0]["M"] == M and any(np.isnan(st["x"]).any() for st in before)
    raw0 = _items(_raw(f, tmp_path))
    mask = _masks(f, before, 80 + L_max)

    r = f.remove_landmarks(mask)
    after = [f.get_state(b) for b in range(B)]
    raw1 = _items(_raw(f, tmp_path))
    want = [_deleted(st, mask[b]) for b, st in enumerate(before)]
    wrong = [b for b in range(B) if not _same_state(after[b], want[b])]
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from np.delete of their state before: {wrong[:10]}"
    removed = np.array([before[b]["M"] - want[b]["M"] for b in range(B)], dtype=np.int32)
    assert np.array_equal(r["n_removed"], removed) and (removed == 0).sum() >= B // len(KINDS) and (removed > 0).sum() > B // 2
    for b in range(B):
        for name in ("flags", "ts", "truth", "err"):
            assert raw0[name][b] == raw1[name][b], (what, b, name, "a removal does not touch it")
        if removed[b] == 0:
            for name in ("P", "x", "M", "ids"):
                assert raw0[name][b] == raw1[name][b], (what, b, name, "an instance with nothing to remove is not written")
        else:
            ids_row = np.frombuffer(raw1["ids"][b], dtype=np.int32)
            assert not ids_row[want[b]["M"]:].any(), (what, b, "ids are zero from M' up")
    n2 = 3 + 2 * np.array([w["M"] for w in want])
    assert r["rec"][0] == (removed > 0).sum() and r["rec"][1] == removed.sum() and r["rec"][2] == (n2[removed > 0] ** 2).sum() and not r["rec"][3:].any()
    inst = np.zeros((B, 16)); inst[:, 0] = removed > 0; inst[:, 1] = removed; inst[:, 2] = np.where(removed > 0, n2.astype(np.float64) ** 2, 0.0)
    assert _same_bits(fixed_order_record(inst, MAX_ENTRY_8), r["rec"])
    by, prune_ms, total_ms = f.last_map_work()
    assert by == _model_bytes([st["M"] for st in before], removed, L_max, 4 if f32 else 8, False, False) and prune_ms == -1.0 and total_ms == -1.0
    seen, expected = f.map_track()
    assert not seen.any() and not expected.any()

    # (b) five more steps: kept landmarks re-observed, a removed id back again (the step inserts it as new), new ids on ticks 0 and 2
    T = 5
    rng = np.random.default_rng(90 + L_max)
    meas = np.zeros((T, B, 6, 3), np.float32); cnt = np.zeros((T, B), np.int32)
    for b in range(B):
        st = after[b]
        for t in range(T):
            m = [AR.clean(rng, st, int(j), float(st["ids"][j])) for j in rng.permutation(st["M"])[:3]] if np.isfinite(st["x"]).all() else []
            if t == 1 and want[b]["dropped"]:
                m.append([float(want[b]["dropped"][0]), 2.2, 0.3])
            if t in (0, 2):
                m.append([float(5000 + t), 1.7 + 0.1 * t, -0.6])
            meas[t, b, :len(m)] = np.asarray(m, dtype=np.float32).reshape(-1, 3); cnt[t, b] = len(m)
    cmds = np.stack([rng.uniform(0.0, 0.02, (T, B)), rng.uniform(-0.01, 0.01, (T, B))], axis=2).astype(np.float32)
    for t in range(T):
        f.update(cmds[t], meas[t], cnt[t])
    final = [f.get_state(b) for b in range(B)]
    status1 = f.status()
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    wrong, compared, grew = [], 0, 0
    for b in range(B):
        if status[b] != 0:
            continue
        ekf = O.OracleEKF(IR.config_for(rows[b]), L_max=L_max, mode=mode)
        ekf.set_state(want[b]["x"], want[b]["P"], want[b]["ids"], timestep=int(after[b]["timestep"]))
        fl = 0
        for t in range(T):
            fl |= ekf.update(cmds[t, b, 0], cmds[t, b, 1], meas[t, b, :cnt[t, b]])
        twin = ekf.state()
        if fl != status1[b] or not _same_state(final[b], twin):
            wrong.append((b, KINDS[b % len(KINDS)], int(status1[b]), int(fl), final[b]["M"], twin["M"]))
        compared += 1
        grew += twin["M"] > want[b]["M"]
    assert not wrong, f"{what}: {len(wrong)} of {compared} instance(s) differ from the oracle continued from np.delete (b, set, flags dev/oracle, M dev/oracle): {wrong[:10]}"
    assert compared > B // 2 and grew > compared // 2
    for b in np.nonzero(status & IR.INST_INDEX_OOR)[0]:                # a frozen instance does not step: the compacted state stays
        assert _same_state(final[b], want[b]), (what, int(b))
    f.close()


# ---- (c) room again ---------------------------------------------------------------------------------------------------------------------------
def test_a_full_map_reports_no_room_and_inserts_after_a_removal(S):
    L_max = 20
    cfg = _config(S)
    rows, maps = _each(S, cfg, 3)
    f = _handle(S, L_max, L_max, S.F64, cfg, rows, maps, freeze=False)
    assert (f.landmark_counts() == L_max).all()
    meas = np.full((B, KS, 3), SENTINEL, np.float32); cnt = np.ones(B, np.int32)
    meas[:, 0] = [np.nan, 9.0, 0.2]                                     # far from every landmark of the grid: a new one
    cmd = (0.0, 0.0)
    g = f.associate(cmd, meas, cnt, det=False)
    assert (g["verdict"][:, 0] == S.ASSOC_NO_ROOM).all() and (g["count_out"] == 0).all() and g["rec"][10] == B
    mask = np.zeros((B, L_max), np.int32); mask[:, 3] = 1
    r = f.remove_landmarks(mask)
    assert (r["n_removed"] == 1).all() and r["rec"][0] == B and (f.landmark_counts() == L_max - 1).all()
    g = f.associate(cmd, meas, cnt, det=False)
    assert (g["verdict"][:, 0] == S.ASSOC_NEW).all() and (g["count_out"] == 1).all() and g["rec"][10] == 0
    f.step_associated(cmd, meas, cnt, stats=False)
    assert (f.landmark_counts() == L_max).all() and not (f.status() & IR.INST_CAPACITY).any()
    st = f.get_state(B - 1)
    assert st["ids"].tolist() == [100 + j for j in range(L_max) if j != 3] + [100 + L_max]     # base = 1 + max id
    f.close()


# ---- (d) tally and prune against the host hook --------------------------------------------------------------------------------------------
def _clutter_log(T, seed):
    """An id-less log: each of the grid's first 15 cells detected with probability 0.7 (rows 0 and 1 lie inside the shrunk view, row 2 beyond
    the range: expected only when seen), and one clutter detection per instance and tick, uniform in the field of view."""
    rng = np.random.default_rng(seed)
    rr, bb = _grid(15)
    meas = np.full((T, B, KS, 3), SENTINEL, np.float32); cnt = np.zeros((T, B), np.int32)
    for t in range(T):
        for b in range(B):
            cells = np.nonzero(rng.random(15) < 0.7)[0]
            k = cells.shape[0]
            meas[t, b, :k, 0] = np.nan
            meas[t, b, :k, 1] = rr[cells] + 0.02 * rng.standard_normal(k)
            meas[t, b, :k, 2] = bb[cells] + 0.02 * rng.standard_normal(k)
            meas[t, b, k] = [np.nan, rng.uniform(0.6, 2.9), rng.uniform(-1.5, 1.5)]
            cnt[t, b] = k + 1
    cmds = np.zeros((T, 2), np.float32); cmds[:, 0] = 0.002
    return cmds, meas, cnt


def _x_ids(f, b):
    """x and ids of one instance without its P."""
    from live_ekf_slam_amd import _lib
    x = np.zeros(f.n_max); ids = np.zeros(f.L_max, np.int32); M = np.zeros(1, np.int32)
    _lib.check(_lib.lib().slam_get_state(f.h, b, x.ctypes.data_as(_lib._dp), None, M.ctypes.data_as(_lib._ip), ids.ctypes.data_as(_lib._ip), None))
    m = int(M[0])
    return x[:3 + 2 * m].copy(), ids[:m].copy()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_counters_and_prune_decisions_equal_the_host_hook_over_30_ticks_with_clutter(S, f32):
    L_max, M, T = 20, 12, 30
    cfg = _config(S)
    rows, maps = _each(S, cfg, 4)
    mc = S.MapConfig(0.9, 0.1, 4, 0.5, 10)
    vision = (cfg.range_max, cfg.fov_min, cfg.fov_max)
    f = _handle(S, L_max, M, S.F32 if f32 else S.F64, cfg, rows, maps)          # (a few instances are frozen)
    cmds, meas, cnt = _clutter_log(T, 21)
    seen = np.zeros((B, L_max), np.int32); expected = np.zeros((B, L_max), np.int32)
    total_removed = 0
    for t in range(T):
        g = f.associate(cmds[t], meas[t], cnt[t], det=False)
        f.step_managed(cmds[t], meas[t], cnt[t], stats=False, map_cfg=mc)
        status = f.status()
        states = [_x_ids(f, b) for b in range(B)]
        for b, (x, ids) in enumerate(states):
            n = x.shape[0]
            h = S.map_instance_host(x, np.zeros((n, n)), ids, L_max, int(status[b]), meas=g["meas_out"][b], count=int(g["count_out"][b]), k_stride=KS,
                                    assoc_flag=int(g["flags"][b]), vision=vision, f32_storage=f32, cfg=mc, seen=seen[b], expected=expected[b])
            seen[b], expected[b] = h["seen"], h["expected"]
        ds, de = f.map_track()
        assert np.array_equal(ds, seen) and np.array_equal(de, expected), (t, "the counters after the tally", np.nonzero((ds != seen).any(1) | (de != expected).any(1))[0][:10])
        if (t + 1) % mc.prune_every == 0:
            r = f.map_prune(cfg=mc)
            for b, (x, ids) in enumerate(states):
                n = x.shape[0]
                h = S.map_instance_host(x, np.zeros((n, n)), ids, L_max, cfg=mc, seen=seen[b], expected=expected[b], prune=True)
                assert int(h["mask"].sum()) == r["n_removed"][b], (t, b, "the prune decision")
                seen[b], expected[b] = h["seen"], h["expected"]
                x2, ids2 = _x_ids(f, b)
                assert ids2.tolist() == h["ids"].tolist() and x2.tobytes() == h["x"].tobytes(), (t, b, "the state after the prune")
            ds, de = f.map_track()
            assert np.array_equal(ds, seen) and np.array_equal(de, expected), (t, "the counters after the prune")
            assert r["rec"][1] == r["n_removed"].sum()
            total_removed += int(r["n_removed"].sum())
            by, _, _ = f.last_map_work()
            assert by > 0
    assert total_removed > B // 4 and np.median(f.landmark_counts()) >= 10, "clutter went and the landmarks of the grid stayed"
    assert seen.max() > 5 and (expected > seen).any()
    frozen = np.nonzero(f.status() & IR.INST_INDEX_OOR)[0]
    assert frozen.size and not seen[frozen].any(), "a frozen instance is not tallied"
    f.map_track_reset()
    ds, de = f.map_track()
    assert not ds.any() and not de.any()
    f.close()


# ---- (e) the managed run against its loop, and chunking -----------------------------------------------------------------------------------------
def test_manage_run_equals_the_loop_of_managed_steps_and_prunes_whatever_the_chunking(S, tmp_path, monkeypatch):
    L_max, M, T = 20, 12, 25
    cfg = _config(S)
    mc = S.MapConfig(0.9, 0.1, 4, 0.5, 10)
    cmds, meas, cnt = _clutter_log(T, 22)
    rng = np.random.default_rng(13)
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)
    for c in (cmds, each):
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        res = a.manage_run(c, meas, cnt, series=True, map_cfg=mc)
        assert res.recs.shape == (T, 16) and res.n_removed.shape == (T, B) and a.timestep == a.get_state(0)["timestep"]
        prune_ticks = [t for t in range(T) if (t + 1) % mc.prune_every == 0]
        assert prune_ticks == [9, 19] and res.n_removed[prune_ticks].sum() > B // 4
        assert not np.delete(res.n_removed, prune_ticks, axis=0).any()
        loop = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        for t in range(T):
            s = loop.step_managed(c[t], meas[t], cnt[t], map_cfg=mc)
            assert _same_bits(s["rec"], res.recs[t]) and np.array_equal(s["n_drop"], res.n_drop[t]), t
            if t in prune_ticks:
                assert np.array_equal(loop.map_prune(cfg=mc)["n_removed"], res.n_removed[t]), t
        final, track = _raw(a, tmp_path), a.map_track()
        assert _raw(loop, tmp_path) == final, "the checkpoint after slam_manage_run differs from the loop of slam_step_managed and slam_map_prune"
        assert all(np.array_equal(u, v) for u, v in zip(loop.map_track(), track))
        loop.close()
        per_tick = 32 * B + 12 * KS * B + (8 * B if c.ndim == 3 else 0)
        for budget in (1, 3 * per_tick + 7):                     # one tick per chunk, and chunks of three that the prunes fall into
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
            k = _handle(S, L_max, M, S.F64, cfg, freeze=False)
            got = k.manage_run(c, meas, cnt, series=True, map_cfg=mc)
            assert _same_bits(got.recs, res.recs), budget
            assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in ("n_match", "n_new", "n_drop", "flags", "n_removed")), budget
            assert _raw(k, tmp_path) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
            assert all(np.array_equal(u, v) for u, v in zip(k.map_track(), track)), budget
            k.close()
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        by_run, prune_ms, total_ms = a.last_map_work()
        assert by_run > 0 and prune_ms == -1.0 and total_ms > 0.0
        a.set_nav_timing(True)
        a.manage_run(c[:10], meas[:10], cnt[:10], map_cfg=mc)
        by, prune_ms, total_ms = a.last_map_work()
        assert 0.0 <= prune_ms < total_ms and by > 0
        a.close()


# ---- (f) the device-pointer variants ------------------------------------------------------------------------------------------------------------
def test_device_pointer_variants_equal_the_host_pointer_calls(S, hip, tmp_path):
    L_max, M = 50, 48
    cfg = _config(S)
    rows, maps = _each(S, cfg, 6)
    mc = S.MapConfig(0.8, 0.2, 1, 1.0, 1)
    dev = _Dev(hip)
    a = _grown(S, L_max, M, True, cfg, rows, maps)
    d = _grown(S, L_max, M, True, cfg, rows, maps)
    states = [a.get_state(b) for b in range(B)]
    mask = _masks(a, states, 31)
    ra = a.remove_landmarks(mask)
    rd = d.remove_landmarks(dev.put(mask))
    assert np.array_equal(ra["n_removed"], rd["n_removed"]) and _same_bits(ra["rec"], rd["rec"]) and ra["n_removed"].sum() > B
    assert _raw(a, tmp_path) == _raw(d, tmp_path), "slam_remove_landmarks_dev against slam_remove_landmarks"
    assert a.last_map_work() == d.last_map_work()
    cmds, meas, cnt = _clutter_log(2, 32)
    flags = np.zeros(B, np.int32); flags[::7] = 8
    a.map_tally(meas[0], cnt[0], flags, cfg=mc)
    d.map_tally(dev.put(meas[0]), (dev.put(cnt[0]), KS), dev.put(flags), cfg=mc)
    ta, td = a.map_track(), d.map_track()
    assert np.array_equal(ta[0], td[0]) and np.array_equal(ta[1], td[1]) and ta[1].any() and not ta[1][::7].any()
    each = np.stack([np.full(B, 0.002), np.linspace(-0.01, 0.01, B)], axis=1).astype(np.float32)
    for t, c in enumerate((cmds[1], each)):
        sa = a.step_managed(c, meas[t], cnt[t], map_cfg=mc)
        sd = d.step_managed(dev.put(c) if c.ndim == 2 else c, dev.put(meas[t]), (dev.put(cnt[t]), KS), map_cfg=mc)
        assert _same_bits(sa["rec"], sd["rec"]) and np.array_equal(sa["n_drop"], sd["n_drop"]), t
    assert _raw(a, tmp_path) == _raw(d, tmp_path), "slam_step_managed_dev against slam_step_managed"
    ta, td = a.map_track(), d.map_track()
    assert np.array_equal(ta[0], td[0]) and np.array_equal(ta[1], td[1])
    pa, pd = a.map_prune(cfg=mc), d.map_prune(cfg=mc)
    assert np.array_equal(pa["n_removed"], pd["n_removed"]) and _raw(a, tmp_path) == _raw(d, tmp_path)
    a.close(); d.close(); dev.close()


# ---- the kinds and the states the calls refuse -----------------------------------------------------------------------------------------------
def test_unsupported_kinds_and_states_are_refused_and_keep_their_state(S, tmp_path):
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    Lb = _lib.lib()
    L, T, n = 20, 10, 8
    lm, sim_cmds = make_scenario(341, L, T)
    cmd = np.array([0.05, 0.01], np.float32); meas = np.zeros((n, 2, 3), np.float32); cnt = np.zeros(n, np.int32)
    mask = np.ones((n, L), np.int32)
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    err = (lambda: Lb.slam_last_error().decode())
    u = S.BatchedUKF(n, L).readParams()
    u.set_map(lm); u.init(0.0, 0.0, 0.0)
    u.run_sim(sim_cmds)
    before = _raw(u, tmp_path)
    assert Lb.slam_remove_landmarks(u.h, ip(mask), None, None) == UNSUPPORTED and "EKF_SLAM" in err()
    assert Lb.slam_map_tally(u.h, None, fp(meas), ip(cnt), 2, None) == UNSUPPORTED
    assert Lb.slam_map_prune(u.h, None, None, None) == UNSUPPORTED
    assert Lb.slam_map_get_track(u.h, None, None) == UNSUPPORTED
    assert Lb.slam_step_managed(u.h, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == UNSUPPORTED
    assert Lb.slam_manage_run(u.h, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None, None) == UNSUPPORTED
    assert Lb.slam_last_map_work(u.h, None, None, None) == STATE
    assert _raw(u, tmp_path) == before
    u.close()
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_remove_landmarks(e.h, ip(mask), None, None) == STATE and "slam_init" in err()
    assert Lb.slam_map_prune(e.h, None, None, None) == STATE and Lb.slam_step_managed(e.h, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, None, None) == STATE
    e.set_map(lm); e.init(0.0, 0.0, 0.0)
    e.run_sim(sim_cmds)
    e.track_instance(2)
    assert Lb.slam_remove_landmarks(e.h, ip(mask), None, None) == STATE and "slam_track_instance" in err()
    assert Lb.slam_map_tally(e.h, None, fp(meas), ip(cnt), 2, None) == STATE and Lb.slam_manage_run(
        e.h, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None, None) == STATE
    e.track_instance(-1)
    M0 = e.landmark_counts()
    assert M0.max() > 0
    r = e.remove_landmarks(mask)                                    # everything goes; the pose block stays
    assert np.array_equal(r["n_removed"], M0) and not e.landmark_counts().any()
    e.map_tally(meas, cnt)
    e.init(0.0, 0.0, 0.0)                                           # the counters are zero after slam_init
    s, x = e.map_track()
    assert not s.any() and not x.any()
    e.close()
