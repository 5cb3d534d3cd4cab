"""Landmark merging on the MI355X (slam_map_duplicates*, slam_merge_landmarks*, slam_map_merge, slam_manage_merge_run), test_map_gpu's
shapes: batch 257, k_stride 66, per-instance maps and noise rows on, its size classes in both storage types.  States are grown by real
steps in which known-id messages insert one physical landmark under two ids (two or three such duplicates per instance) and then observe
both ids with independent noise; a few instances are frozen or non-finite.
  (a) slam_map_duplicates equals the host hook (the kernels' own per-instance functions compiled for the host) in bits: partners and d2;
  (b) the state after slam_map_merge equals the hook's, in bits; untouched instances are byte-identical in a checkpoint; record, n_merged
      and the bytes model add up;
  (c) five further steps that re-observe the kept id and the dropped id equal, bit for bit, the CPU oracle continued from set_state of
      the hook's result: a wrong leading dimension or a non-zero pad column would show here;
  (d) slam_merge_landmarks with caller pairs, non-mutual and out-of-range entries among them, with track counters;
  (e) slam_manage_merge_run equals the loop of slam_step_managed, slam_map_merge and slam_map_prune under three chunkings;
  (f) the device-pointer variants equal the host-pointer calls."""
import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR
from test_assoc_gpu import B, KS, SENTINEL, _config, _grid, _handle
from record_tree import MAX_ENTRY_8, fixed_order_record
from test_gate_gpu import _Dev, _same_bits
from test_map_gpu import CLASSES, CLASS_IDS, S, hip, _clutter_log, _each, _grown, _items, _model_bytes, _raw, _same_state  # noqa: F401

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = -3, -4
SKIP = 1 | 4 | 32
DUPS = ((1, 700), (4, 701), (7, 702))      # (slot duplicated, the second id); the third only in every third instance


def _duplicated(S, L_max, M, f32, cfg, rows, maps):
    """test_map_gpu's grown handle with M - 3 landmarks, then real steps: one message inserts the duplicates (the detection of the mapped
    slot as the instance's own estimate sees it, under a new id), two more observe both ids of each with independent noise."""
    f = _grown(S, L_max, M - 3, f32, cfg, rows, maps)
    rng = np.random.default_rng(100 + L_max)
    states = [f.get_state(b) for b in range(B)]
    for rnd in range(3):
        meas = np.zeros((B, 6, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b, st in enumerate(states):
            if not np.isfinite(st["x"]).all():
                continue
            m = []
            for k, (slot, ident) in enumerate(DUPS):
                if k == 2 and b % 3:
                    continue
                m.append(AR.clean(rng, st, slot, float(ident)))
                if rnd:
                    m.append(AR.clean(rng, st, slot, float(st["ids"][slot])))
            meas[b, :len(m)] = np.asarray(m, dtype=np.float32); cnt[b] = len(m)
        f.update((0.0, 0.0), meas, cnt)
    return f


def _hooks(S, states, status, L_max, f32, cfg=None, fuse=True, partner=None, track=None):
    out = []
    for b, st in enumerate(states):
        kw = {} if track is None else dict(seen=track[0][b], expected=track[1][b])
        out.append(S.merge_instance_host(st["x"], st["P"], st["ids"], L_max, int(status[b]), f32, cfg, partner=None if partner is None else partner[b],
                                         fuse=fuse, **kw))
    return out


def _merge_model_bytes(states, status, hooks, L_max, esz, counters, find):
    """slam_last_merge_work's model restated: merge_traffic per instance plus the compaction as slam_last_map_work counts it."""
    total = 0
    for st, s, h in zip(states, status, hooks):
        M = st["M"]; n = 3 + 2 * M
        fused = int(h["rec"][1]); attempted = fused + int(h["rec"][3])
        elems = (n * n + n if find and not (s & SKIP) and M >= 2 else 0) + attempted * (8 * n + 2) + fused * (2 * n * n + 2 * n)
        total += elems * esz + 8 + 4 * L_max + 16 + ((4 * M + (24 if counters else 0) * fused) if fused else 0)
    return float(total) + _model_bytes([st["M"] for st in states], [st["M"] - h["M"] for st, h in zip(states, hooks)], L_max, esz, False, counters)


# ---- (a), (b), (c) ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,M,f32", CLASSES, ids=CLASS_IDS)
def test_duplicates_and_the_merge_equal_the_host_hook_and_the_steps_after_follow_the_oracle(S, oracle, tmp_path, L_max, M, f32):
    O = oracle
    cfg = _config(S)
    rows, maps = _each(S, cfg, 170 + L_max)
    f = _duplicated(S, L_max, M, f32, cfg, rows, maps)
    what = CLASS_IDS[CLASSES.index((L_max, M, f32))]
    status = f.status()
    assert (status & IR.INST_INDEX_OOR).any() and (status & IR.INST_NONFINITE).any() and (status == 0).sum() > B // 2
    before = [f.get_state(b) for b in range(B)]
    assert max(st["M"] for st in before) == M
    raw0 = _items(_raw(f, tmp_path))

    # (a) the decision alone
    partner, d2 = f.map_duplicates()
    assert _items(_raw(f, tmp_path)) == raw0, "slam_map_duplicates changes no state"
    hooks = _hooks(S, before, status, L_max, f32, fuse=False)
    wrong = [b for b in range(B) if partner[b].tolist() != hooks[b]["partner"].tolist() or not _same_bits(d2[b], hooks[b]["d2"])]
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the hook's decision: {wrong[:10]}"
    pairs = (partner >= 0).sum(axis=1) // 2
    print(f"{what}: pairs per instance {np.bincount(pairs)}")
    assert (pairs >= 2).sum() > B // 2 and (pairs == 3).sum() > B // 8 and not pairs[(status & SKIP) != 0].any()
    by, merge_ms, total_ms = f.last_merge_work()
    esz = 4 if f32 else 8
    elig = [(3 + 2 * st["M"]) ** 2 + 3 + 2 * st["M"] for st, s in zip(before, status) if not (s & SKIP) and st["M"] >= 2]
    assert by == float(sum(elig) * esz + B * (8 + 4 * L_max + 16)) and merge_ms == -1.0 and total_ms == -1.0

    # (b) find, fuse and compact
    r = f.map_merge()
    after = [f.get_state(b) for b in range(B)]
    raw1 = _items(_raw(f, tmp_path))
    hooks = _hooks(S, before, status, L_max, f32)
    wrong = [b for b in range(B) if not _same_state(after[b], hooks[b])]
    assert not wrong, f"{what}: {len(wrong)} instance(s) differ from the hook's merged state: {wrong[:10]}"
    merged = np.array([before[b]["M"] - hooks[b]["M"] for b in range(B)], dtype=np.int32)
    assert np.array_equal(r["n_merged"], merged) and np.array_equal(merged, pairs), "every pair found was fused"
    for b in range(B):
        for name in ("flags", "ts", "truth", "err"):
            assert raw0[name][b] == raw1[name][b], (what, b, name, "a merge does not touch it")
        if merged[b] == 0:
            for name in ("P", "x", "M", "ids"):
                assert raw0[name][b] == raw1[name][b], (what, b, name, "an instance without a fused pair is not written")
        else:
            ids_row = np.frombuffer(raw1["ids"][b], dtype=np.int32)
            assert not ids_row[hooks[b]["M"]:].any(), (what, b, "ids are zero from M' up")
            kept = ids_row[:hooks[b]["M"]].tolist()
            for i in np.nonzero(partner[b] > np.arange(L_max))[0]:
                assert int(before[b]["ids"][i]) in kept and int(before[b]["ids"][partner[b, i]]) not in kept, (what, b, "the kept id is ids[i]")
    inst = np.stack([h["rec"] for h in hooks])
    assert _same_bits(fixed_order_record(inst, MAX_ENTRY_8), r["rec"]), (what, r["rec"])
    assert r["rec"][0] == (merged > 0).sum() and r["rec"][1] == merged.sum() and r["rec"][3] == 0 and 0 < r["rec"][8] <= S.default_merge_config().gate_merge
    by, _, _ = f.last_merge_work()
    assert by == _merge_model_bytes(before, status, hooks, L_max, esz, False, True)

    # (c) five more steps: the kept id and the dropped id re-observed (the step inserts the dropped one as new), two other landmarks
    T = 5
    rng = np.random.default_rng(190 + L_max)
    meas = np.zeros((T, B, 6, 3), np.float32); cnt = np.zeros((T, B), np.int32)
    for b in range(B):
        st = after[b]
        if not np.isfinite(st["x"]).all():
            continue
        ids = st["ids"].tolist()
        for t in range(T):
            m = [AR.clean(rng, st, int(j), float(st["ids"][j])) for j in rng.permutation(st["M"])[:2]]
            m.append(AR.clean(rng, st, ids.index(101), 101.0))
            if t in (1, 3):
                m.append(AR.clean(rng, st, ids.index(101), 700.0))
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
        ekf.set_state(hooks[b]["x"], hooks[b]["P"], hooks[b]["ids"], timestep=int(after[b]["timestep"]))
        fl = 0
        for t in range(T):
            fl |= ekf.update(cmds[t, b, 0], cmds[t, b, 1], meas[t, b, :cnt[t, b]])
        twin = ekf.state()
        if fl != status1[b] or not _same_state(final[b], twin):
            wrong.append((b, int(status1[b]), int(fl), final[b]["M"], twin["M"]))
        compared += 1
        grew += twin["M"] == hooks[b]["M"] + 1
    assert not wrong, f"{what}: {len(wrong)} of {compared} instance(s) differ from the oracle continued from the hook's merged state: {wrong[:10]}"
    assert compared > B // 2 and grew > compared // 2, "the dropped id came back as one new landmark"
    f.close()


# ---- the size class in which a lane owns several slots (L_max > 256) --------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_map_of_more_than_256_landmarks(S, f32):
    """L_max 300 holding 264 landmarks in 3 instances: the find gives a lane up to four slots, and the pairs (1, 262) and (260, 263) have
    their slots in different ownership rounds.  Decision and merged state against the hook, in bits."""
    nb, L_max, M0 = 3, 300, 262
    cfg = _config(S)
    f = S.BatchedEKF(nb, L_max, dtype=S.F32 if f32 else S.F64).readParams(cfg)
    f.set_seed(11); f.init(0.3, -0.2, 0.4)
    j = np.arange(M0)
    rr, bb, ids = 1.5 + 0.5 * (j // 10), -1.2 + 0.26 * (j % 10), 100.0 + j
    rng = np.random.default_rng(77)
    for rnd in range(4):                                             # insertions, then three rounds of updates
        for lo in range(0, M0, 40):
            hi = min(lo + 40, M0)
            m = np.zeros((nb, hi - lo, 3), np.float32)
            m[:, :, 0] = ids[lo:hi]
            m[:, :, 1] = rr[lo:hi] + min(rnd, 1) * 0.02 * rng.standard_normal((nb, hi - lo))
            m[:, :, 2] = bb[lo:hi] + min(rnd, 1) * 0.002 * rng.standard_normal((nb, hi - lo))
            f.update((0.0, 0.0), m, np.full(nb, hi - lo, np.int32))
    states = [f.get_state(b) for b in range(nb)]
    m = np.zeros((nb, 2, 3), np.float32)
    for b, st in enumerate(states):
        m[b] = [AR.clean(rng, st, 1, 700.0), AR.clean(rng, st, 260, 701.0)]
    f.update((0.0, 0.0), m, np.full(nb, 2, np.int32))
    status = f.status()
    before = [f.get_state(b) for b in range(nb)]
    assert all(st["M"] == M0 + 2 for st in before) and not status.any()
    partner, d2 = f.map_duplicates()
    hooks = _hooks(S, before, status, L_max, f32, fuse=False)
    for b in range(nb):
        assert partner[b].tolist() == hooks[b]["partner"].tolist() and _same_bits(d2[b], hooks[b]["d2"]), b
        assert partner[b, 1] == 262 and partner[b, 260] == 263, (b, np.nonzero(partner[b] >= 0)[0])
    r = f.map_merge()
    hooks = _hooks(S, before, status, L_max, f32)
    assert all(_same_state(f.get_state(b), hooks[b]) for b in range(nb)) and np.array_equal(r["n_merged"], (partner >= 0).sum(axis=1) // 2)
    assert _same_bits(fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8), r["rec"])
    f.close()


# ---- (d) caller pairs ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_caller_pairs_with_entries_that_are_not_mutual_or_out_of_range(S, tmp_path, f32):
    L_max, M = 20, 18
    cfg = _config(S)
    rows, maps = _each(S, cfg, 7)
    f = _duplicated(S, L_max, M, f32, cfg, rows, maps)
    status = f.status()
    before = [f.get_state(b) for b in range(B)]
    rng = np.random.default_rng(41)
    for _ in range(3):                                               # the counters exist and differ from slot to slot
        meas = np.zeros((B, M, 3), np.float32); cnt = np.zeros(B, np.int32)
        for b, st in enumerate(before):
            seen_now = np.nonzero(rng.random(st["M"]) < 0.5)[0]
            meas[b, :len(seen_now), 0] = st["ids"][seen_now]; cnt[b] = len(seen_now)
        f.map_tally(meas, cnt)
    track = f.map_track()
    assert track[0].any() and (track[1] > track[0]).any()
    found, _ = f.map_duplicates()
    partner = found.copy()
    for b in range(B):
        kind = b % 5
        if kind == 1:
            partner[b, 0] = 2                                          # not mutual
        elif kind == 2:
            partner[b, 3] = 3; partner[b, L_max - 1] = L_max - 2; partner[b, L_max - 2] = L_max - 1   # itself; a pair at or above M
        elif kind == 3:
            partner[b, 5] = 1000; partner[b, 6] = -9                   # out of range
        elif kind == 4:
            partner[b] = -1; partner[b, 0] = 2; partner[b, 2] = 0     # two different landmarks: fused all the same
    raw0 = _items(_raw(f, tmp_path))
    r = f.merge_landmarks(partner)
    hooks = _hooks(S, before, status, L_max, f32, partner=partner, track=track)
    after = [f.get_state(b) for b in range(B)]
    wrong = [b for b in range(B) if not _same_state(after[b], hooks[b])]
    assert not wrong, f"{len(wrong)} instance(s) differ from the hook's merged state: {wrong[:10]}"
    assert np.array_equal(r["n_merged"], [st["M"] - h["M"] for st, h in zip(before, hooks)])
    assert _same_bits(fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8), r["rec"]) and r["rec"][2] > B // 2 and r["rec"][1] > B
    seen, expected = f.map_track()
    assert all(np.array_equal(seen[b], hooks[b]["seen"]) and np.array_equal(expected[b], hooks[b]["expected"]) for b in range(B))
    raw1 = _items(_raw(f, tmp_path))
    for b in np.nonzero((status & SKIP) != 0)[0]:
        assert all(raw0[name][b] == raw1[name][b] for name in raw0), (int(b), "a skipped instance honours no entry")
    by, _, _ = f.last_merge_work()
    assert by == _merge_model_bytes(before, status, hooks, L_max, 4 if f32 else 8, True, False)
    f.close()


# ---- (e) the managed run that merges against its loop, and chunking ---------------------------------------------------------------------------
def _outlier_log(T, seed):
    """test_map_gpu's clutter log and, on the ticks 3, 8, 13, ..., one more return of grid cell 2 that lies 0.2 m behind it: beyond
    gate_new = gate_match it becomes a second landmark, which the merge (sigma 0.1 m) fuses with the first."""
    cmds, meas, cnt = _clutter_log(T, seed)
    rr, bb = _grid(15)
    for t in range(3, T, 5):
        for b in range(B):
            meas[t, b, cnt[t, b]] = [np.nan, rr[2] + 0.2, bb[2]]
            cnt[t, b] += 1
    return cmds, meas, cnt


def test_manage_merge_run_equals_its_loop_whatever_the_chunking(S, tmp_path, monkeypatch):
    L_max, M, T = 20, 12, 25
    cfg = _config(S)
    mc = S.MapConfig(0.9, 0.1, 4, 0.5, 10)
    ac = S.AssocConfig(S.default_assoc_config().gate_match, S.default_assoc_config().gate_match)
    gc = S.MergeConfig(S.default_merge_config().gate_merge, 0.1, 5)
    cmds, meas, cnt = _outlier_log(T, 23)
    rng = np.random.default_rng(14)
    each = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)
    names = ("n_match", "n_new", "n_drop", "flags", "n_removed", "n_merged")
    for c in (cmds, each):
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        a = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        res = a.manage_merge_run(c, meas, cnt, series=True, cfg=ac, map_cfg=mc, merge_cfg=gc)
        assert res.recs.shape == (T, 16) and res.n_merged.shape == (T, B) and a.timestep == a.get_state(0)["timestep"]
        merge_ticks = [t for t in range(T) if (t + 1) % gc.merge_every == 0]
        prune_ticks = [t for t in range(T) if (t + 1) % mc.prune_every == 0]
        print("merged per merge tick", res.n_merged[merge_ticks].sum(axis=1), "removed", res.n_removed[prune_ticks].sum(axis=1))
        assert merge_ticks == [4, 9, 14, 19, 24] and res.n_merged[merge_ticks].sum() > B // 4
        assert not np.delete(res.n_merged, merge_ticks, axis=0).any() and not np.delete(res.n_removed, prune_ticks, axis=0).any()
        loop = _handle(S, L_max, M, S.F64, cfg, freeze=False)
        for t in range(T):
            s = loop.step_managed(c[t], meas[t], cnt[t], cfg=ac, map_cfg=mc)
            assert _same_bits(s["rec"], res.recs[t]) and np.array_equal(s["n_drop"], res.n_drop[t]), t
            if t in merge_ticks:                                  # the merge comes before the tick's prune
                assert np.array_equal(loop.map_merge(cfg=gc)["n_merged"], res.n_merged[t]), t
            if t in prune_ticks:
                assert np.array_equal(loop.map_prune(cfg=mc)["n_removed"], res.n_removed[t]), t
        final, track = _raw(a, tmp_path), a.map_track()
        assert _raw(loop, tmp_path) == final, "the checkpoint after slam_manage_merge_run differs from the loop"
        assert all(np.array_equal(u, v) for u, v in zip(loop.map_track(), track))
        loop.close()
        plain = _handle(S, L_max, M, S.F64, cfg, freeze=False)      # slam_manage_run is what it was: it does not merge
        plain.manage_run(c, meas, cnt, cfg=ac, map_cfg=mc)
        assert np.median(plain.landmark_counts()) > np.median(a.landmark_counts())
        plain.close()
        per_tick = 56 * B + 12 * KS * B + (8 * B if c.ndim == 3 else 0)
        for budget in (1, 3 * per_tick + 7):                     # one tick per chunk, and chunks of three that merges and prunes fall into
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
            k = _handle(S, L_max, M, S.F64, cfg, freeze=False)
            got = k.manage_merge_run(c, meas, cnt, series=True, cfg=ac, map_cfg=mc, merge_cfg=gc)
            assert _same_bits(got.recs, res.recs), budget
            assert all(np.array_equal(getattr(got, n), getattr(res, n)) for n in names), budget
            assert _raw(k, tmp_path) == final, f"SLAM_MONITOR_LOG_BYTES={budget}: the checkpoint differs"
            assert all(np.array_equal(u, v) for u, v in zip(k.map_track(), track)), budget
            assert k.last_merge_work()[0] == a.last_merge_work()[0], budget
            k.close()
        monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        by_run, merge_ms, total_ms = a.last_merge_work()
        assert by_run > 0 and merge_ms == -1.0 and total_ms > 0.0
        a.set_nav_timing(True)
        a.manage_merge_run(c[:10], meas[:10], cnt[:10], cfg=ac, map_cfg=mc, merge_cfg=gc)
        by, merge_ms, total_ms = a.last_merge_work()
        assert 0.0 < merge_ms < total_ms and by > 0
        a.close()


# ---- (f) the device-pointer variants ------------------------------------------------------------------------------------------------------------
def test_device_pointer_variants_equal_the_host_pointer_calls(S, hip, tmp_path):
    L_max, M = 50, 48
    cfg = _config(S)
    rows, maps = _each(S, cfg, 8)
    dev = _Dev(hip)
    a = _duplicated(S, L_max, M, True, cfg, rows, maps)
    d = _duplicated(S, L_max, M, True, cfg, rows, maps)
    partner, d2 = a.map_duplicates()
    dp = dev.put(np.zeros((B, L_max), np.int32)); dd = dev.put(np.zeros((B, L_max)))
    assert d.map_duplicates(dev=(dp, dd)) is None
    d.sync()
    assert np.array_equal(dev.get(dp, partner), partner) and _same_bits(dev.get(dd, d2), d2) and (partner >= 0).sum() > 2 * B
    assert a.last_merge_work() == d.last_merge_work()
    ra = a.merge_landmarks(partner)
    rd = d.merge_landmarks(dp)                                      # the array the find left on the device
    assert np.array_equal(ra["n_merged"], rd["n_merged"]) and _same_bits(ra["rec"], rd["rec"]) and ra["n_merged"].sum() > B
    assert _raw(a, tmp_path) == _raw(d, tmp_path), "slam_merge_landmarks_dev against slam_merge_landmarks"
    assert a.last_merge_work() == d.last_merge_work()
    a.close(); d.close(); dev.close()


# ---- the kinds and the states the calls refuse -----------------------------------------------------------------------------------------------
def test_unsupported_kinds_and_states_are_refused_and_keep_their_state(S, tmp_path):
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    Lb = _lib.lib()
    L, T, n = 20, 10, 8
    lm, sim_cmds = make_scenario(341, L, T)
    cmd = np.array([0.05, 0.01], np.float32); meas = np.zeros((n, 2, 3), np.float32); cnt = np.zeros(n, np.int32)
    partner = np.full((n, L), -1, np.int32)
    fp, ip = (lambda a: a.ctypes.data_as(_lib._fp)), (lambda a: a.ctypes.data_as(_lib._ip))
    err = (lambda: Lb.slam_last_error().decode())
    u = S.BatchedUKF(n, L).readParams()
    u.set_map(lm); u.init(0.0, 0.0, 0.0)
    u.run_sim(sim_cmds)
    before = _raw(u, tmp_path)
    assert Lb.slam_map_duplicates(u.h, None, ip(partner), None) == UNSUPPORTED and "EKF_SLAM" in err()
    assert Lb.slam_merge_landmarks(u.h, None, ip(partner), None, None) == UNSUPPORTED
    assert Lb.slam_map_merge(u.h, None, None, None) == Lb.slam_map_prune(u.h, None, None, None) == UNSUPPORTED
    assert Lb.slam_manage_merge_run(u.h, None, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None, None, None) == \
        Lb.slam_manage_run(u.h, None, None, fp(cmd), 0, fp(meas), ip(cnt), 2, 1, None, None, None, None, None, None) == UNSUPPORTED
    assert Lb.slam_last_merge_work(u.h, None, None, None) == STATE
    assert _raw(u, tmp_path) == before
    u.close()
    e = S.BatchedEKF(n, L).readParams()
    assert Lb.slam_map_merge(e.h, None, None, None) == Lb.slam_map_prune(e.h, None, None, None) == STATE and "slam_init" in err()
    e.set_map(lm); e.init(0.0, 0.0, 0.0)
    e.run_sim(sim_cmds)
    e.track_instance(2)
    assert Lb.slam_map_merge(e.h, None, None, None) == STATE and "slam_track_instance" in err()
    assert Lb.slam_map_duplicates(e.h, None, ip(partner), None) == STATE and Lb.slam_merge_landmarks(e.h, None, ip(partner), None, None) == STATE
    e.track_instance(-1)
    before = _raw(e, tmp_path)
    r = e.map_merge()                                                # a simulated map has no duplicates: nothing is written
    assert not r["n_merged"].any() and not r["rec"][:2].any() and _raw(e, tmp_path) == before
    e.close()
