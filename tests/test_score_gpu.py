"""slam_map_score on the MI355X.  The matching, the per-landmark values and the record against the host hook
(slam_map_score_instance_host, the kernel's own source on the host; tests/test_score_reference.py holds the hook to an independent numpy
reference) bit for bit, at every M of both LDS classes, at the lane wraps of the larger classes and at the capacity; nees_matched against
slam_consistency in bits where the matching is the identity, and against the longdouble reference of tests/consistency_reference.py on the
selected sub-block (that module's own rule, MARGIN and CAP) where it is a proper subset; a real id-less run; and the promises of the header.
States are crafted through checkpoint files as tests/test_consistency_gpu.py does."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import consistency_reference as CR
import score_reference as R
from conftest import ROOT
from record_tree import fixed_order_record
from test_consistency_gpu import _load

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _dt(S, f32):
    return S.F32 if f32 else S.F64


def _against_the_hook(f, insts, maps, radius, f32, full=1, label=""):
    """The device's outputs of every instance against the hook on the crafted state (rounded to the storage type), and the record against
    the fixed-order tree over the per-instance contributions.  maps: one map, or one per instance.  Returns the device's outputs."""
    cfg = R.config(radius, full=full)
    d = R.device_score(f, cfg)
    status = f.status()
    recs, wrong = [], []
    for b, it in enumerate(insts):
        m = maps[b] if isinstance(maps, list) else maps
        rc, h = R.host_hook(it["x"], it["P"], it["M"], f.L_max, int(status[b]), it["truth"], m, cfg, f32)
        assert rc == 0 and int(status[b]) == it["status"]
        got = {k: d[k][b] for k in R.BITWISE}
        got["flags"] = got["flags"] & ~R.MATCHED_NOT_PD   # (the factorisation's bit: the hook does not factor; its NaN pattern is checked below)
        bad = R.differences(got, h)
        if bad:
            wrong.append((b, it["M"], bad))
        failed = bool(h["flags"] & R.INSTANCE_FAILED)
        want_dof = 0 if (failed or not full) else 3 + 2 * h["n_matched"]
        if d["dof_matched"][b] != want_dof or (not full and not np.isnan(d["nees_matched"][b])) or (failed and not np.isnan(d["nees_matched"][b])):
            wrong.append((b, it["M"], "dof_matched / nees_matched", int(d["dof_matched"][b]), want_dof, float(d["nees_matched"][b])))
        if np.isnan(d["nees_matched"][b]) != bool(failed or not full or (d["flags"][b] & R.MATCHED_NOT_PD)):
            wrong.append((b, it["M"], "NaN pattern of nees_matched", float(d["nees_matched"][b]), int(d["flags"][b])))
        ref = R.reference(it["x"], it["P"], it["M"], f.L_max, it["status"], it["truth"], m, radius, f32=f32)
        recs.append(R.instance_record(ref, d["nees_matched"][b], int(d["dof_matched"][b])))
    assert not wrong, f"{label}: {len(wrong)} instance(s) differ from the hook: {wrong[:10]}"
    want = fixed_order_record(np.array(recs), R.MAX_ENTRY_7)
    assert R.same_bits(d["rec"], want), (label, d["rec"], want)
    assert d["rec"][0] + d["rec"][1] == len(insts)
    return d


# ---- 1. device against the host hook ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", [20, 50])
def test_every_size_and_every_edge_against_the_hook(S, L_max, f32, tmp_path):
    rng = np.random.default_rng(900 + L_max)
    m = R.grid_map(L_max)
    insts = [R.make(rng, M, m, {int(j): m[rng.integers(L_max)] + (2.0, 2.0) for j in rng.choice(M, M // 4, replace=False)}) for M in range(L_max + 1)]
    edges = R.edge_cases(rng, L_max, m)
    insts += list(edges.values())
    order = rng.permutation(len(insts))
    insts = [insts[i] for i in order]
    f = _load(S, L_max, _dt(S, f32), insts, m, tmp_path)
    d = _against_the_hook(f, insts, m, R.RADIUS, f32, full=1, label="radius")
    assert d["rec"][1] == 3 and d["rec"][5] > 0 and d["rec"][4] > 0 and (d["flags"] & R.LM_NOT_PD).sum() >= 1
    di = _against_the_hook(f, insts, m, math.inf, f32, full=0, label="inf")
    assert di["rec"][5] == 3 and di["rec"][12] == 0      # only the three slots with NaN / inf coordinates are left SPURIOUS
    d2 = R.device_score(f, R.config(R.RADIUS, full=1))
    assert all(R.same_bits(d[k], d2[k]) for k in d), "a second call gives other bits"
    # a radius whose square underflows to 0 is legal: only d2 == 0 is inside, on the device as in the hook
    dz = _against_the_hook(f, insts, m, 1e-200, f32, full=0, label="radius^2 = 0")
    assert dz["rec"][3] == 0 and dz["rec"][5] == dz["rec"][2] > 0
    # NaN has one bit pattern in the call's outputs, whatever produced it (full = 0, a failed instance, a slot without a value)
    quiet = np.array([np.nan]).view(np.uint64)[0]
    for res in (d, di):
        for k in ("nees_matched", "map_rms", "max_err", "lm_err", "lm_nees"):
            v = np.ascontiguousarray(res[k]).ravel()
            assert np.all(v.view(np.uint64)[np.isnan(v)] == quiet), k
    f.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_every_edge_with_maps_of_one_row_fewer_rows_than_slots_and_more_than_the_capacity(S, f32, tmp_path):
    L_max = 20
    rng = np.random.default_rng(950)
    maps, insts = [], []
    for L in (1, 9, L_max - 1, L_max + 7):               # (the edge cases place slots at rows up to 8: they need 9 rows; L = 1 takes the plain states)
        m = R.grid_map(L)
        states = [R.make(rng, M, m, {}) for M in (0, 1, 2, L_max - 1, L_max)]
        if L >= 9:
            states += list(R.edge_cases(rng, L_max, m).values())
        for s in states:
            maps.append(m); insts.append(s)
    assert any(m.shape[0] == 1 and s["M"] > 1 for m, s in zip(maps, insts)) and any(m.shape[0] == s["M"] - 1 for m, s in zip(maps, insts))
    f = _load(S, L_max, _dt(S, f32), insts, maps[0], tmp_path)
    f.set_map(maps)
    d = _against_the_hook(f, insts, maps, R.RADIUS, f32, full=1, label="L_each in {1, 9, L_max - 1, L_max + 7}")
    one = [b for b, m in enumerate(maps) if m.shape[0] == 1 and insts[b]["M"] > 0]
    assert np.all(d["n_matched"][one] <= 1) and np.all(d["row"][one].max(axis=1) <= 0)
    _against_the_hook(f, insts, maps, math.inf, f32, full=1, label="L_each, infinite radius")
    f.close()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_lane_wraps_at_200_landmarks_with_shared_and_per_instance_maps(S, f32, tmp_path):
    L_max = 200
    Ms, Ls = (63, 64, 65, 127, 128, 129, 200), (63, 64, 65, 129, 250)
    rng = np.random.default_rng(1200)
    for L in (63, 250):                                   # a shared map smaller than M and larger than L_max
        m = R.grid_map(L)
        insts = [R.make(rng, M, m, {int(j): m[rng.integers(L)] + (2.0, 2.0) for j in rng.choice(M, M // 5, replace=False)}) for M in Ms]
        f = _load(S, L_max, _dt(S, f32), insts, m, tmp_path, f"s{L}")
        _against_the_hook(f, insts, m, R.RADIUS, f32, full=1, label=f"shared L={L}")
        f.close()
    maps, insts = [], []
    for M in Ms:                                          # every M with every map size, one map per instance (differing L_each)
        for L in Ls:
            m = R.grid_map(L) + rng.integers(-2, 3, 2) * 4.0
            maps.append(m)
            insts.append(R.make(rng, M, m, {int(j): m[rng.integers(L)] + (2.0, 2.0) for j in rng.choice(M, M // 5, replace=False)}))
    f = _load(S, L_max, _dt(S, f32), insts, maps[0], tmp_path, "each")
    f.set_map(maps)
    d = _against_the_hook(f, insts, maps, R.RADIUS, f32, full=1, label="per-instance maps")
    assert d["rec"][12] == len(insts)
    f.close()


def test_the_capacity_of_1000_landmarks_once(S, tmp_path):
    L_max = 1000
    rng = np.random.default_rng(1300)
    m = R.grid_map(1000)
    insts = [R.make(rng, M, m, {int(j): m[rng.integers(1000)] + (2.0, 2.0) for j in rng.choice(M, 100, replace=False)}) for M in (999, 1000)]
    f = _load(S, L_max, S.F64, insts, m, tmp_path)
    d = _against_the_hook(f, insts, m, R.RADIUS, False, full=1, label="L_max = 1000")
    assert np.all(d["n_spurious"] == 100) and np.all(np.isfinite(d["nees_matched"])) and np.all(d["nees_matched"] > 0)
    by, ms = R.last_score_work(f)
    print(f"[score] L_max=1000, M=999 and 1000, full = 1: {ms:.1f} ms on the device, model {by / 1e6:.2f} MB")
    f.close()


# ---- 2. identity matching equals slam_consistency in bits -------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", [20, 50, 60, 200])
def test_identity_matching_has_the_bits_of_slam_consistency(S, L_max, f32, tmp_path):
    rng = np.random.default_rng(2000 + L_max)
    m = R.grid_map(L_max)                                 # least separation 4; the perturbations stay below 0.3 in each coordinate
    insts = []
    for M in sorted(set([0, 1, 2, L_max // 2, L_max - 1, L_max] * 2)) + [L_max] * 3:
        it = R.make(rng, M, m, {})
        ids = rng.permutation(L_max)[:M].astype(np.int32)
        it["ids"] = ids
        it["x"][3:] = (m[ids] + rng.uniform(-0.3, 0.3, (M, 2))).ravel()
        insts.append(it)
    for it in insts:                                      # the premise, on the host: every slot is MATCHED to the row of its id
        rc, h = R.host_hook(it["x"], it["P"], it["M"], L_max, 0, it["truth"], m, None, f32)
        assert rc == 0 and np.array_equal(h["row"][:it["M"]], it["ids"]) and np.all(h["role"][:it["M"]] == R.MATCHED) and h["flags"] == 0
    f = _load(S, L_max, _dt(S, f32), insts, m, tmp_path)
    c = f.consistency()
    d = R.device_score(f, R.config(full=1))
    assert not c["flags"].any() and not d["flags"].any() and np.array_equal(d["n_matched"], [it["M"] for it in insts])
    assert R.same_bits(d["nees_matched"], c["nees_full"]) and R.same_bits(d["map_rms"], c["map_rms"]) and np.array_equal(d["dof_matched"], c["dof"])
    assert np.all(np.isfinite(d["nees_matched"])) and np.all(d["nees_matched"] > 0)
    f.close()


# ---- 3. a proper subset ---------------------------------------------------------------------------------------------------------------------------
def _subset_state(rng, M, m, L_max):
    """MATCHED slots interleaved with DUPLICATE (a second slot at a row already taken, farther) and SPURIOUS ones."""
    rows = rng.permutation(m.shape[0])
    slots, taken = {}, []
    for j in range(M):
        kind = j % 3 if j > 0 else 0
        if kind == 0 or not taken:
            r = int(rows[len(taken)]); taken.append(r)
            slots[j] = m[r] + rng.uniform(-0.2, 0.2, 2)
        elif kind == 1:
            slots[j] = m[taken[rng.integers(len(taken))]] + rng.uniform(0.5, 0.9, 2) * rng.choice([-1.0, 1.0], 2)
        else:
            slots[j] = m[rng.integers(m.shape[0])] + (2.0, 2.0)
    return R.make(rng, M, m, slots)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", [20, 50, 60])
def test_a_proper_subset_against_the_longdouble_reference(S, L_max, f32, tmp_path):
    rng = np.random.default_rng(3000 + L_max)
    m = R.grid_map(L_max)
    insts = [_subset_state(rng, int(M), m, L_max) for M in rng.integers(3, L_max + 1, 36)] + [_subset_state(rng, L_max, m, L_max) for _ in range(4)]
    f = _load(S, L_max, _dt(S, f32), insts, m, tmp_path)
    d = _against_the_hook(f, insts, m, R.RADIUS, f32, full=1, label="subset")
    assert not d["flags"].any() and np.all(d["n_duplicate"][[it["M"] >= 3 for it in insts]] > 0) and np.all(d["n_spurious"] > 0)
    pool = []
    for b, it in enumerate(insts):
        sel = np.flatnonzero(d["role"][b] == R.MATCHED)
        assert 0 < sel.size < it["M"] and d["dof_matched"][b] == 3 + 2 * sel.size
        xs, Ps, ids = R.selected_state(R.stored(it["x"], f32), R.stored(it["P"], f32), it["M"], sel, d["row"][b][sel])
        r = CR.reference(xs, Ps, sel.size, ids, it["truth"], m)
        assert r["flags"] == 0 and r["dof"] == d["dof_matched"][b]
        assert abs(d["map_rms"][b] - float(r["map_rms"])) <= CR.map_rms_bound(sel.size) * float(r["map_rms"])
        pool.append((d["nees_matched"][b], r["nees_full"], r["S"], r["e"], r["z_full"]))
    G, gd, bar, over = CR.judge(pool)
    print(f"[score] subset L_max={L_max} {'f32' if f32 else 'f64'}: {len(pool)} instances, G = {G:.3g}, device max g = {gd:.3g}, bar = {bar:.3g}")
    assert not over, (len(over), gd, bar)
    f.close()


@pytest.mark.parametrize("L_max", [20, 60])
def test_not_pd_inside_and_outside_the_selection(S, L_max, tmp_path):
    rng = np.random.default_rng(3500 + L_max)
    m = R.grid_map(L_max)
    base = _subset_state(rng, 9, m, L_max)                # slots 0, 3, 6 MATCHED, 1, 4, 7 DUPLICATE, 2, 5, 8 SPURIOUS
    insts = []
    for slot in (None, 3, 4, 5):
        it = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        if slot is not None:
            it["P"][3 + 2 * slot, 3 + 2 * slot] = -1e-3
        insts.append(it)
    f = _load(S, L_max, S.F64, insts, m, tmp_path)
    d = _against_the_hook(f, insts, m, R.RADIUS, False, full=1, label="not PD")
    assert [int(r) for r in d["role"][0][:9]] == [R.MATCHED, R.DUPLICATE, R.SPURIOUS] * 3
    # a MATCHED slot: both bits, nees_matched NaN; a DUPLICATE slot: its own lm_nees only; a SPURIOUS slot: nothing at all
    assert list(d["flags"]) == [0, R.MATCHED_NOT_PD | R.LM_NOT_PD, R.LM_NOT_PD, 0]
    assert np.isnan(d["nees_matched"][1]) and np.all(np.isfinite(d["nees_matched"][[0, 2, 3]]))
    assert R.same_bits(d["nees_matched"][[2, 3]], d["nees_matched"][[0, 0]]), "an unselected row reached the factorisation"
    assert np.isnan(d["lm_nees"][2][4]) and np.isfinite(d["lm_nees"][3][:9][[0, 1, 3, 4, 6, 7]]).all()
    f.close()


# ---- 4. a real id-less run -------------------------------------------------------------------------------------------------------------------
def _hook_on_the_state(f, d, maps, cfg, only=None):
    status, truth = f.status(), f.truth()
    wrong = []
    for b in (range(f.batch) if only is None else only):
        st = f.get_state(b)
        m = maps[b] if isinstance(maps, list) else maps
        rc, h = R.host_hook(st["x"], st["P"], st["M"], f.L_max, int(status[b]), truth[b], m, cfg)
        assert rc == 0
        got = {k: d[k][b] for k in R.BITWISE}
        got["flags"] = got["flags"] & ~R.MATCHED_NOT_PD
        bad = R.differences(got, h)
        if bad:
            wrong.append((b, st["M"], bad))
    assert not wrong, wrong[:10]


def test_a_real_idless_run_with_clutter(S):
    from live_ekf_slam_amd.config import noise_rows
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = 20, 256, 300, 16
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = noise_rows(cfg, B, V_00=cfg.V_00 ** 2 / 3, V_11=cfg.V_11 ** 2 / 3, W_00=cfg.W_00 ** 2 / 3, W_11=cfg.W_11 ** 2 / 3)
    sensor = (S.SensorConfig * B)(*[S.default_sensor_config(p_spike=0.05 * (b % 4), spike_lo=0.5, spike_hi=2.0, p_clutter=0.2 * (b % 3), n_clutter=2,
                                                            clutter_r_min=0.3, shuffle=1, erase_ids=1) for b in range(B)])
    f = S.BatchedEKF(B, 2 * L).readParams(cfg)
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows); f.set_sensor(sensor)
    f.manage_merge_run_sim(cmds, series=False, log=False, k_stride=ks)
    cfg_s = R.config(0.5, full=1)
    d = R.device_score(f, cfg_s)
    M = f.landmark_counts()
    # no instance fails: the status carries no NONFINITE / WATCHDOG bit and every pose is finite, so the roles of every instance add up to M
    assert not (f.status() & (R.NONFINITE | R.WATCHDOG)).any() and np.all(np.isfinite(f.poses()))
    assert not (d["flags"] & R.INSTANCE_FAILED).any() and np.array_equal(d["n_matched"] + d["n_duplicate"] + d["n_spurious"], M) and M.max() > 0
    _hook_on_the_state(f, d, lm, cfg_s)
    fin = np.isfinite(d["nees_matched"])
    assert fin.sum() >= B // 2 and np.array_equal(d["dof_matched"][fin], 3 + 2 * d["n_matched"][fin])
    print(f"[score] id-less run L={L} B={B} T={T}: per instance matched {d['n_matched'].mean():.2f}, duplicate {d['n_duplicate'].mean():.2f}, "
          f"spurious {d['n_spurious'].mean():.2f} of {M.mean():.2f} held; map rms {np.nanmean(d['map_rms']):.4f} m; mean lm_nees "
          f"{d['rec'][9] / max(d['rec'][8], 1):.3f}; nees_matched / dof {np.nanmean(d['nees_matched'][fin] / d['dof_matched'][fin]):.3f}")
    f.close()
    # unknown ids inside the step (landmark_id_is_known = 0): slam_consistency has no landmark truth, the score does
    cfg.landmark_id_is_known = 0
    g = S.BatchedEKF(B, L).readParams(cfg)
    g.set_map(lm); g.set_seed(7); g.init(0.0, 0.0, 0.0)
    g.run_sim(cmds[:200])
    Mg = g.landmark_counts()
    dg = R.device_score(g, R.config(0.5, full=1))
    c = g.consistency()
    assert (Mg > 0).all() and np.all(c["flags"] == CR.NO_TRUTH) and np.all(np.isnan(c["nees_full"])) and np.all(np.isnan(c["map_rms"]))
    assert not dg["flags"].any() and np.array_equal(dg["n_matched"] + dg["n_duplicate"] + dg["n_spurious"], Mg) and np.all(np.isfinite(dg["nees_matched"]))
    _hook_on_the_state(g, dg, lm, R.config(0.5, full=1), only=range(0, B, 8))
    g.close()


# ---- 5. promises ----------------------------------------------------------------------------------------------------------------------------------
def _run(S, B, offset=0, L=20, T=120, dtype=None):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, T)
    f = S.BatchedEKF(B, L, dtype=S.F64 if dtype is None else dtype).readParams()
    f.set_seed(11); f.set_instance_offset(offset); f.set_map(lm); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds)
    return f, lm


def _per_instance(d):
    return {k: v for k, v in d.items() if k != "rec"}


def test_nothing_moves_and_the_batch_does_not_matter(S, tmp_path):
    f, lm = _run(S, 17, offset=100)
    before = tmp_path / "before.ckpt"; after = tmp_path / "after.ckpt"
    f.save_state(before)
    d = R.device_score(f, R.config(0.4, full=1))
    f.save_state(after)
    assert open(before, "rb").read() == open(after, "rb").read(), "the call changed the state"
    assert all(R.same_bits(v, R.device_score(f, R.config(0.4, full=1))[k]) for k, v in d.items()), "a second call gives other bits"
    assert not d["flags"].any() and d["n_matched"].min() > 0
    g, _ = _run(S, 300)                                   # the same 17 global instances at offset 100 of a batch of 300
    dg = R.device_score(g, R.config(0.4, full=1))
    for k, v in _per_instance(d).items():
        assert R.same_bits(v, dg[k][100:117]), k
    f.close(); g.close()


def test_chunks_of_the_workspace_class(S, tmp_path, monkeypatch):
    L_max = 60
    rng = np.random.default_rng(5060)
    m = R.grid_map(L_max)
    insts = [_subset_state(rng, int(M), m, L_max) for M in (60, 51, 7, 33, 60, 1, 0)]
    f = _load(S, L_max, S.F64, insts, m, tmp_path)
    monkeypatch.delenv("SLAM_CONSISTENCY_WS_BYTES", raising=False)
    d = _against_the_hook(f, insts, m, R.RADIUS, False, full=1, label="unchunked")
    per = 8 * (3 + 2 * L_max + 1) * (3 + 2 * L_max + 2) // 2
    for budget in (1, 3 * per):                           # chunks of 1 and of 3 instances
        monkeypatch.setenv("SLAM_CONSISTENCY_WS_BYTES", str(budget))
        dc = R.device_score(f, R.config(R.RADIUS, full=1))
        assert all(R.same_bits(d[k], dc[k]) for k in d), budget
    monkeypatch.delenv("SLAM_CONSISTENCY_WS_BYTES")
    f.close()


def test_null_outputs_errors_and_the_work_model(S):
    from live_ekf_slam_amd import _lib
    L = _lib.lib()
    f = S.BatchedEKF(4, 20).readParams()
    none = [None] * 13
    assert L.slam_map_score(f.h, None, *none) == -4 and "slam_init" in L.slam_last_error().decode()
    f.init(0.0, 0.0, 0.0)
    assert L.slam_map_score(f.h, None, *none) == -4 and "slam_set_map" in L.slam_last_error().decode()
    assert L.slam_last_score_work(f.h, None, None) == -4
    f.set_map(np.array([[2.0, 1.0], [-3.0, 2.0], [4.0, -4.0]]))
    for _ in range(5):
        f.update_sim((0.1, 0.02))
    assert L.slam_map_score(f.h, None, *none) == 0       # every output NULL, the default config
    d = R.device_score(f)
    assert np.all(d["dof_matched"] == 0) and np.all(np.isnan(d["nees_matched"])) and d["rec"][0] == 4 and d["rec"][12] == 0
    one = R.device_score(f, None, want=("map_rms",))
    assert R.same_bits(one["map_rms"], d["map_rms"])
    by0, ms0 = R.last_score_work(f)
    R.device_score(f, R.config(full=1))
    by1, ms1 = R.last_score_work(f)
    assert 0 < by0 < by1 and ms0 > 0 and ms1 > 0
    M = f.landmark_counts()
    esz, Lm = 8, 20                                       # full = 0 reads x, the map and the 2 x 2 diagonal blocks only: the model says exactly that
    want = sum((3 + 2 * int(M[b]) + 4 * int(d["n_matched"][b] + d["n_duplicate"][b])) * esz + 8 + 24 + 32 * Lm + 48 + 128
               + (16 * 3 if M[b] > 0 else 0) + 8 * int(d["n_matched"][b]) for b in range(4))
    assert by0 == want
    f.close()
    for u in (S.BatchedUKF(2, 20).readParams(), S.BatchedUKFLoc(2).readParams()):
        u.set_map(np.array([[2.0, 1.0], [-3.0, 2.0]])); u.init(0.0, 0.0, 0.0)
        assert L.slam_map_score(u.h, None, *none) == -3 and "EKF_SLAM only" in L.slam_last_error().decode()
        u.close()


CPP_DRIVER = r"""
#include <cstdio>
#include <cstdlib>
#include "slam_filter.hpp"
#include "slam_scenario.hpp"
using namespace slam_amd;
int main(int argc, char** argv) {
    const int B = atoi(argv[1]), L = atoi(argv[2]), T = atoi(argv[3]);
    const Scenario sc = make_scenario(1234, L, T);
    BatchedEKF ekf(B, L);
    slam_config cfg;
    slam_config_default(&cfg);
    ekf.readParams(cfg);
    ekf.init(0.f, 0.f, 0.f);
    ekf.setMap(sc.map_xy);
    if (slam_run_sim(ekf.handle(), sc.cmds.data(), T) != 0) return 2;
    slam_score_config c;
    slam_score_config_default(&c);
    c.match_radius = 0.5; c.full = 1;
    const BatchedEKF::MapScore s = ekf.mapScore(&c);
    const BatchedEKF::MapScore s0 = ekf.mapScore();
    FILE* f = std::fopen(argv[4], "wb");
    if (!f) return 3;
    std::fwrite(s.rec, 8, 16, f);
    std::fwrite(s.n_matched.data(), 4, B, f); std::fwrite(s.n_duplicate.data(), 4, B, f); std::fwrite(s.n_spurious.data(), 4, B, f);
    std::fwrite(s.map_rms.data(), 8, B, f); std::fwrite(s.max_err.data(), 8, B, f); std::fwrite(s.nees_matched.data(), 8, B, f);
    std::fwrite(s.dof_matched.data(), 4, B, f); std::fwrite(s.flags.data(), 4, B, f);
    std::fwrite(s.row.data(), 4, (size_t)B * L, f); std::fwrite(s.role.data(), 4, (size_t)B * L, f);
    std::fwrite(s.lm_err.data(), 8, (size_t)B * L, f); std::fwrite(s.lm_nees.data(), 8, (size_t)B * L, f);
    std::fwrite(s0.dof_matched.data(), 4, B, f);
    std::fclose(f);
    std::printf("driver ok: score\n");
    return 0;
}
"""


def test_cpp_mirror_gives_the_same_bytes(S, tmp_path):
    from live_ekf_slam_amd.scenario import make_scenario
    B, L, T = 8, 10, 90
    src, exe, dump = tmp_path / "score_driver.cpp", tmp_path / "score_driver", tmp_path / "score.bin"
    src.write_text(CPP_DRIVER)
    lib = os.path.join(ROOT, "live_ekf_slam_amd")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe), "-L" + lib, "-lslam_hip",
                           "-Wl,-rpath," + lib])
    out = subprocess.run([str(exe), str(B), str(L), str(T), str(dump)], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "driver ok: score" in out.stdout, out.stdout + out.stderr
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_map(lm); f.run_sim(cmds)
    d = R.device_score(f, R.config(0.5, full=1))
    order = ("rec", "n_matched", "n_duplicate", "n_spurious", "map_rms", "max_err", "nees_matched", "dof_matched", "flags", "row", "role", "lm_err", "lm_nees")
    want = b"".join(np.ascontiguousarray(d[k]).tobytes() for k in order) + np.zeros(B, np.int32).tobytes()
    assert open(dump, "rb").read() == want and d["n_matched"].min() > 0 and np.all(np.isfinite(d["nees_matched"]))
    f.close()
