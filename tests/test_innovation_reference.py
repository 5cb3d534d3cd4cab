"""The per-instance function of the innovation kernel, compiled for the host (slam_innovation_instance_host: the kernel's own source),
against the CPU oracle and against restatements, without a GPU:
  * on states of the golden measurement streams, both storage types: `post`, rounded to float for fp32 storage, equals the oracle's
    x_t[:3] and P_t[:3, :3] after orc_ekf_update IN BITS, for every step evaluated;
  * the first update of each of those messages against the dense numpy restatement of ekf.cpp:110-135: nu in bits,
    |dS_ij| <= 16 * 2^-53 * (|H_i| |P| |H_j|^T + W_ij);
  * every update slot's nis against nu^T S^-1 nu in np.longdouble from the reported nu and S: 16 kappa_2(S) 2^-53 relative;
  * the crafted messages (innovation_reference.crafted_cases): flags, counts, NaN patterns, and `post` against the oracle in bits."""
import numpy as np
import pytest

import innovation_reference as IR


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("name,every", IR.STREAMS)
def test_post_equals_the_oracle_in_bits_on_the_golden_streams(oracle, name, every, f32):
    steps = updates = firsts = 0
    for t, before, cmd, meas, after, fl, cfg, L in IR.stream_states(oracle, name, every, f32):
        assert fl == 0, (t, fl)
        r = IR.hook(before, cmd, meas, cfg, L, f32)
        assert r["flags"] == 0, (t, r["flags"])
        assert IR.bits(IR.post_as_stored(r["post"], f32)) == IR.bits(IR.oracle_post(after)), (t, r["post"], IR.oracle_post(after))
        known = [int(m[0]) in before["ids"].tolist() for m in meas]
        assert r["n_upd"] == sum(known) and r["n_new"] == len(meas) - sum(known) and r["n_new"] == after["M"] - before["M"], t
        k = len(meas)
        for l in range(IR.MAX_DET):
            assert np.isnan(r["det"][l]).all() == (l >= k or not known[l]) and np.isnan(r["det"][l]).any() == np.isnan(r["det"][l]).all(), (t, l)
        assert IR.check_nis_slots(r["det"], k) == r["n_upd"]
        fin = [r["det"][l, 0] for l in range(k) if known[l]]
        acc = 0.0
        for v in fin:
            acc = acc + v
        assert IR.bits(r["nis_sum"]) == IR.bits(acc), t
        assert all(v > 0 for v in fin)
        if known and known[0]:   # the chain has not started: the dense restatement applies to slot 0
            nu, S, A = IR.dense_first_update(oracle, before, cmd, meas[0], IR.effective_noise(cfg), f32)
            assert IR.bits(nu) == IR.bits(r["det"][0, 1:3]), (t, nu, r["det"][0])
            got = np.array([[r["det"][0, 3], r["det"][0, 4]], [r["det"][0, 4], r["det"][0, 5]]])
            assert np.all(np.abs(got - S) <= 16 * IR.EPS * A), (t, got - S, 16 * IR.EPS * A)
            firsts += 1
        steps += 1; updates += r["n_upd"]
    print(f"{name} {'f32' if f32 else 'f64'}: {steps} steps, {updates} updates, {firsts} first updates against the dense restatement")
    assert steps >= 30 and updates >= 20 and firsts >= 10


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_crafted_messages(oracle, f32):
    L_max = IR.MAX_LM + 4
    cmd = np.array([0.08, -0.03], dtype=np.float32)
    seen = set()
    for case in IR.crafted_cases(77, L_max, f32):
        cfg = IR.config_for(case["noise"])
        noise = IR.effective_noise(cfg)
        r = IR.hook(case["st"], cmd, case["meas"], cfg, L_max, f32, status=case["status"], noise=noise)
        name = case["name"]
        assert r["flags"] == case["flags"], (name, r["flags"])
        assert r["n_upd"] == case["n_upd"] and r["n_new"] == case["n_new"], (name, r["n_upd"], r["n_new"])
        seen.add(r["flags"])
        k = min(len(case["meas"]), IR.MAX_DET)
        if case["flags"] & (IR.FROZEN | IR.WOULD_FREEZE | IR.TOO_LONG):
            assert np.isnan(r["nis_sum"]) and np.isnan(r["post"]).all() and np.isnan(r["det"]).all(), name
            assert r["rec"][[1, 3, 2][[IR.FROZEN, IR.WOULD_FREEZE, IR.TOO_LONG].index(case["flags"])]] == 1.0 and r["rec"].sum() == 1.0, name
            if case["flags"] == IR.WOULD_FREEZE:
                _, fl = IR.oracle_step(oracle, case["st"], cmd, case["meas"], cfg, L_max, f32)
                assert fl & IR.INST_INDEX_OOR, name
            continue
        assert r["rec"][0] == 1.0 and r["rec"][6] == r["n_new"] and r["rec"][15] == 0.0, name
        if case["status"] & IR.INST_INDEX_OOR == 0:
            after, fl = IR.oracle_step(oracle, case["st"], cmd, case["meas"], cfg, L_max, f32)
            assert not fl & IR.INST_INDEX_OOR, name
            assert bool(fl & IR.INST_S_SINGULAR) == bool(r["flags"] & IR.S_SINGULAR), (name, fl)
            want, got = IR.oracle_post(after), IR.post_as_stored(r["post"], f32)
            if case["flags"] & IR.S_SINGULAR:   # 0 / 0 in the pivot: NaN from there on, on both sides (the sign of a NaN is not compared)
                assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any(), (name, got, want)
                assert np.isnan(r["det"][0, 0]) and r["det"][0, 3] == 0.0 and r["det"][0, 5] == 0.01 and r["nis_sum"] == 0.0 and r["rec"][4] == 1.0
                assert r["rec"][5] == 0.0
                continue
            assert IR.bits(got) == IR.bits(want), (name, got, want)
            assert after["M"] - case["st"]["M"] == (0 if case["st"]["M"] == L_max else r["n_new"]), name
        upd = [l for l in range(k) if not np.isnan(r["det"][l, 0])]
        assert len(upd) == r["n_upd"] == IR.check_nis_slots(r["det"], k) == r["rec"][5], name
        assert all(np.isnan(r["det"][l]).all() for l in range(IR.MAX_DET) if l not in upd), name
        s = 0.0
        for l in upd:
            s = s + r["det"][l, 0]
        assert IR.bits(s) == IR.bits(r["nis_sum"]) == IR.bits(r["rec"][7]), name
        assert r["rec"][8] == (max(r["det"][l, 0] for l in upd) if upd else 0.0), name
    assert seen == {0, IR.FROZEN, IR.WOULD_FREEZE, IR.S_SINGULAR, IR.TOO_LONG}


def test_the_quirk_switch_reads_the_landmark_from_x_pred(oracle):
    """ekf_landmark_from_x_pred: the second update of one landmark sees the position the first one left; bits against the oracle."""
    rng = np.random.default_rng(5)
    st = IR.synthetic_state(rng, 4)
    meas = np.array([IR.detection(rng, st, 1), IR.detection(rng, st, 1), IR.detection(rng, st, 3)], dtype=np.float32)
    cmd = np.array([0.05, 0.02], dtype=np.float32)
    posts = []
    for quirk in (0, 1):
        cfg = IR.config_for(None)
        cfg.ekf_landmark_from_x_pred = quirk
        r = IR.hook(st, cmd, meas, cfg, 8)
        after, fl = IR.oracle_step(oracle, st, cmd, meas, cfg, 8)
        assert fl == 0 and r["flags"] == 0 and IR.bits(r["post"]) == IR.bits(IR.oracle_post(after)), quirk
        posts.append(r["det"].copy())
    assert IR.bits(posts[0][0]) == IR.bits(posts[1][0]) and IR.bits(posts[0][1]) != IR.bits(posts[1][1])


def test_the_record_band_counts(oracle):
    from live_ekf_slam_amd.config import InnovationConfig
    from live_ekf_slam_amd.filters import innovation_instance_host
    rng = np.random.default_rng(6)
    st = IR.synthetic_state(rng, 6)
    meas = np.array([IR.detection(rng, st, j) for j in range(6)], dtype=np.float32)
    cfg = IR.config_for(None)
    cmd = np.array([0.05, 0.02], dtype=np.float32)
    base = IR.hook(st, cmd, meas, cfg, 8)
    nis = np.sort(base["det"][:6, 0])
    lo, hi = 0.5 * (nis[1] + nis[2]), 0.5 * (nis[4] + nis[5])
    r = innovation_instance_host(st["x"], st["P"], st["ids"], 8, 0, cmd, meas, IR.effective_noise(cfg), cfg=InnovationConfig(lo, hi))
    assert r["rec"][9] == 2.0 and r["rec"][10] == 1.0 and r["rec"][5] == 6.0
    nu = base["det"][:6, 1:3]
    for col, (i, sq) in zip((11, 12, 13, 14), ((0, False), (1, False), (0, True), (1, True))):
        s = 0.0
        for l in range(6):
            s = s + (nu[l, i] * nu[l, i] if sq else nu[l, i])
        assert IR.bits(s) == IR.bits(r["rec"][col]), col
