"""The composed reference of tests/edit_walk.py checked without a GPU:
  (a) with no edits the walker reproduces oracle.run_ekf_batch in bits (x, P, M, ids, flags, truth, avg_err): this pins its timestep /
      RNG-step convention and its error statistic;
  (b) the same program walked a second time with every edit done by the library's host hooks (map_instance_host, merge_instance_host)
      gives the same bits at every edit and at the end;
  (c) every fixed program of tests/test_run_after_map_edit_gpu.py meets that test's preconditions, from the walker alone: more than half
      of the instances have at least 10 update-only ticks of 1 to 6 detections in the run segments after every edit, a tick that inserts a
      removed id again, a prune that drops something, a prune that drops a withheld slot and a fused pair; M is ragged after every edit; no flag is raised; the margins of
      map_reference.check_margins and merge_reference.check_margins hold (the walker asserts them as it goes)."""
import numpy as np
import pytest

import edit_walk as EW


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    return S


# ---- (a) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("L_max,f32", [(20, False), (20, True), (50, False), (50, True)], ids=["L20_f64", "L20_f32", "L50_f64", "L50_f32"])
def test_without_edits_the_walker_is_the_oracles_batch_run(S, oracle, L_max, f32, each):
    O = oracle
    B, T, seed, inst0 = 4, 60, 77, 300
    lm = EW.make_maps(np.random.default_rng(L_max), 1, L_max - 3, 0)[0]     # (the reference's default config, quirk and all)
    cmds = EW.drive_commands(T)
    cfg = S.default_config()
    rows = S.config.noise_rows(cfg, B)
    setup = EW.Setup(cfg, rows, np.tile(lm, (B, 1, 1)), L_max, f32, seed, inst0)
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    rng = np.random.default_rng(5)
    per = (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)
    grew = 0
    for b in range(B):
        c = per[:, b] if each else cmds
        r = O.run_ekf_batch(lm, c, 1, L_max, seed=seed, inst0=inst0 + b, cfg=cfg, mode=mode)
        w = EW.walk(O, setup, [("run", per if each else cmds)], b)["final"]
        M = int(r["M"][0]); n = 3 + 2 * M
        want = dict(x=r["x"][0, :n], P=r["P"][0, :n * n].reshape(n, n), ids=r["ids"][0, :M], M=M, flags=int(r["flags"][0]), timestep=T, truth=r["truth"][0],
                    avg_err=r["avg_err"][0])
        assert EW.same_snapshot(w, want, counters=False) == [], (b, EW.same_snapshot(w, want, counters=False))
        grew += M > 3
    assert grew == B, "every instance mapped something"


# ---- (b) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L20_f64", "L20_f32", "L50_f32", "L20_f64_unknown_ids"])
def test_edits_by_the_reference_and_by_the_host_hooks_give_the_same_bits(S, oracle, name):
    setup, program, walks, _ = EW.fixed_case(oracle, S, name)
    edited = 0
    for b in range(0, setup.B, 4):
        h = EW.walk(oracle, setup, program, b, hooks=S)
        w = walks[b]
        assert len(h["after"]) == len(w["after"]) > 0
        for i, (u, v) in enumerate(zip(h["after"], w["after"])):
            assert EW.same_snapshot(u, v) == [], (name, b, "edit", i, w["edits"][i]["kind"], EW.same_snapshot(u, v))
        assert EW.same_snapshot(h["final"], w["final"]) == [], (name, b, EW.same_snapshot(h["final"], w["final"]))
        edited += sum(e["M_after"] < e["M"] for e in w["edits"])
    assert edited > setup.B // 4


# ---- (c) -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(EW.CASES))
def test_every_fixed_program_meets_the_preconditions_of_the_gpu_test(S, oracle, name):
    setup, program, walks, pre = EW.fixed_case(oracle, S, name)      # (preconditions() has asserted; the counts for the record)
    print(name, pre)
    B = setup.B
    assert pre["update_only"] > B // 2 and pre["reinsert"] > B // 2 and pre["instances"] == B
    assert sum(e["M_after"] < e["M"] for w in walks for e in w["edits"] if e["kind"] == "prune") > B // 2, "the prune removes something"
    if "merge" in [op[0] for op in program]:
        assert pre["withheld"] > B // 2 and pre["fused"] > B // 2
        second = sum(w["edits"][-1]["fused"] > 0 for w in walks)
        assert second > B // 2, "the dropped id came back and the second merge found a pair again"
    masks = next(op[1] for op in program if op[0] == "remove")
    Ms = [w["edits"][0]["M"] for w in walks]
    kinds = {("all" if M and masks[b, :M].all() else "slot 0" if M and masks[b, 0] and not masks[b, 1:M].any() else
              "a single survivor" if M > 1 and masks[b, :M].sum() == M - 1 else "other") for b, M in enumerate(Ms)}
    assert {"all", "slot 0", "a single survivor"} <= kinds, kinds
