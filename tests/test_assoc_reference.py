"""The per-instance function of the association kernel, compiled for the host (slam_associate_instance_host: the kernel's own source),
without a GPU, against the INDEPENDENT reference of assoc_reference (costs by the ungated innovation hook alone, decisions in plain
Python), IN BITS: the cost matrix, best and second best, slot, nu, every verdict, the labelled message, the counts and the record, on the
crafted cases of assoc_reference.crafted_cases at L_max 20 and 50 (and 70 with 66 landmarks: more than one group of 64), storage fp64 and
fp32.  Then the chain: the CPU oracle's known-id step on the labelled message appends the NEW landmarks in rank order under the ids
base + rank, and the innovation hook on the labelled message sees the MATCHED detections as updates of slot[l] at the cost d2_best."""
import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR

SHAPES = [(20, False, None), (20, True, None), (50, False, None), (50, True, None), (70, False, 66), (70, True, 66)]
IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L70_M66_f64", "L70_M66_f32"]


@pytest.fixture(scope="module")
def evaluated():
    """Every crafted case with its reference matrix, computed once per shape and shared (never modified)."""
    memo = {}

    def get(L_max, f32, M):
        key = (L_max, f32, M)
        if key not in memo:
            cases = AR.crafted_cases(1, L_max, f32, M)   # (seeds 1, 3, 4, 5 keep the margins at every shape used)
            memo[key] = [(c, ) + AR.reference_costs(c, AR.CMD, f32) for c in cases]
        return memo[key]
    return get


@pytest.mark.parametrize("L_max,f32,M", SHAPES, ids=IDS)
def test_crafted_cases_against_the_reference_in_bits(evaluated, L_max, f32, M):
    seen = set()
    names = set()
    for case, cost, nu in evaluated(L_max, f32, M):
        name = case["name"]
        names.add(name)
        ref = AR.reference_associate(case, cost, nu)
        g = AR.ahook(case, f32=f32)
        AR.check_against_reference(g, ref, name, row_in=AR.padded_row(case), cost=cost)
        AR.check_margins(case, cost, name)
        assert g["flags"] == case["flags"], name
        k = cost.shape[0]
        if case["verdicts"] is not None:
            assert g["verdict"][:k].tolist() == case["verdicts"], (name, g["verdict"][:k].tolist())
        assert not g["verdict"][k:].any() and (g["slot"][k:] == -1).all() and np.isnan(g["det"][k:]).all(), name
        seen |= set(g["verdict"].tolist())
        if "conflict" in case:      # two detections of one landmark: the lower (d2, l) wins
            a, b = case["conflict"]
            assert g["slot"][a] == g["slot"][b]
            win = a if (g["det"][a, 0], a) < (g["det"][b, 0], b) else b
            assert g["verdict"][win] == AR.MATCHED and g["verdict"][a + b - win] == AR.CONFLICT, name
        if name.startswith("an exact tie"):
            assert IR.bits(g["det"][1]) == IR.bits(g["det"][2]) and g["det"][1, 0] > 0
        if name.startswith("every mapped"):
            assert g["n_match"] == k and sorted(g["meas_out"][:k, 0].tolist()) == sorted(float(case["st"]["ids"][j]) for j in g["slot"][:k])
            assert np.isnan(case["meas"][:, 0]).any(), "the id column holds garbage and NaN: it is not read"
        if name.startswith("M = 0"):
            assert g["meas_out"][:2, 0].tolist() == [0.0, 1.0] and (g["slot"][:2] == -1).all() and np.isnan(g["det"][:2]).all()
        if name.startswith("ids near"):
            assert g["meas_out"][0, 0] == float(AR.ID_LIMIT - 1)
        if name.startswith("sentinels"):
            assert (g["meas_out"][3:] == 7.0).all() and g["count_out"] == 2 and not g["meas_out"][2].any()
        if case["flags"]:
            kin = min(max(case["meas"].shape[0] if case.get("count") is None else case["count"], 0), AR.padded_row(case).shape[0])
            assert g["count_out"] == 0 and not g["verdict"].any() and not g["meas_out"][:kin].any() and g["rec"][0] == 0.0, name
    assert seen == set(range(7)), seen
    assert len(names) >= 19


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_in_place_output(f32):
    from live_ekf_slam_amd import _lib
    import ctypes as C
    cases = [c for c in AR.crafted_cases(3, 20, f32) if c["name"] in ("updates around two new detections", "two detections of one landmark",
                                                                        "frozen status", "sentinels behind the count")]
    assert len(cases) == 4
    for case in cases:
        g = AR.ahook(case, f32=f32)
        row = AR.padded_row(case)
        buf = row.copy()
        st = case["st"]
        M = st["ids"].shape[0]
        co = C.c_int32(-1)
        cnt = case["meas"].shape[0] if case.get("count") is None else case["count"]
        d = (lambda a: a.ctypes.data_as(_lib._dp))
        rc = _lib.lib().slam_associate_instance_host(
            d(np.ascontiguousarray(st["x"])), d(np.ascontiguousarray(st["P"])), st["ids"].ctypes.data_as(_lib._ip), M, case["L_max"], case["status"],
            AR.CMD.ctypes.data_as(_lib._fp), buf.ctypes.data_as(_lib._fp), cnt, row.shape[0], C.byref(case["noise"]), 0, int(f32),
            C.byref(AR.assoc_cfg()), None, None, None, None, None, None, None, None, None, buf.ctypes.data_as(_lib._fp), C.byref(co))
        assert rc == 0 and co.value == g["count_out"] and buf.tobytes() == g["meas_out"].tobytes(), case["name"]


@pytest.mark.parametrize("L_max,f32,M", SHAPES[:4], ids=IDS[:4])
def test_the_known_id_step_consumes_the_labelled_message(oracle, evaluated, L_max, f32, M):
    chained = 0
    for case, cost, nu in evaluated(L_max, f32, M):
        if case["flags"] or case["noise"] is AR.SINGULAR_NOISE or np.isnan(case["meas"][:, 1:]).any():
            continue
        g = AR.ahook(case, f32=f32)
        name = case["name"]
        st = case["st"]
        Mst = st["ids"].shape[0]
        labelled = g["meas_out"][:g["count_out"]]
        k = cost.shape[0]
        kept = [l for l in range(k) if g["verdict"][l] in (AR.MATCHED, AR.NEW)]
        # the ungated innovation hook on the labelled message: the MATCHED are updates, the NEW insertions, nothing freezes
        u = IR.hook(st, AR.CMD, labelled, IR.config_for(case["noise"]), L_max, f32, noise=case["noise"])
        if g["n_match"] <= IR.MAX_LM:                          # (the replay of the innovation statistics holds at most MAX_LM landmarks)
            assert u["flags"] == 0 and u["n_upd"] == g["n_match"] and u["n_new"] == g["n_new"], (name, u["flags"], u["n_upd"], u["n_new"])
            for p, l in enumerate(kept):
                if g["verdict"][l] == AR.MATCHED:
                    assert labelled[p, 0] == float(st["ids"][g["slot"][l]]), (name, l)
                    assert np.isfinite(u["det"][p, 0]), (name, l, "an update slot")
                else:
                    assert np.isnan(u["det"][p, 0]), (name, l, "an insertion slot")
            if kept and g["verdict"][kept[0]] == AR.MATCHED:   # the first update sees the pre-step state: its nis is the cost, in bits
                assert IR.bits(u["det"][0, :3]) == IR.bits(g["det"][kept[0], [0, 2, 3]]), name
        else:
            assert u["flags"] == IR.TOO_LONG, name
        # the CPU oracle's step: NEW landmarks appended in rank order under base + rank
        after, fl = IR.oracle_step(oracle, st, AR.CMD, labelled, IR.config_for(case["noise"]), L_max, f32)
        assert not fl & IR.INST_INDEX_OOR, name
        base = 0 if Mst == 0 else 1 + int(st["ids"].max())
        ids_after = np.asarray(after["ids"])[:Mst + g["n_new"]].tolist()
        assert ids_after == st["ids"].tolist() + [base + r for r in range(g["n_new"])], (name, ids_after[Mst:])
        assert int(after["M"]) == Mst + g["n_new"], name
        chained += 1
    assert chained >= 12
