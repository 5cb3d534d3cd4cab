"""The per-instance function of the gate kernel, compiled for the host (slam_gate_instance_host: the kernel's own source), without a GPU:
  * gate = +inf: every output equals slam_innovation_instance_host's, bit for bit, the output message is the input, n_rej = 0;
  * the rejected set against an INDEPENDENT reference built from the ungated hook alone (gate_reference.reference_gate): the surviving
    message, each survivor's and each rejected slot's six det values, post, nis_sum and the record, bit for bit;
  * closure: the CPU oracle's step on the gated hook's output message leaves the pose and the 3 x 3 block whose bits are `post`;
  * the crafted messages (gate_reference.crafted_cases) at L_max 20 and 50, storage fp64 and fp32: the verdicts stated with each case,
    with every clean nis < gate / 2 and every spiked nis > 2 gate as the ungated hook sees them;
  * a nis equal to the gate is accepted, the next smaller gate rejects it; a singular S is never rejected."""
import numpy as np
import pytest

import gate_reference as GR
import innovation_reference as IR

SHAPES = [(20, False), (20, True), (50, False), (50, True)]
IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32"]


@pytest.mark.parametrize("L_max,f32", SHAPES, ids=IDS)
def test_an_infinite_gate_is_the_innovation_hook(L_max, f32):
    n = 0
    for case in GR.crafted_cases(31 + L_max, L_max, f32):
        for quirk in (False, True):
            g = GR.ghook(case, GR.CMD, gate=float("inf"), f32=f32, lm_from_pred=quirk)
            u = GR.uhook(case, GR.CMD, case["meas"], f32, lm_from_pred=quirk)
            name = case["name"]
            for key in ("rec", "det", "post", "nis_sum"):
                a, b = np.ravel(np.asarray(g[key], dtype=np.float64)), np.ravel(np.asarray(u[key], dtype=np.float64))
                assert not ((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))).any(), (name, key)
            assert (g["flags"], g["n_upd"], g["n_new"]) == (u["flags"], u["n_upd"], u["n_new"]), name
            k = case["meas"].shape[0]
            assert g["n_rej"] == 0 and g["count_out"] == k and g["meas_out"][:k].tobytes() == case["meas"].tobytes(), name
            assert not (g["verdict"] == GR.REJECTED).any(), name
            assert int((g["verdict"] == GR.ACCEPTED).sum()) == u["n_upd"], name
            n += 1
    assert n >= 30


@pytest.mark.parametrize("L_max,f32", SHAPES, ids=IDS)
def test_crafted_messages_against_the_reference_loop_and_the_oracle(oracle, L_max, f32):
    seen_flags, rejected, accepted = set(), 0, 0
    for case in GR.crafted_cases(77 + L_max, L_max, f32):
        name = case["name"]
        g = GR.ghook(case, GR.CMD, f32=f32)
        ref = GR.reference_gate(case, GR.CMD, f32=f32)
        assert g["flags"] == case["flags"], (name, g["flags"])
        seen_flags.add(g["flags"])
        GR.check_against_reference(g, ref, case, name)
        k = case["meas"].shape[0]
        if case["main"]:
            # the margins: no verdict of a main case hangs on rounding
            assert all(v < GR.GATE / 2 or v > 2 * GR.GATE for v in ref["nis"]), (name, sorted(ref["nis"]))
            assert g["verdict"][:k].tolist() == case["verdicts"], (name, g["verdict"][:k].tolist())
            rejected += g["n_rej"]; accepted += int((g["verdict"] == GR.ACCEPTED).sum())
        # closure: the oracle's step on the filtered message leaves `post`
        if case["status"] & IR.INST_INDEX_OOR or g["flags"] & GR.PASS:
            continue
        cfg = IR.config_for(case["noise"])
        after, fl = IR.oracle_step(oracle, case["st"], GR.CMD, g["meas_out"][:g["count_out"]], cfg, L_max, f32)
        assert not fl & IR.INST_INDEX_OOR, name
        want, got = IR.oracle_post(after), IR.post_as_stored(g["post"], f32)
        if g["flags"] & IR.S_SINGULAR:
            assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(got).any(), name
        else:
            assert IR.bits(got) == IR.bits(want), (name, got, want)
    assert seen_flags == {0, IR.FROZEN, IR.WOULD_FREEZE, IR.S_SINGULAR, IR.TOO_LONG}
    assert rejected >= 20 and accepted >= 60


def test_a_singular_slot_is_never_rejected():
    case = next(c for c in GR.crafted_cases(5, 20) if c["name"].startswith("singular"))
    g = GR.ghook(case, GR.CMD, gate=1e-300)        # the smallest of gates rejects every finite nis, and only those
    assert g["flags"] == IR.S_SINGULAR and np.isnan(g["det"][0, 0]) and g["verdict"][0] == GR.ACCEPTED
    assert g["rec"][4] == 1.0 and g["rec"][5] == 0.0
    fin = np.isfinite(g["det"][:2, 0])
    assert g["verdict"][:2].tolist() == [GR.REJECTED if f else GR.ACCEPTED for f in fin] and g["n_rej"] == int(fin.sum())
    assert g["count_out"] == 2 - g["n_rej"]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_nis_equal_to_the_gate_is_accepted(f32):
    rng = np.random.default_rng(9)
    st = IR.synthetic_state(rng, 4, f32)
    case = dict(st=st, status=0, noise=GR.NOISE, L_max=20,
                meas=np.asarray([IR.detection(rng, st, 1), IR.detection(rng, st, 3)], dtype=np.float32))
    u = GR.uhook(case, GR.CMD, case["meas"], f32)
    nis = float(max(u["det"][0, 0], u["det"][1, 0]))
    top = int(np.argmax(u["det"][:2, 0]))
    assert np.isfinite(u["det"][:2, 0]).all() and nis > 0
    at = GR.ghook(case, GR.CMD, gate=nis, f32=f32)
    assert at["verdict"][:2].tolist() == [GR.ACCEPTED, GR.ACCEPTED] and at["n_rej"] == 0 and at["count_out"] == 2
    assert IR.bits(at["post"]) == IR.bits(u["post"])
    lower = float(np.nextafter(nis, 0.0))
    below = GR.ghook(case, GR.CMD, gate=lower, f32=f32)
    assert below["verdict"][top] == GR.REJECTED and below["count_out"] == 2 - below["n_rej"]
    for gate in (nis, lower):
        GR.check_against_reference(GR.ghook(case, GR.CMD, gate=gate, f32=f32), GR.reference_gate(case, GR.CMD, gate=gate, f32=f32), case, gate)


def test_the_row_beyond_the_count_and_a_count_beyond_the_row():
    case = next(c for c in GR.crafted_cases(6, 20) if c["name"] == "the first slot rejected")
    m = case["meas"]
    k = m.shape[0]
    row = np.concatenate([m, np.full((2, 3), 7.0, np.float32)])
    g = GR.ghook(case, GR.CMD, meas=row, count=k, k_stride=k + 2)
    assert g["count_out"] == k - 1 and g["meas_out"][:k - 1].tobytes() == m[1:].tobytes()
    assert not g["meas_out"][k - 1].any() and (g["meas_out"][k:] == 7.0).all(), "zeros up to count_in, nothing written from there"
    g2 = GR.ghook(case, GR.CMD, meas=m, count=k + 3, k_stride=k)      # the count is clamped to the row, as the step clamps it
    assert g2["count_out"] == k - 1 and g2["verdict"][:k].tolist() == g["verdict"][:k].tolist()
    frozen = dict(case, status=IR.INST_INDEX_OOR)
    g3 = GR.ghook(frozen, GR.CMD, meas=m, count=k + 3, k_stride=k)    # passed through: the count as given
    assert g3["flags"] == IR.FROZEN and g3["count_out"] == k + 3 and g3["meas_out"].tobytes() == m.tobytes() and g3["n_rej"] == 0
