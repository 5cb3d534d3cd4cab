"""Landmark merging compiled for the host (slam_merge_instance_host: the kernels' own source, live_ekf_slam_amd/csrc/merge_kernel.h),
without a GPU, against the INDEPENDENT numpy reference of merge_reference, IN BITS, in both storage types: the partner of every slot,
the d2 of its best candidate, the record, M', x', P', ids' and the track counters.  Crafted states are SPD, P = A A^T through a copy
transform plus small independent noise; every test asserts the margin of every d2 to gate_merge first (duplicates below gate / 2, every
other pair above 2 gate), so no decision is a coin toss.  Then the property the fusion must have: after a sigma = 0 fusion x' and P' are
the conditional Gaussian given l_i = l_j, evaluated in np.longdouble; and the CPU oracle steps on from the merged state."""
import numpy as np
import pytest

import innovation_reference as IR
import merge_reference as R
from live_ekf_slam_amd.config import MergeConfig, default_config, default_merge_config

SHAPES = [(20, False), (20, True), (50, False), (50, True)]
IDS = ["L20_f64", "L20_f32", "L50_f64", "L50_f32"]
E1, E2 = (0.8, 0.3), (-0.5, 0.9)      # displacements of a copy in units of its noise: d2 = 0.365 and 0.53


def _compare(st, L_max, f32, name, cfg=None, pairs=None, status=0, seen=None, expected=None, partner=None):
    """hook == reference in bits; returns (hook result, reference result).  pairs: the duplicates the case was built with (margins)."""
    cfg = cfg or default_merge_config()
    ref = R.reference_merge(st["x"], st["P"], st["ids"], L_max, cfg, status, f32, seen, expected, partner)
    if pairs is not None and ref["D"] is not None:
        R.check_margins(ref["D"], pairs, cfg.gate_merge, name)
    got = R.hook(st, L_max, f32, cfg, status=status, seen=seen, expected=expected, partner=partner)
    assert got["partner"].tolist() == ref["partner"].tolist(), name
    assert R.same_values(got["d2"], ref["d2"]), name
    assert R.same_values(got["rec"], ref["rec"]), (name, got["rec"], ref["rec"])
    assert got["M"] == ref["M"] and got["ids"].tolist() == ref["ids"].tolist(), name
    assert R.same_values(got["x"], ref["x"]) and R.same_values(got["P"], ref["P"]), name
    if ref["ids_row"] is not None:
        assert got["ids_row"].tolist() == ref["ids_row"].tolist(), (name, "ids are zero from M' up to L_max")
    for key in ("seen", "expected"):
        if ref[key] is not None:
            assert got[key].tolist() == ref[key].tolist(), (name, key)
    return got, ref


@pytest.mark.parametrize("L_max,f32", SHAPES, ids=IDS)
def test_pair_sets_against_the_reference_in_bits(L_max, f32):
    rng = np.random.default_rng(31 + L_max + int(f32))
    M = L_max - 3
    cases = [("no pair", M, {}, []),
             ("one pair", M, {7: (2, E1, True)}, [(2, 7)]),
             ("the pair (0, M - 1)", M, {M - 1: (0, E2, True)}, [(0, M - 1)]),
             ("several disjoint pairs", M, {5: (1, E1, True), 6: (3, E2, True), M - 2: (4, E1, True), M - 1: (M - 3, E2, True)},
              [(1, 5), (3, 6), (4, M - 2), (M - 3, M - 1)]),
             ("M = L_max", L_max, {L_max - 1: (L_max - 2, E1, True), 3: (0, E2, True)}, [(L_max - 2, L_max - 1), (0, 3)]),
             ("M = 2, a pair", 2, {1: (0, E1, True)}, [(0, 1)]),
             ("M = 2, no pair", 2, {}, [])]
    fused = 0
    for name, m, copies, pairs in cases:
        st = R.crafted_state(rng, R.layout_with(m, copies), f32)
        seen = rng.integers(0, 40, L_max).astype(np.int32); expected = seen + rng.integers(0, 9, L_max).astype(np.int32)
        seen[m:] = 0; expected[m:] = 0
        got, ref = _compare(st, L_max, f32, name, pairs=pairs)
        assert got["M"] == m - len(pairs) and got["rec"][R.REC_FUSED] == len(pairs) and got["rec"][R.REC_NOT_MUTUAL] == 0, name
        for i, j in pairs:
            assert got["partner"][i] == j and got["partner"][j] == i, name
            assert int(st["ids"][i]) in got["ids"].tolist() and int(st["ids"][j]) not in got["ids"].tolist(), (name, "the kept id is ids[i]")
        if not pairs:
            assert R.same_bits(got["x"], st["x"]) and R.same_bits(got["P"], st["P"]), (name, "an instance without a pair is not written")
        got, ref = _compare(st, L_max, f32, name + ", counters", pairs=pairs, seen=seen, expected=expected)
        for i, j in pairs:
            e2 = max(expected[i], expected[j])
            k = got["ids"].tolist().index(int(st["ids"][i]))
            assert got["expected"][k] == e2 and got["seen"][k] == min(seen[i] + seen[j], e2), name
        fused += len(pairs)
    assert fused >= 9


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_chain_fuses_only_its_mutual_pair(f32):
    """a - b - c: copies of one landmark with d2(a, b) = 0.125, d2(a, c) = 1.125 and d2(b, c) = 2: c's best candidate is a, a's is b."""
    rng = np.random.default_rng(5)
    L_max, M = 20, 12
    st = R.crafted_state(rng, R.layout_with(M, {7: (3, (0.5, 0.0), True), 9: (3, (-1.5, 0.0), True)}), f32)
    got, ref = _compare(st, L_max, f32, "chain", pairs=[(3, 7), (3, 9), (7, 9)])
    assert got["partner"][3] == 7 and got["partner"][7] == 3 and got["partner"][9] == -1
    assert abs(got["d2"][9] - 1.125) < 1e-3 and abs(got["d2"][3] - 0.125) < 1e-3
    assert got["M"] == M - 1 and got["rec"][R.REC_FUSED] == 1 and got["rec"][R.REC_NOT_MUTUAL] == 1
    assert int(st["ids"][9]) in got["ids"].tolist() and int(st["ids"][7]) not in got["ids"].tolist()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_small_maps_have_no_pairs(f32):
    rng = np.random.default_rng(6)
    for M in (0, 1):
        st = R.crafted_state(rng, R.layout_with(M, {}), f32)
        got, ref = _compare(st, 20, f32, f"M = {M}")
        assert got["M"] == M and (got["partner"] == -1).all() and np.isnan(got["d2"]).all() and not got["rec"].any()


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_exact_copies_are_singular_without_sigma_and_fuse_with_it(f32):
    rng = np.random.default_rng(8)
    L_max, M = 20, 9
    st = R.crafted_state(rng, R.layout_with(M, {6: (2, (0.0, 0.0), False)}), f32)
    assert R.same_bits(st["P"][7:9, 7:9], st["P"][15:17, 15:17]) and R.same_bits(st["x"][7:9], st["x"][15:17])
    got, ref = _compare(st, L_max, f32, "exact copies, sigma = 0")
    assert (got["partner"] == -1).all() and got["M"] == M, "S = 0 has no inverse: the cost is NaN and the find offers no pair"
    partner = np.full(L_max, -1, dtype=np.int32); partner[2] = 6; partner[6] = 2
    got, ref = _compare(st, L_max, f32, "exact copies given by the caller, sigma = 0", partner=partner)
    assert got["rec"][R.REC_SINGULAR] == 1 and got["rec"][R.REC_FUSED] == 0 and got["rec"][R.REC_TOUCHED] == 0 and got["M"] == M
    assert R.same_bits(got["x"], st["x"]) and R.same_bits(got["P"], st["P"]) and got["ids"].tolist() == st["ids"].tolist()
    cfg = MergeConfig(default_merge_config().gate_merge, 0.01, 10)
    got, ref = _compare(st, L_max, f32, "exact copies, sigma = 0.01", cfg=cfg, pairs=[(2, 6)])
    assert got["partner"][2] == 6 and got["d2"][2] == 0.0 and got["M"] == M - 1 and got["rec"][R.REC_FUSED] == 1


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_caller_pairs_that_are_not_mutual_or_out_of_range_are_ignored_and_counted(f32):
    rng = np.random.default_rng(9)
    L_max, M = 20, 10
    st = R.crafted_state(rng, R.layout_with(M, {8: (1, E1, True)}), f32)
    partner = np.full(L_max, -1, dtype=np.int32)
    partner[1] = 8; partner[8] = 1            # honoured
    partner[0] = 4; partner[4] = 5            # not mutual: 2 entries
    partner[3] = 3                            # itself
    partner[6] = 15; partner[15] = 6          # slots at or above M: 2 entries
    partner[7] = -7; partner[9] = 1000        # out of range
    got, ref = _compare(st, L_max, f32, "caller pairs", partner=partner)
    assert got["rec"][R.REC_FUSED] == 1 and got["rec"][R.REC_NOT_MUTUAL] == 7 and got["M"] == M - 1
    # a pair the find would never offer (two different landmarks) is fused all the same when the caller names it: gate_merge is not consulted
    partner = np.full(L_max, -1, dtype=np.int32); partner[0] = 2; partner[2] = 0
    got, ref = _compare(st, L_max, f32, "a far pair by the caller", partner=partner)
    assert got["rec"][R.REC_FUSED] == 1 and got["rec"][R.REC_MAX_D2] > 2 * default_merge_config().gate_merge


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_nan_in_P_and_frozen_instances(f32):
    rng = np.random.default_rng(10)
    L_max, M = 20, 11
    copies = {9: (4, E1, True), 10: (5, E2, True)}
    st = R.crafted_state(rng, R.layout_with(M, copies), f32, nan_slot=5)
    got, ref = _compare(st, L_max, f32, "NaN in slot 5", pairs=[(4, 9)])
    assert got["partner"][4] == 9 and got["partner"][5] == -1 and got["partner"][10] == -1, "a pair with a NaN costs NaN: no candidate"
    assert got["M"] == M - 1 and np.isnan(got["P"][13, :]).all() and np.isfinite(got["P"][:13, :13]).all(), "the NaNs stay where they were"
    st = R.crafted_state(rng, R.layout_with(M, copies), f32)
    partner = np.full(L_max, -1, dtype=np.int32); partner[4] = 9; partner[9] = 4
    for status in (1, 4, 32, 4 | 2):
        got, ref = _compare(st, L_max, f32, f"status {status}", status=status)
        assert (got["partner"] == -1).all() and got["M"] == M and not got["rec"].any()
        assert R.same_bits(got["x"], st["x"]) and R.same_bits(got["P"], st["P"])
        got, ref = _compare(st, L_max, f32, f"status {status}, caller pairs", status=status, partner=partner)
        assert got["M"] == M and got["rec"][R.REC_NOT_MUTUAL] == 2 and got["rec"][R.REC_FUSED] == 0
    got, ref = _compare(st, L_max, f32, "a status that does not stop the step", status=2 | 8, pairs=[(4, 9), (5, 10)])
    assert got["M"] == M - 2


def _conditional_longdouble(x, P, i, j):
    """x and P given l_i = l_j, in np.longdouble, slot j deleted."""
    n = len(x)
    ii, jj = 3 + 2 * i, 3 + 2 * j
    H = np.zeros((2, n), dtype=np.longdouble)
    H[0, ii] = H[1, ii + 1] = 1; H[0, jj] = H[1, jj + 1] = -1
    xl, Pl = x.astype(np.longdouble), P.astype(np.longdouble)
    S = H @ Pl @ H.T
    det = S[0, 0] * S[1, 1] - S[0, 1] * S[1, 0]
    Si = np.array([[S[1, 1], -S[0, 1]], [-S[1, 0], S[0, 0]]], dtype=np.longdouble) / det
    K = Pl @ H.T @ Si
    x2 = xl - K @ (H @ xl)
    P2 = Pl - K @ (H @ Pl)
    idx = [jj, jj + 1]
    return np.delete(x2, idx), np.delete(np.delete(P2, idx, 0), idx, 1)


def _conditional_float64(x, P, i, j):
    """The same in float64 matrix products: the rounding spread of a second evaluation."""
    n = len(x)
    ii, jj = 3 + 2 * i, 3 + 2 * j
    H = np.zeros((2, n))
    H[0, ii] = H[1, ii + 1] = 1; H[0, jj] = H[1, jj + 1] = -1
    K = P @ H.T @ np.linalg.inv(H @ P @ H.T)
    idx = [jj, jj + 1]
    return np.delete(x - K @ (H @ x), idx), np.delete(np.delete(P - K @ (H @ P), idx, 0), idx, 1)


@pytest.mark.parametrize("L_max", [20, 50])
def test_a_fusion_is_the_conditional_gaussian(L_max):
    """After a sigma = 0 fusion x' and P' are x and P conditioned on l_i = l_j.  The bound is not fixed here: it is 10 x the deviation of
    a plain float64 numpy evaluation of the same conditional from the np.longdouble one on the same case (the project's "10 x rounding
    spread" convention).  Measured on this machine, max abs deviation from the longdouble result, hook | float64 numpy:
    L_max 20: x 1.1e-16 | 1.1e-16, P 2.7e-20 | 2.7e-20;  L_max 50: x 1.1e-16 | 1.1e-16, P 2.7e-20 | 2.7e-20 (half an ulp of the
    largest entries: x of about 1, P of about 4e-4)."""
    rng = np.random.default_rng(40 + L_max)
    M = L_max - 1
    i, j = 4, M - 2
    st = R.crafted_state(rng, R.layout_with(M, {j: (i, E1, True)}), False)
    got = R.hook(st, L_max, False)
    assert got["M"] == M - 1 and got["partner"][i] == j
    xl, Pl = _conditional_longdouble(st["x"], st["P"], i, j)
    xd, Pd = _conditional_float64(st["x"], st["P"], i, j)
    dev = lambda a, b: float(np.abs(a.astype(np.longdouble) - b).max())
    spread_x, spread_P = dev(xd, xl), dev(Pd, Pl)
    got_x, got_P = dev(got["x"], xl), dev(got["P"], Pl)
    print(f"L_max {L_max}: x {got_x:.2g} | {spread_x:.2g}, P {got_P:.2g} | {spread_P:.2g}")
    assert spread_x > 0 and spread_P > 0
    assert got_x <= 10 * spread_x and got_P <= 10 * spread_P, (got_x, spread_x, got_P, spread_P)


@pytest.mark.parametrize("L_max,f32", SHAPES, ids=IDS)
def test_the_oracle_steps_on_from_the_merged_state(oracle, L_max, f32):
    """The merged state is an ordinary state: the CPU oracle stepped five times from the hook's result equals, bit for bit, its twin stepped
    from the reference's, on messages that re-observe the kept id, the dropped id (inserted as new) and others."""
    O = oracle
    rng = np.random.default_rng(50 + L_max + int(f32))
    cfg = default_config()
    M = L_max - 4
    st = R.crafted_state(rng, R.layout_with(M, {M - 1: (1, E1, True), 6: (2, E2, True)}), f32)
    got, ref = _compare(st, L_max, f32, "two pairs", pairs=[(1, M - 1), (2, 6)])
    a = dict(x=got["x"], P=got["P"], ids=got["ids"]); b = dict(x=ref["x"], P=ref["P"], ids=ref["ids"])
    kept, dropped = int(st["ids"][1]), int(st["ids"][M - 1])
    for step in range(5):
        cur = dict(x=a["x"], ids=np.asarray(a["ids"], dtype=np.int32))
        slot = cur["ids"].tolist().index(kept)
        dets = [IR.detection(rng, cur, slot), IR.detection(rng, cur, int(rng.integers(0, len(cur["ids"])))),
                [float(dropped)] + IR.detection(rng, cur, slot)[1:]]
        cmd = (0.05, 0.02 * step)
        a, fa = IR.oracle_step(O, a, cmd, dets, cfg, L_max, f32)
        b, fb = IR.oracle_step(O, b, cmd, dets, cfg, L_max, f32)
        assert fa == fb and a["M"] == b["M"] and list(a["ids"]) == list(b["ids"]), step
        assert R.same_bits(a["x"], b["x"]) and R.same_bits(a["P"], b["P"]), step
    assert a["M"] == M - 2 + 1 and not fa, "the dropped id came back as one new landmark"
