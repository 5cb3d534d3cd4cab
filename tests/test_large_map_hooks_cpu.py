"""The kernels around the step at maps beyond 66 landmarks, up to the capacity of 1000, WITHOUT a GPU: the host hooks (the kernels' own
per-instance functions compiled for the host) against the INDEPENDENT numpy references of map_reference, merge_reference and fix_reference
with those modules' own comparators, and every premise of the case tables of large_map_cases.py, which test_large_map_kernels_gpu.py runs
on the device.  "Device == hook in bits" cannot see an error in the code both share; this leg can, and until now it ended at L_max 50.

The edges and where they come from:
  assoc   assoc_cost_phase (assoc_kernel.h, shared by assoc_instance_kernel and the joint kernel): lanes walk the slots 64 at a time and
          join each trip's (best, second, slot, nu) into the running values, an earlier trip keeping a tie.  M = 63, 64, 65, 127, 128, 129,
          1000 (one, two, three and sixteen trips), each in a full handle and in one with room for one more: the best in the last trip
          with the second in the first and the reverse; two slots of different trips with bit-identical costs (identical x entries and
          blocks of P: the lower slot is reported); a map whose only finite cost sits in a trip's last lane (63, 127) or first lane
          (64, 128); messages of 0, 1, 64 and 65 (TOO_LONG) detections.  Five instances of different M per handle: one past a workgroup.
  joint   joint_kernel.h keeps kJointMaxCand = 4 candidates per detection, inserted trip by trip: five or six landmarks inside the
          individual gate over three trips, the kept four being the reference's; the fourth and fifth best tie in bits, in different
          trips, so JointSink::pair's "entries already there stay in front on a tie" decides.  Three instances per handle.  (A tie of
          the two BEST costs has two equally good hypotheses, which joint_reference's margins rule out: slam_associate runs that one.)
  gate    gate and innovation at L_max 1000 holding 1000 (and 999) landmarks: slots 0, 63, 64, 998, 999, exactly SLAM_INNOV_MAX_LM = 16
          distinct landmarks and one more.  The step behind assoc, joint and gate at L_max 129 (step class 403) and 201 (streamed kernel).
  merge   launch_merge_find (merge_kernel.hip): kind 0 | 1 at L_max 64 | 65, 1 | 2 at 256 | 257; a lane's third and fourth owned slot
          (j = tid + k * 256) from 513 and 769; the panel depth TP = clamp(57344 / (32 npad), 1, 8) at 126 (7), 147 (6), 177 (5), 222 (4),
          297 (3), 447 (1) with landmark counts that are no multiple of TP; lds + 8192 > 64 KiB from L_max 895 (slam_allow_full_lds);
          launch_merge_fuse: 8 (4 (3 + 2 L_max) + 2) + 4096 > 64 KiB from 959; the capacity 1000 holding 998 - 1000 landmarks.
          Duplicates straddle every owner index: (5, 261), (255, 256), (300, 700), (511, 512), (767, 768), (2, M - 1); a chain a - b - c
          across owners (10, 270, 530) leaves a non-mutual slot; (40, 41) and (255, 256) are adjacent.
  map     map_compact_kernel (map_kernel.hip, map_kernel.h): the kept list is built 64 slots at a time (M = 64, 65, 128, 129, 1000; the
          removal sets of map_reference and "exactly slots 63 and 64", "one whole 64-slot trip", "every slot but the last"); P moves in
          chunks of 256 lanes x kMapChunk = 8 elements (one chunk at 18 landmarks, about 1960 at 1000); the tally walks a message in
          blocks of kMapIdBlock = 64 ids (63, 64, 65, 128, 129 ids).
  fix     fix_instance_kernel (fix_kernel.hip): 256 lanes over n rows, n = 255, 257, 511, 513 and 2003 (M = 126, 127, 254, 255, 1000),
          every scenario of test_fix_gpu.HOWS, position, heading and both, at every size; launch_fix raises the LDS limit at
          8 (6 n + 3) + 4096 > 64 KiB, from L_max 639 (cases at 638 and 639).
pytest -s prints, per case, L_max, the landmark counts, the path and the number of instances compared."""
import numpy as np
import pytest

import assoc_reference as AR
import fix_reference as FR
import gate_reference as GR
import innovation_reference as IR
import joint_reference as JR
import large_map_cases as LC
import map_reference as MR
import merge_reference as R
from live_ekf_slam_amd import fix_instance_host
from live_ekf_slam_amd.config import MapConfig, default_config
from test_fix_gpu import HOWS
from test_fix_gpu import _fix_row as fix_row
from test_fix_reference import _bits, _state
from test_map_reference import _check_removal
from test_merge_reference import _compare as _compare_merge


def _compare_fix(x, P, L_max, row, kinds, f32, what):
    """test_fix_reference's comparison of the hook with fix_reference.reference_fix, in bits: (hook result, reference result)."""
    h = fix_instance_host(x, P, L_max, row, kinds, f32_storage=f32)
    r = FR.reference_fix(x, P, row, kinds, f32=f32)
    assert h["verdict"] == r["verdict"], (what, h["verdict"], r["verdict"])
    assert _bits(h["nis"]) == _bits(r["nis"]) and _bits(h["rec"]) == _bits(r["rec"]), (what, h["nis"], r["nis"], h["rec"], r["rec"])
    assert _bits(h["x"]) == _bits(r["x"]) and _bits(h["P"]) == _bits(r["P"]), what
    if not r["written"]:                  # an instance without an applied part keeps its bytes
        assert _bits(h["x"]) == _bits(x) and _bits(h["P"]) == _bits(P), what
    else:
        assert _bits(h["P"]) != _bits(P), what
    return h, r


# ---- premises ---------------------------------------------------------------------------------------------------------------------------------
def test_premises_merge_launch_rules():
    """The table of the issue against the restated rules of launch_merge_find and launch_merge_fuse, and the rules at their boundaries."""
    for L, want in LC.MERGE_TABLE.items():
        f, u = LC.merge_find_rule(L), LC.merge_fuse_rule(L)
        assert (f["kind"], f["TP"], f["full_lds"], u["full_lds"]) == want, (L, f, u)
    assert {LC.merge_find_rule(L)["TP"] for L in LC.MERGE_TABLE} == {1, 3, 4, 5, 6, 7, 8}       # (TP 2 is what L_max 300 ran)
    assert LC.merge_find_rule(300)["TP"] == 2 and LC.merge_find_rule(201)["TP"] == 4 and LC.merge_find_rule(66)["TP"] == 8
    for L in (126, 147, 177, 222, 297, 447):                   # the largest L_max of each TP: one more landmark and a slot less fits
        assert LC.merge_find_rule(L + 1)["TP"] == LC.merge_find_rule(L)["TP"] - 1 or LC.merge_find_rule(L)["TP"] == 1, L
    assert [L for L in range(1, LC.CAPACITY + 1) if LC.merge_find_rule(L)["full_lds"]][0] == 895
    assert [L for L in range(1, LC.CAPACITY + 1) if LC.merge_fuse_rule(L)["full_lds"]][0] == 959
    assert LC.merge_find_rule(1000)["lds"] == 64096 and LC.merge_fuse_rule(1000)["lds"] == 64112
    assert {L for L, _ in LC.MERGE_CASES} == set(LC.MERGE_TABLE)
    assert {f32 for L, f32 in LC.MERGE_CASES if LC.merge_find_rule(L)["full_lds"]} == {False, True}
    assert {f32 for L, f32 in LC.MERGE_CASES if LC.merge_fuse_rule(L)["full_lds"]} == {False, True}


def test_premises_merge_placements():
    """Which owned slot every partner falls in, in every handle: each placement of the issue occurs, a lane owns a third slot from L_max
    513 and a fourth from 769, and the handles of a TP between 3 and 7 hold a landmark count that is no multiple of it."""
    seen_pairs, chains = set(), set()
    for L in LC.MERGE_TABLE:
        rule = LC.merge_find_rule(L)
        counts = LC.merge_counts(L)
        assert counts[0] == L and all(2 <= M <= L for M in counts)
        if 126 <= L <= 447:
            assert any(M % rule["TP"] for M in counts) or rule["TP"] == 1, L
        rounds = set()
        for M in counts:
            copies, pairs, chain = LC.merge_layout(M)
            slots = [s for p in pairs for s in p] + list(chain)
            assert len(set(slots)) == len(slots) and max(slots) < M and len(pairs) >= 3, (L, M)
            assert set(copies) == {j for _, j in pairs} | set(chain[1:])
            seen_pairs.update(pairs); chains.add(chain)
            rounds.update(LC.owned_round(s) for s in slots)
        assert max(rounds) == (L - 1) // 256 if L in (513, 769, 1000) else max(rounds) <= (L - 1) // 256, (L, rounds)
    assert {(5, 261), (255, 256), (300, 700), (511, 512), (767, 768), (2, 999), (40, 41)} <= seen_pairs
    assert [tuple(LC.owned_round(s) for s in p) for p in ((5, 261), (255, 256), (300, 700), (511, 512), (767, 768), (2, 999))] == \
        [(0, 1), (0, 1), (1, 2), (1, 2), (2, 3), (0, 3)]
    assert (10, 270, 530) in chains and [LC.owned_round(s) for s in (10, 270, 530)] == [0, 1, 2], "the non-mutual slot lies across owners"
    assert (511, 512) in seen_pairs and (767, 768) in seen_pairs, "slot 512 is a lane's third slot, slot 768 its fourth"
    assert 998 in LC.merge_counts(1000) and 1000 in LC.merge_counts(1000)


def test_premises_map_chunks_and_trips():
    """How many chunks of 2048 elements the compaction of P takes, which 64-slot trips the removal sets touch, the tally's id blocks."""
    assert LC.compact_chunks(17, 8) == 1, "at 18 landmarks less one, P is one chunk"
    assert LC.compact_chunks(59, 4) == 8, "the largest P compacted so far (60 landmarks less one, fp32) has 8 chunks"
    most = 0
    for L_max, M, f32 in LC.MAP_CASES:
        assert M in LC.MAP_COUNTS + (999,) and M in (L_max, L_max - 1)
        for kind in LC.REMOVAL_SETS:
            mask = LC.removal_mask(kind, M, np.random.default_rng(1))
            assert mask.shape == (M,)
            most = max(most, LC.compact_chunks(M - int(mask.sum()), 4 if f32 else 8) if mask.any() else 0)
    assert most > 1000, most
    assert set(LC.MAP_CHUNKS) == set(LC.MAP_CASES) and all(len(v) == len(LC.FIXED_REMOVAL_SETS) == 9 for v in LC.MAP_CHUNKS.values())
    assert LC.compact_chunks(999, 4) == 1959 and LC.compact_chunks(999, 8) == 1957   # ceil(2001 * 2004 / 2048), ceil(2001 * 2002 / 2048)
    for M in LC.MAP_COUNTS:
        assert any(L == M for L, m, _ in LC.MAP_CASES if m == M) and any(L == M + 1 for L, m, _ in LC.MAP_CASES if m == M) or M == 1000, M
        two = LC.removal_mask("exactly slots 63 and 64", M)
        assert np.nonzero(two)[0].tolist() == ([63, 64] if M > 64 else [63])
        trip = np.nonzero(LC.removal_mask("one whole 64-slot trip", M))[0]
        assert len(trip) == 64 and trip[0] % 64 == 0 and trip[-1] % 64 == 63
        assert np.nonzero(LC.removal_mask("every slot but the last", M) == 0)[0].tolist() == [M - 1]
    assert any(M == 1000 and L == 1000 for L, M, _ in LC.MAP_CASES) and any(M == 999 and L == 1000 for L, M, _ in LC.MAP_CASES)
    assert [(-(-k // 64), k % 64) for k in LC.TALLY_LENGTHS] == [(1, 63), (1, 0), (2, 1), (2, 0), (3, 1)]
    assert {f32 for _, _, f32 in LC.MAP_CASES} == {False, True}


def test_premises_fix_sizes():
    assert [3 + 2 * M for M in LC.FIX_COUNTS] == [255, 257, 511, 513, 2003]
    for M in LC.FIX_COUNTS:
        assert any(m == M and L == M for L, m, _ in LC.FIX_CASES) and (M == 1000 or any(m == M and L == M + 1 for L, m, _ in LC.FIX_CASES)), M
    assert {f32 for _, _, f32 in LC.FIX_CASES} == {False, True} and 3 + 2 * LC.CAPACITY == 2003
    assert [L for L in range(1, LC.CAPACITY + 1) if LC.fix_rule(L)["full_lds"]][0] == 639 and LC.fix_rule(1000)["lds"] == 96168
    raised = {(L, f32) for L, _, f32 in LC.FIX_CASES if LC.fix_rule(L)["full_lds"]}
    assert {f32 for _, f32 in raised} == {False, True} and (639, True) in raised and (638, True) in {(L, f32) for L, _, f32 in LC.FIX_CASES}
    assert HOWS == ("near", "far_pos", "far_yaw", "nan_sigma", "neg_sigma", "inf_z", "near")


def test_premises_association_handles():
    """Every landmark count sits once in a full handle and once in one with room for one more, in an instance of the roles tie or near;
    the five instances of a handle mix trip counts; the slots of every role lie in the trips the role is about."""
    main = {(L, M) for L, Ms in LC.ASSOC_HANDLES.items() for M, role in zip(Ms, LC.ASSOC_ROLES) if role in ("tie", "near")}
    for M in LC.ASSOC_COUNTS:
        assert (M, M) in main and ((M + 1, M) in main or M == LC.CAPACITY), M
    assert (1000, 999) in main and [-(-M // 64) for M in LC.ASSOC_COUNTS] == [1, 1, 2, 2, 2, 3, 16]
    for L, Ms in LC.ASSOC_HANDLES.items():
        assert len(Ms) == 5 and max(Ms) <= L and (len({-(-M // 64) for M in Ms}) > 1 or L <= 64), (L, "one workgroup mixes trip counts")
        for M, role in zip(Ms, LC.ASSOC_ROLES):
            sl = LC.assoc_slots(role, M)
            last = (M - 1) // 64
            if role in ("tie", "near") and last:
                assert LC.trip(sl[0]) == 0 and LC.trip(sl[1]) == last and (role == "near" or sl[1] % 64 == 0), (L, M, role)
            if role == "lone last lane" and M >= 64:
                assert sl[0] % 64 == 63
            if role == "lone first lane" and M >= 65:
                assert sl[0] % 64 == 0 and sl[0] >= 64
    assert LC.assoc_slots("lone last lane", 129) == (127,) and LC.assoc_slots("lone first lane", 129) == (128,)
    assert LC.assoc_slots("lone last lane", 65) == (63,) and LC.assoc_slots("lone first lane", 65) == (64,)
    assert LC.ASSOC_TICK2[:4] == (0, 1, 64, 65) and AR.MAX_DET == 64 and set(LC.STEP_BEHIND) <= set(LC.ASSOC_HANDLES)


# ---- 1. association: hook == reference ---------------------------------------------------------------------------------------------------------------
def assoc_case(role, st, L_max, triplets):
    return dict(name=role, st=st, status=0, meas=np.asarray(triplets, dtype=np.float32).reshape(-1, 3), noise=AR.NOISE, L_max=L_max, verdicts=None,
                flags=AR.TOO_LONG if len(triplets) > AR.MAX_DET else 0, main=False)


def assoc_premises(role, M, cost, slot, second):
    """What the role is about, from the reference's cost matrix of its first-tick message and the (slot, second best) reported: returns
    the line printed.  The detections of a role's own slots cannot keep assoc_reference.check_margins (own < gate_match / 2, every other
    > 2 gate_new): their runner-up lies inside the gate on purpose.  For them no finite cost may lie within 1e-3 relative of a gate, and
    the cost matrix is compared in bits; check_margins itself runs on the clean and the new detections of the same message."""
    sl = LC.assoc_slots(role, M)
    fin = cost[np.isfinite(cost)]
    for g in (AR.GATE_MATCH, AR.GATE_NEW):
        assert (np.abs(fin - g) > 1e-3 * g).all(), (role, M, "a cost at a gate")
    order = [np.argsort(np.where(np.isfinite(c), c, np.inf), kind="stable") for c in cost]
    if role == "tie":
        a, b = sl
        assert AR.same_bits(cost[0, a], cost[0, b]) and AR.same_bits(cost[1, a], cost[1, b]) and np.isfinite(cost[0, a]), (M, "two costs are the same bits")
        assert order[0][:2].tolist() == [a, b] and slot[0] == slot[1] == a and AR.same_bits(second[0], cost[0, a]), (M, "the lower slot is reported")
        return f"tie of slots {a} (trip {LC.trip(a)}) and {b} (trip {LC.trip(b)})"
    if role == "near":
        e, l = sl
        if M > 1:
            assert order[0][:2].tolist() == [e, l] and order[1][:2].tolist() == [l, e] and slot[0] == e and slot[1] == l, (M, order[0][:2], order[1][:2])
            assert AR.same_bits(second[0], cost[0, l]) and AR.same_bits(second[1], cost[1, e])
        return f"best {e} (trip {LC.trip(e)}) with second {l} (trip {LC.trip(l)}), and the reverse"
    assert np.isfinite(cost[0]).sum() == 1 and np.isfinite(cost[0, sl[0]]) and slot[0] == sl[0] and np.isnan(second[0]), (role, M)
    return f"the only finite cost in slot {sl[0]} (lane {sl[0] % 64} of trip {LC.trip(sl[0])})"


@pytest.mark.parametrize("L_max,f32", LC.ASSOC_CASES, ids=LC.ASSOC_IDS)
def test_association_hook_against_the_reference_at_every_trip_edge(L_max, f32):
    """The five instances of the handle, both ticks: cost matrix, best and second, slot, nu, verdicts, the labelled message, counts and
    record against assoc_reference in bits (costs by the ungated innovation hook alone, one call per pair), and the premises of each role."""
    rng = np.random.default_rng(131 + L_max + int(f32))
    lines, flagged = [], 0
    for b, (role, M) in enumerate(zip(LC.ASSOC_ROLES, LC.ASSOC_HANDLES[L_max])):
        st = LC.assoc_state(role, M, f32, rng)
        for k in (None, LC.ASSOC_TICK2[b]):
            case = assoc_case(role, st, L_max, LC.assoc_messages(role, st, rng, k))
            cost, nu = AR.reference_costs(case, AR.CMD, f32)
            ref = AR.reference_associate(case, cost, nu)
            g = AR.ahook(case, f32=f32)
            AR.check_against_reference(g, ref, f"{role}, M {M}, k {k}", row_in=AR.padded_row(case), cost=cost)
            if k is None:
                lines.append(f"M {M} ({-(-M // 64)} trips): " + assoc_premises(role, M, cost, ref["slot"], ref["det"][:, 1]))
                plain = [l for l in range(len(case["meas"])) if l >= len(LC.assoc_slots(role, M)) and np.isfinite(cost[l]).any()]
                want = [AR.MATCHED if l > len(LC.assoc_slots(role, M)) else (AR.NEW if M < L_max else AR.NO_ROOM) for l in plain]
                AR.check_margins(dict(main=True, verdicts=want), cost[plain], f"{role}, M {M}: the clean and the new detections")
                assert [int(g["verdict"][l]) for l in plain] == want and (len(plain) == 3 or M <= 12 or role.startswith("lone")), (role, M, plain)
                assert g["n_match"] >= 1 and g["n_new"] >= (1 if M < L_max else 0) and g["flags"] == 0
            else:
                assert g["flags"] == (AR.TOO_LONG if k == 65 else 0) and (k != 0 or g["count_out"] == 0) and (k != 64 or g["rec"][3] == 64)
                flagged += g["flags"] != 0
    assert flagged == 1, "one message is one detection too long"
    print(f"assoc L_max {L_max} {'f32' if f32 else 'f64'}: " + "; ".join(lines) + f"; second tick of {LC.ASSOC_TICK2} detections; 10 messages compared")


def test_premises_joint_handles():
    main = {(L, M) for L, Ms in LC.JOINT_HANDLES.items() for M, role in zip(Ms, LC.JOINT_ROLES) if role != "lone"}
    for M in LC.ASSOC_COUNTS:
        assert (M, M) in main and ((M + 1, M) in main or M == LC.CAPACITY), M
    assert (1000, 999) in main and JR.MAX_CAND == 4 and set(LC.STEP_BEHIND) <= set(LC.JOINT_HANDLES)
    for L, Ms in LC.JOINT_HANDLES.items():
        assert len(Ms) == 3 and max(Ms) <= L
        sl = LC.cluster_slots(Ms[1])
        assert len(set(sl)) == len(sl) > JR.MAX_CAND and max(sl) == sl[-1] < Ms[1] and len(LC.CLUSTER[len(sl)]) == len(sl)
        assert len({LC.trip(s) for s in sl}) >= min(3, -(-Ms[1] // 64)), (L, sl)
    assert {LC.joint_role("lone", L) for L in LC.JOINT_HANDLES} == {"lone last lane", "lone first lane"}
    assert any(len({LC.trip(s) for s in LC.cluster_slots(Ms[1])}) >= 3 for Ms in LC.JOINT_HANDLES.values())
    for Ms in LC.JOINT_HANDLES.values():
        lo, hi = LC.cluster_tie(Ms[1])
        sl = LC.cluster_slots(Ms[1])
        assert lo < hi < sl[-1] and LC.CLUSTER[len(sl)][sl.index(lo)] == LC.CLUSTER[len(sl)][sl.index(hi)]
        assert sorted(LC.CLUSTER[len(sl)])[3:5] == [0.10, 0.10] and (Ms[1] <= 101 or LC.trip(lo) != LC.trip(hi)), Ms


# ---- 1. (joint) hook == reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", LC.JOINT_CASES, ids=LC.JOINT_IDS)
def test_joint_association_hook_against_the_reference_at_every_trip_edge(L_max, f32):
    """The three instances of the handle, both ticks, through test_joint_reference._run: joint_reference's margins first, then decisions,
    slots, verdicts, counts, node count, candidate counts and the output message equal the reference's.  The cluster: more than
    SLAM_JOINT_MAX_CAND landmarks inside the individual gate, over three trips where the map has them; the kept four are the reference's."""
    from test_joint_reference import _case, _run
    rng = np.random.default_rng(171 + L_max + int(f32))
    lines = []
    for b, (role, M) in enumerate(zip(LC.JOINT_ROLES, LC.JOINT_HANDLES[L_max])):
        role = LC.joint_role(role, L_max)
        st = LC.joint_state(role, M, f32, rng)
        for k in (None, LC.JOINT_TICK2[b]):
            case = _case(st, LC.joint_messages(role, st, rng, k), L_max=L_max, noise=AR.NOISE, cmd=AR.CMD, name=f"{role}, M {M}, k {k}")
            g, ref, cost, nu = _run(case, f32=f32, exhaustive=False)
            if k is not None:
                assert g["flags"] & AR.TOO_LONG if k == 65 else not g["flags"] & AR.TOO_LONG, (role, k, g["flags"])
                continue
            assert g["flags"] == 0 and g["n_match"] >= 1, (role, M, g["flags"])
            if role == "cluster":
                sl = LC.cluster_slots(M)
                inside = [j for j in range(M) if np.isfinite(cost[0, j]) and cost[0, j] <= JR.joint_cfg().gate_match]
                assert len(inside) > JR.MAX_CAND and set(inside) <= set(sl) and g["ncand"][0] == JR.MAX_CAND, (M, inside)
                kept = sorted(inside, key=lambda j: (cost[0, j], j))[:JR.MAX_CAND]
                assert [j for _, j in JR.candidates(case, cost, JR.joint_cfg())[0]] == kept and kept[0] == sl[-1] and g["slot"][0] in kept
                lo, hi = LC.cluster_tie(M)                # the fourth and fifth best are the same bits: the lower slot is the one kept
                order = sorted(inside, key=lambda j: (cost[0, j], j))
                assert AR.same_bits(cost[0, lo], cost[0, hi]) and order[3:5] == [lo, hi] and kept[3] == lo and hi not in kept, (M, order)
                assert g["slot"][0] not in (lo, hi), "the pairing does not hang on the tie"
                lines.append(f"M {M}: {len(inside)} landmarks inside the gate in trips {[LC.trip(j) for j in inside]}, kept {kept}, "
                             f"tie of the 4th and 5th best in slots {lo} (trip {LC.trip(lo)}) and {hi} (trip {LC.trip(hi)})")
            elif role == "near" and M > 1:
                e, l = LC.assoc_slots(role, M)
                assert g["ncand"][:2].tolist() == [2, 2] and sorted(g["slot"][:2].tolist()) == [e, l], (M, g["ncand"][:2], g["slot"][:2])
                lines.append(f"M {M}: candidates {e} (trip {LC.trip(e)}) and {l} (trip {LC.trip(l)}) for two detections")
            else:
                s0 = LC.assoc_slots(role, M)[0]
                assert np.isfinite(cost[0]).sum() == 1 and g["slot"][0] == s0 and g["ncand"][0] == 1 and len(case["meas"]) == 1
                lines.append(f"M {M}: k = 1, the only finite cost in slot {s0} (lane {s0 % 64} of trip {LC.trip(s0)})")
    print(f"joint L_max {L_max} {'f32' if f32 else 'f64'}: " + "; ".join(lines) + f"; second tick of {LC.JOINT_TICK2} detections; 6 messages compared")


def test_premises_filter_messages():
    """Every landmark count of the gate / innovation handles has its sixteen distinct slots and one more, the first five being the first
    and last slots and both sides of the first 64-slot boundary; the messages are 5, 16, 17 and 4 detections long."""
    rng = np.random.default_rng(1)
    for L, Ms in LC.FILTER_HANDLES.items():
        for M in Ms:
            first, more = LC.filter_slots(M)
            assert M <= L and first == (0, 63, 64, M - 2, M - 1) and len(more) == 11 and max(first + more) < M
            msgs = LC.filter_messages(rng, AR.grid_state(rng, M))
            assert [len(m[1]) for m in msgs] == [5, IR.MAX_LM, IR.MAX_LM + 1, 4] and [m[3] for m in msgs] == [0, 0, IR.TOO_LONG, 0]
    assert LC.filter_slots(LC.CAPACITY)[0] == (0, 63, 64, 998, 999)


# ---- 2. gate and innovation at the capacity: hook == reference -----------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_gate_and_innovation_hooks_at_1000_landmarks(oracle, f32):
    """One state of 1000 landmarks in a handle of L_max 1000, messages that name slots 0, 63, 64, 998 and 999, exactly SLAM_INNOV_MAX_LM = 16
    distinct landmarks and one more.  Gate: gate_reference's loop over the UNGATED hook and its comparator, in bits, with the margins of
    test_gate_reference (nis < GATE / 2 or > 2 GATE).  Innovation: post against the oracle's step in bits, every nis against
    nu^T S^-1 nu in np.longdouble (check_nis_slots), the first update against the dense restatement (16 u |H| |P| |H|^T), the bars of
    test_innovation_reference."""
    L_max = M = LC.CAPACITY
    assert LC.filter_slots(M)[0] == (0, 63, 64, 998, 999) and set(LC.STEP_BEHIND) | {L_max} == set(LC.FILTER_HANDLES)
    rng = np.random.default_rng(211 + int(f32))
    st = AR.grid_state(rng, M, f32)
    cfg = IR.config_for(GR.NOISE)
    lines = []
    for name, m, verdicts, flags in LC.filter_messages(rng, st):
        case = dict(name=name, st=st, status=0, meas=np.asarray(m, dtype=np.float32).reshape(-1, 3), noise=GR.NOISE, L_max=L_max)
        k = len(m)
        g = GR.ghook(case, GR.CMD, f32=f32)
        ref = GR.reference_gate(case, GR.CMD, f32=f32)
        GR.check_against_reference(g, ref, case, name)
        assert g["flags"] == flags, (name, g["flags"])
        r = IR.hook(st, GR.CMD, case["meas"], cfg, L_max, f32, noise=GR.NOISE)
        assert r["flags"] == flags, (name, r["flags"])
        if flags:
            assert np.isnan(r["post"]).all() and np.isnan(r["det"]).all() and r["rec"][2] == 1.0 and r["rec"].sum() == 1.0, name
            lines.append(f"{name}: TOO_LONG")
            continue
        assert all(v < GR.GATE / 2 or v > 2 * GR.GATE for v in ref["nis"]), (name, sorted(ref["nis"]))
        assert g["verdict"][:k].tolist() == verdicts, (name, g["verdict"][:k].tolist())
        after, fl = IR.oracle_step(oracle, st, GR.CMD, g["meas_out"][:g["count_out"]], cfg, L_max, f32)
        assert fl in (0, IR.INST_CAPACITY) and IR.bits(IR.post_as_stored(g["post"], f32)) == IR.bits(IR.oracle_post(after)), (name, fl, "the gated post")
        after, fl = IR.oracle_step(oracle, st, GR.CMD, case["meas"], cfg, L_max, f32)
        assert IR.bits(IR.post_as_stored(r["post"], f32)) == IR.bits(IR.oracle_post(after)), (name, "the ungated post")
        assert IR.check_nis_slots(r["det"], k) == r["n_upd"] == sum(v != GR.NONE for v in verdicts), name
        nu, Sm, A = IR.dense_first_update(oracle, st, GR.CMD, case["meas"][0], GR.NOISE, f32)
        assert IR.bits(nu) == IR.bits(r["det"][0, 1:3]), (name, nu, r["det"][0])
        got = np.array([[r["det"][0, 3], r["det"][0, 4]], [r["det"][0, 4], r["det"][0, 5]]])
        assert np.all(np.abs(got - Sm) <= 16 * IR.EPS * A), (name, got - Sm)
        lines.append(f"{name}: {g['n_rej']} rejected of {r['n_upd']} updates")
    print(f"gate and innovation L_max {L_max} M {M} {'f32' if f32 else 'f64'}: " + "; ".join(lines) + f"; {len(lines)} messages compared")


# ---- 4. merge: hook == reference ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", LC.MERGE_CASES, ids=LC.MERGE_IDS)
def test_merge_hook_against_the_reference_in_bits(oracle, L_max, f32):
    """merge_reference.reference_merge (the cost of EVERY pair in Python floats, the mutual nearest neighbours, the sequential fusion,
    np.delete) against the hook in bits, with check_margins on every pair first.  Up to L_max 257 every landmark count of the handle;
    beyond, where the reference takes seconds, the full map.  Then the merged state is an ordinary state: one oracle step from the hook's
    result equals, in bits, its twin from the reference's (the kept id, the last slot and the dropped id, which comes back as new)."""
    O = oracle
    rule, fuse = LC.merge_find_rule(L_max), LC.merge_fuse_rule(L_max)
    counts = LC.merge_counts(L_max) if L_max <= 257 else LC.merge_counts(L_max)[:1]
    for M in counts:
        st, pairs, chain = LC.merge_state(L_max, M, f32)
        a, b, c = chain
        got, ref = _compare_merge(st, L_max, f32, f"L_max {L_max}, M {M}", pairs=pairs + [(a, b), (a, c), (b, c)])
        for i, j in pairs + [(a, b)]:
            assert got["partner"][i] == j and got["partner"][j] == i, (M, i, j)
        assert got["partner"][c] == -1 and int(np.nanargmin(ref["D"][c])) == a and int(np.nanargmin(ref["D"][a])) == b, "c's best candidate is a, a's is b"
        assert got["M"] == M - len(pairs) - 1 and got["rec"][R.REC_FUSED] == len(pairs) + 1 and got["rec"][R.REC_NOT_MUTUAL] == 1
        assert (got["partner"] >= 0).sum() == 2 * (len(pairs) + 1) and np.isfinite(got["d2"]).sum() == 2 * len(pairs) + 3
        only = R.hook(st, L_max, f32, fuse=False)
        assert only["partner"].tolist() == ref["partner"].tolist() and R.same_values(only["d2"], ref["d2"]) and only["M"] == M
        if LC.merge_by_pairs(L_max, f32):                # the fusion of caller pairs: the find's, one entry not mutual, one above M
            row, ignored = LC.caller_pairs(ref["partner"], chain, M, L_max)
            got2, ref2 = _compare_merge(st, L_max, f32, f"L_max {L_max}, M {M}, caller pairs", partner=row)
            assert got2["rec"][R.REC_NOT_MUTUAL] == ignored and got2["M"] == got["M"] and R.same_bits(got2["P"], got["P"])
        rng = np.random.default_rng(3)
        cur = dict(x=got["x"], ids=got["ids"])
        i, j = pairs[0]
        kept = got["ids"].tolist().index(int(st["ids"][i]))
        dets = [IR.detection(rng, cur, kept), IR.detection(rng, cur, got["M"] - 1), [float(st["ids"][j])] + IR.detection(rng, cur, kept)[1:]]
        s1, fa = IR.oracle_step(O, dict(x=got["x"], P=got["P"], ids=got["ids"]), (0.05, 0.01), dets, default_config(), L_max, f32)
        s2, fb = IR.oracle_step(O, dict(x=ref["x"], P=ref["P"], ids=ref["ids"]), (0.05, 0.01), dets, default_config(), L_max, f32)
        assert fa == fb == 0 and s1["M"] == s2["M"] == got["M"] + 1 and list(s1["ids"]) == list(s2["ids"]), M
        assert R.same_bits(s1["x"], s2["x"]) and R.same_bits(s1["P"], s2["P"]), M
    print(f"merge L_max {L_max} {'f32' if f32 else 'f64'}: M {list(counts)}, kind {rule['kind']}, TP {rule['TP']}, find LDS {rule['lds']}"
          f"{' (raised)' if rule['full_lds'] else ''}, fuse LDS {fuse['lds']}{' (raised)' if fuse['full_lds'] else ''}, pairs {pairs}, "
          f"chain {chain}; {len(counts)} instance(s) compared")


# ---- 3. map: hook == reference ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,M,f32", LC.MAP_CASES, ids=LC.MAP_IDS)
def test_removal_sets_against_np_delete_in_bits(L_max, M, f32):
    rng = np.random.default_rng(11 + L_max + M + int(f32))
    st = MR.crafted_state(rng, M, f32)
    seen = rng.integers(0, 40, L_max).astype(np.int32); expected = seen + rng.integers(0, 40, L_max).astype(np.int32)
    seen[M:] = 0; expected[M:] = 0
    chunks = {}
    for kind in LC.REMOVAL_SETS:
        mask = LC.removal_mask(kind, M, rng)
        got = _check_removal(st, mask, L_max, f32, f"M = {M}, {kind}", seen, expected)
        chunks[kind] = LC.compact_chunks(got["M"], 4 if f32 else 8) if mask.any() else 0
        if kind == "slot 0":
            _check_removal(st, mask, L_max, f32, f"M = {M}, {kind}, no counters")
    print(f"map L_max {L_max} M {M} {'f32' if f32 else 'f64'}: chunks of P per removal set {chunks}; {len(chunks)} removals compared")
    assert tuple(chunks[k] for k in LC.FIXED_REMOVAL_SETS) == LC.MAP_CHUNKS[(L_max, M, f32)], chunks


@pytest.mark.parametrize("L_max,M,f32", LC.MAP_CASES, ids=LC.MAP_IDS)
def test_tally_of_long_messages_and_the_prune_against_the_reference(L_max, M, f32):
    """Messages of 63, 64, 65, 128 and 129 ids (kMapIdBlock = 64) that name slots of every 64-slot trip, the last slot last; then the prune
    decision and its compaction.  Margins of the view test asserted first, as test_map_reference does."""
    rng = np.random.default_rng(29 + L_max + M + int(f32))
    cfg = MapConfig(0.9, 0.1, 3, 0.5, 10)
    st = MR.crafted_state(rng, M, f32)
    MR.check_margins(MR.as_stored(st["x"], f32), M, cfg, f"M = {M}")
    seen = np.zeros(L_max, dtype=np.int32); expected = np.zeros(L_max, dtype=np.int32)
    for k in LC.TALLY_LENGTHS:
        meas = LC.tally_message(rng, st, k)
        named = MR.message_ids(meas, k, k + 1)
        assert int(st["ids"][M - 1]) in named and len({int(np.nonzero(st["ids"] == i)[0][0]) // 64 for i in named if i in st["ids"]}) == -(-M // 64)
        ref_s, ref_e = MR.reference_tally(st["x"], st["ids"], meas, k, k + 1, 0, 0, seen, expected, cfg, f32)
        got = MR.hook(st, L_max, f32, cfg, meas=meas, count=k, k_stride=k + 1, seen=seen, expected=expected)
        assert got["seen"].tolist() == ref_s.tolist() and got["expected"].tolist() == ref_e.tolist(), (M, k)
        assert got["M"] == M and not got["mask"].any() and ref_s[M - 1] == seen[M - 1] + 1
        seen, expected = ref_s, ref_e
    mask = MR.reference_decide(seen, expected, M, L_max, cfg)
    ref = MR.reference_remove(st["x"], st["P"], st["ids"], mask, L_max, seen, expected, f32)
    got = MR.hook(st, L_max, f32, cfg, seen=seen, expected=expected, prune=True)
    assert got["mask"].tolist() == mask.tolist() and 0 < mask.sum() < M, (M, "the prune decision removes some and keeps some")
    assert got["M"] == ref["M"] and MR.same_bits(got["x"], ref["x"]) and MR.same_bits(got["P"], ref["P"]) and got["ids"].tolist() == ref["ids"].tolist()
    assert got["seen"].tolist() == ref["seen"].tolist() and got["expected"].tolist() == ref["expected"].tolist()
    print(f"map L_max {L_max} M {M} {'f32' if f32 else 'f64'}: tally of {LC.TALLY_LENGTHS} ids, pruned {int(mask.sum())}, "
          f"{LC.compact_chunks(ref['M'], 4 if f32 else 8)} chunks; 1 instance compared")


# ---- 5. fix: hook == reference ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,M,f32", LC.FIX_CASES, ids=LC.FIX_IDS)
def test_fix_hook_against_the_reference_in_bits(oracle, L_max, M, f32):
    """Every scenario of HOWS with position, heading and both at n = 3 + 2 M, the capacity included, then one oracle step from the hook's
    state against its twin from the reference's."""
    O = oracle
    rng = np.random.default_rng(43 + L_max + M + int(f32))
    x, P = _state(rng, M, f32)
    ids = (100 + np.arange(M)).astype(np.int32)
    todo = [(how, kinds) for how in HOWS[:-1] for kinds in LC.FIX_KINDS]
    verdicts = set()
    for how, kinds in todo:
        row = fix_row(rng, x, how)
        got, ref = _compare_fix(x, P, L_max, row, kinds, f32, f"n {3 + 2 * M}, {how}, kinds {kinds}")
        verdicts.add(int(got["verdict"]))
        assert FR.model_bytes([M], [got["verdict"]], 4 if f32 else 8) > 0
    assert {0x11, 0x12, 0x01, 0x10, 0x02, 0x20, 0x21, 0x04, 0x40, 0x44} <= verdicts, sorted(hex(v) for v in verdicts)
    row = fix_row(rng, x, "near")
    got, ref = _compare_fix(x, P, L_max, row, 3, f32, "the fix before the step")
    cur = dict(x=got["x"], ids=ids)
    dets = [IR.detection(rng, cur, 0), IR.detection(rng, cur, M - 1)]
    a, fa = IR.oracle_step(O, dict(x=got["x"], P=got["P"], ids=ids), (0.05, 0.01), dets, default_config(), L_max, f32)
    b, fb = IR.oracle_step(O, dict(x=ref["x"], P=ref["P"], ids=ids), (0.05, 0.01), dets, default_config(), L_max, f32)
    assert fa == fb == 0 and a["M"] == b["M"] == M
    assert R.same_bits(a["x"], b["x"]) and R.same_bits(a["P"], b["P"])
    rule = LC.fix_rule(L_max)
    print(f"fix L_max {L_max} M {M} n {3 + 2 * M} {'f32' if f32 else 'f64'}: LDS {rule['lds']}{' (limit raised)' if rule['full_lds'] else ''}, {len(todo) + 1} fixes compared, verdicts {sorted(hex(v) for v in verdicts)}")
