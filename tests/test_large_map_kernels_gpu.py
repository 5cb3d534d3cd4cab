"""The kernels around the step on the MI355X at maps beyond 66 landmarks, up to the capacity of 1000: the device against the host hook (the
kernels' own per-instance functions compiled for the host) IN BITS for every instance, the bytes of a checkpoint outside what a call may
change, the records against the fixed-order sums, the byte models of slam_last_*_work, and one plain step afterwards against the CPU
oracle in bits.  test_large_map_hooks_cpu.py holds the other leg - hook against the independent numpy references - and asserts every
premise of the case tables (large_map_cases.py) without a GPU.  States are crafted (merge_reference.crafted_state,
map_reference.crafted_state, test_fix_reference._state) and loaded through a checkpoint, as test_consistency_gpu does.

Each of these kernels decomposes the landmark slots in its own way; none inherits anything from the step kernel's size classes:
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
  merge   launch_merge_find (merge_kernel.hip) picks one of three instantiations by L_max - split over four wavefronts up to 64, one slot
          per lane up to 256, up to kMergeOwn = 4 slots per lane (j = tid + k * 256) beyond: 64 | 65, 256 | 257, the third owned slot from
          513, the fourth from 769.  Panel depth TP = clamp(57344 / (32 npad), 1, 8): 126 (7), 147 (6), 177 (5), 222 (4), 297 (3), 447 (1),
          each with landmark counts that are no multiple of TP.  lds + 8192 > 64 KiB raises the kernel's LDS limit (slam_allow_full_lds,
          lds_attr.h) from L_max 895; launch_merge_fuse does at 8 (4 (3 + 2 L_max) + 2) + 4096 > 64 KiB, from 959: both boundaries on
          both sides, and the capacity holding 998 - 1000 landmarks.  Duplicates straddle every owner index - (5, 261), (255, 256),
          (300, 700), (511, 512), (767, 768), (2, M - 1) - with an adjacent pair and a chain a - b - c across owners whose c is not mutual.
  map     map_compact_kernel (map_kernel.hip): wavefront 0 builds the kept list 64 slots at a time (M = 64, 65, 128, 129, 999, 1000;
          the removal sets of map_reference and "exactly slots 63 and 64", "one whole 64-slot trip", "every slot but the last"); P is
          compacted in place in chunks of 256 lanes x kMapChunk = 8 elements, up to 1959 of them; the tally walks messages of 63, 64, 65,
          128 and 129 ids in blocks of kMapIdBlock = 64.
  fix     fix_instance_kernel (fix_kernel.hip): 256 lanes per instance over n = 255, 257, 511, 513 and 2003 rows, every scenario of
          test_fix_gpu.HOWS, position, heading and both, at every size; launch_fix raises the LDS limit at 8 (6 n + 3) + 4096 > 64 KiB,
          from L_max 639: 638 | 639 in fp32, 639 and 1000 in fp64.
A frozen instance rides in every handle: it carries its flag on purpose, is compared like the others and is counted.  pytest -s prints, per
case, L_max, the landmark counts, the path and the number of instances compared."""
import os

import numpy as np
import pytest

import assoc_reference as AR
import fix_reference as FR
import innovation_reference as IR
import large_map_cases as LC
import map_reference as MR
from batch_state import ckpt_layout
from test_assoc_gpu import _config
from test_consistency_gpu import _write
from test_fix_gpu import _check_fix, _fix_row
from test_fix_gpu import _hooks as _fix_hooks
from test_fix_reference import _state as _fix_state
from record_tree import MAX_ENTRY_8, fixed_order_record
from test_gate_gpu import _same_bits
from test_map_gpu import S, _model_bytes, _same_state  # noqa: F401
from test_merge_gpu import _hooks as _merge_hooks
from test_merge_gpu import _merge_model_bytes

pytestmark = pytest.mark.gpu

FROZEN = IR.INST_INDEX_OOR
TRUTH = np.array([0.3, -0.2, 0.4])


def _load(S, L_max, f32, states, status, tmp_path, cfg):
    """A handle whose instances hold the crafted states (dicts of x, P, ids, M), through a checkpoint; the state read back is the state
    written, in bits."""
    insts = [dict(P=st["P"], x=st["x"], M=st["M"], ids=st["ids"], truth=TRUTH, status=int(s)) for st, s in zip(states, status)]
    dt = S.F32 if f32 else S.F64
    path = tmp_path / "crafted.ckpt"
    _write(S, L_max, dt, insts, path, tmp_path)
    f = S.BatchedEKF(len(insts), L_max, dtype=dt).readParams(cfg)
    f.load_state(path)
    os.remove(path); os.remove(tmp_path / "init.ckpt")
    assert f.status().tolist() == [int(s) for s in status]
    return f


def _rows(f, tmp_path):
    """The per-instance rows of a checkpoint: dict name -> [B] list of bytes (test_map_gpu._items for any batch)."""
    p = tmp_path / "rows.ckpt"
    f.save_state(p)
    _, off, hd = ckpt_layout(p)
    raw = open(p, "rb").read()
    os.remove(p)
    out = {}
    for name, (o, nb) in off.items():
        sz = nb // hd["B"]
        out[name] = [raw[o + b * sz:o + (b + 1) * sz] for b in range(hd["B"])]
    return out


def _unmoved(raw0, raw1, names, instances, what):
    for b in instances:
        for name in names:
            assert raw0[name][b] == raw1[name][b], (what, b, name, "the call does not touch it")


def _step_against_the_oracle(O, f, cfg, start, status, msgs, L_max, f32, what):
    """One plain step of every instance on its message; the oracle continued from `start` (the hooks' states) for the instances that
    step, the state unchanged for the frozen ones.  Returns the number of instances compared (all of them)."""
    nb = len(start)
    k = max(len(m) for m in msgs)
    meas = np.zeros((nb, k, 3), np.float32); cnt = np.zeros(nb, np.int32)
    for b, m in enumerate(msgs):
        meas[b, :len(m)] = np.asarray(m, dtype=np.float32).reshape(-1, 3); cnt[b] = len(m)
    cmds = np.stack([np.linspace(0.01, 0.02, nb), np.linspace(-0.01, 0.01, nb)], axis=1).astype(np.float32)
    ts = [f.get_state(b)["timestep"] for b in range(nb)]
    f.update(cmds, meas, cnt)
    status1 = f.status()
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    for b in range(nb):
        final = f.get_state(b)
        if status[b] & FROZEN:
            assert _same_state(final, start[b]) and status1[b] == status[b], (what, b, "a frozen instance does not step")
            continue
        ekf = O.OracleEKF(cfg, L_max=L_max, mode=mode)
        ekf.set_state(start[b]["x"], start[b]["P"], start[b]["ids"], timestep=int(ts[b]))
        fl = ekf.update(cmds[b, 0], cmds[b, 1], meas[b, :cnt[b]])
        twin = ekf.state()
        assert fl == status1[b] and _same_state(final, twin), (what, b, int(status1[b]), int(fl), final["M"], twin["M"], "the step after differs from the oracle")
    return nb


def _step_kernel(f, L_max, f32):
    """The step kernel behind a filter call, by name: class 403 at L_max 129 in fp64, the streamed kernel at 201 (and at 129 in fp32)."""
    name = f.kernel_info()["name"]
    assert name.startswith("ekf_step_kernel<403,") if (L_max == 129 and not f32) else name == "ekf_big_step_kernel", (L_max, f32, name)
    return name


# ---- 1. and 6. association, and the step behind it ---------------------------------------------------------------------------------------------
KS = IR.MAX_DET + 2
SENTINEL = 7.0


def _packed(msgs):
    meas = np.full((len(msgs), KS, 3), SENTINEL, dtype=np.float32)
    for b, m in enumerate(msgs):
        meas[b, :len(m)] = np.asarray(m, dtype=np.float32).reshape(-1, 3)
    return meas, np.array([len(m) for m in msgs], dtype=np.int32)


@pytest.mark.parametrize("L_max,f32", LC.ASSOC_CASES, ids=LC.ASSOC_IDS)
def test_association_at_every_trip_edge_and_the_associated_step_behind_it(S, tmp_path, L_max, f32):
    """Five instances of different landmark counts (one past a workgroup of four wavefronts, so a workgroup mixes trip counts), two ticks:
    slam_associate against the hook in bits for every instance, the record, a checkpoint that does not move; what each role is about is
    asserted on the device's own output.  At L_max 129 (step class 403) and 201 (the streamed kernel) slam_step_associated then equals,
    byte for byte, the plain step of a twin on the hook-labelled message."""
    from test_assoc_gpu import _check_against_hooks
    from test_assoc_gpu import _hooks as _assoc_hooks
    cfg = _config(S)
    Ms = LC.ASSOC_HANDLES[L_max]
    nb = len(Ms)
    rng = np.random.default_rng(131 + L_max + int(f32))
    states = [LC.assoc_state(role, M, f32, rng) for role, M in zip(LC.ASSOC_ROLES, Ms)]
    status = np.zeros(nb, np.int32)
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    assert all(_same_state(f.get_state(b), states[b]) for b in range(nb)), "the state read back is the crafted state"
    nonfinite = [b for b in range(nb) if not np.isfinite(f.get_state(b)["x"]).all()]
    assert nonfinite == [2, 3], "the two lone instances hold NaN landmarks on purpose; they are compared like the others"
    cmds = np.stack([np.linspace(0.005, 0.02, nb), np.linspace(-0.01, 0.01, nb)], axis=1).astype(np.float32)
    raw0 = _rows(f, tmp_path)
    lines = []
    for tick in (0, 1):
        meas, cnt = _packed([LC.assoc_messages(role, st, rng, None if tick == 0 else LC.ASSOC_TICK2[b])
                             for b, (role, st) in enumerate(zip(LC.ASSOC_ROLES, states))])
        r = f.associate(cmds, meas, cnt)
        hooks = _assoc_hooks(S, f, cmds, meas, cnt, cfg, None)
        _check_against_hooks(r, hooks, r["meas_out"], r["count_out"], meas, cnt, f"assoc L_max {L_max} tick {tick}")
        assert all((r["meas_out"][b, cnt[b]:] == SENTINEL).all() for b in range(nb)), "something was written from count_in up"
        _unmoved(raw0, _rows(f, tmp_path), list(raw0), range(nb), "slam_associate")
        if tick == 0:
            first = (meas, cnt, r, hooks)
            for b, (role, M) in enumerate(zip(LC.ASSOC_ROLES, Ms)):
                sl = LC.assoc_slots(role, M)
                if role == "tie":
                    assert r["slot"][b, 0] == r["slot"][b, 1] == sl[0] and _same_bits(r["det"][b, 0, 0], r["det"][b, 0, 1]), (b, "the lower slot keeps the tie")
                elif role == "near" and M > 1:
                    assert r["slot"][b, :2].tolist() == list(sl) and hooks[b]["cost"][0, sl[1]] == r["det"][b, 0, 1] and hooks[b]["cost"][1, sl[0]] == r["det"][b, 1, 1], b
                elif role.startswith("lone"):
                    assert r["slot"][b, 0] == sl[0] and np.isnan(r["det"][b, 0, 1]) and np.isfinite(hooks[b]["cost"][0]).sum() == 1, b
                lines.append(f"M {M} ({-(-M // 64)} trips) {role} {sl}")
            assert not r["flags"].any() and r["rec"][4] == r["n_match"].sum() >= nb
        else:
            assert r["flags"].tolist() == [0, 0, 0, IR.TOO_LONG, 0] and r["count_out"][0] == 0 and r["rec"][3] == 0 + 1 + 64 + 64
        assert f.last_associate_work()[0] > 0
    behind = ""
    if L_max in LC.STEP_BEHIND:
        meas, cnt, r, hooks = first                                   # the first tick's messages: updates in every trip of every map
        s = f.step_associated(cmds, meas, cnt)
        assert np.array_equal(s["n_drop"], r["n_drop"]) and _same_bits(s["rec"], r["rec"])
        twin = _load(S, L_max, f32, states, status, tmp_path, cfg)
        twin.update(cmds, np.stack([h["meas_out"] for h in hooks]), np.array([h["count_out"] for h in hooks], dtype=np.int32))
        a, t = _rows(f, tmp_path), _rows(twin, tmp_path)
        assert sorted(a) == sorted(t)
        _unmoved(t, a, list(t), range(nb), "slam_step_associated against the plain step on the hook-labelled message")
        assert f.landmark_counts().sum() > sum(Ms) and r["n_match"].sum() >= 2 * nb, "the step updated and inserted"
        assert sorted(b for b in range(nb) if not np.isfinite(f.get_state(b)["x"]).all()) == nonfinite, "no other instance became non-finite"
        behind = f"; associated step == plain step ({_step_kernel(f, L_max, f32)})"
        twin.close()
    print(f"assoc L_max {L_max} {'f32' if f32 else 'f64'}: " + "; ".join(lines) + f"; second tick of {LC.ASSOC_TICK2} detections{behind}; "
          f"{nb} instances compared on each of 2 ticks ({len(nonfinite)} with NaN landmarks)")
    f.close()


@pytest.mark.parametrize("L_max,f32", LC.JOINT_CASES, ids=LC.JOINT_IDS)
def test_joint_association_at_every_trip_edge_and_the_joint_step_behind_it(S, tmp_path, L_max, f32):
    """Three instances of different landmark counts (one past a workgroup of two), two ticks: slam_associate_joint against the hook in bits
    for every instance (candidate counts, nodes and d2_joint too), the record, a checkpoint that does not move.  The cluster instance has
    more than SLAM_JOINT_MAX_CAND landmarks inside the individual gate, over three trips where the map has them.  At L_max 129 and 201
    slam_step_associated_joint then equals, byte for byte, the plain step of a twin on the hook-labelled message."""
    import joint_reference as JR
    from test_joint_gpu import _check_against_hooks
    from test_joint_gpu import _hooks as _joint_hooks
    cfg = _config(S)
    Ms = LC.JOINT_HANDLES[L_max]
    roles = [LC.joint_role(role, L_max) for role in LC.JOINT_ROLES]
    nb = len(Ms)
    rng = np.random.default_rng(171 + L_max + int(f32))
    states = [LC.joint_state(role, M, f32, rng) for role, M in zip(roles, Ms)]
    status = np.zeros(nb, np.int32)
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    assert all(_same_state(f.get_state(b), states[b]) for b in range(nb)), "the state read back is the crafted state"
    assert [b for b in range(nb) if not np.isfinite(states[b]["x"]).all()] == [2], "the lone instance holds NaN landmarks on purpose"
    cmds = np.stack([np.linspace(0.005, 0.02, nb), np.linspace(-0.01, 0.01, nb)], axis=1).astype(np.float32)
    raw0 = _rows(f, tmp_path)
    lines = []
    for tick in (0, 1):
        meas, cnt = _packed([LC.joint_messages(role, st, rng, None if tick == 0 else LC.JOINT_TICK2[b]) for b, (role, st) in enumerate(zip(roles, states))])
        r = f.associate_joint(cmds, meas, cnt)
        hooks = _joint_hooks(S, f, cmds, meas, cnt, cfg, None, None)
        _check_against_hooks(r, hooks, r["meas_out"], r["count_out"], meas, cnt, f"joint L_max {L_max} tick {tick}")
        assert all((r["meas_out"][b, cnt[b]:] == SENTINEL).all() for b in range(nb)), "something was written from count_in up"
        _unmoved(raw0, _rows(f, tmp_path), list(raw0), range(nb), "slam_associate_joint")
        if tick == 0:
            first = (meas, cnt, r, hooks)
            e, l = LC.assoc_slots("near", Ms[0])
            assert r["ncand"][0, :2].tolist() == [2, 2] and sorted(r["slot"][0, :2].tolist()) == [e, l]
            sl = LC.cluster_slots(Ms[1])
            inside = [j for j in range(Ms[1]) if np.isfinite(hooks[1]["cost"][0, j]) and hooks[1]["cost"][0, j] <= JR.joint_cfg().gate_match]
            assert len(inside) > JR.MAX_CAND and set(inside) <= set(sl) and r["ncand"][1, 0] == JR.MAX_CAND and r["slot"][1, 0] in inside, (inside, r["ncand"][1, 0])
            lo, hi = LC.cluster_tie(Ms[1])
            order = sorted(inside, key=lambda j: (hooks[1]["cost"][0, j], j))
            assert _same_bits(hooks[1]["cost"][0, lo], hooks[1]["cost"][0, hi]) and order[3:5] == [lo, hi], (order, "the 4th and 5th best tie in bits")
            s0 = LC.assoc_slots(roles[2], Ms[2])[0]
            assert cnt[2] == 1 and r["slot"][2, 0] == s0 and r["ncand"][2, 0] == 1
            assert not r["flags"].any()
            lines = [f"M {Ms[0]} near {(e, l)}", f"M {Ms[1]} cluster of {len(inside)} inside the gate in trips {[LC.trip(j) for j in inside]}",
                     f"M {Ms[2]} {roles[2]} {s0} with k = 1"]
        else:
            assert r["count_out"][0] == 0 and r["flags"][2] & IR.TOO_LONG and not r["flags"][1] & IR.TOO_LONG
    behind = ""
    if L_max in LC.STEP_BEHIND:
        meas, cnt, r, hooks = first                                   # the first tick's messages
        s = f.step_associated_joint(cmds, meas, cnt)
        assert np.array_equal(s["n_drop"], r["n_drop"]) and _same_bits(s["rec"], r["rec"])
        twin = _load(S, L_max, f32, states, status, tmp_path, cfg)
        twin.update(cmds, np.stack([h["meas_out"] for h in hooks]), np.array([h["count_out"] for h in hooks], dtype=np.int32))
        a, t = _rows(f, tmp_path), _rows(twin, tmp_path)
        _unmoved(t, a, list(t), range(nb), "slam_step_associated_joint against the plain step on the hook-labelled message")
        assert a["P"][1] != raw0["P"][1], "the step moved the state"
        behind = f"; joint step == plain step ({_step_kernel(f, L_max, f32)})"
        twin.close()
    print(f"joint L_max {L_max} {'f32' if f32 else 'f64'}: " + "; ".join(lines) + f"; second tick of {LC.JOINT_TICK2} detections{behind}; "
          f"{nb} instances compared on each of 2 ticks (1 with NaN landmarks)")
    f.close()


# ---- 2. and 6. gate and innovation, and the step behind the gate -----------------------------------------------------------------------------
@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", sorted(LC.FILTER_HANDLES))
def test_gate_and_innovation_up_to_capacity_and_the_gated_step_behind_them(S, tmp_path, L_max, f32):
    """slam_gate and slam_innovation against their hooks in bits for every instance, on messages that name the first and the last slots,
    both sides of the first 64-slot boundary, exactly SLAM_INNOV_MAX_LM = 16 distinct landmarks and one more; nothing moves.  At L_max
    129 and 201 slam_step_gated then equals, byte for byte, the plain step of a twin on the hook-filtered message."""
    import gate_reference as GR
    from test_gate_gpu import _check_against_hooks
    from test_gate_gpu import _hooks as _gate_hooks
    from test_innovation_gpu import _against_hook
    cfg = _config(S)
    Ms = LC.FILTER_HANDLES[L_max] + (LC.FILTER_HANDLES[L_max][0],)
    nb = len(Ms)
    rng = np.random.default_rng(211 + L_max + int(f32))
    states = [AR.grid_state(rng, M, f32) for M in Ms]
    status = np.zeros(nb, np.int32); status[nb - 1] = FROZEN
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    assert all(_same_state(f.get_state(b), states[b]) for b in range(nb)), "the state read back is the crafted state"
    msgs = [LC.filter_messages(rng, st) for st in states]
    cmds = np.stack([np.linspace(0.005, 0.02, nb), np.linspace(-0.01, 0.01, nb)], axis=1).astype(np.float32)
    raw0 = _rows(f, tmp_path)
    names = [m[0] for m in msgs[0]]
    for t in range(len(names)):                                       # every instance sees every message once
        pick = [msgs[b][(t + b) % len(names)] for b in range(nb)]
        meas, cnt = _packed([p[1] for p in pick])
        r = f.gate(cmds, meas, cnt)
        hooks = _gate_hooks(S, f, cmds, meas, cnt, cfg, None)
        _check_against_hooks(r, hooks, r["meas_out"], r["count_out"], meas, cnt, f"gate L_max {L_max} tick {t}")
        for b, p in enumerate(pick[:nb - 1]):
            assert r["flags"][b] == p[3] and (p[2] is None or r["verdict"][b, :len(p[2])].tolist() == p[2]), (t, b, p[0])
        assert r["flags"][nb - 1] == IR.FROZEN
        i = f.innovation(cmds, meas, cnt)
        _against_hook(f, i, cmds, meas, cnt, cfg, None, f"innovation L_max {L_max} tick {t}")
        assert [int(v) for v in i["flags"]] == [p[3] for p in pick[:nb - 1]] + [IR.FROZEN]
    _unmoved(raw0, _rows(f, tmp_path), list(raw0), range(nb), "slam_gate and slam_innovation")
    behind = ""
    if L_max in LC.STEP_BEHIND:
        s = f.step_gated(cmds, meas, cnt)
        assert np.array_equal(s["n_rej"], r["n_rej"]) and _same_bits(s["rec"], r["rec"]) and s["n_rej"].sum() > 0
        twin = _load(S, L_max, f32, states, status, tmp_path, cfg)
        twin.update(cmds, np.stack([h["meas_out"] for h in hooks]), np.array([h["count_out"] for h in hooks], dtype=np.int32))
        a, tw = _rows(f, tmp_path), _rows(twin, tmp_path)
        _unmoved(tw, a, list(tw), range(nb), "slam_step_gated against the plain step on the hook-filtered message")
        assert a["P"][0] != raw0["P"][0], "the step moved the state"
        behind = f"; gated step == plain step ({_step_kernel(f, L_max, f32)})"
        twin.close()
    print(f"gate and innovation L_max {L_max} {'f32' if f32 else 'f64'}: M {list(Ms[:-1])} + frozen, messages {names}{behind}; "
          f"{nb} instances compared on each of {len(names)} ticks (1 frozen)")
    f.close()


# ---- 4. duplicate find and merge ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L_max,f32", LC.MERGE_CASES, ids=LC.MERGE_IDS)
def test_duplicates_and_the_merge_at_every_kind_panel_depth_and_lds_branch(S, oracle, tmp_path, L_max, f32):
    """Three instances holding L_max, L_max - 1 and L_max - 2 landmarks and a frozen fourth: slam_map_duplicates, then slam_map_merge (find,
    fuse, compaction) or, in the fp64 handles up to 513, slam_merge_landmarks on the find's pairs, against the hook in bits, what a merge may not touch, record, n_merged and the bytes model, then one step."""
    O = oracle
    cfg = _config(S)
    rule, fuse = LC.merge_find_rule(L_max), LC.merge_fuse_rule(L_max)
    counts = LC.merge_counts(L_max)
    crafted = [LC.merge_state(L_max, M, f32) for M in counts]
    states = [c[0] for c in crafted] + [crafted[0][0]]
    status = np.array([0, 0, 0, FROZEN], np.int32)
    nb = len(states)
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    before = [f.get_state(b) for b in range(nb)]
    assert all(_same_state(before[b], states[b]) for b in range(nb)), "the state read back is the crafted state"
    raw0 = _rows(f, tmp_path)
    esz = 4 if f32 else 8

    partner, d2 = f.map_duplicates()
    hooks = _merge_hooks(S, before, status, L_max, f32, fuse=False)
    wrong = [b for b in range(nb) if partner[b].tolist() != hooks[b]["partner"].tolist() or not _same_bits(d2[b], hooks[b]["d2"])]
    assert not wrong, f"L_max {L_max}: instance(s) {wrong} differ from the hook's decision"
    for b, (_, pairs, (a, m, c)) in enumerate(crafted):
        for i, j in pairs + [(a, m)]:
            assert partner[b, i] == j and partner[b, j] == i, (b, i, j)
        assert partner[b, c] == -1 and np.isfinite(d2[b, c]) and (partner[b] >= 0).sum() == 2 * len(pairs) + 2, (b, "the chain's c is not mutual")
    assert (partner[3] == -1).all() and np.isnan(d2[3]).all(), "a frozen instance offers no pair"
    _unmoved(raw0, _rows(f, tmp_path), list(raw0), range(nb), "slam_map_duplicates")
    elig = [(3 + 2 * st["M"]) ** 2 + 3 + 2 * st["M"] for st, s in zip(before, status) if not s]
    assert f.last_merge_work()[0] == float(sum(elig) * esz + nb * (8 + 4 * L_max + 16))

    by_pairs = LC.merge_by_pairs(L_max, f32)
    ignored = 3                                                       # (the three chains' c, counted by the find)
    if by_pairs:                                                      # slam_merge_landmarks: the find's pairs and entries to ignore
        rows = [LC.caller_pairs(partner[b], crafted[b % 3][2], before[b]["M"], L_max) for b in range(nb)]
        caller = np.stack([row for row, _ in rows]); ignored = sum(n for _, n in rows)
        r = f.merge_landmarks(caller)
        hooks = _merge_hooks(S, before, status, L_max, f32, partner=caller)
    else:
        r = f.map_merge()
        hooks = _merge_hooks(S, before, status, L_max, f32)
    after = [f.get_state(b) for b in range(nb)]
    raw1 = _rows(f, tmp_path)
    wrong = [b for b in range(nb) if not _same_state(after[b], hooks[b])]
    assert not wrong, f"L_max {L_max}: instance(s) {wrong} differ from the hook's merged state"
    merged = np.array([before[b]["M"] - hooks[b]["M"] for b in range(nb)], dtype=np.int32)
    assert np.array_equal(r["n_merged"], merged) and merged.tolist() == [len(c[1]) + 1 for c in crafted] + [0]
    assert _same_bits(fixed_order_record(np.stack([h["rec"] for h in hooks]), MAX_ENTRY_8), r["rec"]), r["rec"]
    assert r["rec"][0] == 3 and r["rec"][1] == merged.sum() and r["rec"][2] == ignored and r["rec"][3] == 0
    assert f.last_merge_work()[0] == _merge_model_bytes(before, status, hooks, L_max, esz, False, not by_pairs)
    _unmoved(raw0, raw1, ("flags", "timestep", "truth", "err"), range(nb), "slam_map_merge")
    _unmoved(raw0, raw1, ("P", "x", "M", "ids"), [3], "slam_map_merge on a frozen instance")
    for b in range(3):
        ids_row = np.frombuffer(raw1["ids"][b], dtype=np.int32)
        assert not ids_row[hooks[b]["M"]:].any() and ids_row[:hooks[b]["M"]].tolist() == hooks[b]["ids"].tolist(), (b, "ids are zero from M' up")

    rng = np.random.default_rng(190 + L_max)
    msgs = []
    for b in range(nb):
        st = after[b]
        i, j = crafted[b % 3][1][0]
        kept = st["ids"].tolist().index(int(states[b]["ids"][i]))
        msgs.append([AR.clean(rng, st, kept, float(st["ids"][kept])), AR.clean(rng, st, st["M"] - 1, float(st["ids"][st["M"] - 1])),
                     AR.clean(rng, st, kept, float(states[b]["ids"][j]))])       # the dropped id comes back as a new landmark
    compared = _step_against_the_oracle(O, f, cfg, hooks, status, msgs, L_max, f32, f"merge L_max {L_max}")
    assert [f.get_state(b)["M"] for b in range(3)] == [hooks[b]["M"] + 1 for b in range(3)]
    print(f"merge L_max {L_max} {'f32' if f32 else 'f64'}: M {list(counts)} + frozen, kind {rule['kind']}, TP {rule['TP']}, find LDS {rule['lds']}"
          f"{' (limit raised)' if rule['full_lds'] else ''}, fuse LDS {fuse['lds']}{' (limit raised)' if fuse['full_lds'] else ''}, owned slots "
          f"{1 + (L_max - 1) // 256 if rule['kind'] == 2 else 1}, fused {merged.tolist()} by {'slam_merge_landmarks' if by_pairs else 'slam_map_merge'}; {compared} instances compared (1 frozen)")
    f.close()


# ---- 3. map removal, tally and prune ----------------------------------------------------------------------------------------------------------
def _sets(L_max, M):
    """One instance per removal set (nine); at the capacity the sets are shared out between the handles of 1000 and of 999 landmarks."""
    sets = [k for k in LC.REMOVAL_SETS if k != "random"]
    if L_max < LC.CAPACITY:
        return sets
    first = ["slot 0", "alternating"] + list(LC.NEW_REMOVAL_SETS)
    return first if M == L_max else [k for k in sets if k not in first] + ["slot 0"]


@pytest.mark.parametrize("L_max,M,f32", LC.MAP_CASES, ids=LC.MAP_IDS)
def test_tally_removal_and_prune_at_the_trip_edges_and_with_thousands_of_chunks(S, oracle, tmp_path, L_max, M, f32):
    """One instance per removal set, the last one frozen.  Five tallies of 63 .. 129 ids, slam_remove_landmarks, slam_map_prune on the
    compacted maps, each against the hook in bits with the counters, then one step."""
    O = oracle
    cfg = _config(S)
    mc = S.MapConfig(0.9, 0.1, 3, 0.5, 10)
    vision = (cfg.range_max, cfg.fov_min, cfg.fov_max)
    sets = _sets(L_max, M)
    nb = len(sets)
    rng = np.random.default_rng(61 + L_max + M + int(f32))
    states = [MR.crafted_state(rng, M, f32) for _ in range(nb)]
    status = np.zeros(nb, np.int32); status[nb - 1] = FROZEN
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    before = [f.get_state(b) for b in range(nb)]
    assert all(_same_state(before[b], states[b]) for b in range(nb)), "the state read back is the crafted state"
    esz = 4 if f32 else 8

    # the tally: every instance sees every message length once
    ks = max(LC.TALLY_LENGTHS) + 1
    seen = np.zeros((nb, L_max), np.int32); expected = np.zeros((nb, L_max), np.int32)
    for t in range(len(LC.TALLY_LENGTHS)):
        meas = np.full((nb, ks, 3), 7.0, np.float32); cnt = np.zeros(nb, np.int32)
        for b in range(nb):
            k = LC.TALLY_LENGTHS[(t + b) % len(LC.TALLY_LENGTHS)]
            meas[b, :k] = LC.tally_message(rng, states[b], k); cnt[b] = k
        f.map_tally(meas, cnt, cfg=mc)
        for b in range(nb):
            h = S.map_instance_host(before[b]["x"], np.zeros((3 + 2 * M, 3 + 2 * M)), before[b]["ids"], L_max, int(status[b]), meas=meas[b],
                                    count=int(cnt[b]), k_stride=ks, vision=vision, f32_storage=f32, cfg=mc, seen=seen[b], expected=expected[b])
            seen[b], expected[b] = h["seen"], h["expected"]
        ds, de = f.map_track()
        assert np.array_equal(ds, seen) and np.array_equal(de, expected), (t, "the counters after the tally")
    assert seen[:nb - 1, M - 1].min() == 5 and not seen[nb - 1].any() and (expected > seen).any(), "the last slot was named every time; the frozen one is not tallied"
    raw0 = _rows(f, tmp_path)

    # the removal by mask
    mask = rng.integers(0, 2, (nb, L_max)).astype(np.int32)           # (entries at or above M are ignored)
    for b, kind in enumerate(sets):
        mask[b, :M] = LC.removal_mask(kind, M, rng)
    r = f.remove_landmarks(mask)
    hooks = [S.map_instance_host(st["x"], st["P"], st["ids"], L_max, int(status[b]), f32_storage=f32, cfg=mc, seen=seen[b], expected=expected[b],
                                 remove=mask[b, :M]) for b, st in enumerate(before)]
    after = [f.get_state(b) for b in range(nb)]
    raw1 = _rows(f, tmp_path)
    wrong = [sets[b] for b in range(nb) if not _same_state(after[b], hooks[b])]
    assert not wrong, f"L_max {L_max} M {M}: the removal sets {wrong} differ from the hook"
    removed = np.array([M - h["M"] for h in hooks], dtype=np.int32)
    assert np.array_equal(r["n_removed"], removed) and removed.tolist() == [int(mask[b, :M].sum()) for b in range(nb)]
    n2 = 3 + 2 * np.array([h["M"] for h in hooks])
    inst = np.zeros((nb, 16)); inst[:, 0] = removed > 0; inst[:, 1] = removed; inst[:, 2] = np.where(removed > 0, n2.astype(np.float64) ** 2, 0.0)
    assert _same_bits(fixed_order_record(inst, MAX_ENTRY_8), r["rec"]), r["rec"]
    assert f.last_map_work()[0] == _model_bytes([M] * nb, removed, L_max, esz, False, True)
    ds, de = f.map_track()
    seen = np.stack([h["seen"] for h in hooks]); expected = np.stack([h["expected"] for h in hooks])
    assert np.array_equal(ds, seen) and np.array_equal(de, expected), "the counters move with their slots"
    _unmoved(raw0, raw1, ("flags", "timestep", "truth", "err"), range(nb), "slam_remove_landmarks")
    _unmoved(raw0, raw1, ("P", "x", "M", "ids"), [b for b in range(nb) if removed[b] == 0], "slam_remove_landmarks with nothing to remove")
    for b in np.nonzero(removed)[0]:
        assert not np.frombuffer(raw1["ids"][b], dtype=np.int32)[hooks[b]["M"]:].any(), (sets[b], "ids are zero from M' up")
    chunks = {sets[b]: LC.compact_chunks(hooks[b]["M"], esz) if removed[b] else 0 for b in range(nb)}

    # the prune of the compacted maps, decided from the counters that moved
    r = f.map_prune(cfg=mc)
    pruned = [S.map_instance_host(h["x"], h["P"], h["ids"], L_max, int(status[b]), f32_storage=f32, cfg=mc, seen=seen[b], expected=expected[b],
                                  prune=True) for b, h in enumerate(hooks)]
    final = [f.get_state(b) for b in range(nb)]
    wrong = [sets[b] for b in range(nb) if not _same_state(final[b], pruned[b])]
    assert not wrong, f"L_max {L_max} M {M}: after the prune the instances {wrong} differ from the hook"
    gone = np.array([h["M"] - p["M"] for h, p in zip(hooks, pruned)], dtype=np.int32)
    assert np.array_equal(r["n_removed"], gone) and gone.sum() > 0 and r["rec"][1] == gone.sum()
    assert f.last_map_work()[0] == _model_bytes([h["M"] for h in hooks], gone, L_max, esz, True, True)
    ds, de = f.map_track()
    assert np.array_equal(ds, np.stack([p["seen"] for p in pruned])) and np.array_equal(de, np.stack([p["expected"] for p in pruned]))

    msgs = []
    for b in range(nb):
        st = final[b]
        m = [AR.clean(rng, st, j, float(st["ids"][j])) for j in sorted({0, st["M"] - 1} if st["M"] else set())]
        msgs.append(m + [[5000.0, 1.7, -0.6]])                        # and a new landmark
    compared = _step_against_the_oracle(O, f, cfg, pruned, status, msgs, L_max, f32, f"map L_max {L_max} M {M}")
    print(f"map L_max {L_max} M {M} {'f32' if f32 else 'f64'}: tallies of {LC.TALLY_LENGTHS} ids, chunks of P per removal set {chunks}, "
          f"pruned {gone.tolist()}; {compared} instances compared (1 frozen)")
    f.close()


# ---- 5. fixes ------------------------------------------------------------------------------------------------------------------------------------
FIXES = [("near", 3), ("far_pos", 3), ("far_yaw", 3), ("nan_sigma", 1), ("neg_sigma", 2), ("inf_z", 3), ("near", 1), ("near", 2), ("near", 3)]


@pytest.mark.parametrize("L_max,M,f32", LC.FIX_CASES, ids=LC.FIX_IDS)
def test_the_fix_at_every_pass_edge_of_the_256_lanes_and_at_capacity(S, oracle, tmp_path, L_max, M, f32):
    """One instance per (scenario, kinds) of FIXES - every scenario of test_fix_gpu.HOWS, at the capacity too - the last one frozen; the
    rejected and invalid rows write nothing, also where launch_fix raises the LDS limit (L_max >= 639).  slam_fix against the hook in bits (state, verdict, nis, record, bytes), what
    a fix may not touch, then one step."""
    O = oracle
    cfg = _config(S)
    todo = FIXES
    nb = len(todo)
    rng = np.random.default_rng(83 + L_max + M + int(f32))
    states = []
    for b in range(nb):
        x, P = _fix_state(rng, M, f32)
        states.append(dict(x=x, P=P, ids=(100 + rng.permutation(M)).astype(np.int32), M=M))
    status = np.zeros(nb, np.int32); status[nb - 1] = FROZEN
    f = _load(S, L_max, f32, states, status, tmp_path, cfg)
    before = [f.get_state(b) for b in range(nb)]
    assert all(_same_state(before[b], states[b]) for b in range(nb)), "the state read back is the crafted state"
    raw0 = _rows(f, tmp_path)
    fix = np.stack([_fix_row(rng, before[b]["x"], how) for b, (how, _) in enumerate(todo)])
    kinds = np.array([k for _, k in todo], np.int32)
    r = f.fix(fix, kinds)
    after = [f.get_state(b) for b in range(nb)]
    raw1 = _rows(f, tmp_path)
    hooks = _fix_hooks(S, before, status, L_max, f32, fix, kinds)
    what = f"fix L_max {L_max} M {M}"
    hv = _check_fix(S, f, r, before, status, hooks, after, f32, what)
    want = [0x11, 0x12, 0x21, 0x04, 0x40, 0x44, 0x01, 0x10, 0x00]
    assert hv.tolist() == want, [hex(v) for v in hv]
    applied = ((hv & 15) == 1) | ((hv >> 4) == 1)
    assert r["rec"][0] == applied.sum() and r["rec"][13] == 1, "one frozen instance is skipped"
    _unmoved(raw0, raw1, ("M", "ids", "flags", "timestep", "truth", "err"), range(nb), "slam_fix")
    _unmoved(raw0, raw1, ("P", "x"), np.nonzero(~applied)[0], "slam_fix without an applied part")
    assert all(raw0["P"][b] != raw1["P"][b] for b in np.nonzero(applied)[0])
    start = [dict(x=h["x"], P=h["P"], ids=before[b]["ids"], M=M) for b, h in enumerate(hooks)]
    msgs = [[AR.clean(rng, st, j, float(st["ids"][j])) for j in (0, M // 2, M - 1)] for st in after]
    compared = _step_against_the_oracle(O, f, cfg, start, status, msgs, L_max, f32, what)
    print(f"{what} n {3 + 2 * M} {'f32' if f32 else 'f64'}: passes of 256 lanes over the rows {-(-(3 + 2 * M) // 256)}, LDS {LC.fix_rule(L_max)['lds']}{' (limit raised)' if LC.fix_rule(L_max)['full_lds'] else ''}, verdicts {[hex(v) for v in hv]}, "
          f"bytes {f.last_fix_work()[0]:.0f}; {compared} instances compared (1 frozen)")
    f.close()
