"""Runs continued after map edits on the MI355X: every run path handed a compacted state, against the composed CPU reference of
tests/edit_walk.py (OracleSim + OracleEKF for the ticks, map_reference / merge_reference for the edits), bit for bit on every instance.

slam_remove_landmarks, slam_map_prune and slam_map_merge end in the in-place compaction of csrc/map_kernel.h and promise "an ordinary state
of fewer landmarks".  test_map_gpu (b) and test_merge_gpu (c) continue such a state with host-fed single steps only.  Here the program
    run T1 -> remove -> run T2 -> tally_ticks -> prune -> run T3 -> merge -> run T4 -> merge -> run T5        (25 ticks each)
goes through the multi-step simulator launches (slam_run_sim / slam_run_sim_each: generator wavefront, decoupled loop, resident thin rows,
insertions that switch buffers) with per-instance maps and noise rows, a seed and a non-zero instance offset; removed ids come back and are
inserted as new, the maps hold three physical landmarks under two ids each so that the merges find pairs, and M is ragged across the batch
after every edit (tests/test_edit_walk_cpu.py asserts all that of every fixed program from the walker alone).  After every edit and at the
end x, P, M, ids, status, timestep, truth, error statistics and the track counters of every instance equal the walker's.  No tolerance.

That the run segments really are multi-step launches is read from the device's counters (_took_multi_step_launches): a handle that has
once been asked for its last message (slam_get_last_meas) dumps messages from then on and runs every tick as a launch of its own, so
the tally of these handles is fed the walker's messages, which one test shows to be the device's, in bits.

Cases: 1 every size class and storage type; 2 SLAM_RUN_CHUNK 1 / 7 / whole; 3 per-instance commands; 4 unknown ids (the over-provisioned
leading dimension and its re-pack); 5 an edit on a lazy queue; 6 a checkpoint across an edit; 7 a shard; 8 the closed loop after an edit;
9 the read-only evaluators on a compacted state; 10 a monitored run after an edit; and the comparator's teeth (one ulp in one P entry)."""
import numpy as np
import pytest

import edit_walk as EW
import merge_reference as GR
from batch_state import ckpt_layout
from test_consistency_gpu import _collect as _consistency_collect, _judge as _consistency_judge
from test_failure_flags_gpu import _kernel as _kernel_of
from test_map_gpu import S, _raw  # noqa: F401
from test_monitor_gpu import _against_reference as _monitor_against_reference, _judge as _monitor_judge

pytestmark = pytest.mark.gpu

CLASSES = ["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L100_f64", "L200_f64", "L66_f32_streamed", "L201_M30_f64_streamed"]


def _kernel(f, setup):
    """The multi-step kernel instantiation of the handle is the one its size class is meant to reach (n <= 43, 103, 203, 403 with a control
    wavefront and streamers, or the streamed kernel)."""
    return _kernel_of(f, True, setup.L_max, setup.f32)


def _stamped(program, log):
    """A way to issue the "run" segments (the run= of EW.drive) that has the kernel stamp the ticks of the LAST one (debug flag 32: the
    step kernel writes (clock, detections) into slot t of a buffer at the end of tick t of its launch; the buffer is zero when the flag is
    first set): appends that segment's step_stamps to log.  Every other segment runs with no flag set."""
    last = sum(op[0] == "run" and len(op[1]) > 0 for op in program)
    seen = [0]

    def run(f, cmds):
        seen[0] += 1
        if seen[0] == last:
            f.set_debug_flags(32)
        f.run_sim(cmds)
        if seen[0] == last:
            log.append(f.step_stamps(len(cmds)))
            f.set_debug_flags(0)
    return run


def _took_multi_step_launches(log, walks, what, chunk=None):
    """The last run segment of the program, T ticks after every edit, went through launches of `chunk` ticks (None: one launch of all T),
    by the stamps the kernel left: a launch of n ticks writes the slots 0 .. n - 1 and no other, with the detections the walker counted at
    those ticks.  How slam_run_sim cuts a call into launches depends on the handle alone, not on the call (capi_step.cpp: a handle whose
    measurement dump was ever switched on runs one tick per launch from then on), so this holds for the segments before it too."""
    (stamps, k), = log
    B, T = stamps.shape
    per = min(chunk or T, T)
    assert T >= 20 and stamps.shape == (len(walks), T)
    written = stamps != 0
    assert np.array_equal(written, np.broadcast_to(np.arange(T) < per, (B, T))), (what, "slots written", written.sum(axis=1))
    if per == T:
        assert (np.diff(stamps, axis=1) >= 0).all(), (what, "the stamps of one launch go forward in time")
        want = np.array([[min(t["k"], 15) for t in w["ticks"][-T:]] for w in walks])
        assert np.array_equal(k, want), (what, "detections per tick of the launch")
    print(f"{what}: the last run segment: {T} ticks in launches of {per}")


def _compare(after, final, walks, what, counters=True):
    """Every edit's snapshots and the final ones against the walker's; returns the number of instance comparisons."""
    n = 0
    for i, snaps in enumerate(after):
        bad = EW.differing(snaps, [w["after"][i] for w in walks], counters)
        assert not bad, f"{what}: after edit {i} ({walks[0]['edits'][i]['kind']}) {len(bad)} of {len(snaps)} instance(s) differ from the walker: {bad[:10]}"
        n += len(snaps)
    bad = EW.differing(final, [w["final"] for w in walks], counters)
    assert not bad, f"{what}: at the end {len(bad)} of {len(final)} instance(s) differ from the walker: {bad[:10]}"
    return n + len(final)


def _walked(S, oracle, name):
    setup, program, walks, pre = EW.fixed_case(oracle, S, name)
    print(f"{name}: {pre}")
    return setup, program, walks


# ---- 1. size classes and storage ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", CLASSES)
def test_every_size_class_runs_on_after_every_edit_as_the_walker_does(S, oracle, name):
    setup, program, walks = _walked(S, oracle, name)
    f = EW.make_handle(S, setup)
    _kernel(f, setup)
    log = []
    after, final = EW.drive(f, program, walks, run=_stamped(program, log))
    n = _compare(after, final, walks, name)
    print(f"{name}: {n} instance comparisons, M at the end {sorted({s['M'] for s in final})}")
    assert len(after) == 4 and all(s["timestep"] == 150 for s in final)
    if "streamed" not in name:
        _took_multi_step_launches(log, walks, name)
    else:
        # ekf_big_kernel.hip leaves no stamps.  What the host decides by is the same for every kernel, though: slam_run_sim issues launches
        # of several ticks unless the handle's measurement dump is on, and only a handle whose dump is off lets a simulated tick wait in
        # its step queue (slam_step_sim).  Asked after the comparison, since it is one tick more.
        from live_ekf_slam_amd import _lib
        assert not log[0][0].any()
        f.update_sim(program[-1][1][-1])
        assert _lib.lib().slam_queued_steps(f.h) == 1, f"{name}: this handle runs one tick per launch"
    f.close()


@pytest.mark.parametrize("name", ["L20_f32", "L20_f64_unknown_ids"])
def test_the_tally_is_fed_what_the_device_measured(S, oracle, name):
    """The handles of this file are fed the walker's messages in the tally, because reading a handle's own (slam_get_last_meas) switches
    its measurement dump on for good, and with it every later run to one tick per launch.  On a handle that runs nothing afterwards: the
    messages update_sim dumps at the tally's ticks, without the withheld detections, are the walker's in bits, and so is the prune."""
    setup, program, walks = _walked(S, oracle, name)
    end = next(i for i, op in enumerate(program) if op[0] == "prune") + 1
    f = EW.make_handle(S, setup)
    KS, after, n = setup.L_max, [], 0
    for seg, op in enumerate(program[:end]):
        if op[0] == "tally_ticks":
            f.last_meas(KS)                                   # (the first call only switches the dump on)
            for c, (want, want_n) in zip(op[1], EW.tally_messages(walks, seg, KS)):
                f.update_sim(c)
                meas, cnt = f.last_meas(KS)
                got = np.zeros_like(meas); got_n = np.zeros_like(cnt)
                for b in range(setup.B):
                    kept = [m for m in meas[b, :cnt[b]] if int(m[0]) not in op[2]]
                    got[b, :len(kept)] = np.asarray(kept, dtype=np.float32).reshape(-1, 3); got_n[b] = len(kept)
                assert np.array_equal(got_n, want_n) and got.tobytes() == want.tobytes(), (name, seg)
                n += int(got_n.sum())
                f.map_tally(got, got_n, cfg=op[3])
        else:
            EW.drive_op(f, op)
        if op[0] in EW.EDITS:
            after.append(EW.snapshots(f))
    assert n > 10 * setup.B
    for i, snaps in enumerate(after):
        assert not EW.differing(snaps, [w["after"][i] for w in walks]), (name, i)
    f.close()


# ---- 2. chunking ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L50_f64", "L20_f32"])
def test_launch_boundaries_between_an_edit_and_the_next_insertion_change_no_bit(S, oracle, tmp_path, monkeypatch, name):
    setup, program, walks = _walked(S, oracle, name)
    raws = {}
    for chunk in ("1", "7", None):
        if chunk is None:
            monkeypatch.delenv("SLAM_RUN_CHUNK", raising=False)
        else:
            monkeypatch.setenv("SLAM_RUN_CHUNK", chunk)
        f = EW.make_handle(S, setup)
        log = []
        after, final = EW.drive(f, program, walks, run=_stamped(program, log))
        _compare(after, final, walks, f"{name}, SLAM_RUN_CHUNK={chunk}")
        _took_multi_step_launches(log, walks, f"{name}, SLAM_RUN_CHUNK={chunk}", chunk=chunk and int(chunk))
        raws[chunk] = (_raw(f, tmp_path), f.map_track())
        f.close()
    for chunk in ("1", "7"):
        assert raws[chunk][0] == raws[None][0], f"{name}: the checkpoint under SLAM_RUN_CHUNK={chunk} differs from the whole-call launch"
        assert all(np.array_equal(u, v) for u, v in zip(raws[chunk][1], raws[None][1]))


# ---- 3. per-instance commands -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["L20_f64_each", "L50_f32_each"])
def test_per_instance_commands(S, oracle, name):
    setup, program, walks = _walked(S, oracle, name)
    assert all(op[1].ndim == 3 for op in program if op[0] == "run")
    f = EW.make_handle(S, setup)
    _kernel(f, setup)
    log = []
    after, final = EW.drive(f, program, walks, run=_stamped(program, log))
    _compare(after, final, walks, name)
    _took_multi_step_launches(log, walks, name)
    f.close()


# ---- 4. unknown ids ---------------------------------------------------------------------------------------------------------------------------
def test_unknown_ids_the_over_provisioned_leading_dimension_and_its_re_pack(S, oracle):
    name = "L20_f64_unknown_ids"
    setup, program, walks = _walked(S, oracle, name)
    assert setup.cfg.landmark_id_is_known == 0 and [op[0] for op in program if op[0] in EW.EDITS] == ["remove", "prune"]
    f = EW.make_handle(S, setup)
    log = []
    after, final = EW.drive(f, program, walks, run=_stamped(program, log))
    _compare(after, final, walks, name)
    _took_multi_step_launches(log, walks, name)
    f.close()


# ---- 5. an edit on a lazy queue -----------------------------------------------------------------------------------------------------------------
def test_an_edit_runs_the_lazy_queue_first(S, oracle):
    """set_lazy_steps(16), five update_sim ticks, then the edit on a queue that is not empty - a removal, a prune and a merge."""
    from live_ekf_slam_amd import _lib
    name = "L20_f64"
    setup, fixed, _ = _walked(S, oracle, name)
    program = []
    for op in fixed:                     # the last five ticks before the prune are plain ticks: they wait in the queue
        program += [op[:1] + (op[1][:-5],) + op[2:], ("run", op[1][-5:])] if op[0] == "tally_ticks" else [op]
    walks = [EW.walk(oracle, setup, program, b) for b in range(setup.B)]
    assert sum(e["M_after"] < e["M"] for w in walks for e in w["edits"] if e["kind"] == "prune") > setup.B // 2
    queued = []

    def drive(lazy):
        f = EW.make_handle(S, setup, lazy=16 if lazy else 0)
        after = []
        for i, op in enumerate(program):
            if op[0] == "run" and i + 1 < len(program) and program[i + 1][0] in EW.EDITS:
                if len(op[1]) > 5:
                    f.run_sim(op[1][:-5])
                for c in op[1][-5:]:
                    f.update_sim(c)
                if lazy:
                    queued.append(_lib.lib().slam_queued_steps(f.h))
            else:
                EW.drive_op(f, op, tally=EW.tally_messages(walks, i, setup.L_max) if op[0] == "tally_ticks" else None)
            if op[0] in EW.EDITS:
                after.append(EW.snapshots(f))
        final = EW.snapshots(f)
        f.close()
        return after, final
    a1, f1 = drive(True)
    assert len(queued) == 4 and all(q > 0 for q in queued), queued
    _compare(a1, f1, walks, name + " lazy")
    a0, f0 = drive(False)
    _compare(a0, f0, walks, name + " twin without the queue")


# ---- 6. a checkpoint across an edit, and the comparator's teeth ------------------------------------------------------------------------------
def _resume(S, setup, path):
    g = EW.make_handle(S, setup)
    g.load_state(path)
    g.set_noise(setup.rows); g.set_map(np.ascontiguousarray(setup.maps))       # (inputs, not state)
    return g


def test_a_checkpoint_across_an_edit(S, oracle, tmp_path):
    name = "L20_f32"
    setup, program, walks = _walked(S, oracle, name)
    cut = next(i for i, op in enumerate(program) if op[0] == "remove") + 1
    f = EW.make_handle(S, setup)
    after, _ = EW.drive(f, program[:cut], walks)
    path = tmp_path / "edited.ckpt"
    f.save_state(path)
    g = _resume(S, setup, path)
    f.map_track_reset()          # the counters are outside the checkpoint format (the walker's are zero here: the tally comes later)
    assert all(not w["after"][0]["seen"].any() and not w["after"][0]["expected"].any() for w in walks)
    for h, what in ((f, "the original"), (g, "the resumed handle")):
        log = []
        a, fin = EW.drive(h, program[cut:], walks, run=_stamped(program[cut:], log), seg0=cut)
        _compare(after + a, fin, walks, f"{name}, {what}")
        _took_multi_step_launches(log, walks, f"{name}, {what}")
    assert _raw(f, tmp_path, "a.ckpt") == _raw(g, tmp_path, "b.ckpt")
    f.close(); g.close()


def test_the_comparator_has_teeth_one_ulp_in_one_entry_of_p(S, oracle, tmp_path):
    """One P entry of one instance one ulp off in a checkpoint taken after the removal: the comparison with the walker, the one every
    case here uses, reports that instance, that field, and nothing else."""
    name = "L20_f64"
    setup, program, walks = _walked(S, oracle, name)
    cut = next(i for i, op in enumerate(program) if op[0] == "remove") + 1
    victim = next(b for b, w in enumerate(walks) if w["after"][0]["M"] >= 3)
    f = EW.make_handle(S, setup)
    EW.drive(f, program[:cut], walks)
    path = tmp_path / "poked.ckpt"
    f.save_state(path)
    f.close()
    head, off, hd = ckpt_layout(path)
    assert hd["B"] == setup.B and hd["esz"] == 8
    ram = np.memmap(path, dtype=np.float64, mode="r+", offset=off["P"][0], shape=(setup.B * hd["pstride"],))
    i0 = victim * hd["pstride"]                     # P(0, 0) of the instance: the slab starts with row 0
    assert ram[i0] == walks[victim]["after"][0]["P"][0, 0]
    ram[i0] = np.nextafter(ram[i0], np.inf)
    ram.flush(); del ram
    g = _resume(S, setup, path)
    bad = EW.differing(EW.snapshots(g), [w["after"][0] for w in walks])
    assert bad == [(victim, ["P"])], bad
    _, final = EW.drive(g, program[cut:], walks, seg0=cut)         # (125 ticks on, rounding may have absorbed the ulp; nobody else may differ)
    bad = EW.differing(final, [w["final"] for w in walks])
    print(f"one ulp in P(0, 0) of instance {victim}: at the end of the program {bad}")
    assert [b for b, _ in bad] in ([], [victim]), bad
    g.close()


# ---- 7. a shard -------------------------------------------------------------------------------------------------------------------------------
def test_the_upper_half_as_a_handle_of_its_own(S, oracle):
    name = "L20_f64"
    setup, program, walks = _walked(S, oracle, name)
    lo = setup.B // 2
    part = setup.part(lo, setup.B)
    assert part.inst0 == setup.inst0 + lo and part.B == setup.B - lo
    f = EW.make_handle(S, part)
    log = []
    after, final = EW.drive(f, EW.part_program(program, lo, setup.B), walks[lo:], run=_stamped(program, log))
    _compare(after, final, walks[lo:], name + " upper half")
    _took_multi_step_launches(log, walks[lo:], name + " upper half")
    f.close()


# ---- 8. the closed loop after an edit -------------------------------------------------------------------------------------------------------
def test_the_closed_loop_after_an_edit(S, oracle):
    from live_ekf_slam_amd.navigation import PurePursuitBatch
    name = "L20_f64"
    setup, program, walks = _walked(S, oracle, name)
    cut = next(i for i, op in enumerate(program) if op[0] == "remove") + 1
    T = 40
    f = EW.make_handle(S, setup)
    after, _ = EW.drive(f, program[:cut], walks)
    rng = np.random.default_rng(8)
    paths = [np.array([[0.0, 2.0], [0.0, 2.0]]) + 2.4 * np.stack([np.cos(a + np.array([0.0, 0.7])), np.sin(a + np.array([0.0, 0.7]))], axis=1)
             for a in rng.uniform(0.3, 0.9, setup.B)]           # two waypoints ahead of the drive, outside its circle
    f.set_paths(paths)
    cmds = f.run_nav(T, return_cmds=True)
    assert cmds.shape == (T, setup.B, 2) and cmds.any() and np.isfinite(cmds).all()
    final = EW.snapshots(f)
    nav = f.nav_state()
    replay = program[:cut] + [("run", cmds)]
    pp = PurePursuitBatch(setup.B, paths, d_max=setup.cfg.d_max, th_max=setup.cfg.th_max)
    ws = [EW.walk(oracle, setup, replay, b) for b in range(setup.B)]
    t0 = len(ws[0]["wire"]) - T
    for t in range(T):
        want = pp.next_cmds(np.stack([w["wire"][t0 + t] for w in ws]), np.zeros(setup.B, bool))
        assert want.tobytes() == cmds[t].tobytes(), (t, np.nonzero((want != cmds[t]).any(axis=1))[0][:10])
    _compare(after, final, ws, name + " closed loop")
    assert np.array_equal(nav["remaining"], pp.remaining) and np.array_equal(nav["finish_tick"], pp.finish_tick)
    assert nav["integ"].tobytes() == pp.integ.tobytes() and nav["err_prev"].tobytes() == pp.err_prev.tobytes()
    assert sum(t["inserted"] > 0 for w in ws for t in w["ticks"][t0:]) > 0, "the closed loop inserted landmarks on the compacted state"
    f.close()


# ---- 9. read-only evaluators on a compacted state ------------------------------------------------------------------------------------------
def test_read_only_evaluators_on_a_compacted_state(S, oracle, tmp_path):
    name = "L20_f64"
    setup, program, walks = _walked(S, oracle, name)
    gc = next(op[1] for op in program if op[0] == "merge")
    kinds = ["edited"] * setup.B
    pairs = []

    def visit(i, f):
        what = f"{name} after edit {i}"
        want = [w["after"][i] for w in walks]
        assert not EW.differing(EW.snapshots(f), want), what
        raw0 = _raw(f, tmp_path)
        m, c, (partner, d2) = f.monitor_now(), f.consistency(), f.map_duplicates(cfg=gc)
        assert _raw(f, tmp_path) == raw0, what + ": an evaluator changed the state"
        pools = {}
        _monitor_against_reference(f, m, kinds, pools, what)        # (the device's state is the walker's, in bits: asserted above)
        _monitor_judge(pools, what)
        cp, _ = _consistency_collect(f, c, setup.maps, kinds)
        _consistency_judge(cp, what)
        for b, w in enumerate(want):
            r = GR.reference_find(w["x"], w["P"], w["M"], setup.L_max, gc, w["flags"], setup.f32)
            assert partner[b].tolist() == r["partner"].tolist() and GR.same_values(d2[b], r["d2"]), (what, b)
        pairs.append(int((partner >= 0).sum()) // 2)
    f = EW.make_handle(S, setup)
    log = []
    after, final = EW.drive(f, program, walks, run=_stamped(program, log), on_edit=visit)
    _compare(after, final, walks, name)
    _took_multi_step_launches(log, walks, name)
    assert len(pairs) == 4 and pairs[0] > 0, pairs
    f.close()


# ---- 10. a monitored run after an edit -----------------------------------------------------------------------------------------------------
def test_a_monitored_run_after_an_edit(S, oracle, tmp_path):
    name = "L20_f32"
    setup, program, walks = _walked(S, oracle, name)
    f = EW.make_handle(S, setup)
    after, final = EW.drive(f, program, walks, run=lambda h, c: h.monitor_run(c))
    _compare(after, final, walks, name + " monitor_run")
    g = EW.make_handle(S, setup)
    EW.drive(g, program, walks)
    assert _raw(f, tmp_path, "a.ckpt") == _raw(g, tmp_path, "b.ckpt"), "monitor_run leaves the bits of run_sim"
    f.close(); g.close()
