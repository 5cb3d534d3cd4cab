"""The composed reference of a simulated run with map edits in it: one instance of a handle walked on the CPU through a PROGRAM of
segments and edits.  A helper: no tests in here, and nothing in here needs a GPU.

A program is a list of
    ("run", cmds)                         cmds (T, 2) shared or (T, B, 2) per instance: T simulated ticks
    ("remove", mask)                      mask (B, L_max): slam_remove_landmarks
    ("tally_ticks", cmds, withheld_ids)   simulated ticks, each followed by the tally of its message without the detections whose id is
                                          in withheld_ids (a withheld slot is expected and never seen)
    ("prune", map_cfg)                    slam_map_prune
    ("merge", merge_cfg)                  slam_map_merge
    ("vision", (range_max, fov_min, fov_max))   slam_set_vision for the ticks that follow
    ("track_reset",)                      slam_map_track_reset
The walker composes the pieces that exist: OracleSim.step_philox and OracleEKF.update for the ticks (the simulator's RNG step of a tick is
the handle's tick counter, EkfStepParams::step), map_reference / merge_reference for the edits, OracleEKF.set_state to go on from an
edited state.  With hooks=S the edits are done by the library's host hooks (map_instance_host, merge_instance_host) instead.
drive() is the same program on a handle.  It never reads slam_get_last_meas from that handle: the first such call switches the handle's
measurement dump on for good, and a handle with the dump on issues every later run one step per launch (capi_step.cpp), which is not
the path these tests are about.  The tally of a handle is fed the walker's messages instead (tally_messages); test_run_after_map_edit_gpu
reads the device's own on a handle that runs nothing afterwards and finds the same bits."""
import numpy as np

import innovation_reference as IR
import map_reference as MR
import merge_reference as GR

EDITS = ("remove", "prune", "merge")


class OnMargin(AssertionError):
    """A prune or merge decision of a program lies within the references' margins of a threshold: change the input, or draw it again."""


def _margin(check, *args):
    try:
        check(*args)
    except AssertionError as e:
        raise OnMargin(*e.args) from e
DEFAULT_VISION = MR.VISION


class Setup:
    """What a handle of B instances is made of: the config, one noise row and one map per instance (rows / maps indexed by the instance's
    place in the handle), L_max, the storage type, the seed and the global id of instance 0."""

    def __init__(self, cfg, rows, maps, L_max, f32, seed, inst0, init=(0.0, 0.0, 0.0)):
        self.cfg, self.rows, self.maps, self.L_max, self.f32, self.seed, self.inst0, self.init = cfg, rows, maps, int(L_max), bool(f32), seed, inst0, init
        self.B = len(maps)

    def part(self, lo, hi):
        """The instances lo .. hi - 1 as a handle of their own (a shard)."""
        return Setup(self.cfg, [self.rows[b] for b in range(lo, hi)], self.maps[lo:hi], self.L_max, self.f32, self.seed, self.inst0 + lo, self.init)


def part_program(program, lo, hi):
    """The program of the instances lo .. hi - 1."""
    out = []
    for op in program:
        if op[0] in ("run", "tally_ticks") and np.ndim(op[1]) == 3:
            op = (op[0], op[1][:, lo:hi]) + tuple(op[2:])
        elif op[0] == "remove":
            op = ("remove", op[1][lo:hi])
        out.append(op)
    return out


def filter_config(setup, b):
    """The oracle filter's config of instance b: IR.config_for of its row, with the handle's settings that are not noise (the handle's
    replicate_vw_quirk maps the row's keys to the effective V / W)."""
    c = IR.config_for(setup.rows[b])
    for name in ("replicate_vw_quirk", "landmark_id_is_known", "min_landmark_separation", "ekf_abs_is_int", "ekf_landmark_from_x_pred"):
        setattr(c, name, getattr(setup.cfg, name))
    return c


def sim_config(setup, b, vision=None):
    """The simulator's side of a noise row: the handle's config with the half-widths of the row's sim_* fields."""
    c = setup.cfg.copy()
    r = setup.rows[b]
    c.V_00, c.V_11, c.W_00, c.W_11 = r.sim_V_00, r.sim_V_11, r.sim_W_00, r.sim_W_11
    c.init_x, c.init_y, c.init_yaw = setup.init
    if vision is not None:
        c.range_max, c.fov_min, c.fov_max = vision
    return c


def _snap(st, flags, truth, errsum, seen, expected):
    ts = st["timestep"]
    return dict(x=st["x"].copy(), P=st["P"].copy(), ids=np.asarray(st["ids"], np.int32).copy(), M=st["M"], flags=int(flags), timestep=ts,
                truth=np.array(truth), errsum=errsum, avg_err=errsum / ts if ts > 0 else 0.0, seen=seen.copy(), expected=expected.copy())


def walk(O, setup, program, b, hooks=None, margins=True, keep_meas=False):
    """Instance b of the handle through the program.  Returns dict(final, after (one snapshot per edit, in order), ticks, edits, wire):
    snapshots of x, P, ids, M, flags, timestep, truth, errsum, avg_err, seen, expected; ticks = one dict per simulated tick (seg: index of
    the program entry, kind "run" or "tally_ticks", k detections, inserted, reinserted, M before; of a tally tick also tally: its message
    without the withheld detections; with keep_meas the detected ids and the message); edits = one dict per edit (kind, dropped ids,
    withheld dropped, fused pairs); wire = the float32 (x, y, yaw) estimate before every tick (what a controller reads)."""
    L_max, f32 = setup.L_max, setup.f32
    g = setup.inst0 + b
    lm = np.ascontiguousarray(setup.maps[b], dtype=np.float64)
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    ekf = O.OracleEKF(filter_config(setup, b), L_max=L_max, mode=mode)
    ekf.init(*setup.init)
    vision = (setup.cfg.range_max, setup.cfg.fov_min, setup.cfg.fov_max)
    sim = O.OracleSim(lm, sim_config(setup, b))
    truth = np.array(setup.init, dtype=np.float64)
    flags, t, errsum = 0, 0, 0.0
    seen = np.zeros(L_max, np.int32); expected = np.zeros(L_max, np.int32)
    observed, withheld_all = set(), set()
    ticks, edits, after, wire = [], [], [], []

    def tick(cmd, seg, kind):
        nonlocal truth, flags, t, errsum
        st0 = ekf.state()
        wire.append(st0["x"][:3].astype(np.float32))
        truth, meas = sim.step_philox(cmd[0], cmd[1], setup.seed, g, t)
        flags |= ekf.update(cmd[0], cmd[1], meas)
        st = ekf.state()
        errsum = errsum + O.average_error([float(np.float32(st["x"][0]))], [float(np.float32(st["x"][1]))], [truth[0]], [truth[1]], math=O.MATH_DET)
        t += 1
        got = {int(m[0]) for m in meas}
        inserted = st["M"] - st0["M"]
        ticks.append(dict(seg=seg, kind=kind, k=len(meas), inserted=inserted, reinserted=max(0, inserted - len(got - observed)), M=st0["M"]))
        if keep_meas:
            ticks[-1]["ids"] = sorted(got); ticks[-1]["meas"] = np.array(meas, dtype=np.float32).reshape(-1, 3)
        observed.update(got)
        return meas, st

    def put(new):
        ekf.set_state(new["x"], new["P"], new["ids"], timestep=t)

    for seg, op in enumerate(program):
        kind = op[0]
        if kind in ("run", "tally_ticks"):
            cmds = np.asarray(op[1], dtype=np.float32)
            cmds = cmds[:, b] if cmds.ndim == 3 else cmds
            for c in cmds:
                meas, st = tick(c, seg, kind)
                if kind == "tally_ticks":
                    withheld_all.update(op[2])
                    kept = np.asarray([m for m in meas if int(m[0]) not in op[2]], dtype=np.float32).reshape(-1, 3)
                    ticks[-1]["tally"] = kept
                    cfg = op[3] if len(op) > 3 else None
                    if margins:
                        _margin(MR.check_margins, MR.as_stored(st["x"], f32), st["M"], cfg or MR.default_map_config(), (g, t), vision)
                    if hooks is not None:
                        h = hooks.map_instance_host(st["x"], st["P"], st["ids"], L_max, flags, meas=kept, count=len(kept), k_stride=max(len(kept), 1),
                                                    vision=vision, f32_storage=f32, cfg=cfg, seen=seen, expected=expected)
                        seen, expected = h["seen"], h["expected"]
                    else:
                        s2, e2 = MR.reference_tally(st["x"], st["ids"], kept, len(kept), max(len(kept), 1), flags, 0, seen[:st["M"]], expected[:st["M"]],
                                                    cfg or MR.default_map_config(), f32, vision)
                        seen[:st["M"]], expected[:st["M"]] = s2, e2
        elif kind == "vision":
            vision = tuple(op[1])
            sim = O.OracleSim(lm, sim_config(setup, b, vision))
            O.lib().orc_sim_reset(sim.h, truth[0], truth[1], truth[2])
        elif kind == "track_reset":
            seen[:] = 0; expected[:] = 0
        elif kind in EDITS:
            st = ekf.state()
            M = st["M"]
            info = dict(kind=kind, seg=seg, M=M, fused=0)
            if kind == "merge":
                cfg = op[1]
                if hooks is not None:
                    new = hooks.merge_instance_host(st["x"], st["P"], st["ids"], L_max, flags, f32, cfg, seen=seen, expected=expected)
                else:
                    new = GR.reference_merge(st["x"], st["P"], st["ids"], L_max, cfg, flags, f32, seen=seen, expected=expected)
                    if margins and new["D"] is not None:
                        pairs = [(s, int(p)) for s, p in enumerate(new["partner"][:M]) if p > s]
                        _margin(GR.check_margins, new["D"], pairs, cfg.gate_merge, (g, t))
                info["fused"] = M - new["M"]
            else:
                if kind == "remove":
                    mask = np.asarray(op[1][b][:M], dtype=np.int32)
                elif hooks is None:
                    mask = MR.reference_decide(seen, expected, M, L_max, op[1])[:M]
                if hooks is not None:
                    new = hooks.map_instance_host(st["x"], st["P"], st["ids"], L_max, flags, f32_storage=f32, cfg=op[1] if kind == "prune" else None,
                                                  seen=seen, expected=expected, remove=mask if kind == "remove" else None, prune=kind == "prune")
                else:
                    new = MR.reference_remove(st["x"], st["P"], st["ids"], mask, L_max, seen, expected, f32)
            kept = set(int(i) for i in new["ids"])
            info["dropped"] = [int(i) for i in st["ids"] if int(i) not in kept]
            info["withheld_dropped"] = [i for i in info["dropped"] if i in withheld_all] if kind == "prune" else []
            if new["M"] != M:
                put(new)
                seen, expected = np.array(new["seen"], np.int32), np.array(new["expected"], np.int32)
            info["M_after"] = new["M"]
            edits.append(info)
            after.append(_snap(ekf.state(), flags, truth, errsum, seen, expected))
        else:
            raise ValueError(f"unknown program entry {kind!r}")
    return dict(final=_snap(ekf.state(), flags, truth, errsum, seen, expected), after=after, ticks=ticks, edits=edits, wire=wire)


def same_snapshot(a, b, counters=True):
    """Every bit of two snapshots: the names of the fields that differ (an empty list: the same)."""
    bad = []
    if a["M"] != b["M"] or np.asarray(a["ids"], np.int32).tolist() != np.asarray(b["ids"], np.int32).tolist():
        bad.append("M/ids")
    for name in ("x", "P", "truth"):
        if np.ascontiguousarray(a[name], dtype=np.float64).tobytes() != np.ascontiguousarray(b[name], dtype=np.float64).tobytes():
            bad.append(name)
    if a["flags"] != b["flags"]:
        bad.append("flags")
    if a["timestep"] != b["timestep"]:
        bad.append("timestep")
    if np.float64(a["avg_err"]).tobytes() != np.float64(b["avg_err"]).tobytes():
        bad.append("avg_err")
    if counters and not (np.array_equal(a["seen"], b["seen"]) and np.array_equal(a["expected"], b["expected"])):
        bad.append("track counters")
    return bad


# ---- the same program on a handle ----------------------------------------------------------------------------------------------------------
def make_handle(S, setup, lazy=None):
    """A handle of the setup.  lazy: slam_set_lazy_steps (0 = no step queue; None: the handle's default, which queues simulated ticks)."""
    f = S.BatchedEKF(setup.B, setup.L_max, dtype=S.F32 if setup.f32 else S.F64).readParams(setup.cfg)
    f.set_seed(setup.seed); f.set_instance_offset(setup.inst0)
    f.set_noise(setup.rows); f.set_map(np.ascontiguousarray(setup.maps))
    if lazy is not None:
        f.set_lazy_steps(lazy)
    f.init(*setup.init)
    return f


def snapshots(f):
    """The snapshot of every instance of a handle, in the walker's fields."""
    status, truth, err = f.status(), f.truth(), f.error_stats()
    seen, expected = f.map_track()
    out = []
    for b in range(f.batch):
        st = f.get_state(b)
        out.append(dict(x=st["x"], P=st["P"], ids=st["ids"], M=st["M"], flags=int(status[b]), timestep=st["timestep"], truth=truth[b], avg_err=err[b],
                        seen=seen[b], expected=expected[b]))
    return out


def tally_messages(walks, seg, k_stride):
    """What map_tally is given after each tick of the tally segment `seg` of the program: [(meas (B, k_stride, 3), count (B,))] per tick, the
    walker's messages of those ticks without the withheld detections."""
    per = [[t["tally"] for t in w["ticks"] if t["seg"] == seg] for w in walks]
    out = []
    for k in range(len(per[0])):
        meas = np.zeros((len(walks), k_stride, 3), np.float32); cnt = np.zeros(len(walks), np.int32)
        for b, msgs in enumerate(per):
            meas[b, :len(msgs[k])] = msgs[k]; cnt[b] = len(msgs[k])
        out.append((meas, cnt))
    return out


def drive_op(f, op, run=None, tally=None):
    """One program entry on a handle.  run(f, cmds): how a "run" segment is issued (default f.run_sim); tally: tally_messages() of a
    "tally_ticks" entry.  Returns what the edit returned."""
    kind = op[0]
    if kind == "run":
        if len(op[1]):
            (run or (lambda h, c: h.run_sim(c)))(f, np.ascontiguousarray(op[1], dtype=np.float32))
    elif kind == "tally_ticks":
        cmds = np.asarray(op[1], dtype=np.float32)
        assert len(tally) == len(cmds)
        for c, (meas, cnt) in zip(cmds, tally):
            f.update_sim(c)
            f.map_tally(meas, cnt, cfg=op[3] if len(op) > 3 else None)
    elif kind == "vision":
        f.set_vision(*op[1])
    elif kind == "track_reset":
        f.map_track_reset()
    elif kind == "remove":
        return f.remove_landmarks(op[1])
    elif kind == "prune":
        return f.map_prune(cfg=op[1])
    elif kind == "merge":
        return f.map_merge(cfg=op[1])
    else:
        raise ValueError(f"unknown program entry {kind!r}")


def drive(f, program, walks, run=None, on_edit=None, seg0=0):
    """The program on a handle whose instances the walker has walked (walks: one per instance, for the tally's messages); returns (snapshots
    after every edit, final snapshots).  on_edit(index of the edit, f): a visit right after an edit and its snapshot.  seg0: the place of
    program[0] in the program that was walked, where `program` is its tail."""
    after = []
    for seg, op in enumerate(program, seg0):
        drive_op(f, op, run, tally_messages(walks, seg, f.L_max) if op[0] == "tally_ticks" else None)
        if op[0] in EDITS:
            after.append(snapshots(f))
            if on_edit is not None:
                on_edit(len(after) - 1, f)
    return after, snapshots(f)


def differing(got, want, counters=True):
    """[(instance, fields)] where the handle's snapshots differ from the walker's."""
    return [(b, bad) for b, (g, w) in enumerate(zip(got, want)) for bad in [same_snapshot(g, w, counters)] if bad]


# ---- the fixed programs of the tests ----------------------------------------------------------------------------------------------------------
SPACING = 2.0        # m between the cells of the jittered grid the maps are drawn on: about 3.5 landmarks in the normal sensor's view
UNLIMITED = (1e9, -4.0, 4.0)


def make_maps(rng, B, L, pairs):
    """B maps of L landmarks around the drive of drive_commands (a circle of 2 m radius about (0, 2)).  Rows 0 .. pairs - 1 lie 3.2 m from
    its centre, ahead of where the vehicle is at the ticks 40, 85 and 110; the last `pairs` rows are copies of them, 1 cm away: one physical
    landmark under two ids.  The other rows are the cells of a grid of SPACING m nearest to the ring the sensor sweeps, jittered by +-0.5 m
    per instance; no cell lies within 1.6 m of a pair, so two different landmarks are at least 0.9 m apart."""
    n = L - 2 * pairs
    centre = np.array([0.0, 2.0])
    phase = -np.pi / 2 + 0.03 * np.array([40.0, 85.0, 110.0, 20.0, 60.0])[:pairs] + 0.6
    first = centre + 3.2 * np.stack([np.cos(phase), np.sin(phase)], axis=1) if pairs else np.zeros((0, 2))
    side = int(np.ceil(np.sqrt(n))) + 4
    c = (np.arange(side) - (side - 1) / 2.0) * SPACING
    cells = np.array([(x + 0.3, y + 2.3) for x in c for y in c])
    cells = cells[[i for i, q in enumerate(cells) if all(np.hypot(*(q - f)) >= 1.6 for f in first)]]
    cells = cells[np.argsort(np.abs(np.hypot(cells[:, 0] - centre[0], cells[:, 1] - centre[1]) - 3.0), kind="stable")][:n]
    assert len(cells) == n
    maps = np.zeros((B, L, 2))
    for b in range(B):
        maps[b, :pairs] = first + rng.uniform(-0.1, 0.1, (pairs, 2))
        maps[b, pairs:pairs + n] = cells + rng.uniform(-0.5, 0.5, (n, 2))
        maps[b, pairs + n:] = maps[b, :pairs] + rng.uniform(-1.0, 1.0, (pairs, 2)) * 0.01 / np.sqrt(2.0)
    return maps


def make_setup(S, B, L_max, L, f32, seed, inst0, pairs=3, id_known=1):
    """test_assoc_gpu's config, the per-instance noise rows of test_map_gpu._each for a batch of B (that helper is tied to its own batch of
    257), and make_maps."""
    from test_assoc_gpu import _config
    cfg = _config(S)
    cfg.landmark_id_is_known = id_known
    rng = np.random.default_rng(seed)
    W = rng.uniform(1.5e-3, 5e-3, B)
    rows = S.config.noise_rows(cfg, B, W_00=W, W_11=W[::-1].copy(), V_00=rng.uniform(5e-5, 2e-4, B))
    return Setup(cfg, rows, make_maps(rng, B, L, pairs), L_max, f32, seed, inst0)


def drive_commands(T, B=None, rng=None):
    """A slow left turn of 2 m radius; with B, every instance's commands scaled by its own factor in [0.5, 1]."""
    cmds = np.tile(np.array([0.06, 0.03], np.float32), (T, 1))
    if B is None:
        return cmds
    return (cmds[:, None, :] * rng.uniform(0.5, 1.0, (1, B, 1))).astype(np.float32)


def removal_masks(O, setup, program_head, seed):
    """test_map_gpu._masks on the walker's states after program_head: MR.REMOVAL_SETS in turn plus random ones, one kind per instance."""
    kinds = MR.REMOVAL_SETS + ("random", "random", "random")
    rng = np.random.default_rng(seed)
    mask = rng.integers(0, 2, (setup.B, setup.L_max)).astype(np.int32)
    for b in range(setup.B):
        M = walk(O, setup, program_head, b)["final"]["M"]
        mask[b, :M] = MR.removal_mask(kinds[b % len(kinds)], M, rng)
    return mask


def _often_detected(O, setup, head, cmds, skip, want=2):
    """The `want` ids outside `skip` that instance 0's simulator detects on the most ticks of `cmds` after the program `head`."""
    seg = len(head)
    w = walk(O, setup, head + [("run", cmds)], 0, keep_meas=True)
    count = {}
    for t in w["ticks"]:
        for i in (t["ids"] if t["seg"] == seg else ()):
            count[i] = count.get(i, 0) + (i not in skip)
    return sorted(sorted(count), key=lambda i: -count[i])[:want]


def fixed_program(O, S, setup, seg=25, each=False, fill=False, edits=("remove", "prune", "merge", "merge")):
    """run T1 -> remove -> run T2 -> tally_ticks -> prune -> run T3 -> merge -> run T4 -> merge -> run T5, every segment `seg` ticks; with
    fill, a first tick under an unlimited sensor that maps every landmark.  The ids withheld from the tally are the two landmarks without
    a copy that instance 0 detects most often in the tally's ticks."""
    n_seg = 2 + len(edits) + ("prune" in edits)
    rng = np.random.default_rng(setup.seed + 1)
    cmds = drive_commands(seg * n_seg, setup.B if each else None, rng)
    L = setup.maps.shape[1]
    pairs = {i for i in range(L) if np.hypot(*(setup.maps[0, i] - setup.maps[0]).T).min(initial=1.0, where=np.arange(L) != i) < 0.1}
    mc = S.MapConfig(0.9, 0.1, 4, 0.5, 10)
    gc = S.MergeConfig(0.5, 0.1, 5)      # (the default gate would reach landmarks 1 m apart that the fill tick mapped from afar and nothing saw again)
    cut = [cmds[i * seg:(i + 1) * seg] for i in range(n_seg)]
    head = [("vision", UNLIMITED), ("run", cut[0][:1]), ("vision", DEFAULT_VISION), ("run", cut[0][1:])] if fill else [("run", cut[0])]
    program, i = list(head), 1
    for e in edits:
        if e == "remove":
            program.append(("remove", removal_masks(O, setup, head, setup.seed + 2)))
        elif e == "prune":
            withheld = frozenset(_often_detected(O, setup, program, cut[i], pairs)); i += 1
            program.append(("tally_ticks", cut[i - 1], withheld, mc))
            program.append(("prune", mc))
        else:
            program.append(("merge", gc))
        program.append(("run", cut[i])); i += 1
    return program


def preconditions(walks, need=("update_only", "reinsert", "pruned", "withheld", "fused")):
    """What the tests require of a fixed program, counted from the walker's classification over the instances: dict of counts, asserted:
    more than half of the instances have, after EVERY edit, at least 10 update-only ticks of 1 to 6 detections in "run" segments (the
    decoupled loop's: a tally's ticks are issued one per launch and do not count), and a tick that inserts a removed id again, a prune
    that drops a slot (pruned), a prune that drops a withheld slot and a fused pair somewhere; M is ragged after every edit; no flag is
    raised."""
    B = len(walks)
    n_edits = len(walks[0]["edits"])
    ok = dict(update_only=0, reinsert=0, pruned=0, withheld=0, fused=0)
    total = dict(update_only_ticks=0, reinsertions=0, instances=B)
    for w in walks:
        segs = [e["seg"] for e in w["edits"]] + [10 ** 9]
        per_edit = [sum(1 for t in w["ticks"] if t["kind"] == "run" and segs[i] < t["seg"] < segs[i + 1] and 1 <= t["k"] <= 6 and t["inserted"] == 0)
                    for i in range(n_edits)]
        re = sum(t["reinserted"] > 0 for t in w["ticks"])
        ok["update_only"] += min(per_edit) >= 10
        ok["reinsert"] += re > 0
        ok["pruned"] += any(e["kind"] == "prune" and e["M_after"] < e["M"] for e in w["edits"])
        ok["withheld"] += any(e["withheld_dropped"] for e in w["edits"])
        ok["fused"] += any(e["fused"] for e in w["edits"])
        total["update_only_ticks"] += sum(per_edit); total["reinsertions"] += re
        assert w["final"]["flags"] == 0, "an instance raised a flag"
    for name in need:
        assert ok[name] > B // 2, (name, ok, total)
    for i in range(n_edits):
        assert len({w["after"][i]["M"] for w in walks}) > 1, ("M is not ragged after edit", i)
    return dict(ok, **total)


# name -> B, L_max, landmarks of the map, fp32 storage, seed, first global id, ticks per segment, per-instance commands, fill tick, known ids
CASES = {
    "L20_f64": dict(B=96, L_max=20, L=17, f32=False, seed=411, inst0=1000, fill=False),
    "L20_f32": dict(B=96, L_max=20, L=17, f32=True, seed=412, inst0=2000, fill=False),
    "L50_f64": dict(B=96, L_max=50, L=40, f32=False, seed=413, inst0=3000, fill=True),
    "L50_f32": dict(B=96, L_max=50, L=40, f32=True, seed=414, inst0=4000, fill=True),
    "L100_f64": dict(B=24, L_max=100, L=90, f32=False, seed=415, inst0=5000, fill=True),
    "L200_f64": dict(B=6, L_max=200, L=180, f32=False, seed=416, inst0=6000, fill=True),
    "L66_f32_streamed": dict(B=12, L_max=66, L=60, f32=True, seed=417, inst0=7000, fill=True),
    "L201_M30_f64_streamed": dict(B=12, L_max=201, L=30, f32=False, seed=418, inst0=8000, fill=False),
    "L20_f64_each": dict(B=96, L_max=20, L=17, f32=False, seed=419, inst0=9000, fill=False, each=True),
    "L50_f32_each": dict(B=96, L_max=50, L=40, f32=True, seed=420, inst0=10000, fill=True, each=True),
    "L20_f64_unknown_ids": dict(B=96, L_max=20, L=14, f32=False, seed=421, inst0=11000, fill=False, pairs=0, id_known=0, edits=("remove", "prune")),
}
_cache = {}


def fixed_case(O, S, name):
    """(setup, program, walks of every instance, the counts of preconditions()) of a fixed case, computed once per process."""
    if name not in _cache:
        c = CASES[name]
        setup = make_setup(S, c["B"], c["L_max"], c["L"], c["f32"], c["seed"], c["inst0"], c.get("pairs", 3), c.get("id_known", 1))
        edits = c.get("edits", ("remove", "prune", "merge", "merge"))
        program = fixed_program(O, S, setup, c.get("seg", 25), c.get("each", False), c["fill"], edits)
        walks = [walk(O, setup, program, b) for b in range(setup.B)]
        # (without known ids the simulator's ids are not the filter's, so "a withheld id was dropped" cannot be read off the ids: there the
        # prune must drop something)
        need = ("update_only", "reinsert", "pruned") + (("withheld", "fused") if "merge" in edits else ())
        _cache[name] = (setup, program, walks, preconditions(walks, need))
    return _cache[name]
