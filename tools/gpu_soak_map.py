#!/usr/bin/env python3
"""Map-edit soak of the batched EKF against the composed CPU reference of tests/edit_walk.py (BIT-EXACT): a simulated run with landmarks
leaving the state in the middle of it.  Random size class (L_max 20 / 50 / 100 and the streamed 66 fp32 / 201 fp64), storage type, batch,
seed, instance offset, SLAM_RUN_CHUNK, lazy steps, known or unknown ids, shared or per-instance commands, and a random interleaving of
update_sim (one step), run_sim (many steps per launch), slam_remove_landmarks (random masks), tally ticks + slam_map_prune, slam_map_merge,
getters and checkpoint / resume into a NEW handle.  At the end x, P, ids, M, flags, timestep, truth, error statistics and track counters of
every instance equal the walker's.  A program whose prune or merge decision comes within the references' margins of a threshold (where libm
and the library agree to an ulp, not to the bit) is drawn again, not compared.
usage: gpu_soak_map.py [seconds] [seed]"""
import os, sys, time, tempfile
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from oracle import oracle as O
import live_ekf_slam_amd as S
import edit_walk as EW

budget = float(sys.argv[1]) if len(sys.argv) > 1 else 120.0
rng = np.random.default_rng(int(sys.argv[2]) if len(sys.argv) > 2 else 1)
t_end = time.time() + budget
runs = fails = redrawn = 0
CLASSES = [(20, 17, False), (20, 17, True), (50, 40, False), (50, 40, True), (100, 60, False), (66, 40, True), (201, 30, False)]
while time.time() < t_end:
    L_max, L, f32 = CLASSES[int(rng.integers(0, len(CLASSES)))]
    B = int(rng.integers(1, 13))
    seed, inst0 = int(rng.integers(1, 1 << 30)), int(rng.integers(0, 1 << 20))
    known = rng.random() < 0.8
    each = rng.random() < 0.4
    fill = rng.random() < 0.5
    lazy = [None, 0, 2, 16][int(rng.integers(0, 4))]       # (None: the handle's default queue)
    chunk = int(rng.choice([1, 2, 7, 1000]))
    T = int(rng.integers(30, 140))
    os.environ["SLAM_RUN_CHUNK"] = str(chunk)
    desc = f"L_max={L_max} L={L} f32={f32} B={B} seed={seed} inst0={inst0} known={known} each={each} fill={fill} lazy={lazy} chunk={chunk} T={T}"
    if os.environ.get("SOAK_VERBOSE"): print("RUN", desc, flush=True)
    setup = EW.make_setup(S, B, L_max, L, f32, seed, inst0, pairs=3 if known else 0, id_known=int(known))
    cmds = EW.drive_commands(T, B if each else None, rng)
    mc = S.MapConfig(0.9, 0.1, int(rng.integers(2, 6)), 0.5, 10)
    gc = S.MergeConfig(0.5, 0.1, 5)
    # the program (what the walker runs) and, next to each entry, how the handle is driven through it
    program, how, log = [], [], []
    t = 0
    if fill:
        program += [("vision", EW.UNLIMITED), ("run", cmds[:1]), ("vision", EW.DEFAULT_VISION)]; how += ["op", "simN", "op"]; t = 1
    while t < T:
        op = str(rng.choice(["sim1", "simN", "simN", "remove", "prune", "merge" if known else "remove", "get", "ckpt"]))
        if op in ("sim1", "simN"):
            n = 1 if op == "sim1" else int(rng.integers(1, 40))
            program.append(("run", cmds[t:t + n])); how.append(op); t = min(T, t + n)
        elif op == "remove":
            program.append(("remove", (rng.random((B, L_max)) < rng.choice([0.1, 0.5, 1.0])).astype(np.int32))); how.append("op")
        elif op == "prune":
            n = int(rng.integers(2, 9))
            withheld = frozenset(int(i) for i in rng.choice(L, 3, replace=False))
            program += [("tally_ticks", cmds[t:t + n], withheld, mc), ("prune", mc)]; how += ["op", "op"]; t = min(T, t + n)
        elif op == "merge":
            program.append(("merge", gc)); how.append("op")
        elif op == "ckpt":
            program.append(("track_reset",)); how.append("ckpt")         # (the counters are outside the checkpoint format)
        else:
            program.append(("run", cmds[t:t])); how.append("get")
        log.append(op)
    try:
        walks = [EW.walk(O, setup, program, b) for b in range(B)]
    except EW.OnMargin:
        redrawn += 1
        continue
    f = EW.make_handle(S, setup, lazy=lazy)
    for seg, (op, h) in enumerate(zip(program, how)):
        if h == "sim1":
            f.update_sim(op[1][0])
        elif h == "get":
            b = int(rng.integers(0, B)); k = int(rng.integers(0, 4))
            if k == 0: f.get_state(b)
            elif k == 1: f.poses()
            elif k == 2: f.map_track()
            else: f.status()
        elif h == "ckpt":
            with tempfile.NamedTemporaryFile(suffix=".ckpt") as tf:
                f.save_state(tf.name)
                g = EW.make_handle(S, setup, lazy=lazy); g.load_state(tf.name)
            g.set_noise(setup.rows); g.set_map(np.ascontiguousarray(setup.maps))
            f.close(); f = g
        else:       # (the tally is fed the walker's messages: reading the handle's own would switch every later run to one step per launch)
            EW.drive_op(f, op, tally=EW.tally_messages(walks, seg, L_max) if op[0] == "tally_ticks" else None)
    bad =EW.differing(EW.snapshots(f), [w["final"] for w in walks])
    edits = sum(e["M_after"] < e["M"] for w in walks for e in w["edits"])
    f.close()
    runs += 1
    if os.environ.get("SOAK_VERBOSE"): print(f"  {edits} instance edits that dropped landmarks, M at the end {[w['final']['M'] for w in walks]}", flush=True)
    if bad:
        fails += 1
        print(f"MISMATCH {desc}: instances (fields) {bad[:8]}; ops: {' | '.join(log)[:600]}", flush=True)
if redrawn > runs:
    print(f"WARNING: more programs drawn again on a margin ({redrawn}) than compared ({runs}): the soak spends its time on the CPU")
print(f"{runs} random map-edit programs in {budget:.0f} s ({redrawn} drawn again on a margin), {fails} mismatches")
sys.exit(1 if fails or not runs else 0)
