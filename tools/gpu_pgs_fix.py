#!/usr/bin/env python3
"""Absolute fixes as unary pose factors of the pose graph (pgs_fix*, pgs_fix_sense*, pgs_run_sim_fix) on one MI355X: what they do to a graph
that loses its landmarks, and what they cost.  Prints; asserts nothing.

Part 1, the effect.  Graphs of --effect-poses poses (L = --landmarks) built by the device-side simulator whose landmarks are OUT OF VIEW FOR
THE MIDDLE THIRD (the simulator's map is swapped for one far out of range for those ticks): the stretch is odometry integrated open loop.
The same seed is solved four ways: with no fixes; with position fixes every 10 poses (half-width --fix-halfwidth, sigma = half-width /
sqrt 3); with 5 % of the fixes jumping by 1 to 3 m and no fix loss; with the same jumps and Geman-McClure (k = 3) on the fixes.  Printed per
variant: the batch-mean position error of the result against the simulator's truth over each third of the poses (the truth is read tick by
tick with a noiseless pgs_fix_sense, which advances nothing), and the fix parts stored / jumped.

Part 2, the cost.  Batch --batch graphs of --poses poses, built once without fixes and once with a position + heading fix every 10 poses
(pgs_run_sim_fix), solved --reps times ALTERNATING in the same process: milliseconds per solve (host clock around a synchronised solve),
mean lambda trials, and from a profiled solve the milliseconds in the linearise and evaluate launches - the two kernels a fix adds work to.
Medians; one JSON line per part."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _handle(S, B, N, L, KP, lm, seed):
    pg = S.BatchedPoseGraph(B, num_iterations=N, L_max=L, k_per_pose=KP).readParams()
    pg.set_map(lm); pg.set_seed(seed); pg.init(0.0, 0.0, 0.0)
    return pg


def effect(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, every = args.landmarks, args.effect_batch, args.effect_poses - 1, 10
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    far = lm + 1e4                                                  # every landmark out of range: no detections
    a = args.fix_halfwidth
    exact = dict(kinds=3)                                           # zero half-widths: the emitted row IS the truth
    clean = dict(pos_halfwidth=a, sigma_pos=a / math.sqrt(3.0), kinds=S.FIX_POS)
    jumps = dict(clean, p_jump=0.05, jump_lo=1.0, jump_hi=3.0)
    variants = [("no_fixes", None, None), ("position_fixes", clean, None), ("jumps_gaussian", jumps, None), ("jumps_geman_mcclure", jumps, (2, 3.0))]
    thirds = [(0, T // 3), (T // 3, 2 * T // 3), (2 * T // 3, T + 1)]
    out = dict(tool="gpu_pgs_fix", part="effect", L=L, batch=B, poses=T + 1, fix_every=every, fix_halfwidth=a, landmarks_out_of_view=[T // 3, 2 * T // 3])
    for name, sensor, loss in variants:
        pg = _handle(S, B, T + 1, L, args.k_per_pose, lm, 2025)
        truth = np.zeros((B, T + 1, 2))
        stored = jumped = 0
        for t in range(T):
            if t == T // 3:
                pg.set_map(far)
            if t == 2 * T // 3:
                pg.set_map(lm)
            pg.run_sim(cmds[t:t + 1])
            pg.set_fix_sensor(exact)
            truth[:, t + 1] = pg.fix_sense()["fix"][:, :2]
            if sensor and (t + 1) % every == 0:
                pg.set_fix_sensor(sensor)
                s = pg.fix_sense()
                v = pg.fix(s["fix"], s["kinds"])
                stored += int(np.count_nonzero(v & 15 == 1)); jumped += int(s["jumped"].sum())
        if loss:
            pg.set_fix_robust(*loss)
        t0 = time.perf_counter()
        pg.solvePoseGraph(); pg.sync()
        ms = (time.perf_counter() - t0) * 1e3
        st = pg.stats()
        err = np.zeros((B, T + 1))
        for b in range(B):
            p = pg.get_graph(b, 1)["poses"]
            err[b] = np.hypot(p[:, 0] - truth[b, :, 0], p[:, 1] - truth[b, :, 1])
        row = dict(mean_error_m_per_third=[round(float(err[:, lo:hi].mean()), 4) for lo, hi in thirds], fix_parts_stored=stored, jumped=jumped,
                   solve_ms=round(ms, 2), mean_trials=round(float(st["trials"].mean()), 2), flagged=int(np.count_nonzero(st["flags"] & 24)))
        if loss:
            w = pg.fix_weights(1)[:, :, 0]
            row["fix_parts_with_w_below_half"] = int(np.count_nonzero(w < 0.5))
        out[name] = row
        pg.close()
    print(json.dumps(out), flush=True)


def cost(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = args.landmarks, args.batch, args.poses - 1
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    sensor = dict(pos_halfwidth=args.fix_halfwidth, sigma_pos=args.fix_halfwidth / math.sqrt(3.0), yaw_halfwidth=0.02, sigma_yaw=0.02 / math.sqrt(3.0), kinds=3)
    handles = {}
    for name in ("without", "with"):
        pg = _handle(S, B, T + 1, L, args.k_per_pose, lm, 2025)
        if name == "with":
            pg.set_fix_sensor(sensor)
            pg.run_sim_fix(cmds, 10)
        else:
            pg.run_sim(cmds)
        pg.solvePoseGraph(); pg.sync()                               # warm-up: allocations, code objects
        handles[name] = pg
    ms = {k: [] for k in handles}
    for _ in range(args.reps):
        for name, pg in handles.items():
            t0 = time.perf_counter()
            pg.solvePoseGraph(); pg.sync()
            ms[name].append((time.perf_counter() - t0) * 1e3)
    out = dict(tool="gpu_pgs_fix", part="cost", L=L, batch=B, poses=T + 1, fix_every=10, reps=args.reps)
    for name, pg in handles.items():
        st = pg.stats()
        pg.set_profiling(True)
        pg.solvePoseGraph(); pg.sync()
        k = pg.last_solve_kernel_ms()
        pg.set_profiling(False)
        parts = sum(int(np.count_nonzero(pg.fixes(b)["kinds"] & 1)) + int(np.count_nonzero(pg.fixes(b)["kinds"] & 2)) for b in range(min(B, 4)))
        out[name] = dict(solve_ms_median=round(statistics.median(ms[name]), 3), solve_ms_min=round(min(ms[name]), 3), mean_trials=round(float(st["trials"].mean()), 2),
                         profiled_linearize_ms=round(k["linearize"], 3), profiled_evaluate_ms=round(k["evaluate"], 3), fix_parts_in_first_4_graphs=parts)
        pg.close()
    a, b = out["without"], out["with"]
    out["per_trial_ms"] = dict(without=round(a["solve_ms_median"] / max(a["mean_trials"], 1e-9), 4), **{"with": round(b["solve_ms_median"] / max(b["mean_trials"], 1e-9), 4)})
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--k-per-pose", type=int, default=8)
    ap.add_argument("--effect-poses", type=int, default=301)
    ap.add_argument("--effect-batch", type=int, default=32)
    ap.add_argument("--fix-halfwidth", type=float, default=0.1)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", choices=("effect", "cost"))
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    if args.only != "cost":
        effect(S, args)
    if args.only != "effect":
        cost(S, args)


if __name__ == "__main__":
    main()
