#!/usr/bin/env python3
"""Pose graph: build and solve of heterogeneous batches (pgs_*_each) beside the shared calls, at BASELINE configs[4] shape.

One process, one command: for each batch (default 2048 and 256) graphs of 1000 poses x 200 landmarks (k_per_pose 32, seed 2025) are built
by the device simulator and solved, three ways:
  shared    one scenario (make_scenario(1234, ...)) through set_map / init / run_sim((T, 2))
  each-1    the same scenario through the per-instance calls, every row equal: set_map((B, L, 2)) / init((B, 3)) / run_sim((T, B, 2))
  each-8    8 different scenarios (make_scenario(1234 + s, ...)), instance b runs scenario b % 8
The build (run_sim: host call to stream synchronise, host clock; it includes the copy of the commands) is timed once per handle, the solve
--reps times after one warm-up solve (HIP events around a stream synchronise; every solve starts from the same initial estimate).  One JSON
line per batch and leg with solves/s (median), all solve times, the build time, the LM trials of the solve, and at the end the ratios
each-1 / shared and each-8 / each-1 in solves/s.  The each-1 leg is checked to give the bits of the shared leg."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="2048,256")
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=200)
    ap.add_argument("--k-per-pose", type=int, default=32)
    ap.add_argument("--scenarios", type=int, default=8)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.scenario import make_scenario
    if not torch.cuda.is_available():
        sys.exit("no HIP device")
    dev = torch.device("cuda", 0)
    T, L = args.poses - 1, args.landmarks
    scen = [make_scenario(1234 + s, L, T) for s in range(args.scenarios)]
    for B in (int(b) for b in args.batches.split(",")):
        rate, first = {}, {}
        for leg in ("shared", "each-1", f"each-{args.scenarios}"):
            pg = S.BatchedPoseGraph(B, num_iterations=args.poses, L_max=L, k_per_pose=args.k_per_pose).readParams()
            stream = torch.cuda.Stream(device=dev)
            pg.set_stream(stream.cuda_stream)
            pg.set_seed(2025)
            if leg == "shared":
                pg.set_map(scen[0][0]); pg.init(0.0, 0.0, 0.0)
                cmds = scen[0][1]
            else:
                pick = np.arange(B) % (1 if leg == "each-1" else args.scenarios)
                pg.set_map(np.stack([scen[s][0] for s in pick])); pg.init(np.zeros((B, 3), np.float32))
                cmds = np.ascontiguousarray(np.stack([scen[s][1] for s in pick], axis=1))
            with torch.cuda.stream(stream):
                stream.synchronize()
                t0 = time.perf_counter()
                pg.run_sim(cmds); stream.synchronize()
                build_ms = (time.perf_counter() - t0) * 1e3
                pg.solvePoseGraph(); stream.synchronize()   # warm-up (first-call allocations, code objects)
                ms = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record(stream); pg.solvePoseGraph(); e1.record(stream)
                    stream.synchronize()
                    ms.append(e0.elapsed_time(e1))
            st = pg.stats()
            _, trials = pg.last_solve_work()
            rate[leg] = B / (statistics.median(ms) * 1e-3)
            if leg == "shared":
                first = dict(poses=pg.get_graph(B - 1, 1)["poses"], trials=st["trials"].copy())
            elif leg == "each-1":
                same = np.array_equal(first["poses"], pg.get_graph(B - 1, 1)["poses"]) and np.array_equal(first["trials"], st["trials"])
                if not same:
                    sys.exit("each-1 differs from the shared leg")
            print(json.dumps(dict(batch=B, leg=leg, solves_per_s=round(rate[leg], 1), solve_ms=[round(v, 2) for v in ms], build_ms=round(build_ms, 2),
                                  trials_launched=int(trials), lm_iterations_mean=round(float(st["iterations"].mean()), 2),
                                  flagged=int((st["flags"] != 0).sum()))), flush=True)
            pg.close()
        print(json.dumps(dict(batch=B, each_over_shared=round(rate["each-1"] / rate["shared"], 4),
                              scenarios_over_one=round(rate[f"each-{args.scenarios}"] / rate["each-1"], 4))), flush=True)


if __name__ == "__main__":
    main()
