#!/usr/bin/env python3
"""Pose graph: time of the marginal covariances (pgs_marginals) beside the solve, at BASELINE configs[4] shape.

One process, one command: for each batch (default 256 and 2048) the graphs of bench.py --filter pgs (1000 poses x 200 landmarks,
k_per_pose 32, scenario 1234, seed 2025) are built on the device, then after a warm-up of both calls `solve` and `marginals` alternate
--reps times, each timed with HIP events around a stream synchronise.  Per batch: ms per call (median and all), instances/s, the achieved
FLOP/s of marginals by its model (pgs_last_marginals_work: 3N n^2 + 12 * 3N n + 2 n^3 / 3 + 3N n^2 + n^3 / 3 per instance, n = 2 M)
over the 78.6 TFLOP/s fp64 matrix peak, and the ratio to the solve's time in the same run; one JSON line per batch.

For the per-kernel split run the same command under `rocprofv3 --kernel-trace --stats -- python tools/gpu_pgs_marginals.py --batches 256`
(no counters together with tracing); the new kernels are pgs_marg_begin / inv / back / gram_kernel, the factorisation before them the
solve's own linearize / chain / syrk / chol kernels."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_FP64_MATRIX = 78.6e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="256,2048")
    ap.add_argument("--poses", type=int, default=1000)
    ap.add_argument("--landmarks", type=int, default=200)
    ap.add_argument("--k-per-pose", type=int, default=32)
    ap.add_argument("--reps", type=int, default=4)
    args = ap.parse_args()
    import torch
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.scenario import make_scenario
    if not torch.cuda.is_available():
        sys.exit("no HIP device")
    dev = torch.device("cuda", 0)
    lm, cmds = make_scenario(1234, args.landmarks, args.poses - 1)
    for B in (int(b) for b in args.batches.split(",")):
        pg = S.BatchedPoseGraph(B, num_iterations=args.poses, L_max=args.landmarks, k_per_pose=args.k_per_pose).readParams()
        stream = torch.cuda.Stream(device=dev)
        pg.set_stream(stream.cuda_stream)
        pg.set_map(lm); pg.set_seed(2025); pg.init(0.0, 0.0, 0.0)
        t_solve, t_marg, flop = [], [], 0.0

        def timed(fn):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream); fn(); e1.record(stream)
            stream.synchronize()
            return e0.elapsed_time(e1)

        with torch.cuda.stream(stream):
            pg.run_sim(cmds)
            pg.solvePoseGraph(); pg.marginals(1); stream.synchronize()   # warm-up (first-call allocations, code objects)
            for _ in range(args.reps):
                t_solve.append(timed(pg.solvePoseGraph))
                t_marg.append(timed(lambda: pg.marginals(1)))
                flop, ms_lib = pg.last_marginals_work()
        singular = sum(pg.get_marginals(b)["status"] for b in range(0, B, max(1, B // 64)))
        flags = pg.stats()["flags"]
        pg.close()
        ms_s, ms_m = statistics.median(t_solve), statistics.median(t_marg)
        print(json.dumps({
            "batch": B, "poses": args.poses, "landmarks": args.landmarks,
            "solve_ms": round(ms_s, 3), "solve_ms_all": [round(v, 3) for v in t_solve],
            "marginals_ms": round(ms_m, 3), "marginals_ms_all": [round(v, 3) for v in t_marg], "marginals_ms_library_events_last": round(ms_lib, 3),
            "marginals_instances_per_s": round(B / (ms_m * 1e-3), 1), "solves_per_s": round(B / (ms_s * 1e-3), 1),
            "marginals_model_flop": flop, "marginals_tflops": round(flop / (ms_m * 1e-3) / 1e12, 3),
            "fraction_of_fp64_matrix_peak": round(flop / (ms_m * 1e-3) / PEAK_FP64_MATRIX, 4),
            "marginals_over_solve": round(ms_m / ms_s, 3), "singular_in_sample": int(singular), "flagged": int((flags != 0).sum())}), flush=True)


if __name__ == "__main__":
    main()
