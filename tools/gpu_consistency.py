#!/usr/bin/env python3
"""EKF batch: time of the NEES consistency statistics (slam_consistency) beside the EKF timestep, at the benchmark shapes.

One process, one command: for (L, batch, dtype) in --shapes (default 20x4096 f64, 50x65536 f64, 50x65536 f32; scenario
make_scenario(321 + L, L, 1000), seed 2025) the handle runs run_sim for --steps timesteps (timed: one EKF timestep = that time /
steps), then after a warm-up call consistency() is timed --reps times: the host clock around the call (it ends synchronised, results
on the host) and the device time of slam_last_consistency_work (HIP events around the launch).  Per shape one JSON line: ms per call
(median and all), instances/s, the model's bytes over the time over 8 TB/s, the EKF timestep of the same handle in the same run and
the ratio, the time of the route without the call - get_state per instance + a numpy Cholesky solve on the host - measured on 1024
instances and scaled to the batch, and the consistency_summary of the batch.

For the kernel's own time run the same command under `rocprofv3 --kernel-trace --stats -- python tools/gpu_consistency.py --shapes
50x65536` (no counters together with tracing); the kernel is consistency_kernel<103, 256, 1, 64, false, double>."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_HBM = 8.0e12


def host_route(f, lm, count):
    """What a caller had to do without the call, per instance: get_state (a synchronise and a copy of P), symmetrise, Cholesky, solve."""
    truth = f.truth()
    t0 = time.perf_counter()
    for b in range(count):
        s = f.get_state(b)
        M = s["M"]
        e = np.concatenate([s["x"][:3] - truth[b], s["x"][3:] - lm[s["ids"]].ravel()])
        e[2] = np.remainder(e[2] + np.pi, 2 * np.pi) - np.pi
        L = np.linalg.cholesky(0.5 * (s["P"] + s["P"].T))
        y = np.linalg.solve(L, e)   # (numpy has no triangular solve; the factorisation dominates either way)
        float(y @ y); float(y[:3] @ y[:3]); float(np.sqrt(np.mean(np.sum((e[3:].reshape(M, 2)) ** 2, axis=1)))) if M else 0.0
    return (time.perf_counter() - t0) / count


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="20x4096,50x65536,50x65536:f32", help="L x batch[:f32], comma separated")
    ap.add_argument("--steps", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=1024)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.filters import consistency_summary
    from live_ekf_slam_amd.scenario import make_scenario
    for shape in args.shapes.split(","):
        dims, _, dt = shape.partition(":")
        L, B = (int(v) for v in dims.split("x"))
        lm, cmds = make_scenario(321 + L, L, args.steps)
        f = S.BatchedEKF(B, L, dtype=S.F32 if dt == "f32" else S.F64).readParams()
        f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
        f.run_sim(cmds[:8]); f.sync()                      # warm-up of the step kernel
        t0 = time.perf_counter()
        f.run_sim(cmds[8:]); f.sync()
        step_ms = (time.perf_counter() - t0) * 1e3 / max(1, args.steps - 8)
        f.consistency()                                    # warm-up (first-call allocations, code object)
        host_ms, dev_ms = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            c = f.consistency()
            host_ms.append((time.perf_counter() - t0) * 1e3)
            nbytes, ms = f.last_consistency_work()
            dev_ms.append(ms)
        per_inst = host_route(f, lm, min(B, args.host_sample))
        ok = c["flags"] == 0
        summary = consistency_summary(c["nees_full"], c["dof"], c["flags"]) if int(c["dof"][ok].sum()) >= 30 else None
        pose = consistency_summary(c["nees_pose"], np.full(B, 3), c["flags"]) if 3 * int(ok.sum()) >= 30 else None
        f.close()
        hm, dm = statistics.median(host_ms), statistics.median(dev_ms)
        print(json.dumps({
            "L": L, "batch": B, "dtype": "f32" if dt == "f32" else "f64", "steps": args.steps,
            "consistency_ms": round(hm, 3), "consistency_ms_all": [round(v, 3) for v in host_ms],
            "consistency_device_ms": round(dm, 3), "consistency_device_ms_all": [round(v, 3) for v in dev_ms],
            "instances_per_s": round(B / (hm * 1e-3), 1), "model_bytes": nbytes,
            "fraction_of_hbm_read_bound_device": round(nbytes / (dm * 1e-3) / PEAK_HBM, 4),
            "fraction_of_hbm_read_bound_call": round(nbytes / (hm * 1e-3) / PEAK_HBM, 4),
            "ekf_timestep_ms": round(step_ms, 4), "consistency_over_timestep": round(hm / step_ms, 2),
            "host_route_ms_scaled_to_batch": round(per_inst * B * 1e3, 1), "host_route_sample": min(B, args.host_sample),
            "host_route_over_consistency": round(per_inst * B * 1e3 / hm, 1),
            "flagged": int((~ok).sum()), "map_rms_mean": float(np.nanmean(c["map_rms"])), "summary_full": summary, "summary_pose": pose}), flush=True)


if __name__ == "__main__":
    main()
