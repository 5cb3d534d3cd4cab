#!/usr/bin/env python3
"""UKF matrix square root, eigen (reference-exact) vs Cholesky (SLAM_UKF_SQRT_CHOLESKY, not bit-identical), in one process on the
bench scenario (tools/gpu_ukf_time.py, bench.py --filter ukf): L = 20 (BASELINE configs[2]) and L = 50, batch 4096.

Per mode and L:
  * steps/s of run_sim (the simulator + filter path bench.py times), the two modes alternated over `--reps` windows;
  * the sqrt stage vs the step kernel: predictionStage (the square root: ukf_chol_kernel + the eigen kernel's fallback launch, or
    ukf_sqrt_kernel) and updateStage (ukf_step_kernel, empty messages) timed apart with HIP events on one stream;
  * Cholesky factorisations / eigen fallbacks of the timed run_sim windows (slam_ukf_sqrt_stats), mean position error, flags.
A kernel-level split of the run_sim path: run this tool under `rocprofv3 --kernel-trace --stats`.
usage: gpu_ukf_sqrt_modes.py [--L 20,50] [--batch 4096] [--steps 40] [--reps 3]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import live_ekf_slam_amd as S                                   # noqa: E402
from live_ekf_slam_amd.scenario import make_scenario           # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--L", default="20,50")
ap.add_argument("--batch", type=int, default=4096)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--reps", type=int, default=3)
args = ap.parse_args()

hip = C.CDLL("libamdhip64.so")
hip.hipStreamCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipStreamDestroy.argtypes = [C.c_void_p]
hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
hip.hipEventSynchronize.argtypes = [C.c_void_p]
hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
hip.hipEventDestroy.argtypes = [C.c_void_p]


def hipcheck(rc):
    if rc != 0:
        raise RuntimeError(f"HIP error {rc}")


PRE = 20
MODES = ("eigen", "cholesky")


def make(L, B, lm, cmds, mode):
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode(mode)
    f.set_vision(1e9, -4.0, 4.0); f.update_sim(cmds[0]); f.set_vision(3.0, -1.57, 1.57)   # every landmark mapped at step 0
    f.run_sim(cmds[1:1 + PRE]); f.sync()
    return f


def run_sim_rate(L, B, lm, cmds):
    """steps/s per mode over `reps` alternated windows of `steps` steps (host clock around run_sim + stream synchronise)."""
    fs = {m: make(L, B, lm, cmds, m) for m in MODES}
    rates = {m: [] for m in MODES}
    for m in MODES:
        fs[m].sqrt_stats(reset=True)
    t = 1 + PRE
    for _ in range(args.reps):
        for m in MODES:
            f = fs[m]
            t0 = time.perf_counter(); f.run_sim(cmds[t:t + args.steps]); f.sync(); dt = time.perf_counter() - t0
            rates[m].append(B * args.steps / dt)
        t += args.steps
    out = {}
    for m in MODES:
        f = fs[m]
        out[m] = dict(rates=rates[m], stats=f.sqrt_stats().tolist(), err=float(f.error_stats().mean()),
                      flags=int(np.count_nonzero(f.status())), M=float(f.landmark_counts().mean()))
        f.close()
    return out


def stage_times(L, B, lm, cmds, mode, steps):
    """Mean ms per step of predictionStage (the square root) and updateStage (the step kernel, empty messages), one stream."""
    f = make(L, B, lm, cmds, mode)
    st = C.c_void_p(); hipcheck(hip.hipStreamCreate(C.byref(st))); f.set_stream(st.value)
    ev = [C.c_void_p() for _ in range(3)]
    for e in ev:
        hipcheck(hip.hipEventCreate(C.byref(e)))
    tp = tu = 0.0
    ms = C.c_float()
    for i in range(steps + 2):
        c = S.Command(*cmds[1 + PRE + i])
        hipcheck(hip.hipEventRecord(ev[0], st)); f.predictionStage(c)
        hipcheck(hip.hipEventRecord(ev[1], st)); f.updateStage()
        hipcheck(hip.hipEventRecord(ev[2], st)); hipcheck(hip.hipEventSynchronize(ev[2]))
        if i >= 2:   # two warm-up steps on the new stream
            hipcheck(hip.hipEventElapsedTime(C.byref(ms), ev[0], ev[1])); tp += ms.value
            hipcheck(hip.hipEventElapsedTime(C.byref(ms), ev[1], ev[2])); tu += ms.value
    f.close()
    for e in ev:
        hip.hipEventDestroy(e)
    hip.hipStreamDestroy(st)
    return tp / steps, tu / steps


for L in (int(x) for x in args.L.split(",")):
    B = args.batch
    lm, cmds = make_scenario(1234, L, 1 + PRE + args.steps * args.reps + 8)
    r = run_sim_rate(L, B, lm, cmds)
    print(f"== L={L} (n={4 + 2 * L}) batch={B}: run_sim, {args.reps} alternated windows of {args.steps} steps", flush=True)
    for m in MODES:
        rr = r[m]
        fact, fb = rr["stats"]
        share = f"Cholesky {fact}, fallbacks {fb} ({100.0 * fb / max(1, fact + fb):.1f} %)" if m == "cholesky" else "-"
        print(f"   {m:8s} {np.median(rr['rates']) / 1e3:9.1f} k steps/s (windows {', '.join(f'{x / 1e3:.1f}' for x in rr['rates'])})"
              f"  mean err {rr['err']:.4f} m  M {rr['M']:.1f}  flagged {rr['flags']}  {share}", flush=True)
    sp = np.median(r["cholesky"]["rates"]) / np.median(r["eigen"]["rates"])
    print(f"   speedup cholesky / eigen: {sp:.2f}x", flush=True)
    for m in MODES:
        ps, us = stage_times(L, B, lm, cmds, m, 6)
        print(f"   {m:8s} one stream: sqrt stage {ps:.3f} ms, step kernel {us:.3f} ms per step (empty messages): "
              f"sqrt {100.0 * ps / (ps + us):.1f} % of the step", flush=True)
