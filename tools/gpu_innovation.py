#!/usr/bin/env python3
"""The innovation statistics (slam_innovation_run) on one MI355X: a noise sweep judged WITHOUT the truth, and what the evaluation costs.

Part 1, the sweep of tools/gpu_noise_sweep.py: one EKF handle of --batch instances (default 65 536) at L = --landmarks (default 50),
replicate_vw_quirk = 0, map and commands of make_scenario(321 + L, L, T), seed 2025, --groups groups of consecutive instances whose filter
rows scale V_00, V_11, W_00, W_11 by a factor from a logarithmic grid; the simulator rows stay the config's.  The run goes through
innovation_run; per group the tool prints the mean NIS per update over the whole run with the chi-square band of that mean for the group's
update count (2 degrees of freedom per update), and beside it the ANEES / dof of the pose and of the full state that the sweep tool
prints from consistency() after the run, with their bands.  Nothing is asserted about where a band is entered: the tool reports it.

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration, on ONE handle, after a warm-up of both routes, --reps repetitions ALTERNATING
  (a) innovation_run of T ticks, records only: per tick the innovation's three launches and the one-step launch, device time of the whole
      run by HIP events (slam_last_innovation_work), per-tick event pairs OFF;
  (b) the unmonitored once-per-tick run the parent commit has: set_run_chunk(1) + run_sim, one launch per timestep, host clock ending
      synchronised;
then (c) once with an event pair around every tick's innovation launches (set_nav_timing): their device time and share of the run.
Medians; one JSON line per part and configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"L50_f64": (50, 65536, False), "L50_f32": (50, 65536, True), "L20_f64": (20, 4096, False)}


def sweep(S, args):
    from live_ekf_slam_amd.config import noise_rows
    from live_ekf_slam_amd.filters import chi2_quantile, consistency_summary
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, G, T = args.landmarks, args.batch, args.groups, args.sweep_ticks
    lm, cmds = make_scenario(321 + L, L, T)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    f = S.BatchedEKF(B, L).readParams(cfg)
    f.set_map(lm); f.set_seed(2025)
    factors = np.logspace(np.log10(args.lo), np.log10(args.hi), G)
    group = np.minimum(np.arange(B) * G // B, G - 1)
    scale = factors[group]
    f.set_noise(noise_rows(cfg, B, V_00=cfg.V_00 * scale, V_11=cfg.V_11 * scale, W_00=cfg.W_00 * scale, W_11=cfg.W_11 * scale))
    f.init(0.0, 0.0, 0.0)
    nis, upd = np.zeros(B), np.zeros(B, dtype=np.int64)
    flagged = 0
    for t0 in range(0, T, args.series_chunk):      # (the series of a chunk of ticks at a time: [ticks][batch] doubles on the host)
        res = f.innovation_run(cmds[t0:t0 + args.series_chunk], series=True)
        ok = res.flags == 0
        fin = ok & (res.n_upd > 0)
        nis += np.where(fin, res.nis_sum, 0.0).sum(axis=0); upd += np.where(fin, res.n_upd, 0).sum(axis=0)
        flagged += int((~ok).sum())
    c = f.consistency()
    table = []
    print(f"# EKF L = {L}, batch {B}, {G} groups, {T} ticks, fp64 storage, replicate_vw_quirk = 0; instance-ticks with a flag: {flagged}")
    print("# factor on V, W | updates | mean NIS / 2 per update [band] | ANEES/dof pose [band] | ANEES/dof full [band]")
    for g in range(G):
        sel = group == g
        n = int(upd[sel].sum())
        mean = float(nis[sel].sum() / n) / 2.0
        lo, hi = chi2_quantile(0.025, 2 * n) / (2 * n), chi2_quantile(0.975, 2 * n) / (2 * n)
        full = consistency_summary(c["nees_full"][sel], c["dof"][sel], c["flags"][sel] & (f.FULL_NOT_PD | f.NO_TRUTH | f.INSTANCE_FAILED))
        pose = consistency_summary(c["nees_pose"][sel], np.full(int(sel.sum()), 3), c["flags"][sel] & (f.POSE_NOT_PD | f.NO_TRUTH | f.INSTANCE_FAILED))
        inside = lambda v, a, b: "in " if a <= v <= b else "out"
        table.append(dict(factor=float(factors[g]), updates=n, nis_per_dof=mean, nis_band=[lo, hi], anees_pose=pose["normalised"],
                          pose_band=[pose["lower"], pose["upper"]], anees_full=full["normalised"], full_band=[full["lower"], full["upper"]]))
        print(f"{factors[g]:10.3e} | {n:9d} | {mean:10.4g} {inside(mean, lo, hi)} [{lo:.4f}, {hi:.4f}] | "
              f"{pose['normalised']:10.4g} {inside(pose['normalised'], pose['lower'], pose['upper'])} [{pose['lower']:.4f}, {pose['upper']:.4f}] | "
              f"{full['normalised']:10.4g} {inside(full['normalised'], full['lower'], full['upper'])} [{full['lower']:.4f}, {full['upper']:.4f}]")
    print(json.dumps(dict(tool="gpu_innovation", part="sweep", L=L, batch=B, groups=G, ticks=T, flagged=flagged, table=table)), flush=True)
    f.close()


def cost(S, name, L, B, f32, args):
    from live_ekf_slam_amd.filters import innovation_summary
    from live_ekf_slam_amd.scenario import make_scenario
    T = args.ticks
    lm, cmds = make_scenario(321 + L, L, T)
    f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams()
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    f.set_run_chunk(1)
    w = args.warmup
    f.innovation_run(cmds[:w]); f.run_sim(cmds[:w]); f.sync()
    a_ms, b_ms = [], []
    for _ in range(args.reps):
        res = f.innovation_run(cmds)
        a_ms.append(f.last_innovation_work()[1])
        f.sync()
        t0 = time.perf_counter()
        f.run_sim(cmds)
        f.sync()
        b_ms.append((time.perf_counter() - t0) * 1e3)
    f.set_nav_timing(True)
    f.innovation_run(cmds)
    c_inn, c_total = f.last_innovation_work()
    f.set_nav_timing(False)
    summ = innovation_summary(res.recs[-1])
    status = f.status()
    f.close()
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    print(json.dumps({
        "tool": "gpu_innovation", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T, "reps": args.reps,
        "a_innovation_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "b_plain_once_per_tick_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms],
        "a_minus_b_ms_per_tick": round((a - b) / T, 5), "a_over_b": round(a / b, 4),
        "c_innovation_ms_per_tick": round(c_inn / T, 5), "c_innovation_share_of_tick": round(c_inn / c_total, 5),
        "c_timed_run_ms_per_tick": round(c_total / T, 4),
        "last_tick": {k: float(v[0]) for k, v in summ.items()}, "flagged": int((status != 0).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--sweep-ticks", type=int, default=200)
    ap.add_argument("--series-chunk", type=int, default=25)
    ap.add_argument("--lo", type=float, default=1e-6, help="smallest factor on the filter's V and W")
    ap.add_argument("--hi", type=float, default=1e1, help="largest factor")
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["sweep"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    if args.only in (None, "sweep"):
        sweep(S, args)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args)


if __name__ == "__main__":
    main()
