#!/usr/bin/env python3
"""A tuning sweep of the filter's assumed noise in ONE EKF handle (slam_set_noise_each), on one MI355X.

One handle of --batch instances (default 65 536) at L = --landmarks (default 50), replicate_vw_quirk = 0, map and commands of
make_scenario(321 + L, L, T), seed 2025.  The batch is cut into --groups groups of consecutive instances; group g scales the filter's
V_00, V_11, W_00, W_11 by a factor from a logarithmic grid (--lo .. --hi); the simulator rows stay the config's (half-widths V_00 ..
W_11 of the uniform draws), so every group sees the same kind of noise and only what the filter ASSUMES changes.  After run_sim of
--ticks timesteps, consistency() gives the NEES of every instance; per group the tool prints ANEES / dof for the full state and for the
pose with the band of consistency_summary, and the mean position error.  Nothing is asserted about where the band is entered: the tool
reports it.

Cost of the feature: the same handle runs the same commands from the same start with the rows set and with the rows unset (the config's
values), --reps repetitions ALTERNATING the two, host clock from before run_sim to after a final synchronise; medians in ms per timestep.
One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--groups", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--lo", type=float, default=1e-6, help="smallest factor on the filter's V and W")
    ap.add_argument("--hi", type=float, default=1e1, help="largest factor")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--f32", action="store_true", help="fp32 storage")
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.config import noise_rows
    from live_ekf_slam_amd.filters import consistency_summary
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, G, T = args.landmarks, args.batch, args.groups, args.ticks
    if G < 1 or B < G:
        sys.exit("need 1 <= groups <= batch")
    lm, cmds = make_scenario(321 + L, L, T)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    f = S.BatchedEKF(B, L, dtype=S.F32 if args.f32 else S.F64).readParams(cfg)
    f.set_map(lm); f.set_seed(2025)
    factors = np.logspace(np.log10(args.lo), np.log10(args.hi), G)
    group = np.minimum(np.arange(B) * G // B, G - 1)          # consecutive instances
    scale = factors[group]
    rows = noise_rows(cfg, B, V_00=cfg.V_00 * scale, V_11=cfg.V_11 * scale, W_00=cfg.W_00 * scale, W_11=cfg.W_11 * scale)

    def run(with_rows):
        f.set_noise(rows if with_rows else None)
        f.init(0.0, 0.0, 0.0)
        f.sync()
        t0 = time.perf_counter()
        f.run_sim(cmds)
        f.sync()
        return (time.perf_counter() - t0) * 1e3 / T

    run(True); run(False)                                     # warm-up of both routes
    on_ms, off_ms = [], []
    for _ in range(args.reps):
        off_ms.append(run(False))
        on_ms.append(run(True))                               # (the last run leaves the swept state in the handle)
    c = f.consistency()
    err = f.error_stats()
    status = f.status()
    table = []
    print(f"# EKF L = {L}, batch {B}, {G} groups, {T} ticks, {'fp32' if args.f32 else 'fp64'} storage, replicate_vw_quirk = 0")
    print("# factor on V, W | instances counted | ANEES/dof full [band] | ANEES/dof pose [band] | mean position error")
    for g in range(G):
        sel = group == g
        full = consistency_summary(c["nees_full"][sel], c["dof"][sel], c["flags"][sel] & (f.FULL_NOT_PD | f.NO_TRUTH | f.INSTANCE_FAILED))
        pose = consistency_summary(c["nees_pose"][sel], np.full(int(sel.sum()), 3), c["flags"][sel] & (f.POSE_NOT_PD | f.NO_TRUTH | f.INSTANCE_FAILED))
        inside = lambda s: "in " if s["lower"] <= s["normalised"] <= s["upper"] else "out"
        row = dict(factor=float(factors[g]), count=full["count"], left_out=full["left_out"], anees_full=full["normalised"],
                   full_band=[full["lower"], full["upper"]], anees_pose=pose["normalised"], pose_band=[pose["lower"], pose["upper"]],
                   mean_err=float(err[sel].mean()), failed=int((status[sel] != 0).sum()))
        table.append(row)
        print(f"{factors[g]:10.3e} | {full['count']:6d} | {full['normalised']:10.4g} {inside(full)} [{full['lower']:.4f}, {full['upper']:.4f}] | "
              f"{pose['normalised']:10.4g} {inside(pose)} [{pose['lower']:.4f}, {pose['upper']:.4f}] | {row['mean_err']:.5f}")
    print(json.dumps(dict(tool="gpu_noise_sweep", L=L, batch=B, groups=G, ticks=T, f32=bool(args.f32),
                          ms_per_step_rows_set=on_ms, ms_per_step_rows_unset=off_ms,
                          median_rows_set=statistics.median(on_ms), median_rows_unset=statistics.median(off_ms), table=table)))
    f.close()


if __name__ == "__main__":
    main()
