#!/usr/bin/env python3
"""The run monitor (slam_monitor_run) beside the unmonitored once-per-step run and the getter route it replaces, on one MI355X.

One process, three configurations unless --only picks one: EKF L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096 fp64;
map and commands of make_scenario(321 + L, L, .), seed 2025.  Per configuration, on ONE handle, after a warm-up of every route:
  (a) monitor_run of T ticks, records only: per tick one one-step launch of the simulator + filter and the monitor's two launches, on one
      stream; device time of the whole run by HIP events (slam_last_monitor_work), per-tick event pairs OFF;
  (b) the same handle without the monitor, the parent commit's once-per-tick route: T calls of slam_run_sim_each(h, cmds, 1) (run_sim of
      one (1, batch, 2) command block: an upload of 8 bytes per instance and one one-step launch), host clock from before the first call
      to after a final synchronise;
  (b') the same handle open loop with shared commands, one launch per timestep (set_run_chunk(1) + run_sim), host clock ending synchronised;
--reps repetitions ALTERNATE (a), (b), (b'), medians are reported.  Then
  (c) the monitor's share: monitor_run with an event pair around every tick's monitor launches (set_nav_timing), its device time over the
      run's; once more with full_every = 100 (slam_consistency's evaluation on every 100th tick) and with the three per-instance series;
  (d) the getter route a per-tick curve needed before: poses() + truth() + consistency() after every update_sim, --getter-ticks ticks, host
      clock.
One JSON line per configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CONFIGS = {"L50_f64": (50, 65536, False), "L50_f32": (50, 65536, True), "L20_f64": (20, 4096, False)}


def measure(S, name, L, B, f32, args):
    from live_ekf_slam_amd.filters import monitor_summary
    from live_ekf_slam_amd.scenario import make_scenario
    T = args.ticks
    lm, cmds = make_scenario(321 + L, L, T)
    each = np.ascontiguousarray(np.broadcast_to(cmds[:, None, :], (T, B, 2)), dtype=np.float32)
    f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams()
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    f.set_run_chunk(1)
    w = args.warmup
    f.monitor_run(cmds[:w]); f.run_sim(each[:1]); f.run_sim(cmds[:w]); f.sync()
    a_ms, b_ms, o_ms = [], [], []
    for _ in range(args.reps):
        f.monitor_run(cmds)
        a_ms.append(f.last_monitor_work()[1])
        f.sync()
        t0 = time.perf_counter()
        for t in range(T):
            f.run_sim(each[t:t + 1])
        f.sync()
        b_ms.append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        f.run_sim(cmds)
        f.sync()
        o_ms.append((time.perf_counter() - t0) * 1e3)
    # (c) the monitor's own share, then with a full evaluation at a stride and with the series
    f.set_nav_timing(True)
    f.monitor_run(cmds)
    c_mon, c_total = f.last_monitor_work()
    f.monitor_run(cmds, cfg=dict(full_every=100))
    cf_mon, cf_total = f.last_monitor_work()
    f.set_nav_timing(False)
    t0 = time.perf_counter()
    res = f.monitor_run(cmds, series=True)
    s_host = (time.perf_counter() - t0) * 1e3
    s_total = f.last_monitor_work()[1]
    summ = monitor_summary(res.recs[-1])
    # (d) the getter route
    f.set_lazy_steps(0)
    for t in range(2):
        f.update_sim(cmds[t]); f.poses(); f.truth(); f.consistency()
    t0 = time.perf_counter()
    for t in range(args.getter_ticks):
        f.update_sim(cmds[t]); f.poses(); f.truth(); f.consistency()
    d_ms = (time.perf_counter() - t0) * 1e3
    cons_ms = f.last_consistency_work()[1]
    kinfo = f.kernel_info(multi_step=False)
    status = f.status()
    f.close()
    a, b, o = statistics.median(a_ms), statistics.median(b_ms), statistics.median(o_ms)
    print(json.dumps({
        "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T, "reps": args.reps, "step_kernel": kinfo["name"],
        "a_monitored_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "b_run_sim_each_1_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms],
        "b2_open_loop_shared_ms_per_tick": round(o / T, 4), "b2_ms_all": [round(v, 2) for v in o_ms],
        "a_minus_b_ms_per_tick": round((a - b) / T, 5), "a_minus_b2_ms_per_tick": round((a - o) / T, 5),
        "c_monitor_ms_per_tick": round(c_mon / T, 5), "c_monitor_share_of_tick": round(c_mon / c_total, 5), "c_timed_run_ms_per_tick": round(c_total / T, 4),
        "c_full_every_100_monitor_ms_per_tick": round(cf_mon / T, 5), "c_full_every_100_share": round(cf_mon / cf_total, 5),
        "c_series_run_device_ms_per_tick": round(s_total / T, 4), "c_series_run_host_ms_per_tick": round(s_host / T, 4),
        "d_getter_route_ms_per_tick": round(d_ms / args.getter_ticks, 2), "d_getter_ticks": args.getter_ticks, "d_consistency_device_ms": round(cons_ms, 2),
        "a_over_d": round((d_ms / args.getter_ticks) / (a / T), 1),
        "last_tick": {k: float(v[0]) for k, v in summ.items()}, "flagged": int((status != 0).sum())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--getter-ticks", type=int, default=5)
    ap.add_argument("--only", choices=sorted(CONFIGS), default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            measure(S, name, L, B, f32, args)


if __name__ == "__main__":
    main()
