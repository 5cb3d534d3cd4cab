#!/usr/bin/env python3
"""Closed-loop runs (slam_nav_run): ticks per second beside the open-loop step rate and the host route, on one MI355X.

One process: EKF fp64, L landmarks (default 50), batch (default 65536), map of make_scenario(321 + L, L, .), seed 2025.  The path is the
map's first --waypoints landmarks, shared by the batch; pure pursuit with loose control unless --method / --control say otherwise.  After a
warm-up of each route, --reps repetitions ALTERNATE between
  (a) run_nav(T): per tick the controller kernel and one one-step launch of the simulator + filter, on one stream;
  (b) the same handle open loop, one launch per timestep: set_run_chunk(1) + run_sim of T precomputed commands;
both timed by HIP events on the handle's stream ((a): slam_last_nav_work; (b): torch events around the call on that stream's device,
after a synchronise) and reported as medians.  Then
  (c) the host route, --host-ticks ticks on a second handle: nav_estimates (a synchronise and a copy), navigation.PurePursuitBatch on
      the host, run_sim with per-instance commands of one timestep (an upload and a launch), by the host clock;
  (d) the controller's share of a tick of (a), from slam_last_nav_work;
  (e) the same WORK without the controller: a fresh handle runs run_nav(T) from the start pose and returns its commands, a second fresh
      handle replays them open loop, one launch per timestep (run_sim of (T, batch, 2) commands, set_run_chunk(1)) - the same states,
      detections and bits tick by tick (tests/test_nav_gpu.py::test_replay_of_the_issued_commands), so the difference of the two times
      is what the closed loop adds on the stream: the controller kernels and their launch boundaries (no per-tick events on this handle).
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--L", type=int, default=50)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--ticks", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-ticks", type=int, default=20)
    ap.add_argument("--waypoints", type=int, default=5)
    ap.add_argument("--method", default="pp", choices=["pp", "direct"])
    ap.add_argument("--control", default="loose", choices=["loose", "tight"])
    args = ap.parse_args()
    import torch
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.navigation import PurePursuitBatch
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T = args.L, args.batch, args.ticks
    lm, cmds = make_scenario(321 + L, L, T)
    nav = dict(method=S.NAV_PP if args.method == "pp" else S.NAV_DIRECT, control=S.NAV_LOOSE if args.control == "loose" else S.NAV_TIGHT)
    path = lm[:args.waypoints]

    def handle():
        f = S.BatchedEKF(B, L).readParams()
        f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
        f.set_path(path, nav=nav)
        return f

    f = handle()
    stream = torch.cuda.Stream()
    f.set_stream(stream.cuda_stream)            # kernels run on a stream torch.cuda.Event can see
    f.set_run_chunk(1)
    f.set_nav_timing(True)                      # (d) needs an event pair per controller launch; the handle of leg (e) runs without
    f.run_nav(args.warmup); f.run_sim(cmds[:args.warmup]); f.sync()
    nav_ms, ctrl_ms, open_ms = [], [], []
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(args.reps):
        f.run_nav(T)
        c, t = f.last_nav_work()
        ctrl_ms.append(c); nav_ms.append(t)
        e0.record(stream)
        f.run_sim(cmds)
        e1.record(stream)
        e1.synchronize()
        open_ms.append(e0.elapsed_time(e1))
    state = f.nav_state()
    status = f.status()
    err = f.error_stats()
    kinfo = f.kernel_info(multi_step=False)
    f.close()
    # (e) closed loop from the start pose, and the replay of its commands
    x = handle(); x.set_stream(stream.cuda_stream); x.set_run_chunk(1)
    issued = x.run_nav(T, return_cmds=True)
    _, e_nav = x.last_nav_work()
    x.close()
    y = handle(); y.set_stream(stream.cuda_stream); y.set_run_chunk(1)
    y.run_sim(issued); y.init(0.0, 0.0, 0.0); y.sync()           # (the device command buffer exists before the timed call; init returns to the start)
    e0.record(stream)
    y.run_sim(issued)
    e1.record(stream)
    e1.synchronize()
    e_replay = e0.elapsed_time(e1)
    y.close()
    del issued
    # (c) the host route
    g = handle()
    pp = PurePursuitBatch(B, path, method=nav["method"], control=nav["control"], d_max=g.cfg.d_max, th_max=g.cfg.th_max)
    for _ in range(2):
        g.run_sim(pp.next_cmds(g.nav_estimates())[None])
    g.sync()
    t0 = time.perf_counter()
    t_ctrl = 0.0
    for _ in range(args.host_ticks):
        est = g.nav_estimates()
        t1 = time.perf_counter()
        c = pp.next_cmds(est)
        t_ctrl += time.perf_counter() - t1
        g.run_sim(c[None])
    g.sync()
    host_s = time.perf_counter() - t0
    g.close()
    a, b, c_ms = statistics.median(nav_ms), statistics.median(open_ms), statistics.median(ctrl_ms)
    print(json.dumps({
        "L": L, "batch": B, "ticks": T, "reps": args.reps, "method": args.method, "control": args.control, "waypoints": int(path.shape[0]),
        "step_kernel": kinfo["name"],
        "a_nav_ticks_per_s": round(T / (a * 1e-3), 1), "a_nav_ms_per_tick": round(a / T, 4), "a_nav_ms_all": [round(v, 2) for v in nav_ms],
        "b_open_loop_steps_per_s": round(T / (b * 1e-3), 1), "b_open_loop_ms_per_step": round(b / T, 4), "b_open_loop_ms_all": [round(v, 2) for v in open_ms],
        "c_host_route_ticks_per_s": round(args.host_ticks / host_s, 2), "c_host_route_ms_per_tick": round(host_s * 1e3 / args.host_ticks, 2),
        "c_host_controller_ms_per_tick": round(t_ctrl * 1e3 / args.host_ticks, 2), "c_host_ticks": args.host_ticks,
        "d_controller_ms_per_tick": round(c_ms / T, 5), "d_controller_share_of_tick": round(c_ms / a, 5),
        "a_minus_b_ms_per_tick": round((a - b) / T, 5), "a_over_c": round((T / a * 1e3) / (args.host_ticks / host_s), 1),
        "e_nav_from_start_ms_per_tick": round(e_nav / T, 4), "e_replay_ms_per_step": round(e_replay / T, 4),
        "e_nav_minus_replay_ms_per_tick": round((e_nav - e_replay) / T, 5),
        "finished": int((state["finish_tick"] >= 0).sum()), "remaining_mean": float(state["remaining"].mean()),
        "flagged": int((status != 0).sum()), "mean_position_error_m": float(err.mean())}), flush=True)


if __name__ == "__main__":
    main()
