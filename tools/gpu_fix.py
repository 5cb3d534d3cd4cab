#!/usr/bin/env python3
"""Absolute position and heading fixes (slam_fix*, slam_fix_sense*, slam_fix_run) on one MI355X: what they do to a run that loses its
landmarks, and what they cost.

Part 1, the effect.  A simulated run of --effect-ticks ticks (L = --landmarks, filter rows at the variances of the simulator's uniform
draws) whose landmarks are OUT OF VIEW FOR ITS MIDDLE THIRD (slam_set_vision with range_max 0 for those ticks): dead reckoning.  The run is
replayed four ways from the same seed, as the loop of single calls slam_fix_run is equal to: with no fixes; with position fixes every 10
ticks (half-width --fix-halfwidth, sigma = half-width / sqrt 3); with 5 % of the fixes jumping by 1 to 3 m, gated (the default 0.999
gates) and ungated (infinite gates).  Printed per replay at the end of each third: the batch-mean position error and the mean pose NEES
(slam_monitor_now), and over the run the jumps that were rejected and accepted.  Then all four again in closed loop (NAV: the controller
steers by the estimate, so a bad estimate also bends the true path).

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration, on ONE handle with a full map whose stream this tool owns (so HIP events can bracket single calls), after a
warm-up of each route, --reps repetitions ALTERNATING, 5 calls between one event pair each:
  (a) slam_fix_dev with the position part only, the heading part only and both (every part applied: P is read and written once per call);
  (b) the two parts as two separate calls;
  (c) the merge's worst case of the same handle - one fused pair in every instance, slam_merge_landmarks_dev (fuse and compact), the
      duplicate re-inserted by one plain step before each - and a device-to-device hipMemcpyAsync that reads and writes the number of
      bytes slam_last_fix_work reports for the both-parts call (a copy of half of them), on the same stream;
  (d) slam_fix_run over --ticks ticks with fix_every = 1, 10 and ticks + 1 (no fix tick), beside the plain once-per-tick slam_run_sim
      (run chunk 1) of the same commands on the same handle: device ms per tick by the run's own events and by an event pair.
No time is fixed in advance: the yardsticks are the copy and the plain run of the same process.  Medians; one JSON line per part and
configuration."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_associate import CONFIGS, _hip, _put  # noqa: E402
from tools.gpu_gate import consistent_rows  # noqa: E402
from tools.gpu_map_manage import Events  # noqa: E402

PATH = np.array([[0.6, 0.1], [1.4, 0.6], [2.2, 0.2], [3.0, 0.9], [3.8, 0.3], [4.6, 1.0], [5.4, 0.4]])


def effect(S, args, closed_loop):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, every = args.landmarks, args.effect_batch, args.effect_ticks, 10
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    a = args.fix_halfwidth
    clean = dict(pos_halfwidth=a, sigma_pos=a / math.sqrt(3.0), kinds=S.FIX_POS)
    jumps = dict(clean, p_jump=0.05, jump_lo=1.0, jump_hi=3.0)
    inf = S.FixConfig(math.inf, math.inf, every)
    variants = [("no_fixes", None, None), ("position_fixes", clean, None), ("jumps_gated", jumps, None), ("jumps_ungated", jumps, inf)]
    thirds = [T // 3, 2 * T // 3, T]
    out = dict(tool="gpu_fix", part="effect_closed_loop" if closed_loop else "effect", L=L, batch=B, ticks=T, fix_every=every, fix_halfwidth=a,
               landmarks_out_of_view=[thirds[0], thirds[1]], gates=[S.default_fix_config().gate_pos, S.default_fix_config().gate_yaw])
    for name, sensor, fc in variants:
        f = S.BatchedEKF(B, L).readParams(cfg)
        f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        if closed_loop:
            f.set_path(PATH)
        f.set_fix_sensor(sensor)
        range_max, fov = cfg.range_max, (cfg.fov_min, cfg.fov_max)
        acc = rej = emitted = 0
        phases = []
        for t in range(T):
            if t == thirds[0]:
                f.set_vision(0.0, *fov)                   # nothing in view
            if t == thirds[1]:
                f.set_vision(range_max, *fov)
            if closed_loop:
                f.run_nav(1)
            else:
                f.update_sim(cmds[t])
            if sensor is not None and (t + 1) % every == 0:
                s = f.fix_sense()
                r = f.fix(s["fix"], s["kinds"], cfg=fc)
                jumped = s["jumped"] != 0
                emitted += int((s["kinds"] != 0).sum())
                acc += int((jumped & ((r["verdict"] & 15) == S.FIX_APPLIED)).sum()); rej += int((jumped & ((r["verdict"] & 15) == S.FIX_REJECTED)).sum())
            if t + 1 in thirds:
                m = f.monitor_now()
                ok = np.isfinite(m["nees_pose"])
                phases.append(dict(tick=t + 1, pos_err_mean=float(np.nanmean(m["err_pos"])), nees_pose_mean=float(m["nees_pose"][ok].mean())))
        out[name] = dict(phases=phases, fixes_emitted=emitted, jumps_accepted=acc, jumps_rejected=rej, flagged_instances=int((f.status() != 0).sum()))
        f.close()
        print(f"#   {name:16s} " + " | ".join(f"tick {p['tick']}: error {p['pos_err_mean']:.4f} m, pose NEES {p['nees_pose_mean']:.2f}" for p in phases) +
              f" | jumps accepted {acc}, rejected {rej} of {emitted} fixes")
    print(json.dumps(out), flush=True)


def cost(S, name, L, B, f32, args, hip):
    from live_ekf_slam_amd.scenario import make_scenario
    T, w, calls = args.ticks, args.warmup, 5
    dt = S.F32 if f32 else S.F64
    esz = 4 if f32 else 8
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11 = (v ** 2 / 3 for v in (cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11))   # (no rows: one config for the batch)
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    ev = Events(hip)
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_stream(ev.stream.value)
    f.set_seed(2025); f.set_map(lm)

    # ---- (d) the run beside the plain once-per-tick run ----
    f.set_run_chunk(1)
    a = 0.03
    f.set_fix_sensor(dict(pos_halfwidth=a, yaw_halfwidth=0.01, sigma_pos=a / math.sqrt(3.0), sigma_yaw=0.01 / math.sqrt(3.0), kinds=3))
    strides = (1, 10, T + 1)

    def fix_route(every, n=T):
        f.init(0.0, 0.0, 0.0)
        f.fix_run(cmds[:n], cfg=S.FixConfig(S.default_fix_config().gate_pos, S.default_fix_config().gate_yaw, every))
        return f.last_fix_work()

    def plain_route(n=T):
        f.init(0.0, 0.0, 0.0)
        return ev.ms(lambda: f.run_sim(cmds[:n]))
    for every in strides:
        fix_route(every, w)
    plain_route(w)
    run_ms = {every: [] for every in strides}
    plain_ms = []
    for _ in range(args.reps):
        for every in strides:
            run_ms[every].append(fix_route(every)[2])
        plain_ms.append(plain_route())
    f.set_nav_timing(True)
    run_bytes, fix_ms_timed, timed_total = fix_route(10)
    f.set_nav_timing(False)

    # ---- (a), (b), (c): single calls on a full map ----
    f.init(0.0, 0.0, 0.0)
    j = np.arange(L - 1)
    full = np.stack([1000.0 + j, 1.0 + 0.04 * j, -1.2 + 2.4 * (j % 10) / 9.0], axis=1).astype(np.float32)
    f.update((0.0, 0.0), np.repeat(full[None], B, axis=0), np.full(B, L - 1, np.int32))
    dup = np.zeros((B, 1, 3), np.float32); one = np.ones(B, np.int32)

    def refill(rep):
        dup[:, 0] = [5000.0 + rep, full[0, 1], full[0, 2]]
        f.update((0.0, 0.0), dup, one)
    refill(0)
    assert (f.landmark_counts() == L).all()
    partner = np.full((B, L), -1, np.int32); partner[:, 0] = L - 1; partner[:, L - 1] = 0
    d_partner = _put(hip, partner)
    pose = f.poses()
    fix = np.concatenate([pose[:, :2] + 0.01, pose[:, 2:3] + 0.003, np.full((B, 1), 0.02), np.full((B, 1), 0.01)], axis=1)
    d_fix = _put(hip, np.ascontiguousarray(fix))
    d_kinds = {k: _put(hip, np.full(B, k, np.int32)) for k in (1, 2, 3)}
    r = f.fix(fix, np.full(B, 3, np.int32))
    assert (r["verdict"] == 0x11).all(), "every part applies"
    both_bytes = f.last_fix_work()[0]
    f.fix(d_fix.value, d_kinds[1].value); pos_bytes = f.last_fix_work()[0]
    f.fix(d_fix.value, d_kinds[2].value); yaw_bytes = f.last_fix_work()[0]

    def fixes(k):
        return lambda: [f.fix(d_fix.value, d_kinds[k].value) for _ in range(calls)]

    def separate():
        for _ in range(calls):
            f.fix(d_fix.value, d_kinds[1].value); f.fix(d_fix.value, d_kinds[2].value)
    half = int(both_bytes // 2)
    src, dst = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(src), half) == 0 and hip.hipMalloc(C.byref(dst), half) == 0
    copy = (lambda: [hip.hipMemcpyAsync(dst, src, half, 3, ev.stream) for _ in range(calls)])           # hipMemcpyDeviceToDevice
    ms = dict(pos=[], yaw=[], both=[], separate=[], copy=[], merge=[])
    merge_bytes = 0.0
    for rep in range(args.reps + 1):                                  # (the first repetition is the warm-up)
        got = dict(pos=ev.ms(fixes(1)) / calls, yaw=ev.ms(fixes(2)) / calls, both=ev.ms(fixes(3)) / calls, separate=ev.ms(separate) / calls,
                   copy=ev.ms(copy) / calls)
        got["merge"] = ev.ms(lambda: f.merge_landmarks(d_partner.value, stats=False))
        merge_bytes = f.last_merge_work()[0]
        assert (f.landmark_counts() == L - 1).all()
        refill(rep + 1)
        if rep:
            for k, v in got.items():
                ms[k].append(v)
    f.close()
    for p in [d_partner, d_fix, src, dst] + list(d_kinds.values()):
        hip.hipFree(p)
    med = {k: statistics.median(v) for k, v in ms.items()}
    runs = {every: statistics.median(v) / T for every, v in run_ms.items()}
    plain = statistics.median(plain_ms) / T
    fixes_in_run = T // 10
    print(json.dumps({
        "tool": "gpu_fix", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T, "reps": args.reps,
        "calls_per_event_pair": calls,
        "a_position_only_ms": round(med["pos"], 4), "pos_ms_all": [round(v, 4) for v in ms["pos"]], "pos_model_bytes": pos_bytes,
        "a_heading_only_ms": round(med["yaw"], 4), "yaw_ms_all": [round(v, 4) for v in ms["yaw"]], "yaw_model_bytes": yaw_bytes,
        "a_both_parts_ms": round(med["both"], 4), "both_ms_all": [round(v, 4) for v in ms["both"]], "both_model_bytes": both_bytes,
        "both_model_GBps": round(both_bytes / (med["both"] * 1e-3) / 1e9, 1), "both_over_position_only": round(med["both"] / med["pos"], 4),
        "b_two_separate_calls_ms": round(med["separate"], 4), "separate_ms_all": [round(v, 4) for v in ms["separate"]],
        "both_over_separate": round(med["both"] / med["separate"], 4),
        "c_copy_of_half_the_both_bytes_ms": round(med["copy"], 4), "copy_ms_all": [round(v, 4) for v in ms["copy"]],
        "copy_read_plus_write_GBps": round(both_bytes / (med["copy"] * 1e-3) / 1e9, 1), "both_over_copy": round(med["both"] / med["copy"], 3),
        "c_merge_worst_fuse_and_compact_ms": round(med["merge"], 4), "merge_ms_all": [round(v, 4) for v in ms["merge"]], "merge_model_bytes": merge_bytes,
        "merge_over_its_share_of_the_copy": round(med["merge"] / (med["copy"] * merge_bytes / both_bytes), 3),
        "slab_bytes": float(B) * esz * (3 + 2 * L) * ((3 + 2 * L + 1) & ~1 if esz == 8 else (3 + 2 * L + 3) & ~3),
        "d_fix_run_ms_per_tick": {str(k): round(v, 4) for k, v in runs.items()}, "d_fix_run_ms_all": {str(k): [round(x, 2) for x in v] for k, v in run_ms.items()},
        "d_plain_run_sim_ms_per_tick": round(plain, 4), "plain_ms_all": [round(v, 2) for v in plain_ms],
        "no_fix_tick_over_plain": round(runs[T + 1] / plain, 4), "fix_launches_ms_per_fix_tick": round(fix_ms_timed / max(fixes_in_run, 1), 5),
        "timed_run_ms_per_tick": round(timed_total / T, 4), "run_model_bytes_per_fix": run_bytes / max(fixes_in_run, 1)}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=20)
    ap.add_argument("--effect-batch", type=int, default=256)
    ap.add_argument("--effect-ticks", type=int, default=300)
    ap.add_argument("--fix-halfwidth", type=float, default=0.05)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["effect"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    hip = _hip()
    if args.only in (None, "effect"):
        effect(S, args, False)
        effect(S, args, True)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args, hip)


if __name__ == "__main__":
    main()
