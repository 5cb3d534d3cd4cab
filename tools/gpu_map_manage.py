#!/usr/bin/env python3
"""Map management (slam_manage_run, slam_map_tally, slam_map_prune, slam_remove_landmarks) on one MI355X: what it does to an id-less log
with clutter, and what it costs.

Part 1, the effect.  The `spread` log of tools/gpu_associate.py (L = --landmarks, filter rows at the variances of the simulator's uniform
draws) with its ids erased and ONE clutter detection per instance and tick, uniform in the field of view and the range.  The log is
replayed on two host-fed handles of capacity L: associate_run (nothing ever leaves the map) and manage_run (the default map config).
Printed per replay at the end of --effect-ticks ticks: landmarks held per instance, detections dropped as NO_ROOM, instances flagged
SLAM_INST_CAPACITY, the mean position error against the recorded truth at the last tick, device ms per tick.

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration, on ONE handle whose stream this tool owns (so HIP events can bracket single calls), after a warm-up of each
route, --reps repetitions ALTERNATING
  (a) manage_run and associate_run on the same log (ids erased, one clutter detection per tick), device time by the runs' own events;
  (b) the tally alone: 20 slam_map_tally_dev calls between one event pair;
  (c) one removal in the WORST case - a full map, slot 0 removed in every instance, so every element of P moves - between an event
      pair, the map refilled by one plain step before each repetition; beside it a device-to-device hipMemcpyAsync that reads and
      writes the same number of bytes slam_last_map_work reports (a copy of half of them), on the same stream;
  (d) the EMPTY prune: slam_map_prune on counters that pick nothing, 20 calls between one event pair (per call: a memset and four
      launches that read a few words per instance).
No time is fixed in advance: the yardstick of (c) is the copy of the same run.  Medians; one JSON line per part and configuration."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_associate import CONFIGS, _hip, _put, record_log  # noqa: E402
from tools.gpu_gate import consistent_rows  # noqa: E402

INST_CAPACITY = 8


class Events:
    """A stream of this tool's own and event pairs on it."""

    def __init__(self, hip):
        self.hip = hip
        hip.hipStreamCreateWithFlags.argtypes = [C.POINTER(C.c_void_p), C.c_uint]
        hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
        hip.hipEventRecord.argtypes = [C.c_void_p, C.c_void_p]
        hip.hipEventSynchronize.argtypes = [C.c_void_p]
        hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
        hip.hipMemcpyAsync.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
        self.stream = C.c_void_p()
        assert hip.hipStreamCreateWithFlags(C.byref(self.stream), 1) == 0          # hipStreamNonBlocking
        self.a, self.b = C.c_void_p(), C.c_void_p()
        assert hip.hipEventCreate(C.byref(self.a)) == 0 and hip.hipEventCreate(C.byref(self.b)) == 0

    def ms(self, work):
        """Device time of what work() enqueues on the stream."""
        assert self.hip.hipEventRecord(self.a, self.stream) == 0
        work()
        assert self.hip.hipEventRecord(self.b, self.stream) == 0
        assert self.hip.hipEventSynchronize(self.b) == 0
        out = C.c_float(0)
        assert self.hip.hipEventElapsedTime(C.byref(out), self.a, self.b) == 0
        return float(out.value)


def with_clutter(S, cfg, meas, cnt, seed):
    """ids erased; one clutter detection per instance and tick, uniform in the view, appended (or in the last slot of a full row)."""
    rng = np.random.default_rng(seed)
    T, B, ks, _ = meas.shape
    out = meas.copy(); out[:, :, :, 0] = np.nan
    at = np.minimum(cnt, ks - 1)
    t_i, b_i = np.meshgrid(np.arange(T), np.arange(B), indexing="ij")
    out[t_i, b_i, at, 0] = np.nan
    out[t_i, b_i, at, 1] = rng.uniform(0.3, cfg.range_max, (T, B))
    out[t_i, b_i, at, 2] = rng.uniform(cfg.fov_min, cfg.fov_max, (T, B))
    return out, (at + 1).astype(np.int32)


def effect(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    meas, cnt, truth = record_log(S, cfg, lm, cmds, B, ks, S.F64, rows, True)
    log, log_cnt = with_clutter(S, cfg, meas, cnt, 7)
    out = dict(tool="gpu_map_manage", part="effect", L=L, batch=B, ticks=T, clutter_per_tick=1, map_config=dict(
        (k, getattr(S.default_map_config(), k)) for k in ("range_shrink", "fov_margin", "min_expected", "min_ratio", "prune_every")))
    for name in ("associate_run", "manage_run"):
        f = S.BatchedEKF(B, L).readParams(cfg)
        f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        res = getattr(f, name)(cmds, log, log_cnt, series=(name == "manage_run"))
        ms = f.last_associate_work()[3] if name == "associate_run" else f.last_map_work()[2]
        err = float(np.hypot(*(f.poses()[:, :2] - truth[T - 1, :, :2]).T).mean())
        out[name] = dict(landmarks_held_mean=float(f.landmark_counts().mean()), landmarks_held_max=int(f.landmark_counts().max()),
                         no_room_drops=float(res.recs[:, 10].sum()), capacity_instances=int(((f.status() & INST_CAPACITY) != 0).sum()),
                         flagged_instances=int((f.status() != 0).sum()), pos_err_at_end=err, ms_per_tick=ms / T,
                         matched=float(res.recs[:, 4].sum()), new=float(res.recs[:, 5].sum()))
        if name == "manage_run":
            out[name]["landmarks_removed"] = int(res.n_removed.sum())
        f.close()
        r = out[name]
        print(f"#   {name:13s} landmarks held {r['landmarks_held_mean']:.2f} (max {r['landmarks_held_max']}) | NO_ROOM drops {r['no_room_drops']:.0f} | "
              f"CAPACITY instances {r['capacity_instances']} | position error at the end {r['pos_err_at_end']:.4f} m | {r['ms_per_tick']:.4f} ms per tick")
    print(json.dumps(out), flush=True)


def cost(S, name, L, B, f32, args, hip):
    from live_ekf_slam_amd.scenario import make_scenario
    T, ks, w = args.ticks, args.k_stride, args.warmup
    dt = S.F32 if f32 else S.F64
    esz = 4 if f32 else 8
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11 = (v ** 2 / 3 for v in (cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11))   # (no rows: one config for the batch)
    sim_cfg = S.default_config(); sim_cfg.replicate_vw_quirk = 0
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    meas, cnt, _ = record_log(S, sim_cfg, lm, cmds, B, ks, dt, None, False)
    log, log_cnt = with_clutter(S, sim_cfg, meas, cnt, 7)
    ev = Events(hip)
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_stream(ev.stream.value)
    f.set_seed(2025)

    def manage_route(n=T):
        f.init(0.0, 0.0, 0.0)
        res = f.manage_run(cmds[:n], log[:n], log_cnt[:n], series=True)
        return f.last_map_work(), res

    def assoc_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.associate_run(cmds[:n], log[:n], log_cnt[:n])
        return f.last_associate_work()[3]
    manage_route(w); assoc_route(w)
    a_ms, b_ms = [], []
    for _ in range(args.reps):
        work, res = manage_route()
        a_ms.append(work[2])
        b_ms.append(assoc_route())
    f.set_nav_timing(True)
    (run_bytes, prune_ms, timed_total), res = manage_route()
    f.set_nav_timing(False)
    prunes = T // S.default_map_config().prune_every

    # (b) the tally alone, on the state the run left and the last message of the log
    d_m, d_c = _put(hip, log[T - 1]), _put(hip, log_cnt[T - 1])
    f.map_tally(d_m.value, (d_c.value, ks)); f.sync()
    tally_ms = [ev.ms(lambda: [f.map_tally(d_m.value, (d_c.value, ks)) for _ in range(20)]) / 20 for _ in range(args.reps)]
    held = float(f.landmark_counts().mean())

    # (c) the worst case and its yardstick; (d) the empty prune
    f.init(0.0, 0.0, 0.0)
    j = np.arange(L)
    full = np.stack([1000.0 + j, 1.0 + 0.04 * j, -1.2 + 2.4 * (j % 10) / 9.0], axis=1).astype(np.float32)
    f.update((0.0, 0.0), np.repeat(full[None], B, axis=0), np.full(B, L, np.int32))
    assert (f.landmark_counts() == L).all()
    mask = np.zeros((B, L), np.int32); mask[:, 0] = 1
    d_mask = _put(hip, mask)
    refill = np.zeros((B, 1, 3), np.float32); one = np.ones(B, np.int32)
    worst_ms, copy_ms, worst_bytes = [], [], 0.0
    src = dst = None
    for rep in range(args.reps + 1):                                  # (the first repetition is the warm-up)
        ms = ev.ms(lambda: f.remove_landmarks(d_mask.value, stats=False))
        worst_bytes = f.last_map_work()[0]
        assert (f.landmark_counts() == L - 1).all()
        if src is None:
            half = int(worst_bytes // 2)
            src, dst = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(src), half) == 0 and hip.hipMalloc(C.byref(dst), half) == 0
            assert hip.hipMemcpyAsync(dst, src, half, 3, ev.stream) == 0
        cp = ev.ms(lambda: hip.hipMemcpyAsync(dst, src, half, 3, ev.stream))           # hipMemcpyDeviceToDevice
        if rep:
            worst_ms.append(ms); copy_ms.append(cp)
        refill[:, 0] = [2000.0 + rep, 2.0, 0.05 * rep]
        f.update((0.0, 0.0), refill, one)
        assert (f.landmark_counts() == L).all()
    f.map_prune(stats=False); f.sync()
    assert (f.landmark_counts() == L).all()
    empty_ms = [ev.ms(lambda: [f.map_prune(stats=False) for _ in range(20)]) / 20 for _ in range(args.reps)]
    empty_bytes = f.last_map_work()[0]
    f.close()
    for p in (d_m, d_c, d_mask, src, dst):
        hip.hipFree(p)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    wm, cm = statistics.median(worst_ms), statistics.median(copy_ms)
    print(json.dumps({
        "tool": "gpu_map_manage", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T,
        "k_stride": ks, "reps": args.reps, "a_manage_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "a_associate_run_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms], "manage_over_associate": round(a / b, 4),
        "prunes_in_the_run": prunes, "prune_launches_ms_per_prune": round(prune_ms / max(prunes, 1), 5), "timed_manage_run_ms_per_tick": round(timed_total / T, 4),
        "run_model_bytes_per_prune": run_bytes / max(prunes, 1), "landmarks_removed_in_the_run": int(res.n_removed.sum()),
        "landmarks_held_mean_at_the_tally": held, "b_tally_ms_per_call": round(statistics.median(tally_ms), 5), "tally_ms_all": [round(v, 5) for v in tally_ms],
        "c_worst_removal_ms": round(wm, 4), "worst_ms_all": [round(v, 4) for v in worst_ms], "worst_model_bytes": worst_bytes,
        "worst_model_GBps": round(worst_bytes / (wm * 1e-3) / 1e9, 1), "c_copy_of_half_the_bytes_ms": round(cm, 4), "copy_ms_all": [round(v, 4) for v in copy_ms],
        "copy_read_plus_write_GBps": round(worst_bytes / (cm * 1e-3) / 1e9, 1), "worst_over_copy": round(wm / cm, 3),
        "slab_bytes": float(B) * esz * (3 + 2 * L) * ((3 + 2 * L + 1) & ~1 if esz == 8 else (3 + 2 * L + 3) & ~3),
        "d_empty_prune_ms_per_call": round(statistics.median(empty_ms), 5), "empty_ms_all": [round(v, 5) for v in empty_ms],
        "empty_model_bytes": empty_bytes}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--effect-batch", type=int, default=256)
    ap.add_argument("--effect-ticks", type=int, default=300)
    ap.add_argument("--k-stride", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["effect"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    hip = _hip()
    if args.only in (None, "effect"):
        effect(S, args)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args, hip)


if __name__ == "__main__":
    main()
