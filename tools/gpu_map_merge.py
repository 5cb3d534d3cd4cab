#!/usr/bin/env python3
"""Landmark merging (slam_map_duplicates, slam_merge_landmarks, slam_map_merge, slam_manage_merge_run) on one MI355X: what it does to an
id-less log whose outliers spawn duplicates, and what it costs.

Part 1, the effect.  The `spread` log of tools/gpu_associate.py (L = --landmarks, filter rows at the variances of the simulator's uniform
draws) with its ids erased, associated with gate_new LOWERED TO gate_match: a detection beyond the match gate is no longer dropped as
ambiguous but inserted, so every outlier return of a mapped landmark spawns a duplicate.  The log is replayed on two host-fed handles of
capacity 2 L: manage_run and manage_merge_run (default map and merge configs).  Printed per replay at the end of --effect-ticks ticks:
landmarks held per instance against the landmarks truly seen (distinct true ids of the instance's log), pairs fused, landmarks pruned,
the mean position error against the recorded truth at the last tick, device ms per tick.

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration, on ONE handle whose stream this tool owns (so HIP events can bracket single calls), after a warm-up of each
route, --reps repetitions ALTERNATING
  (a) manage_merge_run and manage_run on the same log, device time by the runs' own events;
  (b) slam_map_duplicates_dev alone on a full map, 5 calls between one event pair, and beside it the same handle's plain once-per-tick
      step (slam_step_dev of a one-detection message, 5 calls between one event pair): both read all of P;
  (c) the WORST case of one fused pair in every instance - a full map whose last slot duplicates slot 0, so every element of P is
      updated and then moves - as slam_map_merge (find, fuse, compact) and as slam_merge_landmarks_dev (fuse, compact) between an event
      pair each, the duplicate re-inserted by one plain step before each; beside them a device-to-device hipMemcpyAsync that reads and
      writes the same number of bytes slam_last_merge_work reports (a copy of half of them), on the same stream;
  (d) the EMPTY call: slam_map_merge on a map without a pair, 5 calls between one event pair (the find reads P; nothing else does).
No time is fixed in advance: the yardsticks are the step and the copy of the same run.  Medians; one JSON line per part and configuration."""
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
from tools.gpu_map_manage import Events  # noqa: E402


def erased(meas):
    out = meas.copy(); out[:, :, :, 0] = np.nan
    return out


def effect(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    meas, cnt, truth = record_log(S, cfg, lm, cmds, B, ks, S.F64, rows, True)
    seen = np.array([len({int(meas[t, b, l, 0]) for t in range(T) for l in range(min(int(cnt[t, b]), ks))}) for b in range(B)])
    log = erased(meas)
    gm = S.default_assoc_config().gate_match
    ac = S.AssocConfig(gm, gm)
    out = dict(tool="gpu_map_merge", part="effect", L=L, capacity=2 * L, batch=B, ticks=T, gate_match=gm, gate_new=gm,
               landmarks_truly_seen_mean=float(seen.mean()),
               merge_config=dict((k, getattr(S.default_merge_config(), k)) for k in ("gate_merge", "sigma", "merge_every")))
    for name in ("manage_run", "manage_merge_run"):
        f = S.BatchedEKF(B, 2 * L).readParams(cfg)
        f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        res = getattr(f, name)(cmds, log, cnt, series=True, cfg=ac)
        ms = f.last_map_work()[2] if name == "manage_run" else f.last_merge_work()[2]
        held = f.landmark_counts()
        err = float(np.hypot(*(f.poses()[:, :2] - truth[T - 1, :, :2]).T).mean())
        out[name] = dict(landmarks_held_mean=float(held.mean()), landmarks_held_max=int(held.max()), excess_over_seen_mean=float((held - seen).mean()),
                         landmarks_removed=int(res.n_removed.sum()), pairs_fused=int(res.n_merged.sum()) if name == "manage_merge_run" else 0,
                         flagged_instances=int((f.status() != 0).sum()), pos_err_at_end=err, ms_per_tick=ms / T,
                         matched=float(res.recs[:, 4].sum()), new=float(res.recs[:, 5].sum()))
        f.close()
        r = out[name]
        print(f"#   {name:16s} landmarks held {r['landmarks_held_mean']:.2f} (max {r['landmarks_held_max']}) against {seen.mean():.2f} truly seen | "
              f"pairs fused {r['pairs_fused']} | pruned {r['landmarks_removed']} | position error at the end {r['pos_err_at_end']:.4f} m | "
              f"{r['ms_per_tick']:.4f} ms per tick")
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
    log = erased(meas)
    gm = S.default_assoc_config().gate_match
    ac = S.AssocConfig(gm, gm)
    ev = Events(hip)
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_stream(ev.stream.value)
    f.set_seed(2025)

    def merge_route(n=T):
        f.init(0.0, 0.0, 0.0)
        res = f.manage_merge_run(cmds[:n], log[:n], cnt[:n], series=True, cfg=ac)
        return f.last_merge_work(), res

    def manage_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.manage_run(cmds[:n], log[:n], cnt[:n], cfg=ac)
        return f.last_map_work()[2]
    merge_route(w); manage_route(w)
    a_ms, b_ms = [], []
    for _ in range(args.reps):
        work, res = merge_route()
        a_ms.append(work[2])
        b_ms.append(manage_route())
    f.set_nav_timing(True)
    (run_bytes, merge_ms, timed_total), res = merge_route()
    f.set_nav_timing(False)
    merges = T // S.default_merge_config().merge_every

    # a full map whose last slot duplicates slot 0: the same detection under a second id
    f.init(0.0, 0.0, 0.0)
    j = np.arange(L - 1)
    full = np.stack([1000.0 + j, 1.0 + 0.04 * j, -1.2 + 2.4 * (j % 10) / 9.0], axis=1).astype(np.float32)
    f.update((0.0, 0.0), np.repeat(full[None], B, axis=0), np.full(B, L - 1, np.int32))
    dup = np.zeros((B, 1, 3), np.float32); one = np.ones(B, np.int32)
    d_one = _put(hip, one)

    def refill(rep):
        dup[:, 0] = [5000.0 + rep, full[0, 1], full[0, 2]]
        f.update((0.0, 0.0), dup, one)
        assert (f.landmark_counts() == L).all()
    refill(0)
    partner = np.full((B, L), -1, np.int32); partner[:, 0] = L - 1; partner[:, L - 1] = 0
    d_partner = _put(hip, partner)
    d_out = _put(hip, np.zeros((B, L), np.int32)); d_d2 = _put(hip, np.zeros((B, L)))

    # (c) the worst case and its yardstick
    worst_ms, fuse_ms, copy_ms, worst_bytes, fuse_bytes = [], [], [], 0.0, 0.0
    src = dst = None
    for rep in range(args.reps + 1):                                  # (the first repetition is the warm-up)
        ms = ev.ms(lambda: f.map_merge(stats=False))
        worst_bytes = f.last_merge_work()[0]
        assert (f.landmark_counts() == L - 1).all()
        refill(2 * rep + 1)
        ms2 = ev.ms(lambda: f.merge_landmarks(d_partner.value, stats=False))
        fuse_bytes = f.last_merge_work()[0]
        assert (f.landmark_counts() == L - 1).all()
        if src is None:
            half = int(worst_bytes // 2)
            src, dst = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(src), half) == 0 and hip.hipMalloc(C.byref(dst), half) == 0
            assert hip.hipMemcpyAsync(dst, src, half, 3, ev.stream) == 0
        cp = ev.ms(lambda: hip.hipMemcpyAsync(dst, src, half, 3, ev.stream))           # hipMemcpyDeviceToDevice
        if rep:
            worst_ms.append(ms); fuse_ms.append(ms2); copy_ms.append(cp)
        refill(2 * rep + 2)

    # (d) the empty call: the map without its duplicate
    f.merge_landmarks(d_partner.value, stats=False); f.sync()
    assert (f.landmark_counts() == L - 1).all()
    r = f.map_merge()
    assert not r["n_merged"].any()
    empty_ms = [ev.ms(lambda: [f.map_merge(stats=False) for _ in range(5)]) / 5 for _ in range(args.reps)]
    empty_bytes = f.last_merge_work()[0]
    # (b) the find alone, on the full map with its duplicate back, beside the plain step of the same handle (a re-observation of landmark 1)
    step_msg = np.repeat(full[None, 1:2], B, axis=0).astype(np.float32)
    d_step = _put(hip, step_msg)
    cmd0 = np.zeros(2, np.float32)

    def steps():
        for _ in range(5):
            f.update_dev(cmd0, d_step.value, d_one.value, 1)
    refill(99)
    f.map_duplicates(dev=(d_out.value, d_d2.value)); f.sync()
    got = np.zeros((B, L), np.int32)
    assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_out, got.nbytes, 2) == 0
    assert (got[:, 0] == L - 1).all() and (got[:, L - 1] == 0).all() and ((got >= 0).sum(axis=1) == 2).all(), "one pair in every instance"
    steps(); f.sync()
    find_ms, step_ms = [], []
    for _ in range(args.reps):
        find_ms.append(ev.ms(lambda: [f.map_duplicates(dev=(d_out.value, d_d2.value)) for _ in range(5)]) / 5)
        step_ms.append(ev.ms(steps) / 5)
    find_bytes = f.last_merge_work()[0]

    f.close()
    for p in (d_one, d_partner, d_out, d_d2, d_step, src, dst):
        hip.hipFree(p)
    a, b = statistics.median(a_ms), statistics.median(b_ms)
    wm, fm, cm = statistics.median(worst_ms), statistics.median(fuse_ms), statistics.median(copy_ms)
    fd, st = statistics.median(find_ms), statistics.median(step_ms)
    print(json.dumps({
        "tool": "gpu_map_merge", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T,
        "k_stride": ks, "reps": args.reps, "a_manage_merge_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "a_manage_run_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms], "merge_over_manage": round(a / b, 4),
        "merges_in_the_run": merges, "merge_launches_ms_per_merge": round(merge_ms / max(merges, 1), 5), "timed_run_ms_per_tick": round(timed_total / T, 4),
        "run_model_bytes_per_merge": run_bytes / max(merges, 1), "pairs_fused_in_the_run": int(res.n_merged.sum()),
        "b_find_ms_per_call": round(fd, 4), "find_ms_all": [round(v, 4) for v in find_ms], "find_model_bytes": find_bytes,
        "find_model_GBps": round(find_bytes / (fd * 1e-3) / 1e9, 1), "b_plain_step_ms_per_call": round(st, 4), "step_ms_all": [round(v, 4) for v in step_ms],
        "find_over_step": round(fd / st, 3),
        "c_worst_map_merge_ms": round(wm, 4), "worst_ms_all": [round(v, 4) for v in worst_ms], "worst_model_bytes": worst_bytes,
        "worst_model_GBps": round(worst_bytes / (wm * 1e-3) / 1e9, 1), "c_fuse_and_compact_ms": round(fm, 4), "fuse_ms_all": [round(v, 4) for v in fuse_ms],
        "fuse_model_bytes": fuse_bytes, "c_copy_of_half_the_worst_bytes_ms": round(cm, 4), "copy_ms_all": [round(v, 4) for v in copy_ms],
        "copy_read_plus_write_GBps": round(worst_bytes / (cm * 1e-3) / 1e9, 1), "worst_over_copy": round(wm / cm, 3),
        "fuse_over_its_share_of_the_copy": round(fm / (cm * fuse_bytes / worst_bytes), 3),
        "slab_bytes": float(B) * esz * (3 + 2 * L) * ((3 + 2 * L + 1) & ~1 if esz == 8 else (3 + 2 * L + 3) & ~3),
        "d_empty_map_merge_ms_per_call": round(statistics.median(empty_ms), 4), "empty_ms_all": [round(v, 4) for v in empty_ms],
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
