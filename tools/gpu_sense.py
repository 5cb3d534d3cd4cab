#!/usr/bin/env python3
"""The simulator source with a sensor fault model (slam_sense*, the *_run_sim calls) on one MI355X: what the robustness stack does under
outliers, clutter and erased ids with the truth on the device, in open and in closed loop, and what the source costs.

Part a, the sweep.  ONE handle at L = --landmarks, batch --effect-batch: 16 groups of instances (b % 16) over a grid of p_spike x clutter
rate (4 x 4; spikes of 0.5 .. 2 m, up to 2 clutter slots), ids erased and shuffled, filter rows at the variances of the simulator's uniform
draws.  Replayed with associate_run_sim and manage_merge_run_sim (capacity 2 L).  Per group, from the device's own truth: the average
position error (slam_error_stats), the landmarks held against the landmarks truly seen (distinct true rows in the logged `origin`), and -
on a sample of instances, by one more sensed tick through slam_associate - the share of matches whose landmark is the true map row of the
detection (`origin`; the filter's landmark is mapped to the nearest true one).
Part b, the closed loop.  The same id-less, cluttered sensor under source NAV (pure pursuit on each instance's own estimate), beside the
all-off sensor: waypoints reached, position error, instances whose association steered them off (error above 1 m).
Part c, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and fp32 storage, L = 20 x batch 4096 fp64.
Per configuration and per *_run_sim call, on ONE handle, after a warm-up, --reps repetitions ALTERNATING the _sim run and its LOG sibling
fed that run's own logged messages: device ms per tick of both by the runs' own events, and the LOG side's wall time including the upload
of its log.  Beside them a plain once-per-tick slam_run_sim (run chunk 1) and the sense + commit launches alone, 5 pairs between one event
pair.  No time is fixed in advance: the yardsticks are the LOG sibling and the plain run of the same call.  Medians; one JSON line per part
and configuration."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_associate import CONFIGS, _hip, _put  # noqa: E402
from tools.gpu_gate import consistent_rows  # noqa: E402
from tools.gpu_map_manage import Events  # noqa: E402

P_SPIKE = (0.0, 0.05, 0.15, 0.3)
P_CLUTTER = (0.0, 0.1, 0.3, 0.6)
PATH = np.array([[1.0, 0.3], [2.0, -0.4], [3.0, 0.5], [4.0, -0.2], [5.0, 0.6]])


def grid_rows(S, B, erase=True):
    groups = [S.default_sensor_config(p_spike=ps, spike_lo=0.5, spike_hi=2.0, p_clutter=pc, n_clutter=2, clutter_r_min=0.3, shuffle=1,
                                      erase_ids=int(erase)) for ps in P_SPIKE for pc in P_CLUTTER]
    return (S.SensorConfig * B)(*[groups[b % 16] for b in range(B)])


def _handle(S, cfg, lm, B, cap, rows, sensor, dtype=None, stream=None):
    f = S.BatchedEKF(B, cap, dtype=S.F64 if dtype is None else dtype).readParams(cfg)
    if stream is not None:
        f.set_stream(stream)
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    if rows is not None:
        f.set_noise(rows)
    f.set_sensor(sensor)
    return f


def agreement(S, f, lm, cmd, ks, sample):
    """One more sensed tick through slam_associate: per sampled instance (matches, matches whose landmark is the detection's true row)."""
    out = f.sense(cmd, ks)
    a = f.associate(cmd, out["meas"], np.minimum(out["count"], ks), det=False)
    f.sense_commit(stats=False)            # (no step: nothing is committed)
    n = np.zeros(f.batch, int); ok = np.zeros(f.batch, int)
    for b in sample:
        st = f.get_state(int(b))
        if st["M"] == 0:
            continue
        est = st["x"][3:3 + 2 * st["M"]].reshape(-1, 2)
        true_row = np.argmin(((est[:, None, :] - lm[None]) ** 2).sum(axis=2), axis=1)
        for l in range(min(int(out["count"][b]), ks)):
            if a["verdict"][b, l] == S.ASSOC_MATCHED:
                n[b] += 1
                ok[b] += int(true_row[a["slot"][b, l]] == out["origin"][b, l])
    return n, ok


def sweep(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    lm, cmds = make_scenario(321 + L, L, T + 1)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    sensor = grid_rows(S, B)
    group = np.arange(B) % 16
    sample = np.concatenate([np.flatnonzero(group == g)[:args.sample] for g in range(16)])
    out = dict(tool="gpu_sense", part="sweep", L=L, capacity=2 * L, batch=B, ticks=T, k_stride=ks, p_spike=P_SPIKE, p_clutter=P_CLUTTER)
    for name in ("associate_run_sim", "manage_merge_run_sim"):
        f = _handle(S, cfg, lm, B, 2 * L, rows, sensor)
        res = getattr(f, name)(cmds[:T], series=False, log=("origin", "recs"), k_stride=ks)
        org = res.sense.origin
        seen = np.array([len(set(org[:, b][org[:, b] >= 0].tolist())) for b in sample])
        err, held = f.error_stats(), f.landmark_counts()
        n, ok = agreement(S, f, lm, cmds[T], ks, sample)
        flagged = f.status() != 0
        f.close()
        table = []
        for g in range(16):
            m = group == g
            ms = group[sample] == g
            table.append(dict(p_spike=P_SPIKE[g // 4], p_clutter=P_CLUTTER[g % 4], avg_pos_err=float(err[m].mean()), held=float(held[m].mean()),
                              truly_seen=float(seen[ms].mean()), matches=int(n[sample][ms].sum()), matches_agree=int(ok[sample][ms].sum()),
                              flagged=int(flagged[m].sum())))
            r = table[-1]
            print(f"#   {name:22s} p_spike {r['p_spike']:.2f} p_clutter {r['p_clutter']:.2f} | avg position error {r['avg_pos_err']:.4f} m | landmarks held "
                  f"{r['held']:.2f} against {r['truly_seen']:.2f} truly seen | matches agreeing with origin {r['matches_agree']}/{r['matches']}")
        out[name] = dict(groups=table, spiked=float(res.sense.recs[:, 5].sum()), clutter=float(res.sense.recs[:, 6].sum()),
                         committed=float(res.sense.recs[:, 10].sum()))
    print(json.dumps(out), flush=True)


def closed_loop(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.nav_batch, args.nav_ticks, args.k_stride
    lm, _ = make_scenario(321 + L, L, 1)
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    out = dict(tool="gpu_sense", part="closed_loop", L=L, batch=B, ticks=T, source="NAV")
    for label, sensor in (("clean_idless", (S.SensorConfig * B)(*[S.default_sensor_config(shuffle=1, erase_ids=1)] * B)), ("grid", grid_rows(S, B))):
        f = _handle(S, cfg, lm, B, 2 * L, rows, sensor)
        f.set_path(PATH)
        res = f.associate_run_sim(T=T, log=("err_pos", "recs"), k_stride=ks)
        nav = f.nav_state()
        remaining, finish = nav["remaining"], nav["finish_tick"]
        err = f.error_stats()
        last = res.sense.err_pos[-1]
        out[label] = dict(avg_pos_err=float(err.mean()), err_at_end=float(np.nanmean(last)), off_by_more_than_1m=int((last > 1.0).sum()),
                          finished=int((np.asarray(finish) >= 0).sum()), waypoints_left_mean=float(np.asarray(remaining).mean()),
                          flagged=int((f.status() != 0).sum()), matched=float(res.recs[:, 4].sum()), new=float(res.recs[:, 5].sum()))
        f.close()
        r = out[label]
        print(f"#   NAV {label:13s} avg position error {r['avg_pos_err']:.4f} m | at the end {r['err_at_end']:.4f} m | off by more than 1 m "
              f"{r['off_by_more_than_1m']} of {B} | finished the path {r['finished']} | waypoints left {r['waypoints_left_mean']:.2f}")
    print(json.dumps(out), flush=True)


RUNS = {"gate": ("gate_run_sim", "gate_run", "last_gate_work", 1), "associate": ("associate_run_sim", "associate_run", "last_associate_work", 3),
        "associate_joint": ("associate_joint_run_sim", "associate_joint_run", "last_joint_work", 3),
        "manage": ("manage_run_sim", "manage_run", "last_map_work", 2), "manage_merge": ("manage_merge_run_sim", "manage_merge_run", "last_merge_work", 2)}


def cost(S, name, L, B, f32, args, hip):
    from live_ekf_slam_amd.scenario import make_scenario
    T, ks, w = args.ticks, args.k_stride, args.warmup
    dt = S.F32 if f32 else S.F64
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    ev = Events(hip)
    out = {"tool": "gpu_sense", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T, "k_stride": ks,
           "reps": args.reps, "bytes_of_the_two_launches_model": B * (12 * ks + 60)}
    for kind, (sim_name, log_name, work_name, total_at) in RUNS.items():
        idless = kind != "gate"
        sensor = (S.SensorConfig * B)(*[S.default_sensor_config(p_spike=0.05, spike_lo=0.5, spike_hi=2.0, p_clutter=0.3, n_clutter=2, clutter_r_min=0.3,
                                                                shuffle=int(idless), erase_ids=int(idless))] * B)
        f = _handle(S, cfg, lm, B, L, rows, sensor, dtype=dt, stream=ev.stream.value)

        def sim_route(n=T, log=False):
            f.init(0.0, 0.0, 0.0)
            res = getattr(f, sim_name)(cmds[:n], log=log, k_stride=ks)
            return getattr(f, work_name)()[total_at], res

        def log_route(lg, n=T):
            f.init(0.0, 0.0, 0.0)
            t0 = time.perf_counter()
            getattr(f, log_name)(cmds[:n], lg.meas[:n], lg.count[:n])
            f.sync()
            return getattr(f, work_name)()[total_at], (time.perf_counter() - t0) * 1e3
        _, res = sim_route(log=("meas", "count"))
        lg = res.sense
        sim_route(w); log_route(lg, w)
        s_ms, l_ms, l_wall = [], [], []
        for _ in range(args.reps):
            s_ms.append(sim_route()[0])
            dev, wall = log_route(lg)
            l_ms.append(dev); l_wall.append(wall)
        f.close()
        s, lo, lw = statistics.median(s_ms), statistics.median(l_ms), statistics.median(l_wall)
        out[kind] = dict(sim_ms_per_tick=round(s / T, 4), log_device_ms_per_tick=round(lo / T, 4), log_wall_ms_per_tick_with_upload=round(lw / T, 4),
                         sim_minus_log_device_ms_per_tick=round((s - lo) / T, 4), sim_ms_all=[round(v, 2) for v in s_ms], log_ms_all=[round(v, 2) for v in l_ms])
    # the plain once-per-tick run, and the sense + commit launches alone
    f = _handle(S, cfg, lm, B, L, rows, sensor, dtype=dt, stream=ev.stream.value)
    f.set_run_chunk(1)
    f.run_sim(cmds[:w]); f.sync()
    plain = []
    for _ in range(args.reps):
        f.init(0.0, 0.0, 0.0)
        plain.append(ev.ms(lambda: f.run_sim(cmds)) / T)
    d_meas, d_count = _put(hip, np.zeros((B, ks, 3), np.float32)), _put(hip, np.zeros(B, np.int32))
    cmd = cmds[0]

    def pairs():
        for _ in range(5):
            f.sense_dev(cmd, d_meas.value, d_count.value, ks)
            f.sense_commit(stats=False)
    pairs(); f.sync()
    two = [ev.ms(pairs) / 5 for _ in range(args.reps)]
    f.close()
    hip.hipFree(d_meas); hip.hipFree(d_count)
    out["plain_run_sim_once_per_tick_ms_per_tick"] = round(statistics.median(plain), 4)
    out["sense_plus_commit_launches_ms"] = round(statistics.median(two), 5)
    out["sense_plus_commit_all"] = [round(v, 5) for v in two]
    out["model_GBps_of_the_two_launches"] = round(out["bytes_of_the_two_launches_model"] / (statistics.median(two) * 1e-3) / 1e9, 1)
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--effect-batch", type=int, default=65536)
    ap.add_argument("--effect-ticks", type=int, default=200)
    ap.add_argument("--sample", type=int, default=8, help="instances per group whose matches are compared with origin")
    ap.add_argument("--nav-batch", type=int, default=4096)
    ap.add_argument("--nav-ticks", type=int, default=600)
    ap.add_argument("--k-stride", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["sweep", "closed_loop"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    hip = _hip()
    if args.only in (None, "sweep"):
        sweep(S, args)
    if args.only in (None, "closed_loop"):
        closed_loop(S, args)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args, hip)


if __name__ == "__main__":
    main()
