#!/usr/bin/env python3
"""Joint-compatibility association (slam_associate_joint*, slam_step_associated_joint_dev, slam_associate_joint_run) on one MI355X: what
it does to an id-less log on which the pose is uncertain relative to the landmark spacing, and what a jointly associated tick costs.

Part 1, the effect.  Map `lattice`: --rows x --cols landmarks --spacing m apart whose first column stands --stretch m ahead of the start,
beyond the sensor's range, so the tour of slam_scenario (generate_full_trajectory) first drives a stretch without detections.  The
simulator and the filter run under RAISED odometry noise (--odo-scale times the config's V half-widths; filter rows = the variances
a^2 / 3, replicate_vw_quirk = 0, as tools/gpu_associate.py).  One SIM handle of --effect-batch instances records the messages WITH the true
ids and the true poses; the log is replayed three ways on host-fed handles:
  1  true ids      the plain known-id step
  2  associated    ids erased; slam_associate_dev (verdicts), then slam_step_associated_dev
  3  joint         ids erased; slam_associate_joint_dev (verdicts), then slam_step_associated_joint_dev
Printed per replay: position error at the end and its mean over the ticks, landmarks created against landmarks truly seen, the share of
MATCHED detections whose landmark is the one the true id says (first-insertion mapping), detections dropped; for the joint replay also
nodes per instance-tick (mean, max) and the share of instance-ticks with JOINT_BUDGET - and, when there are any, the replay again with 4 x
the budget.  The `spread` and `pairs` maps of tools/gpu_associate.py follow, where the two associations should agree.

Part 2, the cost.  L = 50 x batch 65 536 in fp64 and fp32, L = 20 x 4096 fp64 unless --only picks one: on ONE host-fed handle,
re-initialised before every run, after a warm-up of each route, --reps repetitions ALTERNATING (a) associate_joint_run, (b) associate_run
(device time by HIP events) and (c) a plain slam_step_dev loop over the same log with its ids (host clock, synchronised); then once with an
event pair around every tick's joint launches (set_nav_timing) and the traffic model.  Medians; one JSON line per part and configuration."""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_associate import CONFIGS, _hip, _put, record_log  # noqa: E402
from tools.gpu_gate import consistent_rows  # noqa: E402

BUDGET = 16


def lattice_scenario(args):
    from live_ekf_slam_amd.scenario import generate_full_trajectory
    ys = (np.arange(args.rows) - (args.rows - 1) / 2.0) * args.spacing
    xs = args.stretch + np.arange(args.cols) * args.spacing
    lm = np.array([[x, y] for x in xs for y in ys], dtype=np.float64)
    cmds = generate_full_trajectory(lm, args.effect_ticks, random.Random(4711))
    return lm, np.ascontiguousarray(cmds, dtype=np.float32)


def effect(S, args, hip, which):
    from live_ekf_slam_amd.scenario import make_scenario
    B, T, ks = args.effect_batch, args.effect_ticks, args.k_stride
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    if which == "lattice":
        lm, cmds = lattice_scenario(args)
        cfg.V_00 *= args.odo_scale; cfg.V_11 *= args.odo_scale
    else:
        L = args.landmarks
        lm, cmds = make_scenario(321 + L, L, T)
        if which == "pairs":
            lm = np.concatenate([lm[:L // 2], lm[:L // 2] + np.array([0.6, 0.0])])
        cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    rows = consistent_rows(S, cfg, B)
    meas, cnt, truth = record_log(S, cfg, lm, cmds, B, ks, S.F64, rows, True)
    valid = np.arange(ks)[None, None, :] < cnt[:, :, None]
    true_id = np.where(valid, meas[:, :, :, 0], -1).astype(np.int64)
    erased = meas.copy(); erased[:, :, :, 0] = np.nan
    seen = np.array([np.unique(true_id[:, b][true_id[:, b] >= 0]).size for b in range(B)])
    first_det = int(np.argmax(cnt.sum(axis=1) > 0)) if valid.any() else -1
    Lm = lm.shape[0]

    def replay(kind, max_nodes=None):
        c = S.default_config(); c.replicate_vw_quirk = 0
        f = S.BatchedEKF(B, Lm).readParams(c)
        f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        jcfg = S.default_joint_config()
        if max_nodes:
            jcfg.max_nodes = max_nodes
        first = np.full((B, Lm), -1, np.int64)
        agree, matches, dropped, err_sum = 0, 0, 0, 0.0
        nodes_sum, nodes_max, budget, differ = 0, 0, 0, 0
        d_lab, d_labc = _put(hip, np.zeros_like(erased[0])), _put(hip, np.zeros_like(cnt[0]))
        for t in range(T):
            if kind == "true_ids":
                f.update(cmds[t], meas[t], cnt[t])
            else:
                d_m, d_c = _put(hip, erased[t]), _put(hip, cnt[t])
                M0 = f.landmark_counts()
                if kind == "associated":
                    r = f.associate_dev(cmds[t], d_m.value, d_c.value, ks, d_lab.value, d_labc.value, det=False)
                    f.step_associated_dev(cmds[t], d_m.value, d_c.value, ks, stats=False)
                else:
                    r = f.associate_joint(cmds[t], d_m.value, (d_c.value, ks), det=False, cfg=jcfg, dev_out=(d_lab.value, d_labc.value))
                    f.step_associated_joint(cmds[t], d_m.value, (d_c.value, ks), stats=False, cfg=jcfg)
                    nodes_sum += int(r["nodes"].sum()); nodes_max = max(nodes_max, int(r["nodes"].max()))
                    budget += int(((r["flags"] & BUDGET) != 0).sum()); differ += int(r["rec"][15])
                hip.hipFree(d_m); hip.hipFree(d_c)
                v, sl = r["verdict"][:, :ks], r["slot"][:, :ks]
                new = v == S.ASSOC_NEW
                where = M0[:, None] + np.cumsum(new, axis=1) - 1              # the slot a NEW detection's landmark takes
                b_i, l_i = np.nonzero(new)
                first[b_i, where[b_i, l_i]] = true_id[t][b_i, l_i]
                mt = v == S.ASSOC_MATCHED
                b_i, l_i = np.nonzero(mt)
                agree += int((first[b_i, sl[b_i, l_i]] == true_id[t][b_i, l_i]).sum()); matches += int(mt.sum())
                dropped += int(r["n_drop"].sum())
            e = np.hypot(*(f.poses()[:, :2] - truth[t, :, :2]).T)
            err_sum += float(e.mean())
        out = dict(pos_err_end=float(e.mean()), pos_err_end_max=float(e.max()), pos_err_mean=err_sum / T,
                   landmarks_created_mean=float(f.landmark_counts().mean()), flagged_instances=int((f.status() != 0).sum()))
        if kind != "true_ids":
            out.update(matches=matches, match_agreement=(agree / matches if matches else None), dropped=dropped)
        if kind == "joint":
            out.update(max_nodes=int(jcfg.max_nodes), nodes_mean=nodes_sum / (T * B), nodes_max=nodes_max, budget_share=budget / (T * B),
                       matches_not_individual_best=differ)
        f.close()
        hip.hipFree(d_lab); hip.hipFree(d_labc)
        return out
    res = {k: replay(k) for k in ("true_ids", "associated", "joint")}
    if res["joint"]["budget_share"] > 0.0:
        res["joint_4x_budget"] = replay("joint", 4 * res["joint"]["max_nodes"])
    out = dict(tool="gpu_associate_joint", part="effect", map=which, L=Lm, batch=B, ticks=T, detections=int(valid.sum()),
               first_tick_with_detections=first_det, landmarks_seen_mean=float(seen.mean()), replays=res)
    if which == "lattice":
        out.update(spacing=args.spacing, stretch=args.stretch, odo_scale=args.odo_scale)
    print(f"# map `{which}`: L = {Lm}, batch {B}, {T} ticks, {out['detections']} detections from tick {first_det}, "
          f"{out['landmarks_seen_mean']:.2f} landmarks seen per instance")
    for k, v in res.items():
        a = v.get("match_agreement")
        print(f"#   {k:16s} position error at the end {v['pos_err_end']:.4f} m (mean {v['pos_err_mean']:.4f}) | landmarks created "
              f"{v['landmarks_created_mean']:.2f} | agreement {'n/a' if a is None else format(a, '.4f')} | dropped {v.get('dropped', 0)}")
    print(json.dumps(out), flush=True)


def cost(S, name, L, B, f32, args, hip):
    from live_ekf_slam_amd.scenario import make_scenario
    T, ks, w = args.ticks, args.k_stride, args.warmup
    dt = S.F32 if f32 else S.F64
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11 = (v ** 2 / 3 for v in (cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11))
    sim_cfg = S.default_config(); sim_cfg.replicate_vw_quirk = 0
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    meas, cnt, _ = record_log(S, sim_cfg, lm, cmds, B, ks, dt, None, False)
    d_meas, d_cnt = _put(hip, meas), _put(hip, cnt)
    row_m, row_c = meas[0].nbytes, cnt[0].nbytes
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_seed(2025)

    def joint_route(n=T, series=False):
        f.init(0.0, 0.0, 0.0)
        res = f.associate_joint_run(cmds[:n], meas[:n], cnt[:n], series=series)
        return f.last_joint_work(), res

    def assoc_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.associate_run(cmds[:n], meas[:n], cnt[:n])
        return f.last_associate_work()

    def plain_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.sync()
        t0 = time.perf_counter()
        for t in range(n):
            f.update_dev(cmds[t], d_meas.value + t * row_m, d_cnt.value + t * row_c, ks)
        f.sync()
        return (time.perf_counter() - t0) * 1e3
    joint_route(w); assoc_route(w); plain_route(w)
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        a_ms.append(joint_route()[0][3])
        b_ms.append(assoc_route()[3])
        c_ms.append(plain_route())
    f.set_nav_timing(True)
    (by, lines, d_joint, d_total), res = joint_route(series=True)
    _, _, d_assoc, _ = assoc_route()
    f.set_nav_timing(False)
    f.close()
    hip.hipFree(d_meas); hip.hipFree(d_cnt)
    a, b, c = statistics.median(a_ms), statistics.median(b_ms), statistics.median(c_ms)
    print(json.dumps({
        "tool": "gpu_associate_joint", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T,
        "k_stride": ks, "reps": args.reps, "a_associate_joint_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "b_associate_run_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms],
        "c_plain_step_dev_loop_ms_per_tick": round(c / T, 4), "c_ms_all": [round(v, 2) for v in c_ms],
        "a_over_b": round(a / b, 4), "a_over_c": round(a / c, 4),
        "d_joint_launches_ms_per_tick": round(d_joint / T, 5), "d_assoc_launches_ms_per_tick": round(d_assoc / T, 5),
        "d_timed_joint_run_ms_per_tick": round(d_total / T, 4), "model_bytes_per_tick": by / T, "model_bytes_in_lines_per_tick": lines / T,
        "nodes_mean_per_instance_tick": float(res.nodes.mean()), "nodes_max": int(res.nodes.max()),
        "detections_per_instance_tick": float(res.recs[:, 3].sum() / max(res.recs[:, 0].sum(), 1.0)),
        "budget_share": float(((res.flags & BUDGET) != 0).mean()), "max_nodes": int(S.default_joint_config().max_nodes),
        "matched_per_tick": float(res.recs[:, 4].mean()), "new_per_tick": float(res.recs[:, 5].mean()),
        "unpaired_per_tick": float(res.recs[:, 9].mean())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--rows", type=int, default=6)
    ap.add_argument("--cols", type=int, default=8)
    ap.add_argument("--spacing", type=float, default=0.5)
    ap.add_argument("--stretch", type=float, default=8.0)
    ap.add_argument("--odo-scale", type=float, default=4.0)
    ap.add_argument("--effect-batch", type=int, default=256)
    ap.add_argument("--effect-ticks", type=int, default=300)
    ap.add_argument("--k-stride", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["effect", "lattice"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    hip = _hip()
    if args.only in (None, "effect", "lattice"):
        for which in ("lattice",) if args.only == "lattice" else ("lattice", "spread", "pairs"):
            effect(S, args, hip, which)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args, hip)


if __name__ == "__main__":
    main()
