#!/usr/bin/env python3
"""Robust loss on the pose graph's landmark factors (pgs_set_robust) on one MI355X: what it does to a log with wrong associations, and
what a solve with it costs.

The log.  One SIM handle (BatchedEKF) of --batch instances at L = --landmarks runs --poses - 1 ticks of make_scenario(321 + L, L, T), seed
2025; its messages and true poses are recorded, the secondary filter is the NaiveFilter (dead reckoning, the same for every instance).
A seeded host generator (--seed) then gives a share --fraction (default 5 %) of the NON-FIRST detections - a landmark's first detection
initialises it and stays clean - the range and bearing of ANOTHER landmark's detection in the same message: a wrong association.

Four host-fed BatchedPoseGraph handles replay logs through update(): the clean log with no loss, the corrupted log with no loss, with Huber
(--huber-k) and with Geman-McClure (--gm-k).  Printed per handle: the mean over instances of the average position error of the initial
estimate and of the result (pgs_error_stats' formula - compute_average_error of the pose-graph plot - evaluated on the host against the
recorded true poses: a host-fed handle holds no truth of its own), LM iterations and trials, the share of corrupted factors with
factor_weights(1) < 0.5 and the share of clean ones at or above it, milliseconds per solve (median of --reps, host clock around
solvePoseGraph + sync), and the linearize / evaluate entries of pgs_last_solve_kernel_ms of one profiled solve.  One JSON line each."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def record_log(S, L, B, T, ks):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, T)
    f = S.BatchedEKF(B, L).readParams()
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    f.last_meas(ks)                                  # (switches the measurement dump on)
    meas, cnt, truth = np.zeros((T, B, ks, 3), np.float32), np.zeros((T, B), np.int32), np.zeros((T, B, 3))
    for t in range(T):
        f.update_sim(cmds[t])
        meas[t], cnt[t] = f.last_meas(ks)
        truth[t] = f.truth()
    f.close()
    return np.ascontiguousarray(cmds, dtype=np.float32), meas, np.minimum(cnt, ks), truth


def corrupt(meas, cnt, fraction, seed):
    """(corrupted copy, mask [T][B][ks]): the chosen non-first detections take range and bearing of another detection of their message."""
    T, B, ks, _ = meas.shape
    rng = np.random.default_rng(seed)
    out, bad = meas.copy(), np.zeros((T, B, ks), dtype=bool)
    for b in range(B):
        seen = set()
        for t in range(T):
            n = int(cnt[t, b])
            ids = [int(meas[t, b, s, 0]) for s in range(n)]
            for s in range(n):
                if ids[s] not in seen:
                    seen.add(ids[s])
                    continue
                others = [q for q in range(n) if ids[q] != ids[s]]
                if others and rng.random() < fraction:
                    q = others[int(rng.integers(len(others)))]
                    out[t, b, s, 1:] = meas[t, b, q, 1:]
                    bad[t, b, s] = True
    return out, bad


def avg_error(poses, truth):
    """pgs_error_stats' formula: pose i (float32 on the wire) against the true pose after step i + 1, i < timestep."""
    ts = poses.shape[0] - 1
    d = poses[:ts, :2].astype(np.float32).astype(np.float64) - truth[:ts, :2]
    return float(np.sqrt((d * d).sum(axis=1)).mean()) if ts else 0.0


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--poses", type=int, default=200)
    ap.add_argument("--landmarks", type=int, default=20)
    ap.add_argument("--k-per-pose", type=int, default=8)
    ap.add_argument("--fraction", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--huber-k", type=float, default=1.345)
    ap.add_argument("--gm-k", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.pose_graph import NaiveFilter, LOSS_NONE, LOSS_HUBER, LOSS_GEMAN_MCCLURE
    B, N, L, ks = args.batch, args.poses, args.landmarks, args.k_per_pose
    T = N - 1
    cmds, meas, cnt, truth = record_log(S, L, B, T, ks)
    spoiled, bad = corrupt(meas, cnt, args.fraction, args.seed)
    nf = NaiveFilter(); nf.init(0.0, 0.0, 0.0)
    sec = np.zeros((T, 3))
    for t in range(T):
        nf.update(cmds[t]); sec[t] = nf.getStateVector()
    stored = np.arange(ks)[None, None, :] < cnt[:, :, None]
    print(json.dumps(dict(log=dict(batch=B, poses=N, landmarks=L, k_per_pose=ks, detections=int(stored.sum()), corrupted=int(bad.sum()),
                                   share_of_all=float(bad.sum() / max(stored.sum(), 1))))))
    runs = (("clean, no loss", meas, LOSS_NONE, 0.0), ("corrupted, no loss", spoiled, LOSS_NONE, 0.0),
            ("corrupted, Huber", spoiled, LOSS_HUBER, args.huber_k), ("corrupted, Geman-McClure", spoiled, LOSS_GEMAN_MCCLURE, args.gm_k))
    for name, log, kind, k in runs:
        pg = S.BatchedPoseGraph(B, num_iterations=N, L_max=L, k_per_pose=ks).readParams()
        pg.init(0.0, 0.0, 0.0)
        for t in range(T):
            pg.updateNaiveVehPoseEstimate(sec[t])
            pg.update(cmds[t], log[t], cnt[t])
        pg.set_robust(kind, k)
        pg.solvePoseGraph(); pg.sync()              # warm-up
        ms = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            pg.solvePoseGraph(); pg.sync()
            ms.append(1e3 * (time.perf_counter() - t0))
        st = pg.stats()
        e0 = np.mean([avg_error(pg.get_graph(b, 0)["poses"], truth[:, b]) for b in range(B)])
        e1 = np.mean([avg_error(pg.get_graph(b, 1)["poses"], truth[:, b]) for b in range(B)])
        w = pg.factor_weights(1)[:, 1:]             # [B][T][ks]: pose t + 1 holds the message of tick t
        wb, wc = w[np.swapaxes(bad, 0, 1)], w[np.swapaxes(stored & ~bad, 0, 1)]
        pg.set_profiling(True)
        pg.solvePoseGraph(); pg.sync()
        kms = pg.last_solve_kernel_ms()
        pg.close()
        print(json.dumps(dict(run=name, kind=kind, k=k, avg_err_initial_m=float(e0), avg_err_result_m=float(e1),
                              iterations_mean=float(st["iterations"].mean()), trials_mean=float(st["trials"].mean()), flagged=int((st["flags"] != 0).sum()),
                              corrupted_below_half=float((wb < 0.5).mean()) if wb.size else None, clean_at_or_above_half=float((wc >= 0.5).mean()) if wc.size else None,
                              solve_ms_median=statistics.median(ms), solve_ms_min=min(ms), profiled_linearize_ms=kms["linearize"], profiled_evaluate_ms=kms["evaluate"])))


if __name__ == "__main__":
    main()
