#!/usr/bin/env python3
"""The map score (slam_map_score) on one MI355X: what the id-less robustness stack leaves in the map, scored over the WHOLE batch on the
device, and what the call costs.

Part a, the sweep of tools/gpu_sense.py.  ONE handle at L = --landmarks, batch --effect-batch, capacity 2 L: 16 groups of instances (b % 16)
over the grid of p_spike x clutter rate, ids erased and shuffled.  Replayed with associate_run_sim and with manage_merge_run_sim, then scored
with match_radius --radius and full = 1.  Per group: MATCHED / DUPLICATE / SPURIOUS slots per instance, the map RMS, the mean lm_nees of the
MATCHED slots (2 for a consistent filter) and the mean nees_matched / dof_matched (1 for a consistent filter).
Part b, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and fp32 storage, L = 20 x batch 4096 fp64.
On ONE handle and state (a plain run_sim of --steps timesteps), after a warm-up call each, --reps repetitions of the call with full = 0 and
with full = 1 and of slam_consistency: the device ms of slam_last_score_work / slam_last_consistency_work (HIP events around the launches)
and the model's bytes.  Beside them the route without the call - per instance get_state (a copy of the whole P) and an argmin over the true
map in numpy, as tools/gpu_sense.py::agreement does - measured on --host-sample instances and scaled to the batch.  No time is fixed in
advance.  Medians; one JSON line per part and configuration.

The package has no mirror method for the call yet: the tool goes through the ctypes helpers of tests/score_reference.py."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_reference as R  # noqa: E402
from tools.gpu_associate import CONFIGS  # noqa: E402
from tools.gpu_gate import consistent_rows  # noqa: E402
from tools.gpu_sense import P_CLUTTER, P_SPIKE, _handle, grid_rows  # noqa: E402


def sweep(S, args):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config(); cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    group = np.arange(B) % 16
    out = dict(tool="gpu_map_score", part="sweep", L=L, capacity=2 * L, batch=B, ticks=T, k_stride=ks, match_radius=args.radius, p_spike=P_SPIKE,
               p_clutter=P_CLUTTER)
    for name in ("associate_run_sim", "manage_merge_run_sim"):
        f = _handle(S, cfg, lm, B, 2 * L, rows, grid_rows(S, B))
        getattr(f, name)(cmds, series=False, log=False, k_stride=ks)
        d = R.device_score(f, R.config(args.radius, full=1))
        by, ms = R.last_score_work(f)
        f.close()
        ok = (d["flags"] & R.INSTANCE_FAILED) == 0
        table = []
        for g in range(16):
            m = (group == g) & ok
            matched = d["role"][m] == R.MATCHED
            q = d["lm_nees"][m][matched]
            fin = m & np.isfinite(d["nees_matched"])
            table.append(dict(p_spike=P_SPIKE[g // 4], p_clutter=P_CLUTTER[g % 4], matched=float(d["n_matched"][m].mean()),
                              duplicate=float(d["n_duplicate"][m].mean()), spurious=float(d["n_spurious"][m].mean()),
                              map_rms=float(d["map_rms"][m].mean()), mean_lm_nees=float(np.nanmean(q)) if q.size else None,
                              nees_matched_per_dof=float((d["nees_matched"][fin] / d["dof_matched"][fin]).mean()) if fin.any() else None,
                              failed=int(((group == g) & ~ok).sum())))
            r = table[-1]
            print(f"#   {name:22s} p_spike {r['p_spike']:.2f} p_clutter {r['p_clutter']:.2f} | per instance matched {r['matched']:.2f} duplicate "
                  f"{r['duplicate']:.2f} spurious {r['spurious']:.2f} | map rms {r['map_rms']:.4f} m | mean lm_nees {r['mean_lm_nees']} | "
                  f"nees_matched / dof {r['nees_matched_per_dof']}")
        out[name] = dict(groups=table, record=[float(v) for v in d["rec"]], device_ms=round(ms, 3), model_bytes=by)
    print(json.dumps(out), flush=True)


def host_route(f, lm, count):
    """What a caller did without the call, per instance: get_state (a synchronise and a copy of the whole P), the distances to the true map and
    an argmin in numpy, the roles by a sort.  Seconds per instance."""
    t0 = time.perf_counter()
    for b in range(count):
        s = f.get_state(b)
        if s["M"] == 0:
            continue
        est = s["x"][3:].reshape(-1, 2)
        d2 = ((est[:, None, :] - lm[None]) ** 2).sum(axis=2)
        row = np.argmin(d2, axis=1)
        best = d2[np.arange(s["M"]), row]
        order = np.lexsort((np.arange(s["M"]), best, row))
        first = np.ones(s["M"], bool); first[1:] = row[order][1:] != row[order][:-1]
        float(np.sqrt(best[order][first].mean()))
    return (time.perf_counter() - t0) / count


def cost(S, name, L, B, f32, args):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, args.steps)
    f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams()
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds); f.sync()
    out = {"tool": "gpu_map_score", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "steps": args.steps,
           "reps": args.reps}
    for label, full in (("full0", 0), ("full1", 1)):
        cfg = R.config(args.radius, full=full)
        R.device_score(f, cfg, want=("rec",))               # warm-up (first-call allocations, code object)
        dev, wall = [], []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            d = R.device_score(f, cfg, want=("rec",))
            wall.append((time.perf_counter() - t0) * 1e3)
            by, ms = R.last_score_work(f)
            dev.append(ms)
        out[label] = dict(device_ms=round(statistics.median(dev), 4), device_ms_all=[round(v, 4) for v in dev],
                          call_ms_record_only=round(statistics.median(wall), 3), model_bytes=by,
                          model_GBps=round(by / (statistics.median(dev) * 1e-3) / 1e9, 1), record=[float(v) for v in d["rec"]])
    f.consistency()
    cons = []
    for _ in range(args.reps):
        f.consistency()
        cons.append(f.last_consistency_work()[1])
    out["slam_consistency_device_ms"] = round(statistics.median(cons), 4)
    out["slam_consistency_device_ms_all"] = [round(v, 4) for v in cons]
    per = host_route(f, lm, min(B, args.host_sample))
    out["host_route_ms_scaled_to_batch"] = round(per * B * 1e3, 1)
    out["host_route_sample"] = min(B, args.host_sample)
    f.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--effect-batch", type=int, default=65536)
    ap.add_argument("--effect-ticks", type=int, default=200)
    ap.add_argument("--k-stride", type=int, default=16)
    ap.add_argument("--radius", type=float, default=0.5, help="match_radius in metres")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=256)
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
