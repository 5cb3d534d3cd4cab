#!/usr/bin/env python3
"""Association of detections without ids (slam_associate, slam_step_associated_dev, slam_associate_run) on one MI355X: what it does to a
log whose ids are erased, and what an associated tick costs.

Part 1, the effect.  The simulator draws its noise uniformly with the half-widths a = the config's V_00, V_11, W_00, W_11, so the filter
rows are set to the variances a^2 / 3 (replicate_vw_quirk = 0), as tools/gpu_gate.py does.  One SIM handle of --effect-batch instances
runs --effect-ticks ticks and its messages WITH the true ids (slam_get_last_meas per tick) and true poses are recorded, on two maps: `spread`,
the L = --landmarks map of make_scenario(321 + L, L, T), and `pairs`, L / 2 of its landmarks each with a twin 0.6 m away.  The log is
replayed four ways on host-fed handles:
  1  true ids            the plain known-id step
  2  associated          ids erased; per tick slam_associate_dev (for the verdicts; it changes nothing), then slam_step_associated_dev
  3  reference rule      ids erased; a handle with landmark_id_is_known = 0 (ekf.cpp:82-98: the box test on positions inside the step)
  4  associated, gated   ids erased; slam_associate_dev into a device buffer, then slam_step_gated_dev on it
Printed per replay: the mean position error against the recorded truth over all instances and ticks, the landmarks created per instance
against the landmarks truly seen, and (2 and 4) the share of MATCHED detections whose landmark is the one the true id says, through the
first-insertion mapping (slot of a NEW detection -> its true id).

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration a SIM handle records a log of --ticks ticks (stride --k-stride); then on ONE host-fed handle, re-initialised
before every run, after a warm-up of each route, --reps repetitions ALTERNATING
  (a) associate_run, records only: per tick the association's three launches and the one-step launch; device time by HIP events;
  (b) gate_run on the same log (with its ids): per tick the gate's three launches and the one-step launch; device time by HIP events;
  (c) a plain slam_step_dev loop over the same log (with its ids) held on the device, host clock ending synchronised;
then (d) once with an event pair around every tick's association launches (set_nav_timing): their device time alone, and the traffic
model of slam_last_associate_work.  No time is fixed in advance: the yardstick is the plain loop (c) of the same run.
Medians; one JSON line per part and configuration."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tools.gpu_gate import consistent_rows  # noqa: E402

CONFIGS = {"L50_f64": (50, 65536, False), "L50_f32": (50, 65536, True), "L20_f64": (20, 4096, False)}


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    return hip


def _put(hip, a):
    p = C.c_void_p()
    assert hip.hipMalloc(C.byref(p), max(a.nbytes, 16)) == 0
    assert hip.hipMemcpy(p, a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0
    return p


def record_log(S, cfg, lm, cmds, B, ks, dtype, rows, want_truth):
    T = cmds.shape[0]
    f = S.BatchedEKF(B, lm.shape[0], dtype=dtype).readParams(cfg)
    f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0)
    if rows is not None:
        f.set_noise(rows)
    f.last_meas(ks)                                  # (switches the measurement dump on)
    meas, cnt = np.zeros((T, B, ks, 3), np.float32), np.zeros((T, B), np.int32)
    truth = np.zeros((T, B, 3)) if want_truth else None
    for t in range(T):
        f.update_sim(cmds[t])
        meas[t], cnt[t] = f.last_meas(ks)
        if want_truth:
            truth[t] = f.truth()
    f.close()
    cnt = np.minimum(cnt, ks)
    meas[~(np.arange(ks)[None, None, :] < cnt[:, :, None])] = 0.0   # (the dump leaves the slots beyond the count as they were)
    return meas, cnt, truth


def effect(S, args, hip, which):
    from live_ekf_slam_amd.scenario import make_scenario
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    lm, cmds = make_scenario(321 + L, L, T)
    if which == "pairs":
        lm = np.concatenate([lm[:L // 2], lm[:L // 2] + np.array([0.6, 0.0])])
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    meas, cnt, truth = record_log(S, cfg, lm, cmds, B, ks, S.F64, rows, True)
    valid = np.arange(ks)[None, None, :] < cnt[:, :, None]
    true_id = np.where(valid, meas[:, :, :, 0], -1).astype(np.int64)
    erased = meas.copy(); erased[:, :, :, 0] = np.nan
    seen = np.array([np.unique(true_id[:, b][true_id[:, b] >= 0]).size for b in range(B)])
    Lm = lm.shape[0]

    def handle(known=1):
        c = S.default_config(); c.replicate_vw_quirk = 0; c.landmark_id_is_known = known
        f = S.BatchedEKF(B, Lm).readParams(c)
        f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        return f
    names = ("true_ids", "associated", "reference_rule", "associated_gated")
    hs = dict(true_ids=handle(), associated=handle(), reference_rule=handle(0), associated_gated=handle())
    err = {n: 0.0 for n in names}
    agree = {n: [0, 0] for n in ("associated", "associated_gated")}      # [matches that agree, matches]
    first = {n: np.full((B, Lm), -1, np.int64) for n in agree}            # slot -> true id of the detection that created it
    verdicts = {n: np.zeros(7, np.int64) for n in agree}
    d_lab, d_labc = _put(hip, np.zeros_like(erased[0])), _put(hip, np.zeros_like(cnt[0]))
    for t in range(T):
        hs["true_ids"].update(cmds[t], meas[t], cnt[t])
        hs["reference_rule"].update(cmds[t], erased[t], cnt[t])
        d_m, d_c = _put(hip, erased[t]), _put(hip, cnt[t])
        for n in agree:
            f = hs[n]
            M0 = f.landmark_counts()
            r = f.associate_dev(cmds[t], d_m.value, d_c.value, ks, d_lab.value, d_labc.value, det=False)
            if n == "associated":
                f.step_associated_dev(cmds[t], d_m.value, d_c.value, ks, stats=False)
            else:
                f.step_gated_dev(cmds[t], d_lab.value, d_labc.value, ks, stats=False)
            v, sl = r["verdict"][:, :ks], r["slot"][:, :ks]
            verdicts[n] += np.bincount(v[valid[t]].ravel(), minlength=7)[:7]
            new = v == S.ASSOC_NEW
            where = M0[:, None] + np.cumsum(new, axis=1) - 1              # the slot a NEW detection's landmark takes
            b_i, l_i = np.nonzero(new)
            first[n][b_i, where[b_i, l_i]] = true_id[t][b_i, l_i]
            mt = v == S.ASSOC_MATCHED
            b_i, l_i = np.nonzero(mt)
            agree[n][0] += int((first[n][b_i, sl[b_i, l_i]] == true_id[t][b_i, l_i]).sum()); agree[n][1] += int(mt.sum())
        hip.hipFree(d_m); hip.hipFree(d_c)
        for n in names:
            err[n] += float(np.hypot(*(hs[n].poses()[:, :2] - truth[t, :, :2]).T).mean())
    created = {n: float(hs[n].landmark_counts().mean()) for n in names}
    flagged = {n: int((hs[n].status() != 0).sum()) for n in names}
    for f in hs.values():
        f.close()
    hip.hipFree(d_lab); hip.hipFree(d_labc)
    out = dict(tool="gpu_associate", part="effect", map=which, L=Lm, batch=B, ticks=T, detections=int(valid.sum()),
               landmarks_seen_mean=float(seen.mean()), mean_pos_err={n: err[n] / T for n in names}, landmarks_created_mean=created,
               match_agreement={n: (agree[n][0] / agree[n][1] if agree[n][1] else None) for n in agree}, matches={n: agree[n][1] for n in agree},
               verdicts={n: verdicts[n].tolist() for n in agree}, flagged=flagged,
               gate_match=S.default_assoc_config().gate_match, gate_new=S.default_assoc_config().gate_new)
    print(f"# map `{which}`: EKF L = {Lm}, batch {B}, {T} ticks, filter noise a^2 / 3, {out['detections']} detections, "
          f"{out['landmarks_seen_mean']:.2f} landmarks seen per instance")
    for n in names:
        a = out["match_agreement"].get(n)
        print(f"#   {n:17s} mean position error {out['mean_pos_err'][n]:.4f} m | landmarks created {created[n]:.2f} | "
              f"matches that agree with the true id {'n/a' if a is None else format(a, '.4f')} | flagged instances {flagged[n]}")
    print(json.dumps(out), flush=True)


def cost(S, name, L, B, f32, args, hip):
    from live_ekf_slam_amd.scenario import make_scenario
    T, ks, w = args.ticks, args.k_stride, args.warmup
    dt = S.F32 if f32 else S.F64
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11 = (v ** 2 / 3 for v in (cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11))   # (no rows: one config for the batch)
    sim_cfg = S.default_config(); sim_cfg.replicate_vw_quirk = 0
    lm, cmds = make_scenario(321 + L, L, T)
    cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    meas, cnt, _ = record_log(S, sim_cfg, lm, cmds, B, ks, dt, None, False)
    d_meas, d_cnt = _put(hip, meas), _put(hip, cnt)
    row_m, row_c = meas[0].nbytes, cnt[0].nbytes
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_seed(2025)

    def assoc_route(n=T):
        f.init(0.0, 0.0, 0.0)
        res = f.associate_run(cmds[:n], meas[:n], cnt[:n])
        return f.last_associate_work(), res

    def gate_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.gate_run(cmds[:n], meas[:n], cnt[:n])
        return f.last_gate_work()

    def plain_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.sync()
        t0 = time.perf_counter()
        for t in range(n):
            f.update_dev(cmds[t], d_meas.value + t * row_m, d_cnt.value + t * row_c, ks)
        f.sync()
        return (time.perf_counter() - t0) * 1e3
    assoc_route(w); gate_route(w); plain_route(w)
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        work, res = assoc_route()
        a_ms.append(work[3])
        b_ms.append(gate_route()[1])
        c_ms.append(plain_route())
    f.set_nav_timing(True)
    (by, lines, d_assoc, d_total), _ = assoc_route()
    f.set_nav_timing(False)
    f.close()
    hip.hipFree(d_meas); hip.hipFree(d_cnt)
    a, b, c = statistics.median(a_ms), statistics.median(b_ms), statistics.median(c_ms)
    print(json.dumps({
        "tool": "gpu_associate", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T,
        "k_stride": ks, "reps": args.reps, "a_associate_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "b_gate_run_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms],
        "c_plain_step_dev_loop_ms_per_tick": round(c / T, 4), "c_ms_all": [round(v, 2) for v in c_ms],
        "a_over_b": round(a / b, 4), "a_over_c": round(a / c, 4),
        "d_assoc_launches_ms_per_tick": round(d_assoc / T, 5), "d_timed_associate_run_ms_per_tick": round(d_total / T, 4),
        "model_bytes_per_tick": by / T, "model_bytes_in_lines_per_tick": lines / T,
        "model_GBps_of_the_assoc_launches": round(by / (d_assoc * 1e-3) / 1e9, 1) if d_assoc > 0 else None,
        "matched_per_tick": float(res.recs[:, 4].mean()), "new_per_tick": float(res.recs[:, 5].mean()),
        "dropped_per_tick": float(res.recs[:, [6, 9, 10, 11]].sum(axis=1).mean())}), flush=True)


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
        for which in ("spread", "pairs"):
            effect(S, args, hip, which)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args, hip)


if __name__ == "__main__":
    main()
