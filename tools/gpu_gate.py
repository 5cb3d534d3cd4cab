#!/usr/bin/env python3
"""The chi-square gate (slam_gate, slam_gate_run) on one MI355X: what it does to a log with range spikes, and what a gated tick costs.

Part 1, the effect.  The simulator draws its noise uniformly with the half-widths a = the config's V_00, V_11, W_00, W_11, so the filter
rows are set to the variances a^2 / 3 (replicate_vw_quirk = 0): with the reference configuration S >= 1 and a 1 m spike would have a NIS of
about 1 and pass any gate.  One SIM handle of --effect-batch instances at L = --landmarks runs --effect-ticks ticks of
make_scenario(321 + L, L, T), seed 2025, and its messages and true poses are recorded.  A seeded host generator (--seed) then adds
--spike metres to the range of a fraction --fraction of the detections.  Three host-fed handles replay the log: the clean one taken
plainly, the spiked one taken plainly, the spiked one gated (per tick slam_gate, whose verdicts are compared with the spike mask, then the
plain step on the filtered message - the gated step).  Printed: the mean position error against the recorded truth over all instances
and ticks of each, and the counts of rejected spikes, spikes not rejected (on update slots), and rejected clean detections.

Part 2, the cost.  Three configurations unless --only picks one: L = 50 x batch 65 536 in fp64 and in fp32 storage, L = 20 x batch 4096
fp64.  Per configuration a SIM handle records a log of --ticks ticks (stride --k-stride); then on ONE host-fed handle, re-initialised
before every run, after a warm-up of each route, --reps repetitions ALTERNATING
  (a) gate_run, records only: per tick the gate's three launches and the one-step launch; device time by HIP events (slam_last_gate_work);
  (b) innovation_run with the LOG source on the same log: per tick the innovation's three launches and the one-step launch; device time
      by HIP events (slam_last_innovation_work);
  (c) a plain slam_step_dev loop over the same log held on the device, host clock ending synchronised;
then (d) once each with an event pair around every tick's gate / innovation launches (set_nav_timing): their device time alone.
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

CONFIGS = {"L50_f64": (50, 65536, False), "L50_f32": (50, 65536, True), "L20_f64": (20, 4096, False)}


def consistent_rows(S, cfg, B):
    """filter variances = those of the simulator's uniform draws of half-width a: a^2 / 3"""
    from live_ekf_slam_amd.config import noise_rows
    return noise_rows(cfg, B, V_00=cfg.V_00 ** 2 / 3, V_11=cfg.V_11 ** 2 / 3, W_00=cfg.W_00 ** 2 / 3, W_11=cfg.W_11 ** 2 / 3)


def record_log(S, cfg, L, B, T, ks, dtype, rows, want_truth):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, T)
    f = S.BatchedEKF(B, L, dtype=dtype).readParams(cfg)
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
    return np.ascontiguousarray(cmds, dtype=np.float32), meas, np.minimum(cnt, ks), truth


def effect(S, args):
    L, B, T, ks = args.landmarks, args.effect_batch, args.effect_ticks, args.k_stride
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    rows = consistent_rows(S, cfg, B)
    cmds, meas, cnt, truth = record_log(S, cfg, L, B, T, ks, S.F64, rows, True)
    rng = np.random.default_rng(args.seed)
    valid = np.arange(ks)[None, None, :] < cnt[:, :, None]
    spike = valid & (rng.random((T, B, ks)) < args.fraction)
    spiked = meas.copy()
    spiked[:, :, :, 1] += np.where(spike, np.float32(args.spike), np.float32(0.0))

    def handle():
        f = S.BatchedEKF(B, L).readParams(cfg)
        f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_noise(rows)
        return f
    clean, plain, gated = handle(), handle(), handle()
    err = dict(clean=0.0, plain=0.0, gated=0.0)
    rej_spike = rej_clean = kept_spike = updates = 0
    for t in range(T):
        clean.update(cmds[t], meas[t], cnt[t])
        plain.update(cmds[t], spiked[t], cnt[t])
        g = gated.gate(cmds[t], spiked[t], cnt[t], det=False)
        gated.update(cmds[t], g["meas_out"], g["count_out"])
        v = g["verdict"][:, :ks]
        rej_spike += int(((v == S.GATE_REJECTED) & spike[t]).sum()); rej_clean += int(((v == S.GATE_REJECTED) & ~spike[t]).sum())
        kept_spike += int(((v == S.GATE_ACCEPTED) & spike[t]).sum()); updates += int((v != S.GATE_NOT_UPDATE).sum())
        for name, f in (("clean", clean), ("plain", plain), ("gated", gated)):
            err[name] += float(np.hypot(*(f.poses()[:, :2] - truth[t, :, :2]).T).mean())
    flagged = {name: int((f.status() != 0).sum()) for name, f in (("clean", clean), ("plain", plain), ("gated", gated))}
    for f in (clean, plain, gated):
        f.close()
    out = dict(tool="gpu_gate", part="effect", L=L, batch=B, ticks=T, seed=args.seed, spike_m=args.spike, fraction=args.fraction,
               gate=S.default_gate_config().gate, detections=int(valid.sum()), spiked=int(spike.sum()), update_slots=updates,
               mean_pos_err_clean=err["clean"] / T, mean_pos_err_spiked_plain=err["plain"] / T, mean_pos_err_spiked_gated=err["gated"] / T,
               rejected_spikes=rej_spike, accepted_spikes=kept_spike, rejected_clean=rej_clean, flagged=flagged)
    print(f"# EKF L = {L}, batch {B}, {T} ticks, filter noise a^2 / 3, {out['spiked']} of {out['detections']} detections spiked by {args.spike} m")
    print(f"# mean position error [m]: clean {out['mean_pos_err_clean']:.4f} | spiked, plain {out['mean_pos_err_spiked_plain']:.4f} | "
          f"spiked, gated {out['mean_pos_err_spiked_gated']:.4f}")
    print(f"# of {updates} update slots: rejected spikes {rej_spike}, accepted spikes {kept_spike}, rejected clean detections {rej_clean}")
    print(json.dumps(out), flush=True)


def cost(S, name, L, B, f32, args):
    T, ks, w = args.ticks, args.k_stride, args.warmup
    dt = S.F32 if f32 else S.F64
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11 = (v ** 2 / 3 for v in (cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11))   # (no rows: one config for the batch)
    sim_cfg = S.default_config(); sim_cfg.replicate_vw_quirk = 0
    cmds, meas, cnt, _ = record_log(S, sim_cfg, L, B, T, ks, dt, None, False)
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    d_meas, d_cnt = C.c_void_p(), C.c_void_p()
    assert hip.hipMalloc(C.byref(d_meas), meas.nbytes) == 0 and hip.hipMalloc(C.byref(d_cnt), cnt.nbytes) == 0
    assert hip.hipMemcpy(d_meas, meas.ctypes.data_as(C.c_void_p), meas.nbytes, 1) == 0
    assert hip.hipMemcpy(d_cnt, cnt.ctypes.data_as(C.c_void_p), cnt.nbytes, 1) == 0
    row_m, row_c = meas[0].nbytes, cnt[0].nbytes
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_seed(2025)

    def gate_route(n=T):
        f.init(0.0, 0.0, 0.0)
        res = f.gate_run(cmds[:n], meas[:n], cnt[:n])
        return f.last_gate_work(), res

    def innovation_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.innovation_run(cmds[:n], meas=meas[:n], meas_count=cnt[:n])
        return f.last_innovation_work()

    def plain_route(n=T):
        f.init(0.0, 0.0, 0.0)
        f.sync()
        t0 = time.perf_counter()
        for t in range(n):
            f.update_dev(cmds[t], d_meas.value + t * row_m, d_cnt.value + t * row_c, ks)
        f.sync()
        return (time.perf_counter() - t0) * 1e3
    gate_route(w); innovation_route(w); plain_route(w)
    a_ms, b_ms, c_ms = [], [], []
    for _ in range(args.reps):
        (_, total), res = gate_route()
        a_ms.append(total)
        b_ms.append(innovation_route()[1])
        c_ms.append(plain_route())
    f.set_nav_timing(True)
    (d_gate, d_gate_total), _ = gate_route()
    d_inn, d_inn_total = innovation_route()
    f.set_nav_timing(False)
    f.close()
    hip.hipFree(d_meas); hip.hipFree(d_cnt)
    a, b, c = statistics.median(a_ms), statistics.median(b_ms), statistics.median(c_ms)
    print(json.dumps({
        "tool": "gpu_gate", "part": "cost", "config": name, "L": L, "batch": B, "storage": "fp32" if f32 else "fp64", "ticks": T, "k_stride": ks,
        "reps": args.reps, "a_gate_run_ms_per_tick": round(a / T, 4), "a_ms_all": [round(v, 2) for v in a_ms],
        "b_innovation_run_log_ms_per_tick": round(b / T, 4), "b_ms_all": [round(v, 2) for v in b_ms],
        "c_plain_step_dev_loop_ms_per_tick": round(c / T, 4), "c_ms_all": [round(v, 2) for v in c_ms],
        "a_over_b": round(a / b, 4), "a_over_c": round(a / c, 4), "a_minus_b_ms_per_tick": round((a - b) / T, 5),
        "message_bytes_per_tick": B * ks * 12,
        "d_gate_launches_ms_per_tick": round(d_gate / T, 5), "d_innovation_launches_ms_per_tick": round(d_inn / T, 5),
        "d_timed_gate_run_ms_per_tick": round(d_gate_total / T, 4), "d_timed_innovation_run_ms_per_tick": round(d_inn_total / T, 4),
        "rejected_per_tick": float(res.recs[:, 15].mean()), "accepted_updates_per_tick": float(res.recs[:, 5].mean())}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--landmarks", type=int, default=50)
    ap.add_argument("--effect-batch", type=int, default=1024)
    ap.add_argument("--effect-ticks", type=int, default=300)
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--spike", type=float, default=1.0, help="metres added to the range of a spiked detection")
    ap.add_argument("--fraction", type=float, default=0.05, help="fraction of the detections that get a spike")
    ap.add_argument("--k-stride", type=int, default=16)
    ap.add_argument("--ticks", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", choices=sorted(CONFIGS) + ["effect"], default=None)
    args = ap.parse_args()
    import live_ekf_slam_amd as S
    if args.only in (None, "effect"):
        effect(S, args)
    for name, (L, B, f32) in CONFIGS.items():
        if args.only in (None, name):
            cost(S, name, L, B, f32, args)


if __name__ == "__main__":
    main()
