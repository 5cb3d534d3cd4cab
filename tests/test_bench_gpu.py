"""bench.py end to end on the GPU box: the one-GPU line and the N > 1 control flow (two ranks sharing the one GPU of the box:
gloo rendezvous, shard plan, barrier-bracketed timing, the gather) - what the driver runs at round end."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    return port


def _last_json(out):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


def test_single_gpu_line_has_the_contract_fields():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2", "--batch", "4096",
                          "--full", "--no-long-runs", "--no-cpu-baseline"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
                "data", "config", "roofline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["dtype"] == "f64" and d["value"] > 1e6
    assert d["config"]["state_rmse_vs_oracle"] == 0.0 and d["config"]["instances_flagged"] == 0
    r = d["roofline"]
    # physical by construction: bytes the kernel counted on the device / launch duration / peak
    assert r["bound"] == "hbm" and 0.0 < r["frac"] <= 1.0 and r["traffic"] > 0 and r["peak"] == 8000.0
    assert abs(r["achieved"] - r["traffic"] / (r["kernel_ms"] * 1e-3) / 1e9) <= 0.01 * r["achieved"] + 0.1
    assert r["kernel"].startswith("ekf_step_kernel<103,") and ",true," in r["kernel"]   # the variant actually launched
    assert r["lds_bytes_per_workgroup"] > 0 and r["workgroups_per_cu"] >= 1 and r["cycles_per_workgroup_step_at_2p4GHz"] > 0
    assert 0.0 < r["passes_per_instance_step"] <= 1.0 and 1.0 <= r["updates_per_pass"] <= 4.0
    o = r["once_per_step"]
    assert o["launches"] == 5 and 0.0 < o["frac"] <= 1.0 and ",false," in o["kernel"] and o["traffic"] > 0
    # the once-per-step leg runs the SAME timesteps on a second handle: identical detections, physical (device-counted) fraction
    assert o["window_start"] == d["config"]["window_start"] and o["mean_detections_per_step"] == d["config"]["mean_detections_per_step"]
    assert abs(o["achieved"] - o["traffic"] / (o["kernel_ms"] * 1e-3) / 1e9) <= 0.01 * o["achieved"] + 0.1
    assert d["device_time"]["ms_max_over_ranks"] > 0 and d["device_time"]["value"] >= d["value"] * 0.99
    # the driver's record keeps the first 24 keys of config / roofline: the digest and the once-per-step scalars are inside them
    assert list(d["config"]).index("secondary_digest") == 1 and list(r).index("once_per_step_value") < 24
    assert r["once_per_step_frac"] == o["frac"] and r["once_per_step_value"] == o["value"]
    assert "secondary" not in d   # only the default headline configuration carries the secondary lines


def test_plain_run_prints_the_headline_only():
    """Without --full the default configuration times its K steps and prints the line: no oracle comparison, CPU baseline,
    once-per-step leg, long runs or secondary lines, while the roofline of the timed launch itself stays in the line."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "5", "--warmup", "2"],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert d["metric"].startswith("EKF predict-update steps/sec") and d["unit"] == "steps/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f64" and d["steps"] == 5 and d["warmup"] == 2 and d["n_gpus"] == 1 and d["value"] > 1e6
    assert abs(d["value"] - 65536 * 5 / (d["ms_per_step"] * 5e-3)) <= 1e-3 * d["value"]
    assert "secondary" not in d and "cpu_baseline" not in d
    c, r = d["config"], d["roofline"]
    assert c["parity_check"] is None and c["secondary_digest"] is None and "steady_state_long_run" not in c and "per_k_ms" not in c
    assert c["instances_flagged"] == 0 and c["batch_per_gpu"] == 65536
    assert r["once_per_step"] is None and 0.0 < r["frac"] <= 1.0 and r["launches"] == 1


def test_two_ranks_strong_scaling_on_one_gpu():
    env = dict(os.environ, BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--batch", "8192", "--full", "--no-long-runs", "--no-cpu-baseline"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    d = _last_json(out.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong"
    assert d["config"]["global_batch"] == 8192 and d["config"]["batch_per_gpu"] == 4096
    assert d["config"]["state_rmse_vs_oracle"] == 0.0 and d["config"]["instances_flagged"] == 0


def test_two_ranks_short_window_keeps_the_k_step_definition():
    """`value` is the K timed steps for every N (one definition for a scaling curve); the 1000-step steady-state launch is
    reported beside it (config.steady_state_value), and device_time carries the K steps without the host-side barrier latency."""
    env = dict(os.environ, BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--batch", "4096", "--full", "--no-cpu-baseline", "--no-once-per-step"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    d = _last_json(out.stdout)
    assert d["n_gpus"] == 2 and d["steps"] == 5
    assert "value_source" not in d["config"] and "k_step_window" not in d
    assert abs(d["value"] - 4096 * 5 / (d["ms_per_step"] * 5e-3)) <= 1e-3 * d["value"]          # value IS the K-step window
    assert d["config"]["steady_state_value"] == d["config"]["steady_state_long_run"]["value"] > 0
    assert d["device_time"]["value"] >= d["value"] * 0.99
    assert d["config"]["state_rmse_vs_oracle"] == 0.0


@pytest.mark.parametrize("flt,extra,metric", [
    ("ukf", ["--landmarks", "20", "--batch", "256", "--steps", "6", "--warmup", "2", "--preroll", "10"], "UKF"),
    ("pgs", ["--landmarks", "20", "--poses", "120", "--batch", "24", "--k-per-pose", "8", "--steps", "1", "--warmup", "1"], "pose-graph SLAM solves"),
    ("pgs", ["--iterative", "--landmarks", "20", "--poses", "60", "--batch", "12", "--k-per-pose", "8", "--warmup", "3"], "graph-ticks")])
def test_two_ranks_of_the_secondary_filters_on_one_gpu(flt, extra, metric):
    """`--filter ukf | pgs` under torch.distributed - weak scaling (per-GPU batch), rank r owns the global
    instances [r B, (r + 1) B) (slam / pgs_set_instance_offset), barrier-bracketed timing, the end-of-run gather of the error statistics;
    the in-run oracle check of rank 0's first and last instance is part of the line (global ids)."""
    env = dict(os.environ, BENCH_SHARE_GPU="1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--filter", flt, "--full", "--no-cpu-baseline"] + extra
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert out.returncode == 0, (out.stdout[-1500:], out.stderr[-1500:])
    d = _last_json(out.stdout)
    B = int(extra[extra.index("--batch") + 1])
    assert d["n_gpus"] == 2 and metric in d["metric"] and d["value"] > 0 and d["scaling"] == "weak"
    assert d["config"]["instances_global"] == 2 * B and d["config"]["instances_flagged"] == 0
    pc = d["config"]["parity_check"]
    assert pc["mismatch"] is None
    if flt == "ukf":
        assert pc["max_abs_diff"] == 0.0
    else:
        assert pc["lm_iteration_and_trial_counts_equal"] and pc["max_abs_diff_m"] < 1e-7


@pytest.mark.parametrize("flt,extra,metric", [
    ("ukf", ["--landmarks", "20", "--batch", "256", "--steps", "6", "--warmup", "2", "--preroll", "10"], "UKF"),
    ("pgs", ["--landmarks", "20", "--poses", "120", "--batch", "24", "--k-per-pose", "8", "--steps", "1", "--warmup", "1"], "pose-graph SLAM solves"),
    ("pgs", ["--iterative", "--landmarks", "20", "--poses", "60", "--batch", "12", "--k-per-pose", "8", "--warmup", "3"], "graph-ticks")])
def test_plain_runs_of_the_secondary_filters(flt, extra, metric):
    """`--filter ukf | pgs` without --full: the timed figure only - no oracle comparison, no CPU baseline, and for the one-time pose-graph
    solve no per-kernel-timed solve (its roofline comes with --full)."""
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--filter", flt] + extra,
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    assert metric in d["metric"] and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"] == "f64" and d["higher_is_better"] is True
    assert d["config"]["parity_check"] is None and "cpu_baseline" not in d and d["config"]["instances_flagged"] == 0
    if flt == "pgs" and "--iterative" not in extra:
        assert d["roofline"] is None and d["config"]["kernel_ms_per_solve"] is None and d["config"]["batch_256_value"] is None
    else:   # measured on the timed run itself
        assert d["roofline"]["peak"] == 78.6 and d["roofline"]["achieved"] >= 0.0


def test_two_ranks_over_rccl_on_one_gpu_or_the_reason_why_not():
    """the RCCL branch of bench.py (init_process_group("nccl"), the barrier-bracketed timing, the end-of-run
    all-gather / all-reduce of the error statistics) has only ever run with one rank.  Two ranks on GPU 0 over the nccl backend
    exercise it on a one-GPU box IF RCCL accepts two ranks per device; if it refuses (NCCL's duplicate-GPU check) the refusal itself
    is asserted, so that this test says which of the two happened instead of passing vacuously."""
    env = dict(os.environ, BENCH_SHARE_GPU="nccl", HSA_ENABLE_IPC_MODE_LEGACY="0", NCCL_DEBUG="WARN")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "5", "--warmup", "2",
           "--batch", "8192", "--full", "--no-long-runs", "--no-cpu-baseline", "--no-once-per-step"]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    if out.returncode == 0:
        d = _last_json(out.stdout)
        assert d["n_gpus"] == 2 and d["config"]["global_batch"] == 8192 and d["config"]["state_rmse_vs_oracle"] == 0.0
        return
    txt = (out.stdout + out.stderr)
    assert ("Duplicate GPU" in txt) or ("duplicate" in txt.lower()) or ("invalid usage" in txt.lower()), txt[-3000:]
    pytest.skip("RCCL refuses two ranks on one device (duplicate-GPU check): the nccl branch needs a multi-GPU node; "
                "the gloo path (test_two_ranks_strong_scaling_on_one_gpu) covers the control flow")


def test_dump_outputs_hold_the_state_after_exactly_k_timed_steps(tmp_path, oracle):
    """--dump-outputs writes what the timed path computed in its last step: the dumped state of a sampled instance and its true pose
    equal the oracle's after window_start + K timesteps, so --steps sets the timed steps and the dump is taken right behind them."""
    from live_ekf_slam_amd.scenario import make_scenario
    K, B, L, out_dir = 3, 4096, 50, tmp_path / "dump"
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "2", "--batch", str(B),
                          "--no-long-runs", "--no-cpu-baseline", "--no-once-per-step", "--no-parity-check", "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    d = _last_json(out.stdout)
    a = {p.stem: np.load(p) for p in out_dir.glob("*.npy")}
    assert {"instances", "pose", "truth", "landmark_count", "status", "avg_position_error", "state_instances", "state_x", "state_P"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values()) and sum(v.nbytes for v in a.values()) <= 64 << 20
    assert np.array_equal(a["instances"], np.arange(B)) and np.all(a["status"] == 0)
    T = d["config"]["window_start"] + K
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]
    for i in (0, a["state_instances"].size - 1):
        b = int(a["state_instances"][i])
        r = oracle.run_ekf_batch(lm, cmds, 1, L, seed=2025, inst0=b, mode=oracle.MODE_FAST, vision=vis)
        n = 3 + 2 * int(r["M"][0])
        assert np.array_equal(a["state_x"][i, :n], r["x"][0, :n]), f"instance {b}"
        assert np.array_equal(a["state_P"][i, :n, :n].ravel(), r["P"][0, :n * n]), f"instance {b}"
        assert np.array_equal(a["truth"][b], r["truth"][0]) and np.array_equal(a["pose"][b], r["x"][0, :3])
        assert a["avg_position_error"][b] == r["avg_err"][0] and a["landmark_count"][b] == r["M"][0]
