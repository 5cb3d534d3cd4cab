"""Every instance of the benchmarked EKF batch (65 536 instances, L = 50, one 60-step run_sim launch, fp64 and fp32 storage).

The multi-step launch defers rank-2 updates through an LDS ring shared by control and streamer wavefronts and schedules 64 rounds of
1 024 resident workgroups; a race or round-boundary bug there could corrupt one instance in ten thousand.  So the K-step launch is
compared with the once-per-step path on all 65 536 instances, the oracle on 256 random instances that include the workgroup-round
and shard edges, and a shard at an offset on all of its 8 192 instances, each bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from batch_state import ckpt_layout, describe, differing_instances, state_diff

pytestmark = pytest.mark.gpu

L, B, T = 50, 65536, 61
EDGES = (0, 1023, 1024, 32767, 32768, 65535)    # the first and last instance of workgroup rounds and of the 8-way shards
SHARD0, SHARD_B = 32768, 8192
PERTURBED = 40000


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _scenario():
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]
    return lm, cmds, vis


def _handle(S, dt, lm, batch=B, offset=0):
    f = S.BatchedEKF(batch, L, dtype=dt).readParams(); f.set_map(lm); f.set_seed(2025); f.set_instance_offset(offset); f.init(0, 0, 0)
    return f


def _k_step(S, dt, lm, cmds, vis, batch=B, offset=0):
    """Step 0 on its own, then steps 1..60 in ONE multi-step launch: bench.py's timed path."""
    f = _handle(S, dt, lm, batch, offset)
    f.set_vision(*vis[0]); f.update_sim(cmds[0]); f.set_vision(*vis[1])
    f.run_sim(cmds[1:T])
    return f


def _per_step(S, dt, lm, cmds, vis):
    f = _handle(S, dt, lm)
    for t in range(T):
        f.set_vision(*vis[t]); f.update_sim(cmds[t])
    return f


@pytest.mark.parametrize("dtype", ["f64", "f32"])
def test_every_instance_of_the_benchmarked_ekf_batch(S, oracle, dtype, tmp_path):
    lm, cmds, vis = _scenario()
    dt = S.F32 if dtype == "f32" else S.F64
    f1 = _k_step(S, dt, lm, cmds, vis)
    f2 = _per_step(S, dt, lm, cmds, vis)
    assert np.all(f1.landmark_counts() == L) and not f1.status().any()

    # (i) the K-step launch against the once-per-step path, every instance
    diffs = differing_instances(f1, f2)
    assert not diffs, "run_sim vs update_sim: " + describe(diffs)

    # (ii) the oracle on 256 random instances, the round and shard edges among them
    picks = np.unique(np.concatenate([EDGES, np.random.default_rng(20261015).choice(B, 256 - len(EDGES), replace=False)]))
    assert len(picks) >= 250 and set(EDGES) <= set(picks.tolist())
    mode = oracle.MODE_FAST | (oracle.STORAGE_F32 if dtype == "f32" else 0)
    truth, err = f1.truth(), f1.error_stats()

    def ref(b):
        return b, oracle.run_ekf_batch(lm, cmds, 1, L, seed=2025, inst0=int(b), vision=vis, mode=mode)
    bad = []
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for b, r in pool.map(ref, picks):
            n = 3 + 2 * int(r["M"][0])
            so = dict(M=int(r["M"][0]), ids=r["ids"][0, :r["M"][0]], x=r["x"][0, :n], P=r["P"][0, :n * n].reshape(n, n), timestep=T)
            d = state_diff(f1.get_state(int(b)), so)
            if d is None and not (err[b] == r["avg_err"][0] and np.array_equal(truth[b], r["truth"][0]) and r["flags"][0] == 0):
                d = max(abs(err[b] - r["avg_err"][0]), np.abs(truth[b] - r["truth"][0]).max(), 5e-324)
            if d is not None:
                bad.append((int(b), d))
    assert not bad, "GPU vs oracle: " + describe(bad)

    # (iv) the comparator has teeth: one P entry of one instance one ulp off in a checkpoint of the per-step handle (fp32 only: the
    # checkpoint holds the whole batch, 2.8 GB in fp32 and twice that in fp64; the comparator is the same code for both)
    if dtype == "f32":
        path = tmp_path / "per_step.ckpt"
        f2.save_state(path)
        head, off, hd = ckpt_layout(path)
        assert hd["B"] == B and hd["esz"] == 4
        ram = np.memmap(path, dtype=np.float32, mode="r+", offset=off["P"][0], shape=(B * hd["pstride"],))
        i0 = PERTURBED * hd["pstride"] + 0          # P(0, 0) of the instance: the slab starts with row 0
        ram[i0] = np.nextafter(ram[i0], np.float32(np.inf))
        ram.flush(); del ram
        f3 = _handle(S, dt, lm); f3.load_state(path)
        os.remove(path)
        diffs = differing_instances(f3, f2)
        assert [i for i, _ in diffs] == [PERTURBED], describe(diffs)
        assert 0 < diffs[0][1] <= 2.0 ** -20 * abs(f2.get_state(PERTURBED)["P"][0, 0]), diffs
        f3.close()
    f2.close()

    # (iii) an 8 192-instance shard at a global offset, every instance against the big run
    g = _k_step(S, dt, lm, cmds, vis, SHARD_B, SHARD0)
    diffs = differing_instances(g, f1, b_offset=SHARD0)
    assert not diffs, f"shard at {SHARD0} vs the full batch: " + describe(diffs, base=SHARD0)
    g.close()
    f1.close()
