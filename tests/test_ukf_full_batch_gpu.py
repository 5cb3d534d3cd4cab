"""The UKF at its benchmark batch (bench.py --filter ukf: B = 4 096, L = 20 and L = 50).  At that size ukf_sqrt_kernel<44,256> and the
step kernel run six workgroups per CU (SLAM_UKF_SQRT_WG, SLAM_UKF_STEP_WG), occupancy and scheduling conditions the small-batch parity
tests never reach.  The bench scenario - one wide look, a 40-step preroll and a 90-step run_sim window - is compared on every instance
with the same steps taken one update_sim at a time, and on random instances with the oracle, bit for bit."""
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

from batch_state import describe, differing_instances, state_diff

pytestmark = pytest.mark.gpu

B, T, PRE = 4096, 131, 40
# Oracle instances per L, sized from its measured cost over the 131 steps on 8 cores: 256 instances in 5.2 s at L = 20, 96 in 21.7 s
# at L = 50 (at least 32 each, 0 and 4 095 always among them).
ORACLE_SAMPLES = {20: 256, 50: 96}


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _scenario(L):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(1234, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]
    return lm, cmds, vis


def _pair(S, L, mode):
    """The bench's launches (step 0, a preroll launch, the window launch) and the same steps one update_sim at a time."""
    lm, cmds, vis = _scenario(L)
    hs = []
    for _ in range(2):
        f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(2025); f.init(0.0, 0.0, 0.0); f.set_sqrt_mode(mode)
        hs.append(f)
    a, b = hs
    a.set_vision(*vis[0]); a.update_sim(cmds[0]); a.set_vision(*vis[1])
    a.run_sim(cmds[1:1 + PRE]); a.run_sim(cmds[1 + PRE:])
    for t in range(T):
        b.set_vision(*vis[t]); b.update_sim(cmds[t])
    return a, b, lm, cmds, vis


@pytest.mark.parametrize("L", [20, 50])
def test_every_instance_of_the_benchmarked_ukf_batch(S, oracle, L):
    """Every instance: run_sim against update_sim.  The oracle on 256 random instances at L = 20 (5.2 s on 8 cores) and 96 at L = 50
    (21.7 s on 8 cores), 0 and 4 095 among them.  No instance flagged, one eigen-decomposition per instance-step."""
    a, b, lm, cmds, vis = _pair(S, L, "eigen")
    assert not a.status().any() and not b.status().any(), (np.flatnonzero(a.status())[:20], np.flatnonzero(b.status())[:20])
    assert int(a.sweep_stats()[1]) == B * T and int(b.sweep_stats()[1]) == B * T
    diffs = differing_instances(a, b)
    assert not diffs, "run_sim vs update_sim: " + describe(diffs)
    b.close()

    picks = np.unique(np.concatenate([[0, B - 1], np.random.default_rng(4096 + L).choice(B, ORACLE_SAMPLES[L] - 2, replace=False)]))
    assert len(picks) >= 32 and {0, B - 1} <= set(picks.tolist())
    truth, err = a.truth(), a.error_stats()

    def ref(i):
        return i, oracle.run_ukf_batch(lm, cmds, 1, L, seed=2025, inst0=int(i), vision=vis)
    bad = []
    with ThreadPoolExecutor(max_workers=min(8, os.cpu_count() or 1)) as pool:
        for i, r in pool.map(ref, picks):
            n = 4 + 2 * int(r["M"][0])
            so = dict(M=int(r["M"][0]), ids=r["ids"][0, :r["M"][0]], x=r["x"][0, :n], P=r["P"][0, :n * n].reshape(n, n), timestep=T)
            d = state_diff(a.get_state(int(i)), so)
            if d is None and not (err[i] == r["avg_err"][0] and np.array_equal(truth[i], r["truth"][0]) and r["flags"][0] == 0):
                d = max(abs(err[i] - r["avg_err"][0]), np.abs(truth[i] - r["truth"][0]).max(), 5e-324)
            if d is not None:
                bad.append((int(i), d))
    assert not bad, f"GPU vs oracle at L = {L}: " + describe(bad)
    a.close()


def test_cholesky_mode_at_the_benchmark_batch(S):
    """Cholesky mode (L = 20, where some instance-steps factor): run_sim and update_sim bit-identical on every instance, every
    instance-step counted once as a factorisation or a fallback, nothing flagged."""
    a, b, *_ = _pair(S, 20, "cholesky")
    assert not a.status().any() and not b.status().any()
    sa, sb = a.sqrt_stats(), b.sqrt_stats()
    assert int(sa.sum()) == B * T and sa.tolist() == sb.tolist() and int(sa[0]) > 0, (sa, sb)
    diffs = differing_instances(a, b)
    assert not diffs, "run_sim vs update_sim in Cholesky mode: " + describe(diffs)
    a.close(); b.close()
