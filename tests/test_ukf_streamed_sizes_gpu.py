"""The HBM-streamed UKF class (ukf_big_kernel.hip: every handle of 51 to 200 landmarks) walked over its size edges against the CPU oracle.
Tolerance: ZERO, as everywhere the filters meet the oracle - flags, M, ids, x and P bit for bit.  The oracle's side of the
bargain - its unpadded circle schedule and the root it gives up to n = 404 - is pinned against LAPACK on the CPU (test_oracle_ukf.py,
test_jacobi_schedule.py).

What the LDS classes never run and this class always does: rr_pair over the indices themselves at every n = 2 (mod 4), also at SMALL n (a
streamed handle that holds few landmarks does not pad: the oracle chooses by L_max, not by n); the warm start's V0 extended by the identity
under a new leading dimension (n_v != n); the capacity, L = 200, n = 404; the cold restart after kUkfWarmMaxAge = 100 warm starts.  Every
test asserts from the device's own landmark_counts() that it reached the sizes it is about."""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L_CAP = 200                                   # kUkfMaxLandmarks
CAPACITY, NONFINITE, SQRT_FAILED = 8, 1, 16   # SLAM_INST_* (include/slam_batch.h)
FOREIGN_ID = 900


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def differing(sg, so):
    """The fields of two states (M, ids, x, P) that are not the same bits; the comparison of every test here."""
    bad = []
    if int(sg["M"]) != int(so["M"]): bad.append("M")
    if not np.array_equal(sg["ids"], so["ids"]): bad.append("ids")
    for k in ("x", "P"):
        if not np.array_equal(sg[k], so[k]): bad.append(k)      # (False for different shapes, too)
    return bad


def _worst(sg, so, k):
    return float(np.abs(sg[k] - so[k]).max()) if sg[k].shape == so[k].shape else "shapes %s %s" % (sg[k].shape, so[k].shape)


def _same(sg, so, what):
    bad = differing(sg, so)
    assert not bad, (what, bad, {k: _worst(sg, so, k) for k in bad if k in ("x", "P")})


# ---- 1. one handle of capacity 200, fifteen instances of fifteen sizes --------------------------------------------------------------------------
STARTS = [1, 2, 21, 49, 50, 51, 52, 53, 75, 100, 101, 150, 151, 197, 198]
STEPS = 5


def script(M0):
    """The five messages of the instance that starts with M0 landmarks, [k][3] float32 (id, range, bearing):
    0  ids 0 .. M0 - 1: M0 insertions from the empty state (cold decomposition at n = 4)
    1  twelve known ids (all of them below twelve) and the new id M0: updates with a warm root extended from n_v = 4 to n in one go, then
       one insertion - the parity of M flips
    2  six known ids: the warm root extended by two rows
    3  five known ids, the new id M0 + 1 and a foreign id: a pure warm start (n_v = n), then growth by two - or, with 199 landmarks held,
       by one and SLAM_INST_CAPACITY
    4  an empty message"""
    rng = np.random.default_rng(7000 + M0)
    def msg(ids):
        m = np.zeros((len(ids), 3), dtype=np.float32)
        m[:, 0] = ids; m[:, 1] = rng.uniform(0.5, 6.0, len(ids)); m[:, 2] = rng.uniform(-3.1, 3.1, len(ids))
        return m
    known = lambda M, k: rng.choice(M, min(k, M), replace=False)
    return [msg(np.arange(M0)),
            msg(np.append(known(M0, 12), M0)),
            msg(known(M0 + 1, 6)),
            msg(np.append(known(M0 + 1, 5), [M0 + 1, FOREIGN_ID])),
            msg(np.zeros(0))]


def commands():
    rng = np.random.default_rng(77)
    return np.stack([rng.uniform(0.0, 0.1, STEPS), rng.uniform(-0.05, 0.05, STEPS)], axis=1).astype(np.float32)


def walk_oracle(oracle, M0):
    """The script through one OracleUKF(L_max = 200): (flags OR-ed so far, state) after every step."""
    e = oracle.OracleUKF(L_max=L_CAP); e.init(0, 0, 0)
    out, fl = [], 0
    for cmd, m in zip(commands(), script(M0)):
        fl |= e.update(cmd[0], cmd[1], m)
        out.append((fl, e.state()))
    return out


def test_every_size_edge_of_the_streamed_class(S, oracle):
    """Instance b starts with its own landmark count; the instances sit side by side in one launch, so the batch mixes sizes and parities.
    Checked after EVERY step: an error that a later warm start heals must still show."""
    starts = STARTS
    B = len(starts)
    scripts = [script(M0) for M0 in starts]
    cmds = commands()
    with ThreadPoolExecutor(max_workers=min(8, B)) as pool:
        walks = [pool.submit(walk_oracle, oracle, M0) for M0 in sorted(starts, reverse=True)]   # (the longest first; ctypes releases the GIL)
        walks = dict(zip(sorted(starts, reverse=True), walks))
        f = S.BatchedUKF(B, L_CAP).readParams(); f.init(0.0, 0.0, 0.0)
        got, held, device_s = [], [f.landmark_counts().copy()], 0.0
        for t in range(STEPS):
            ks = np.array([len(s[t]) for s in scripts], dtype=np.int32)
            meas = np.zeros((B, max(1, int(ks.max())), 3), dtype=np.float32)
            for b in range(B): meas[b, :ks[b]] = scripts[b][t]
            t0 = time.perf_counter()
            f.update(cmds[t], meas, ks); f.sync()
            device_s += time.perf_counter() - t0
            got.append((f.status().astype(np.int64), [f.get_state(b) for b in range(B)]))
            held.append(f.landmark_counts().copy())
        f.close()
        walks = {M0: w.result() for M0, w in walks.items()}
    held = np.array(held)                                       # [STEPS + 1][B]: row t = the counts step t started with
    print(f"[streamed sizes] {B} instances, {STEPS} steps: {device_s * 1e3:.1f} ms in update + sync (host clock: message copy and both kernels of every step)")
    print(f"[streamed sizes] landmark counts held, step by step: {held.tolist()}")
    for t in range(STEPS):
        status, states = got[t]
        for b, M0 in enumerate(starts):
            fl, so = walks[M0][t]
            assert int(status[b]) == fl, (M0, t, int(status[b]), fl)
            _same(states[b], so, f"M0 = {M0}, step {t}")
    # the walk was what it claims to be, from the device's own counts
    expect = np.array([[0, M0, M0 + 1, M0 + 1, min(M0 + 3, L_CAP), min(M0 + 3, L_CAP)] for M0 in starts]).T
    assert np.array_equal(held, expect), held.tolist()
    at_start = held[:STEPS]
    final = got[-1][0]
    assert not (final & (SQRT_FAILED | NONFINITE)).any(), final
    capped = [M0 for b, M0 in enumerate(starts) if final[b] & CAPACITY]
    assert capped == [M0 for M0 in starts if M0 + 3 > L_CAP], capped
    assert (at_start[at_start > 0] <= 50).any()                                                # few landmarks in a streamed handle: unpadded at small n
    assert ((at_start > 50) & (at_start % 2 == 1)).any() and ((at_start > 50) & (at_start % 2 == 0)).any()
    assert {21, 22, 50, 51, 52}.issubset(set(at_start.ravel().tolist()))                       # n = 46 (2 mod 4) and both sides of the LDS classes' end
    assert (at_start == L_CAP - 1).any() and (at_start == L_CAP).any() and capped == [198]     # n = 402 and n = 404 both decomposed


# ---- 2. the generator's full state at capacity ------------------------------------------------------------------------------------------------
def test_full_state_at_capacity_from_the_generator(S, oracle):
    """L = 200, n = 404 with device-generated messages: a first look at all 200 landmarks (200 insertions in one message, then the warm
    root extended from n_v = 4 to 404), a second full look (200 updates in one message), ordinary steps; sigma points, weighted mean and
    covariance over nmax = 404 with a sigma stride of 809.  Error statistics and true poses included."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = L_CAP, 6, 2
    lm, cmds = make_scenario(53, L, T)
    vis = np.tile([3.0, -1.57, 1.57], (T, 1)); vis[0] = [1e9, -4.0, 4.0]; vis[3] = [1e9, -4.0, 4.0]
    with ThreadPoolExecutor(max_workers=1) as pool:
        ref = pool.submit(oracle.run_ukf_batch, lm, cmds, B, L, seed=12, nthreads=2, vision=vis)
        f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(12); f.init(0, 0, 0)
        counts = []
        for t in range(T):
            f.set_vision(*vis[t]); f.update_sim(cmds[t]); counts.append(f.landmark_counts().copy())
        r = ref.result()
    print(f"[streamed sizes] generator at capacity: counts after every step {np.array(counts).tolist()}, flags {f.status().tolist()}")
    assert np.all(np.array(counts) == L)                         # mapped at the first look: every later step ran at n = 404
    assert np.array_equal(f.landmark_counts(), r["M"]) and np.array_equal(f.status(), r["flags"]) and not r["flags"].any()
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    n = 4 + 2 * L
    for b in range(B):
        _same(f.get_state(b), dict(M=L, ids=r["ids"][b], x=r["x"][b], P=r["P"][b].reshape(n, n)), f"instance {b}")
    f.close()


# ---- 3. more than a hundred warm starts in a row ----------------------------------------------------------------------------------------------
AGE_SEED = 11     # the scenario seed, chosen with the oracle alone among 1 .. 59: the only one at which every instance holds M (= 5, n = 14)
                  # from step 20 to step 130 under the narrow vision below and still receives detections on the way


def test_a_long_run_crosses_the_warm_start_age_limit(S, oracle):
    """kUkfWarmMaxAge = 100: the 102nd decomposition of a run starts cold again (identity instead of the previous eigenvectors).  130 steps
    of a streamed handle (L_max = 60) in two run_sim calls.  Normal vision for the first 20 steps maps a few landmarks of the 60; from then
    on a narrow one keeps M from changing.  The generator only ever adds landmarks, so a count that is the same after step 20 and after
    step 130 was held at all 110 steps between: the age limit was crossed at a constant size."""
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B, T0 = 60, 130, 4, 20
    lm, cmds = make_scenario(AGE_SEED, L, T)
    wide, narrow = [3.0, -1.57, 1.57], [2.0, -0.5, 0.5]
    vis = np.tile(narrow, (T, 1)); vis[:T0] = wide
    f = S.BatchedUKF(B, L).readParams(); f.set_map(lm); f.set_seed(9); f.init(0, 0, 0)
    f.set_vision(*wide); f.run_sim(cmds[:T0]); at_t0 = f.landmark_counts().copy()
    f.set_vision(*narrow); f.run_sim(cmds[T0:]); at_end = f.landmark_counts().copy()
    r = oracle.run_ukf_batch(lm, cmds, B, L, seed=9, nthreads=4, vision=vis)
    print(f"[streamed sizes] age limit: counts after step {T0} {at_t0.tolist()}, after step {T} {at_end.tolist()}, flags {f.status().tolist()}")
    assert T - T0 > 100 and (at_t0 >= 1).all() and np.array_equal(at_t0, at_end)
    assert np.array_equal(at_end, r["M"]) and np.array_equal(f.status(), r["flags"]) and not r["flags"].any()
    assert np.array_equal(f.error_stats(), r["avg_err"]) and np.array_equal(f.truth(), r["truth"])
    for b in range(B):
        M = int(r["M"][b]); n = 4 + 2 * M
        _same(f.get_state(b), dict(M=M, ids=r["ids"][b, :M], x=r["x"][b, :n], P=r["P"][b, :n * n].reshape(n, n)), f"instance {b}")
    f.close()


# ---- 4. the comparison itself -----------------------------------------------------------------------------------------------------------------
def test_the_comparator_has_teeth(oracle):
    """One ulp in one entry of P at n = 106 (51 landmarks) and `differing` reports P, and only P.  A check of the helper on the CPU; nothing on
    the device is perturbed."""
    so = walk_oracle(oracle, 51)[0][1]
    assert so["M"] == 51 and so["P"].shape == (106, 106)
    poked = {k: np.array(v, copy=True) for k, v in so.items()}
    assert differing(poked, so) == []
    poked["P"][57, 3] = np.nextafter(poked["P"][57, 3], np.inf)
    assert differing(poked, so) == ["P"]
    with pytest.raises(AssertionError):
        _same(poked, so, "one ulp")
    poked["P"][57, 3] = so["P"][57, 3]; poked["x"][105] = np.nextafter(poked["x"][105], -np.inf)
    assert differing(poked, so) == ["x"]
