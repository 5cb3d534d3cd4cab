"""The two orders an update of the decoupled EKF loop can take, at the small shapes where either can go wrong.

The control wavefront (ekf_step_decoupled.h) computes H P / K / x of an update into registers, stages the thin downdate's broadcast operands
K[T_s] / (H P)[T_s] by thin slot, and looks at its ring slot ONCE: free -> the update is stored and published before its thin work; full ->
the thin downdate runs first, then the wait, the store and the publication.  Which of the two a given update takes depends on how far the
streamers are, so each case runs twice: with debug flags 0 (timing decides) and with the test-only flag 1024 (the look always answers
"full": every update takes the deferred order).  Both must give the oracle's bits.

Shapes:

* size class 103 at n = 103 and n = 65 (two trips of 64 lanes, 39 / 1 valid lanes in the second; the staging writes come from lanes of
  either trip, and the launches detect landmarks whose state index is >= 64), on the KG = 6, 5 and 4 instantiations,
* size class 43 at n = 43 (W = 2: the only streamer is pass leader and generator, the control wavefront outruns it most easily),
* fp32 storage at n = 103 and n = 43 (passes end on timestep boundaries; s_wend is written with the deferred store),
* the wide-sensor scenario of test_ekf_control_loop_gpu.py (steps of 0, 1 - 3, 4 - 6 and >= 7 detections in one launch and a landmark that
  leaves the view and returns: a group boundary and a gather follow an update that took the deferred order),
* a state that grows from n = 3 (the corridor map of that file).

Every case is ONE run_sim launch of 80 steps at batch 8 (the corridor: 4) and compares x, P, ids, flags, the true pose and the error
statistic of EVERY instance with the oracle (MODE_FAST, the storage flag for fp32): equality in bits, no tolerance.  The oracle runs once
per configuration and is shared by the cases that need it.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NORMAL = (3.0, -1.57, 1.57)
UNLIMITED = (1e9, -4.0, 4.0)
FORCE_DEFERRED = 1024   # slam_set_debug_flags, tests only (include/slam_batch.h)
FLAGS = [0, FORCE_DEFERRED]
# the lane-boundary cases: scenario 4321, step 0 with the unlimited sensor maps every landmark, then 80 steps in one launch
LANE_SCENARIO, LANE_SEED, LANE_INST0, LANE_T, LANE_B = 4321, 99, 17, 81, 8
# the wide-sensor case of test_ekf_control_loop_gpu.py (scenario 11, a long narrow sensor: instance 0 sees 4 / 39 / 32 / 5 messages of
# 0 / 1 - 3 / 4 - 6 / >= 7 detections in steps 1 .. 80; confirmed below with the oracle's generator)
GROUP_SENSOR = (6.0, -0.8, 0.8)
GROUP_SCENARIO, GROUP_SEED, GROUP_INST0, GROUP_T, GROUP_B = 11, 2025, 0, 81, 8
GROUP_COUNTS_INST0 = (4, 39, 32, 5)
CORRIDOR = -1   # "scenario" of the hand-built map below


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()  # raises if the HIP extension is missing: there is no fallback path to test instead
    return S


@functools.lru_cache(maxsize=None)
def _scenario(seed, L, T):
    from live_ekf_slam_amd.scenario import make_scenario
    if seed == CORRIDOR:
        # a straight drive between two rows of landmarks 2.9 m to either side (test_ekf_control_loop_gpu.py): landmarks come into view one at
        # a time, the state grows from n = 3 to n ~ 71 in 80 steps with update-only steps at nearly every size in between
        gaps = np.where(np.arange(L) < 5, 0.5, 0.19)
        lm = np.stack([0.9 + np.cumsum(gaps) - gaps[0], np.where(np.arange(L) % 2 == 0, 2.9, -2.9)], 1).astype(np.float64)
        cmds = np.tile(np.array([0.1, 0.0], dtype=np.float32), (T, 1))
    else:
        lm, cmds = make_scenario(seed, L, T)
    lm.setflags(write=False); cmds.setflags(write=False)
    return lm, cmds


def _vision(T, sensor, first_unlimited):
    vis = np.tile(np.asarray(sensor, dtype=np.float64), (T, 1))
    if first_unlimited:
        vis[0] = UNLIMITED
    return vis


@functools.lru_cache(maxsize=None)
def _reference(scen, L, T, B, seed, inst0, f32, sensor, first_unlimited):
    """The oracle's batch for one configuration, computed once and left unchanged."""
    from oracle import oracle as O
    lm, cmds = _scenario(scen, L, T)
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    r = O.run_ekf_batch(lm, cmds, B, L, seed=seed, inst0=inst0, nthreads=4, mode=mode, vision=_vision(T, sensor, first_unlimited))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def _messages(scen, L, T, B, seed, inst0, sensor, first_unlimited):
    """Landmark ids of every message, [instance][timestep], from the oracle's measurement generator (the true pose does not depend on the
    sensor, so one generator with the sensor of the launch serves every step of it; the step with the unlimited sensor is left out)."""
    from oracle import oracle as O
    lm, cmds = _scenario(scen, L, T)
    cfg = O.default_config()
    cfg.range_max, cfg.fov_min, cfg.fov_max = sensor
    out = []
    for b in range(B):
        sim = O.OracleSim(lm, cfg)
        rows = []
        for t in range(T):
            _, meas = sim.step_philox(cmds[t, 0], cmds[t, 1], seed, inst0 + b, t)
            rows.append(tuple(int(m[0]) for m in meas))
        out.append(tuple(rows[1:] if first_unlimited else rows))
    return tuple(out)


def _run_gpu(S, monkeypatch, scen, L, T, B, seed, inst0, f32, sensor, first_unlimited, variant, flags):
    """Step 0 on its own when it uses the unlimited sensor, every other step in ONE multi-step launch with the debug flags of the case."""
    from live_ekf_slam_amd import _lib
    monkeypatch.setenv("SLAM_RUN_CHUNK", "0")
    if variant:
        assert _lib.lib().slam_variant_available(L, 1 if f32 else 0, variant), f"kernel variant {variant} is missing from the build"
        monkeypatch.setenv("SLAM_WAVES_PER_FILTER", str(variant))
    else:
        monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)
    lm, cmds = _scenario(scen, L, T)
    f = S.BatchedEKF(B, L, dtype=S.F32 if f32 else S.F64).readParams()
    f.set_map(lm); f.set_seed(seed); f.set_instance_offset(inst0); f.init(0, 0, 0)
    t0 = 0
    if first_unlimited:
        f.set_vision(*UNLIMITED); f.update_sim(cmds[0]); t0 = 1
    f.set_vision(*sensor)
    f.k_histogram(reset=True)
    f.set_debug_flags(flags)
    f.run_sim(cmds[t0:])
    f.set_debug_flags(0)
    return f


def _assert_batch_equal(f, r, T):
    """x, P, ids, flags, true pose and error statistic of every instance, bit for bit."""
    B = f.batch
    assert np.array_equal(f.landmark_counts(), r["M"])
    assert np.array_equal(f.status(), r["flags"])
    assert np.array_equal(f.truth(), r["truth"])
    assert np.array_equal(f.error_stats(), r["avg_err"])
    for b in range(B):
        M = int(r["M"][b]); n = 3 + 2 * M
        s = f.get_state(b)
        assert s["M"] == M and (s["timestep"] == T or r["flags"][b] != 0), f"instance {b}"
        assert np.array_equal(s["ids"], r["ids"][b, :M]), f"instance {b}: ids"
        assert np.array_equal(s["x"], r["x"][b, :n]), f"instance {b}: x off by {np.abs(s['x'] - r['x'][b, :n]).max()}"
        Po = r["P"][b, :n * n].reshape(n, n)
        assert np.array_equal(s["P"], Po), f"instance {b}: P off by {np.abs(s['P'] - Po).max()}"


def _case(S, monkeypatch, scen, L, T, B, seed, inst0, flags, f32=False, sensor=NORMAL, first_unlimited=True, variant=0):
    f = _run_gpu(S, monkeypatch, scen, L, T, B, seed, inst0, f32, sensor, first_unlimited, variant, flags)
    try:
        r = _reference(scen, L, T, B, seed, inst0, f32, sensor, first_unlimited)
        _assert_batch_equal(f, r, T)
        return r, f.k_histogram().astype(np.int64)
    finally:
        f.close()


def _histogram(msgs):
    h = np.zeros(8, dtype=np.int64)
    for rows in msgs:
        for ids in rows:
            h[min(len(ids), 7)] += 1
    return h


def _updates_at_or_beyond(msgs, r, first):
    """Detections, per instance, of landmarks one of whose two state indices is >= first (their K / H P are staged by a lane of the second trip)."""
    out = []
    for b, rows in enumerate(msgs):
        order = [int(i) for i in r["ids"][b, :int(r["M"][b])]]
        out.append(sum(1 for ids in rows for i in ids if 3 + 2 * order.index(i) + 1 >= first))
    return out


def _lane_case(S, monkeypatch, L, flags, f32=False, variant=0):
    r, h = _case(S, monkeypatch, LANE_SCENARIO, L, LANE_T, LANE_B, LANE_SEED, LANE_INST0, flags, f32=f32, variant=variant)
    msgs = _messages(LANE_SCENARIO, L, LANE_T, LANE_B, LANE_SEED, LANE_INST0, NORMAL, True)
    assert np.all(r["M"] == L) and not r["flags"].any()
    assert np.array_equal(h, _histogram(msgs)), (h, _histogram(msgs))   # the kernel counted the messages the generator produced
    assert h[1:7].sum() > 0 and h[7] == 0, h                            # updates, and every step inside the decoupled loop
    return r, msgs


# code = PIPE * 1000 + W * 100 + KG * 10 + UNR: 0 = the default of the class (KG = 6), then the KG = 5 and KG = 4 instantiations
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("variant", [0, 1454, 1444])
@pytest.mark.parametrize("L", [31, 50])
def test_two_trips_of_class_103(S, oracle, monkeypatch, L, variant, flags):
    """n = 65 leaves the second trip of 64 lanes one valid lane, n = 103 leaves it 39 and one pad column.  In both launches landmarks with a
    state index >= 64 are detected (n = 65: the last landmark, whose y is index 64 - ten detections per instance; n = 103: nineteen), so
    the staging array is written by lanes of both trips."""
    r, msgs = _lane_case(S, monkeypatch, L, flags, variant=variant)
    high = _updates_at_or_beyond(msgs, r, 64)
    assert min(high) >= (10 if L == 31 else 19), high


@pytest.mark.parametrize("flags", FLAGS)
def test_class_43_with_one_streamer(S, oracle, monkeypatch, flags):
    """n = 43 in class 43: two wavefronts, the only streamer is pass leader and measurement generator."""
    _lane_case(S, monkeypatch, 20, flags)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("L,variant", [(50, 1462), (20, 0)])
def test_fp32_storage(S, oracle, monkeypatch, L, variant, flags):
    """fp32 storage: a pass ends where a timestep ends (s_wend, written with the deferred store); L = 50 on the (103, 4, 6, 2) instantiation,
    L = 20 in class 43 with two wavefronts."""
    _lane_case(S, monkeypatch, L, flags, f32=True, variant=variant)


def _reentries(msgs, kloop=6):
    """(instance, landmark, t_seen, t_back): seen, absent for at least one step, back - with every message in between short enough for the
    decoupled loop, so the return is a gather inside the loop."""
    out = []
    for b, rows in enumerate(msgs):
        last = {}
        for t, ids in enumerate(rows):
            for i in ids:
                if i in last and last[i] < t - 1 and all(len(rows[u]) <= kloop for u in range(last[i], t + 1)):
                    out.append((b, i, last[i], t))
                last[i] = t
    return out


@pytest.mark.parametrize("flags", FLAGS)
def test_groups_and_gathers_after_a_deferred_update(S, oracle, monkeypatch, flags):
    """One 80-step launch whose messages hold 0, 1 - 3, 4 - 6 (two groups of KP = 3 inside the loop) and >= 7 detections (synchronised
    path), and in which a landmark leaves the view and returns while the loop runs: group formation and the gather read the ring from
    `applied` to `published` right after an update that was published late."""
    msgs = _messages(GROUP_SCENARIO, 50, GROUP_T, GROUP_B, GROUP_SEED, GROUP_INST0, GROUP_SENSOR, True)
    h0 = _histogram(msgs[:1])
    assert (h0[0], h0[1:4].sum(), h0[4:7].sum(), h0[7]) == GROUP_COUNTS_INST0, h0   # instance 0 sees each kind of step
    hs = _histogram(msgs)
    assert hs[0] > 0 and hs[1:4].sum() > 0 and hs[4:7].sum() > 0 and hs[7] > 0, hs
    assert _reentries(msgs), "no landmark leaves the view and returns inside the loop"
    r, h = _case(S, monkeypatch, GROUP_SCENARIO, 50, GROUP_T, GROUP_B, GROUP_SEED, GROUP_INST0, flags, sensor=GROUP_SENSOR)
    assert np.array_equal(h, hs), (h, hs)
    assert np.all(r["M"] == 50) and not r["flags"].any()


@pytest.mark.parametrize("flags", FLAGS)
def test_growing_state(S, oracle, monkeypatch, flags):
    """Capacity 50, nothing mapped, the normal sensor from init: n grows from 3 by insertions (synchronised path) and the decoupled loop is
    re-entered at every size on the way past 64, with most of every thin row being pad."""
    r, h = _case(S, monkeypatch, CORRIDOR, 50, 80, 4, 2025, 5, flags, first_unlimited=False)
    assert r["M"].min() >= 31 and r["M"].max() < 50 and not r["flags"].any(), r["M"]   # 3 + 2 * 31 = 65: every instance crosses n = 64
    assert h[1:7].sum() > 0 and h[7] == 0, h
