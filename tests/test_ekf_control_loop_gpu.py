"""The control wavefront of the decoupled EKF loop at the small shapes where its per-lane code can go wrong.

The multi-step launch hands consecutive timesteps to ONE wavefront (ekf_step_decoupled.h): prediction, H P / K / x, the downdate of the
thin rows / columns, the end of the step - every one of them a loop over the state index in trips of 64 lanes.  The parity tests run it
at n = 103 and n = 43 for hundreds of steps; here the shapes are the ones at which a lane mask, a pad column or a group boundary decides:

* n = 63 / 65 / 103 in size class 103 (two trips of 64 lanes: a full first trip with its pad, one valid lane in the second, one pad column),
* a state that GROWS through the class (the loop is re-entered at n = 5, 7, ... and crosses 64; most of every thin row is pad),
* timesteps of 0, 1 - 3, 4 - 6 (two groups inside the loop) and >= 7 detections (back to the synchronised path) in one launch, with a
  landmark that leaves the view and returns (its row / column is gathered while updates are pending),
* fp32 storage (rounding loop, passes that end on timestep boundaries) at n = 103 and n = 43,
* the KG = 5 and KG = 4 instantiations of class 103.

Every case is ONE run_sim launch and compares x, P, ids, flags and the error statistic of EVERY instance with the oracle (MODE_FAST, the
storage flag for fp32): equality in bits, no tolerance.  The oracle runs once per configuration and is shared by the cases that need it.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NORMAL = (3.0, -1.57, 1.57)
UNLIMITED = (1e9, -4.0, 4.0)
# the widened sensor of the group case: chosen on the CPU (scenario generator + the oracle's measurement generator) so that the 80 steps
# hold empty messages, one-group, two-group and over-long ones, and a landmark that leaves the view and comes back
# (scenario 11, a long narrow sensor: instance 0 sees 4 / 39 / 32 / 5 messages of 0 / 1 - 3 / 4 - 6 / >= 7 detections in steps 1 .. 80)
GROUP_SENSOR = (6.0, -0.8, 0.8)
GROUP_SCENARIO, GROUP_SEED, GROUP_INST0, GROUP_T, GROUP_B = 11, 2025, 0, 81, 8
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
        # A straight drive at the planner's step length (0.1 m) between two rows of landmarks 2.9 m to either side: with the normal sensor
        # (range 3.0, FOV +-1.57) a landmark is in view for about 0.77 m of the drive, so landmarks come into view one at a time - every
        # 0.5 m for the first five, every 0.19 m after that - and at most six are in view at once.  In 80 steps the state grows from
        # n = 3 to n ~ 71 with update-only steps (the decoupled loop) at nearly every size in between; the oracle says so in the test.
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
def _reference(scen, L, L_max, T, B, seed, inst0, f32, sensor, first_unlimited):
    """The oracle's batch for one configuration, computed once and left unchanged."""
    from oracle import oracle as O
    lm, cmds = _scenario(scen, L, T)
    mode = O.MODE_FAST | (O.STORAGE_F32 if f32 else 0)
    r = O.run_ekf_batch(lm, cmds, B, L_max, seed=seed, inst0=inst0, nthreads=4, mode=mode, vision=_vision(T, sensor, first_unlimited))
    for v in r.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return r


def _run_gpu(S, monkeypatch, scen, L, L_max, T, B, seed, inst0, f32, sensor, first_unlimited, variant=0):
    """Step 0 on its own when it uses the unlimited sensor, every other step in ONE multi-step launch."""
    from live_ekf_slam_amd import _lib
    monkeypatch.setenv("SLAM_RUN_CHUNK", "0")
    if variant:
        assert _lib.lib().slam_variant_available(L_max, 1 if f32 else 0, variant), f"kernel variant {variant} is missing from the build"
        monkeypatch.setenv("SLAM_WAVES_PER_FILTER", str(variant))
    else:
        monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)
    lm, cmds = _scenario(scen, L, T)
    f = S.BatchedEKF(B, L_max, dtype=S.F32 if f32 else S.F64).readParams()
    f.set_map(lm); f.set_seed(seed); f.set_instance_offset(inst0); f.init(0, 0, 0)
    t0 = 0
    if first_unlimited:
        f.set_vision(*UNLIMITED); f.update_sim(cmds[0]); t0 = 1
    f.set_vision(*sensor)
    f.k_histogram(reset=True)
    f.run_sim(cmds[t0:])
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


def _case(S, monkeypatch, scen, L, L_max, T, B, seed, inst0, f32=False, sensor=NORMAL, first_unlimited=True, variant=0):
    f = _run_gpu(S, monkeypatch, scen, L, L_max, T, B, seed, inst0, f32, sensor, first_unlimited, variant)
    try:
        r = _reference(scen, L, L_max, T, B, seed, inst0, f32, sensor, first_unlimited)
        _assert_batch_equal(f, r, T)
        return r, f.k_histogram()
    finally:
        f.close()


# code = PIPE * 1000 + W * 100 + KG * 10 + UNR: 0 = the default of the class (KG = 6), then the KG = 5 and KG = 4 instantiations
@pytest.mark.parametrize("variant", [0, 1454, 1444])
@pytest.mark.parametrize("L", [30, 31, 50])
def test_lane_boundaries_of_the_two_trips(S, oracle, monkeypatch, L, variant):
    """n = 63 fills the first trip of 64 lanes together with its pad column, n = 65 leaves the second trip one valid lane, n = 103 has one
    pad column in fp64: all of them in size class 103 (two trips per wavefront).  Step 0 maps every landmark, then 40 steps in one launch."""
    r, h = _case(S, monkeypatch, 4321, L, L, 41, 8, 99, 17, variant=variant)
    assert np.all(r["M"] == L) and not r["flags"].any()
    assert h[1:].sum() > 0, "no update in the launch"


def test_state_much_smaller_than_its_class(S, oracle, monkeypatch):
    """Capacity 50, nothing mapped, the normal sensor from init: n grows by insertions (synchronised path) and the decoupled loop is
    re-entered at n = 5, 7, ... past 64, with most of every thin row being pad."""
    sizes = _update_only_sizes(CORRIDOR, 50, 80, 2025, 5)
    assert min(sizes) == 5 and max(sizes) >= 65 and len(sizes) >= 20, sizes   # update-only steps from n = 5 to beyond the first trip
    r, h = _case(S, monkeypatch, CORRIDOR, 50, 50, 80, 4, 2025, 5, first_unlimited=False)
    assert r["M"].min() >= 31 and r["M"].max() < 50 and not r["flags"].any(), r["M"]   # 3 + 2 * 31 = 65: every instance crosses n = 64
    assert h[1:7].sum() > 0 and h[7] == 0


def _update_only_sizes(scen, L, T, seed, inst):
    """State sizes n at which the instance has a timestep of 1 .. 6 detections, all of known landmarks: the steps the decoupled loop takes."""
    from oracle import oracle as O
    lm, cmds = _scenario(scen, L, T)
    sim = O.OracleSim(lm, O.default_config())
    seen, sizes = set(), set()
    for t in range(T):
        _, meas = sim.step_philox(cmds[t, 0], cmds[t, 1], seed, inst, t)
        ids = {int(m[0]) for m in meas}
        if ids and len(meas) <= 6 and ids <= seen:
            sizes.add(3 + 2 * len(seen))
        seen |= ids
    return sorted(sizes)


def _group_messages():
    """Landmark ids of every message of the group case, [instance][timestep] (the oracle's measurement generator; the true pose does not
    depend on the sensor, so one generator with the widened sensor serves every step after step 0)."""
    from oracle import oracle as O
    lm, cmds = _scenario(GROUP_SCENARIO, 50, GROUP_T)
    cfg = O.default_config()
    cfg.range_max, cfg.fov_min, cfg.fov_max = GROUP_SENSOR
    out = []
    for b in range(GROUP_B):
        sim = O.OracleSim(lm, cfg)
        rows = []
        for t in range(GROUP_T):
            _, meas = sim.step_philox(cmds[t, 0], cmds[t, 1], GROUP_SEED, GROUP_INST0 + b, t)
            rows.append([int(m[0]) for m in meas])
        out.append(rows[1:])   # step 0 runs with the unlimited sensor
    return out


def _histogram(msgs):
    h = np.zeros(8, dtype=np.int64)
    for rows in msgs:
        for ids in rows:
            h[min(len(ids), 7)] += 1
    return h


def _reentries(msgs, kloop=6):
    """(instance, landmark, t_seen, t_back): seen, absent for at least one step, back - with every message in between short enough for the
    decoupled loop (so the return is a gather inside the loop, not a step of the synchronised path).  That updates are still pending in the
    ring at that gather is likely (two groups per step here, passes start at five pending updates) but cannot be shown from outside the
    kernel: it depends on when the streamers claimed their last pass."""
    out = []
    for b, rows in enumerate(msgs):
        last = {}
        for t, ids in enumerate(rows):
            for i in ids:
                if i in last and last[i] < t - 1 and all(len(rows[u]) <= kloop for u in range(last[i], t + 1)):
                    out.append((b, i, last[i], t))
                last[i] = t
    return out


def test_groups_of_detections_inside_the_loop(S, oracle, monkeypatch):
    """One 80-step launch whose messages hold 0, 1 - 3, 4 - 6 (two groups of KP = 3 inside the loop) and >= 7 detections (synchronised
    path), and in which a landmark leaves the view and returns while the loop runs (gather with pending updates)."""
    msgs = _group_messages()
    hs = _histogram(msgs)
    assert hs[0] > 0 and hs[1:4].sum() > 0 and hs[4:7].sum() > 0 and hs[7] > 0, hs
    assert _reentries(msgs), "no landmark leaves the view and returns inside the loop"
    r, h = _case(S, monkeypatch, GROUP_SCENARIO, 50, 50, GROUP_T, GROUP_B, GROUP_SEED, GROUP_INST0, sensor=GROUP_SENSOR)
    h = h.astype(np.int64)
    assert h[0] > 0 and h[1:4].sum() > 0 and h[4:7].sum() > 0 and h[7] > 0, h
    assert np.array_equal(h, hs), (h, hs)   # the kernel counted the messages the generator produced
    assert np.all(r["M"] == 50) and not r["flags"].any()


@pytest.mark.parametrize("L,variant", [(50, 1462), (20, 0)])
def test_fp32_storage(S, oracle, monkeypatch, L, variant):
    """fp32 storage: L = 50 on the (103, 4, 6, 2) instantiation (rounding loop of the thin copies, passes that end where a timestep ends);
    L = 20 in class 43 with two wavefronts and three pad columns at n = 43."""
    r, h = _case(S, monkeypatch, 4321, L, L, 41, 8, 99, 17, f32=True, variant=variant)
    assert np.all(r["M"] == L) and not r["flags"].any()
    assert h[1:].sum() > 0, "no update in the launch"
