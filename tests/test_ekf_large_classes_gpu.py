"""The EKF step kernel's size classes beyond 50 landmarks (ekf_step_kernel<203, ..> and <403, ..>) at every lane and group edge.

test_ekf_control_loop_gpu.py and test_ekf_ring_defer_gpu.py run the decoupled loop (ekf_step_decoupled.h) where a lane mask, a pad column or a
group boundary decides - in class 103, where the control wavefront makes two trips of 64 lanes and the default instantiation has KP = 3.
Classes 203 and 403 are instantiations of their own: four and seven trips, LDP = 204 / 404, KP = 4 (KLOOP = 8).  Here:

1. lane boundaries of EVERY trip: step 0 maps L = L_max landmarks, then 40 steps in one launch at n = 105, 127, 129, 191, 193, 203 (class 203,
   on its default 1454 and on 1444) and n = 205, 255, 257, 319, 321, 383, 385, 403 (class 403), each with debug flags 0 and 1024 (every
   update takes the deferred order); the scenario of each size is chosen so that EVERY instance detects landmarks whose state indices lie in
   every trip of that n, and so that every message of the launch has 1 .. 8 detections (the whole launch stays inside the loop),
2. groups of KP = 4: one 80-step launch per class (203 on both variants, 403, class 103 forced to 1454 and to 1444) whose messages hold
   0, 1 - 4, 5 - 8 (two groups inside the loop) and >= 9 detections (synchronised path), with messages of exactly 4, 5, 8 and 9 and a landmark
   that leaves the view and returns inside the loop,
3. a state that grows from n = 3 through every trip: the corridor map of test_ekf_control_loop_gpu.py with 100 and 200 landmarks, as one
   launch (flags 0 and 1024) and split into launches where the state crosses a trip boundary (compared after each part),
4. capacities 21, 51, 101, 201 (the first of each class and of the streamed kernel): the dispatch by name, a scripted walk of external
   messages compared after every step, messages of exactly the class's message capacity and one more, one streamed launch at 201 landmarks.

Every GPU case compares x, P, ids, flags, the true pose and the error statistic of EVERY instance with the oracle (MODE_FAST): equality in
bits, no tolerance.  Every case asserts from kernel_info() that the class and the variant it names ran, from traffic_counters()
that passes applied every detection, and from k_histogram() that the kernel saw the messages the oracle's generator produced; it prints all
three (pytest -s).  The premises (sizes, trips, detection counts of every scenario) are asserted from the oracle's generator in tests that
need no GPU.  The oracle runs once per configuration and is shared by the cases that need it.
"""
import functools
import re

import numpy as np
import pytest

from test_ekf_control_loop_gpu import CORRIDOR, NORMAL, UNLIMITED, _assert_batch_equal, _reference, _scenario

gpu = pytest.mark.gpu

FORCE_DEFERRED = 1024   # slam_set_debug_flags, tests only (include/slam_batch.h)
FLAGS = [0, FORCE_DEFERRED]
CAPACITY = 8            # SLAM_INST_CAPACITY
# variant code = PIPE * 1000 + W * 100 + KG * 10 + UNR; what variant 0 selects in each class
DEFAULT_VARIANT = {43: 1254, 103: 1464, 203: 1454, 403: 1444}


def _class_of(L_max):
    return 43 if L_max <= 20 else 103 if L_max <= 50 else 203 if L_max <= 100 else 403


# ---- the scenarios, chosen on the CPU with the oracle's generator (test_premises_* below assert every figure) ------------------------------
# 1. lane boundaries.  L = L_max -> (scenario seed, detections' state indices per 64-lane trip in the 40 steps of the launch: the minimum
#    over the eight instances).  Normal sensor, instances 17 .. 24 of seed 99; every message of every instance has 1 .. 8 detections.
LANE_SEED, LANE_INST0, LANE_T, LANE_B = 99, 17, 41, 8
LANE_203 = {51: (2, (72, 72)), 62: (1, (14, 186)), 63: (10, (234, 124, 8)), 94: (1, (24, 164, 38)), 95: (1, (6, 158, 204, 30)),
            100: (1, (8, 148, 198, 30))}
LANE_403 = {101: (1, (18, 150, 190, 29)), 126: (2, (76, 50, 180, 74)), 127: (26, (26, 80, 64, 69, 19)), 158: (2, (77, 39, 158, 57, 91)),
            159: (37, (128, 116, 38, 126, 10, 10)), 190: (2, (86, 68, 32, 6, 42, 76)), 191: (32, (8, 36, 32, 88, 94, 109, 9)),
            200: (2, (86, 68, 32, 6, 42, 76, 4))}
LANE = {**LANE_203, **LANE_403}
# 2. groups of four.  L = L_max -> (scenario seed, sensor, messages of instance 0 with 0 / 4 / 5 / 8 / 9 detections in steps 1 .. 80, messages
#    of all eight instances with 0 / 1 - 4 / 5 - 8 / >= 9).  Instances 0 .. 7 of seed 2025.
GROUP_SEED, GROUP_INST0, GROUP_T, GROUP_B = 2025, 0, 81, 8
GROUP = {50: (273, (6.0, -0.8, 0.8), (1, 11, 8, 3, 1), (8, 374, 250, 8)),
         100: (141, NORMAL, (3, 9, 13, 15, 1), (19, 253, 359, 9)),
         200: (25, NORMAL, (8, 9, 16, 9, 1), (63, 250, 315, 12))}
# 3. the growing state.  L = L_max -> (steps, first instance, the n every instance must reach, M bounds at which the launch is split).  The
#    true pose drifts sideways over hundreds of steps and a row of the corridor 2.9 m away then stays out of the sensor's 3.0 m: the first
#    instance is chosen so that all four instances of seed 2025 see both rows to the end (final M 98 of 100, >= 198 of 200).
GROW_SEED, GROW_B = 2025, 4
GROW = {100: (204, 21, 193, (31, 63, 95)), 200: (400, 122, 385, (31, 63, 95, 127, 159, 191))}


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()  # raises if the HIP extension is missing: there is no fallback path to test instead
    return S


# ---- the generator's messages ----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _messages(scen, L, T, B, seed, inst0, sensor, first_unlimited):
    """(orders, msgs) from the oracle's measurement generator.  msgs [instance][step]: the landmark ids of every message of the launch (the
    true pose does not depend on the sensor, so one generator with the sensor of the launch serves every step of it; the step with the
    unlimited sensor is left out).  orders [instance]: the ids of that first message, i.e. the order of the landmarks in the state."""
    from oracle import oracle as O
    lm, cmds = _scenario(scen, L, T)
    cfg, cfg0 = O.default_config(), O.default_config()
    cfg.range_max, cfg.fov_min, cfg.fov_max = sensor
    cfg0.range_max, cfg0.fov_min, cfg0.fov_max = UNLIMITED
    orders, out = [], []
    for b in range(B):
        sim = O.OracleSim(lm, cfg)
        rows = []
        for t in range(T):
            _, meas = sim.step_philox(cmds[t, 0], cmds[t, 1], seed, inst0 + b, t)
            rows.append(tuple(int(m[0]) for m in meas))
        if first_unlimited:
            _, meas = O.OracleSim(lm, cfg0).step_philox(cmds[0, 0], cmds[0, 1], seed, inst0 + b, 0)
            orders.append(tuple(int(m[0]) for m in meas))
        out.append(tuple(rows[1:] if first_unlimited else rows))
    return tuple(orders), tuple(out)


def _counts(msgs):
    """messages by their exact number of detections, all instances"""
    c = np.zeros(1 + max(len(ids) for rows in msgs for ids in rows), dtype=np.int64)
    for rows in msgs:
        for ids in rows:
            c[len(ids)] += 1
    return c


def _histogram(msgs):
    """what k_histogram() resolves: 0 .. 6 and >= 7"""
    h = np.zeros(8, dtype=np.int64)
    for rows in msgs:
        for ids in rows:
            h[min(len(ids), 7)] += 1
    return h


def _trip_hits(order, rows, kloop=8):
    """State indices of the detections of one instance's loop steps (1 .. kloop detections), counted by the 64-lane trip they fall into:
    landmark slot j holds the indices 3 + 2 j and 4 + 2 j."""
    n = 3 + 2 * len(order)
    slot = {i: j for j, i in enumerate(order)}
    hits = np.zeros((n + 63) // 64, dtype=np.int64)
    for ids in rows:
        if 1 <= len(ids) <= kloop:
            for i in ids:
                hits[(3 + 2 * slot[i]) // 64] += 1
                hits[(4 + 2 * slot[i]) // 64] += 1
    return hits


def _reentries(msgs, kloop=8):
    """(instance, landmark, t_seen, t_back): seen, absent for at least one step, back - with every message in between short enough for the
    decoupled loop, so the return is a gather inside the loop (test_ekf_control_loop_gpu.py, with the loop's limit as a parameter)."""
    out = []
    for b, rows in enumerate(msgs):
        last = {}
        for t, ids in enumerate(rows):
            for i in ids:
                if i in last and last[i] < t - 1 and all(len(rows[u]) <= kloop for u in range(last[i], t + 1)):
                    out.append((b, i, last[i], t))
                last[i] = t
    return out


def _growth(msgs, kloop=8):
    """The growing state from the generator alone: M [instance][step] after every step, and the state sizes n at which an instance has a
    timestep of 1 .. kloop detections, all of known landmarks - the steps the decoupled loop takes (_update_only_sizes of
    test_ekf_control_loop_gpu.py for any loop limit and every instance)."""
    M, sizes = [], set()
    for rows in msgs:
        seen, row = set(), []
        for ids in rows:
            if ids and len(ids) <= kloop and set(ids) <= seen:
                sizes.add(3 + 2 * len(seen))
            seen |= set(ids)
            row.append(len(seen))
        M.append(row)
    return np.array(M), sorted(sizes)


def _split_steps(M, bounds):
    """The launch is cut before the first step at which some instance holds `bound` landmarks: in the part that ends there every instance
    is below that trip boundary (n <= 2 * bound + 1), the next part crosses it."""
    cuts = [int(np.argmax(M.max(axis=0) >= b)) for b in bounds]
    assert all(M.max(axis=0)[c] >= b and c > 0 for c, b in zip(cuts, bounds)) and sorted(set(cuts)) == cuts, cuts
    return cuts


# ---- the premises, on the CPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", sorted(LANE))
def test_premises_of_the_lane_cases(oracle, L):
    """Every message of the 40-step launch has 1 .. 8 detections (all of known landmarks: step 0 mapped them), so every step is a step of
    the decoupled loop; and in EVERY instance the detected landmarks' state indices fall into every 64-lane trip of n = 3 + 2 L."""
    scen, want = LANE[L]
    orders, msgs = _messages(scen, L, LANE_T, LANE_B, LANE_SEED, LANE_INST0, NORMAL, True)
    n = 3 + 2 * L
    assert all(sorted(o) == list(range(L)) for o in orders)          # the first look maps all L landmarks
    c = _counts(msgs)
    assert c[0] == 0 and len(c) <= 9 and c.sum() == LANE_B * (LANE_T - 1), c
    hits = np.array([_trip_hits(o, rows) for o, rows in zip(orders, msgs)])
    assert hits.shape == (LANE_B, (n + 63) // 64) and len(want) == (n + 63) // 64
    assert (hits > 0).all(), hits
    assert tuple(hits.min(axis=0)) == want, hits.min(axis=0)
    if n % 64 == 1:   # n = 129, 193, 257, 321, 385: the last trip has ONE valid lane, the y of the last landmark mapped
        last = [o[-1] for o in orders]
        assert all(any(i in ids for ids in rows) for i, rows in zip(last, msgs))


@pytest.mark.parametrize("L", sorted(GROUP))
def test_premises_of_the_group_cases(oracle, L):
    """Messages of 0, 1 - 4, 5 - 8 and >= 9 detections in one launch, with the edges of both groups of four: exactly 4, 5, 8 and 9; and a
    landmark that returns to the view inside the loop (every message in between has <= 8 detections)."""
    scen, sensor, inst0, kinds = GROUP[L]
    _, msgs = _messages(scen, L, GROUP_T, GROUP_B, GROUP_SEED, GROUP_INST0, sensor, True)
    c0 = _counts(msgs[:1]); c0 = np.concatenate([c0, np.zeros(10, dtype=np.int64)])
    assert tuple(int(c0[k]) for k in (0, 4, 5, 8, 9)) == inst0, c0
    assert min(inst0) > 0                                            # instance 0 alone sees each kind of message
    c = _counts(msgs)
    assert (c[0], c[1:5].sum(), c[5:9].sum(), c[9:].sum()) == kinds and min(kinds) > 0, c
    assert c[4] > 0 and c[5] > 0 and c[8] > 0 and c[9] > 0, c
    assert _reentries(msgs, kloop=8), "no landmark leaves the view and returns inside the loop"


@pytest.mark.parametrize("L", sorted(GROW))
def test_premises_of_the_growing_state(oracle, L):
    """Update-only steps of <= 8 detections at a size within +-4 of every multiple of 64 below the final n, every instance beyond the last
    trip boundary of its class, and a split point for every bound."""
    T, inst0, n_past, bounds = GROW[L]
    _, msgs = _messages(CORRIDOR, L, T, GROW_B, GROW_SEED, inst0, NORMAL, False)
    M, sizes = _growth(msgs)
    n_final = 3 + 2 * int(M[:, -1].min())
    assert n_final >= n_past and M.max() <= L, (n_final, M[:, -1])
    assert min(sizes) == 5 and max(sizes) >= n_past, sizes
    for edge in range(64, n_final, 64):
        assert any(abs(s - edge) <= 4 for s in sizes), (edge, sizes)
    assert max(len(ids) for rows in msgs for ids in rows) <= 8       # no message leaves the loop for its length: only insertions do
    cuts = _split_steps(M, bounds)
    assert len(cuts) == len(bounds) and cuts[-1] < T - 1, cuts


def test_the_comparator_has_teeth(oracle):
    """One ulp in one entry of P of an oracle state at n = 105 (class 203) and _assert_batch_equal reports it; so it does one ulp in x, a
    changed id and a changed flag.  A check of the helper on the CPU: nothing on the device is perturbed."""
    L, B = 51, 2
    r = _reference(LANE[L][0], L, L, 3, B, LANE_SEED, LANE_INST0, False, NORMAL, True)
    n = 3 + 2 * L
    assert np.all(r["M"] == L)

    class Held:   # what _assert_batch_equal reads from a filter handle, served from arrays
        batch = B

        def __init__(self, r):
            self.r = {k: np.array(v, copy=True) for k, v in r.items() if isinstance(v, np.ndarray)}

        landmark_counts = lambda self: self.r["M"]
        status = lambda self: self.r["flags"]
        truth = lambda self: self.r["truth"]
        error_stats = lambda self: self.r["avg_err"]

        def get_state(self, b):
            M = int(self.r["M"][b]); m = 3 + 2 * M
            return dict(M=M, timestep=3, ids=self.r["ids"][b, :M], x=self.r["x"][b, :m], P=self.r["P"][b, :m * m].reshape(m, m))

    _assert_batch_equal(Held(r), r, 3)
    for field, at in (("P", (1, 57 * n + 3)), ("P", (0, n * n - 1)), ("x", (1, n - 1)), ("truth", (0, 2)), ("avg_err", (1,))):
        h = Held(r)
        h.r[field][at] = np.nextafter(h.r[field][at], np.inf)
        with pytest.raises(AssertionError):
            _assert_batch_equal(h, r, 3)
    for field, at in (("ids", (1, L - 1)), ("flags", (0,)), ("M", (1,))):
        h = Held(r)
        h.r[field][at] += 1
        with pytest.raises(AssertionError):
            _assert_batch_equal(h, r, 3)


# ---- one launch on the device -------------------------------------------------------------------------------------------------------------------
def _handle(S, monkeypatch, L_max, B, variant=0, f32=False):
    """A handle on the instantiation the case names, asserted from slam_kernel_info (the variant is read from the environment at creation)."""
    from live_ekf_slam_amd import _lib
    monkeypatch.setenv("SLAM_RUN_CHUNK", "0")
    if variant:
        assert _lib.lib().slam_variant_available(L_max, 1 if f32 else 0, variant), f"kernel variant {variant} is missing from the build"
        monkeypatch.setenv("SLAM_WAVES_PER_FILTER", str(variant))
    else:
        monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)
    f = S.BatchedEKF(B, L_max, dtype=S.F32 if f32 else S.F64).readParams()
    name = f.kernel_info(multi_step=True)["name"]
    code = variant or DEFAULT_VARIANT[_class_of(L_max)]
    want = f"ekf_step_kernel<{_class_of(L_max)},{code // 100 % 10},{code // 10 % 10},{code % 10},{'float' if f32 else 'double'},{code // 1000},true,"
    assert name.startswith(want), (name, want)
    return f, name


def _launch(S, monkeypatch, scen, L, L_max, T, B, seed, inst0, sensor, first_unlimited, variant, flags):
    """Step 0 on its own when it uses the unlimited sensor, every other step in ONE multi-step launch with the debug flags of the case."""
    lm, cmds = _scenario(scen, L, T)
    f, name = _handle(S, monkeypatch, L_max, B, variant)
    f.set_map(lm); f.set_seed(seed); f.set_instance_offset(inst0); f.init(0, 0, 0)
    t0 = 0
    if first_unlimited:
        f.set_vision(*UNLIMITED); f.update_sim(cmds[0]); t0 = 1
    f.set_vision(*sensor)
    f.k_histogram(reset=True); f.traffic_counters(reset=True)
    f.set_debug_flags(flags)
    f.run_sim(cmds[t0:])
    f.set_debug_flags(0)
    return f, name


def _case(S, monkeypatch, what, scen, L, L_max, T, B, seed, inst0, flags, sensor=NORMAL, first_unlimited=True, variant=0):
    """One launch against the oracle, every instance; then the evidence that the launch was the one the case is about.  Returns the
    oracle's batch, the messages and (passes, instance-steps with a detection)."""
    f, name = _launch(S, monkeypatch, scen, L, L_max, T, B, seed, inst0, sensor, first_unlimited, variant, flags)
    try:
        r = _reference(scen, L, L_max, T, B, seed, inst0, False, sensor, first_unlimited)
        h, tc = f.k_histogram().astype(np.int64), f.traffic_counters().astype(np.int64)
        print(f"[large classes] {what}: {name} variant {variant or 'default'} flags {flags}: passes {tc[2]}, updates applied by passes {tc[3]}, "
              f"k histogram {h.tolist()}, M {r['M'].tolist()}")
        _assert_batch_equal(f, r, T)
        _, msgs = _messages(scen, L, T, B, seed, inst0, sensor, first_unlimited)
        hs = _histogram(msgs)
        assert np.array_equal(h, hs), (h, hs)          # the kernel counted the messages the generator produced
        assert tc[2] > 0 and tc[3] > 0, tc             # passes ran and applied updates
        return r, msgs, tc
    finally:
        f.close()


def _detections_of_known(msgs, all_known):
    """Updates the launch must apply: every detection when step 0 mapped the whole map, else the detections of landmarks seen before."""
    if all_known:
        return sum(len(ids) for rows in msgs for ids in rows)
    total = 0
    for rows in msgs:
        seen = set()
        for ids in rows:
            total += len(set(ids) & seen)
            seen |= set(ids)
    return total


# ---- 1. lane boundaries of every trip ---------------------------------------------------------------------------------------------------------
def _lane_case(S, monkeypatch, L, variant, flags):
    scen, _ = LANE[L]
    r, msgs, tc = _case(S, monkeypatch, f"lanes n = {3 + 2 * L}", scen, L, L, LANE_T, LANE_B, LANE_SEED, LANE_INST0, flags, variant=variant)
    assert np.all(r["M"] == L) and not r["flags"].any()
    # every detection is one rank-2 update applied by some pass.  (The pass count itself is printed, not bounded: the streamers start a pass
    # at four pending updates wherever the timesteps end, so a launch of long messages may take more passes than one pass per group would.)
    assert tc[3] == _detections_of_known(msgs, True), tc


@gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("variant", [0, 1444])
@pytest.mark.parametrize("L", sorted(LANE_203))
def test_lane_boundaries_of_the_four_trips_of_class_203(S, oracle, monkeypatch, L, variant, flags):
    """n = 105 (41 valid lanes in the second trip) / 127 and 129 (the second trip full with its pad column, one valid lane in the third) /
    191 and 193 (the same one trip on) / 203 (11 valid lanes in the fourth trip, one pad column of LDP = 204)."""
    _lane_case(S, monkeypatch, L, variant, flags)


@gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("L", sorted(LANE_403))
def test_lane_boundaries_of_the_seven_trips_of_class_403(S, oracle, monkeypatch, L, flags):
    """n = 205 (the smallest state of the class) / 255 and 257 / 319 and 321 / 383 and 385 (a trip that ends with the pad column, one valid
    lane in the next) / 403 (19 valid lanes in the seventh trip, one pad column of LDP = 404)."""
    _lane_case(S, monkeypatch, L, 0, flags)


# ---- 2. groups of four inside the loop --------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("L,variant", [(50, 1454), (50, 1444), (100, 0), (100, 1444), (200, 0)])
def test_groups_of_four_inside_the_loop(S, oracle, monkeypatch, L, variant, flags):
    """KP = 4: a message of 1 - 4 detections is one group, 5 - 8 two groups inside the loop, >= 9 goes back to the synchronised path; the
    launch holds messages of exactly 4, 5, 8 and 9 (asserted from the generator: k_histogram() resolves 0 .. 6 and >= 7) and a landmark
    that returns to the view while the loop runs."""
    scen, sensor, _, _ = GROUP[L]
    r, msgs, tc = _case(S, monkeypatch, f"groups L = {L}", scen, L, L, GROUP_T, GROUP_B, GROUP_SEED, GROUP_INST0, flags, sensor=sensor,
                        variant=variant)
    c = _counts(msgs)
    assert c[0] > 0 and c[4] > 0 and c[5] > 0 and c[8] > 0 and c[9] > 0 and _reentries(msgs, kloop=8)
    assert np.all(r["M"] == L) and not r["flags"].any()
    assert tc[3] == _detections_of_known(msgs, True), tc


# ---- 3. a state that grows through every trip -------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("L", sorted(GROW))
def test_state_grows_through_every_trip_in_one_launch(S, oracle, monkeypatch, L, flags):
    """Capacity 100 / 200, nothing mapped, the normal sensor from init: n grows by insertions (synchronised path) and the decoupled loop is
    re-entered at nearly every size up to n >= 193 / 385, with the rest of every thin row being pad."""
    T, inst0, n_past, _ = GROW[L]
    r, msgs, tc = _case(S, monkeypatch, f"growth to L = {L}", CORRIDOR, L, L, T, GROW_B, GROW_SEED, inst0, flags, first_unlimited=False)
    assert 3 + 2 * int(r["M"].min()) >= n_past and not r["flags"].any(), r["M"]
    assert np.array_equal(r["M"], _growth(msgs)[0][:, -1])
    assert tc[3] == _detections_of_known(msgs, False), tc


@gpu
@pytest.mark.parametrize("L", sorted(GROW))
def test_state_grows_through_every_trip_in_parts(S, oracle, monkeypatch, L):
    """The same run cut into launches where the first instance reaches 31, 63, 95 (127, 159, 191) landmarks, compared after each part: a
    failure names the trip boundary that was crossed in it."""
    T, inst0, n_past, bounds = GROW[L]
    _, msgs = _messages(CORRIDOR, L, T, GROW_B, GROW_SEED, inst0, NORMAL, False)
    M, _ = _growth(msgs)
    cuts = _split_steps(M, bounds) + [T]
    lm, cmds = _scenario(CORRIDOR, L, T)
    f, name = _handle(S, monkeypatch, L, GROW_B)
    try:
        f.set_map(lm); f.set_seed(GROW_SEED); f.set_instance_offset(inst0); f.init(0, 0, 0)
        f.set_vision(*NORMAL)
        f.k_histogram(reset=True); f.traffic_counters(reset=True)
        t0 = 0
        for t1 in cuts:
            f.run_sim(cmds[t0:t1])
            r = _reference(CORRIDOR, L, L, t1, GROW_B, GROW_SEED, inst0, False, NORMAL, False)
            print(f"[large classes] growth to L = {L} in parts: {name}, steps {t0} .. {t1 - 1}: M {r['M'].tolist()}")
            assert np.array_equal(r["M"], M[:, t1 - 1])
            _assert_batch_equal(f, r, t1)
            t0 = t1
        h, tc = f.k_histogram().astype(np.int64), f.traffic_counters().astype(np.int64)
        print(f"[large classes] growth to L = {L} in parts: passes {tc[2]}, updates applied by passes {tc[3]}, k histogram {h.tolist()}")
        assert np.array_equal(h, _histogram(msgs)), (h, _histogram(msgs))
        assert tc[2] > 0 and tc[3] == _detections_of_known(msgs, False), tc
        assert 3 + 2 * int(r["M"].min()) >= n_past and not r["flags"].any()
    finally:
        f.close()


# ---- 4. capacity edges and the dispatch -------------------------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("L_max,f32,want", [(20, False, 43), (21, False, 103), (50, False, 103), (51, False, 203), (100, False, 203),
                                            (101, False, 403), (200, False, 403), (201, False, None),
                                            (20, True, 43), (21, True, 103), (50, True, 103), (51, True, None)])
def test_dispatch_at_the_capacity_edges(S, L_max, f32, want):
    """slam_kernel_info names the class of the table in ekf_kernel.hip for the last capacity of a class and the first of the next; beyond
    200 landmarks (fp32 storage: beyond 50) it names the HBM-streamed kernel."""
    f = S.BatchedEKF(2, L_max, dtype=S.F32 if f32 else S.F64).readParams()
    try:
        for multi in (True, False):
            name = f.kernel_info(multi_step=multi)["name"]
            if want is None:
                assert name == "ekf_big_step_kernel", (L_max, f32, name)
            else:
                m = re.match(r"ekf_step_kernel<(\d+),\d+,\d+,\d+,(double|float),\d+,(true|false),\d+>$", name)
                assert m and int(m.group(1)) == want and m.group(2) == ("float" if f32 else "double") and m.group(3) == str(multi).lower(), \
                    (L_max, f32, name)
        print(f"[large classes] capacity {L_max} {'fp32' if f32 else 'fp64'}: {name}")
    finally:
        f.close()


WALK_STEPS = 5
FOREIGN_ID = 900
# handle capacity -> the landmark counts M0 the instances start with: n = 3 + 2 M0 on both sides of every trip boundary the handle's class can
# reach with that capacity (n = 63 | 65, 127 | 129, 191 | 193 ...), and capacity - 2.  Capacity 21 ends at n = 45, inside the first trip.
WALK_STARTS = {21: (9, 12, 16, 19), 51: (9, 29, 30, 31, 40, 49), 101: (30, 31, 62, 63, 94, 95, 96, 99),
               201: (30, 31, 62, 63, 94, 95, 126, 127, 158, 159, 190, 191, 199)}
WALK_K = (3, 4, 7, 8)


def _script(cap, b):
    """The five messages of instance b of the handle of capacity `cap`, [k][3] float32 (id, range, bearing):
    0  ids 0 .. M0 - 1: M0 insertions in one message
    1  k known ids, k = 3, 4, 7, 8 by instance (one group, a full group, two groups, two full groups of KP = 4), and the new id M0
    2  nine known ids (one more than two groups)
    3  five known ids, the new ids M0 + 1 and M0 + 2 and a foreign id: three insertions - with capacity - 1 landmarks held one of them fits and
       SLAM_INST_CAPACITY is raised
    4  an empty message"""
    M0, k = WALK_STARTS[cap][b], WALK_K[b % 4]
    rng = np.random.default_rng(1000 * cap + M0)
    def msg(ids):
        m = np.zeros((len(ids), 3), dtype=np.float32)
        m[:, 0] = ids; m[:, 1] = rng.uniform(0.5, 6.0, len(ids)); m[:, 2] = rng.uniform(-3.1, 3.1, len(ids))
        return m
    known = lambda M, k: rng.choice(M, k, replace=False)
    return [msg(np.arange(M0)), msg(np.append(known(M0, k), M0)), msg(known(M0 + 1, 9)),
            msg(np.append(known(M0 + 1, 5), [M0 + 1, M0 + 2, FOREIGN_ID])), msg(np.zeros(0))]


def _walk_commands():
    rng = np.random.default_rng(77)
    return np.stack([rng.uniform(0.0, 0.1, WALK_STEPS), rng.uniform(-0.05, 0.05, WALK_STEPS)], axis=1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _walk_oracle(cap, b):
    """The script through one OracleEKF(L_max = cap): (flags OR-ed so far, state) after every step."""
    from oracle import oracle as O
    e = O.OracleEKF(L_max=cap, mode=O.MODE_FAST); e.init(0, 0, 0)
    out, fl = [], 0
    for cmd, m in zip(_walk_commands(), _script(cap, b)):
        fl |= e.update(cmd[0], cmd[1], m)
        out.append((fl, e.state()))
    return out


def _assert_state_equal(sg, so, what):
    assert sg["M"] == so["M"] and sg["timestep"] == so["timestep"], what
    assert np.array_equal(sg["ids"], so["ids"]), f"{what}: ids"
    assert sg["x"].shape == so["x"].shape and np.array_equal(sg["x"], so["x"]), f"{what}: x off by {np.abs(sg['x'] - so['x']).max()}"
    assert sg["P"].shape == so["P"].shape and np.array_equal(sg["P"], so["P"]), f"{what}: P off by {np.abs(sg['P'] - so['P']).max()}"


def test_premises_of_the_scripted_walk():
    """The starts sit on both sides of every trip boundary within the capacity and at capacity - 2; every k of 3, 4, 7, 8 occurs."""
    for cap, starts in WALK_STARTS.items():
        assert cap - 2 in starts and min(starts) >= 9 and max(starts) + 2 <= cap
        for edge in range(64, 3 + 2 * cap - 1, 64):
            assert (edge - 4) // 2 in starts and (edge - 4) // 2 + 1 in starts, (cap, edge)     # n = edge - 1 and n = edge + 1
        assert {WALK_K[b % 4] for b in range(len(starts))} == set(WALK_K)
        for b, M0 in enumerate(starts):
            s = _script(cap, b)
            assert [len(m) for m in s] == [M0, WALK_K[b % 4] + 1, 9, 8, 0]
            assert len(set(s[1][:, 0])) == len(s[1]) and len(set(s[2][:, 0])) == 9 and len(set(s[3][:, 0])) == 8


@gpu
@pytest.mark.parametrize("cap", sorted(WALK_STARTS))
def test_scripted_walk_at_the_first_capacity_of_each_class(S, oracle, cap):
    """Capacities 21, 51, 101 (the smallest handles of classes 103, 203, 403) and 201 (the streamed kernel), external messages through
    update(): instance b starts with its own landmark count, the instances sit side by side in one launch.  Checked after EVERY step."""
    starts = WALK_STARTS[cap]
    B = len(starts)
    scripts, cmds = [_script(cap, b) for b in range(B)], _walk_commands()
    f = S.BatchedEKF(B, cap).readParams(); f.init(0.0, 0.0, 0.0)
    try:
        name = f.kernel_info(multi_step=False)["name"]
        assert name == "ekf_big_step_kernel" if cap > 200 else name.startswith(f"ekf_step_kernel<{_class_of(cap)},"), name
        held = [f.landmark_counts().copy()]
        for t in range(WALK_STEPS):
            ks = np.array([len(s[t]) for s in scripts], dtype=np.int32)
            meas = np.zeros((B, max(1, int(ks.max())), 3), dtype=np.float32)
            for b in range(B):
                meas[b, :ks[b]] = scripts[b][t]
            f.update(cmds[t], meas, ks)
            status = f.status()
            held.append(f.landmark_counts().copy())
            for b, M0 in enumerate(starts):
                fl, so = _walk_oracle(cap, b)[t]
                assert int(status[b]) == fl, (cap, M0, t, int(status[b]), fl)
                _assert_state_equal(f.get_state(b), so, f"capacity {cap}, M0 = {M0}, step {t}")
        held = np.array(held)
        h, tc = f.k_histogram().astype(np.int64), f.traffic_counters().astype(np.int64)
        print(f"[large classes] scripted walk, capacity {cap}: {name}, landmark counts held step by step {held.tolist()}, flags {status.tolist()}, "
              f"passes {tc[2]}, updates applied by passes {tc[3]}, k histogram {h.tolist()}")
        assert np.array_equal(h, _histogram(scripts)), (h, _histogram(scripts))      # the kernel counted the messages of the script
        if cap <= 200:
            assert tc[2] > 0 and tc[3] > 0, tc
        expect = np.array([[0, M0, M0 + 1, M0 + 1, min(M0 + 4, cap), min(M0 + 4, cap)] for M0 in starts]).T
        assert np.array_equal(held, expect), held.tolist()
        assert [int(s) for s in status] == [CAPACITY if M0 + 4 > cap else 0 for M0 in starts], status
        assert (status == CAPACITY).sum() == 1 and (held[-1] == cap).sum() == 1      # the instance that started at capacity - 2, and only it
    finally:
        f.close()


@gpu
@pytest.mark.parametrize("cap", [21, 51])
def test_messages_at_the_message_capacity_of_the_class(S, oracle, cap):
    """ekf_class_message_capacity: a handle of capacity 21 (class 103) holds messages of 50 detections, one of capacity 51 (class 203)
    messages of 100.  Step 1: instance 0 gets exactly that many (repeated known ids), the others ordinary messages - the LDS kernel alone.
    Step 2: instance 1 gets one more, instance 0 the full length again, the others ordinary messages - the host pairs the LDS kernel with
    the streamed one (EkfStepParams::long_mode), which takes instance 1 only.  Bits and flags after every step."""
    from oracle import oracle as O
    B, M0 = 4, 12
    mcap = 50 if cap <= 50 else 100
    rng = np.random.default_rng(cap)
    def msg(ids):
        m = np.zeros((len(ids), 3), dtype=np.float32)
        m[:, 0] = ids; m[:, 1] = rng.uniform(0.5, 6.0, len(ids)); m[:, 2] = rng.uniform(-3.1, 3.1, len(ids))
        return m
    steps = [[msg(np.arange(M0)) for b in range(B)],
             [msg(rng.integers(0, M0, mcap)), msg(rng.choice(M0, 3, replace=False)), msg(rng.choice(M0, 5, replace=False)), msg(np.zeros(0))],
             [msg(rng.integers(0, M0, mcap)), msg(rng.integers(0, M0, mcap + 1)), msg(rng.choice(M0, 2, replace=False)), msg(np.append(rng.choice(M0, 4, replace=False), M0))],
             [msg(rng.choice(M0, 4, replace=False)) for b in range(B)]]
    assert [len(m) for m in steps[1]] == [mcap, 3, 5, 0] and [len(m) for m in steps[2]] == [mcap, mcap + 1, 2, 5]
    cmds = _walk_commands()
    es = []
    for b in range(B):
        e = O.OracleEKF(L_max=cap, mode=O.MODE_FAST); e.init(0, 0, 0); es.append(e)
    f = S.BatchedEKF(B, cap).readParams(); f.init(0.0, 0.0, 0.0)
    try:
        assert f.kernel_info(multi_step=False)["name"].startswith(f"ekf_step_kernel<{_class_of(cap)},")
        of = np.zeros(B, dtype=np.int64)
        for t, msgs in enumerate(steps):
            ks = np.array([len(m) for m in msgs], dtype=np.int32)
            meas = np.zeros((B, max(1, int(ks.max())), 3), dtype=np.float32)
            for b in range(B):
                meas[b, :ks[b]] = msgs[b]
            f.update(cmds[t], meas, ks)
            for b in range(B):
                of[b] |= es[b].update(cmds[t][0], cmds[t][1], msgs[b])
            status = f.status().astype(np.int64)
            print(f"[large classes] message capacity, handle capacity {cap}, step {t}: message lengths {ks.tolist()}, flags {status.tolist()}")
            assert np.array_equal(status, of), (t, status, of)
            for b in range(B):
                _assert_state_equal(f.get_state(b), es[b].state(), f"capacity {cap}, step {t}, instance {b}")
        h, tc = f.k_histogram().astype(np.int64), f.traffic_counters().astype(np.int64)
        print(f"[large classes] message capacity, handle capacity {cap}: passes {tc[2]}, updates applied by passes {tc[3]}, k histogram {h.tolist()}")
        assert tc[2] > 0 and tc[3] > 0, tc
        assert not of.any() and f.landmark_counts().tolist() == [M0, M0, M0, M0 + 1]
    finally:
        f.close()


@gpu
def test_one_streamed_launch_at_capacity_201(S, oracle, monkeypatch):
    """Capacity 201 with a map of 201 landmarks: the first look maps them all (n = 405, the smallest state no LDS class holds), then 20 steps
    of run_sim in one call."""
    L, T, B, scen = 201, 21, 2, 2
    monkeypatch.setenv("SLAM_RUN_CHUNK", "0")
    monkeypatch.delenv("SLAM_WAVES_PER_FILTER", raising=False)
    lm, cmds = _scenario(scen, L, T)
    f = S.BatchedEKF(B, L).readParams()
    try:
        name = f.kernel_info(multi_step=True)["name"]
        assert name == "ekf_big_step_kernel", name
        f.set_map(lm); f.set_seed(LANE_SEED); f.set_instance_offset(LANE_INST0); f.init(0, 0, 0)
        f.set_vision(*UNLIMITED); f.update_sim(cmds[0])
        f.set_vision(*NORMAL); f.k_histogram(reset=True)
        f.run_sim(cmds[1:])
        r = _reference(scen, L, L, T, B, LANE_SEED, LANE_INST0, False, NORMAL, True)
        h = f.k_histogram().astype(np.int64)
        print(f"[large classes] streamed launch: {name}, k histogram {h.tolist()}, M {r['M'].tolist()}")
        _assert_batch_equal(f, r, T)
        _, msgs = _messages(scen, L, T, B, LANE_SEED, LANE_INST0, NORMAL, True)
        assert np.array_equal(h, _histogram(msgs)) and h[1:].sum() > 0, (h, _histogram(msgs))
        assert np.all(r["M"] == L) and not r["flags"].any()
    finally:
        f.close()
