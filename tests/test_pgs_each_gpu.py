"""Heterogeneous pose-graph batches on the GPU (pgs_*_each, include/slam_pgs.h): every graph of a handle with its own start pose, map and
BetweenFactor measurements.

1. rows that are all equal give the bits of the shared calls (simulator, host-fed updates, and a handle that switches between the two);
2. independent scenarios in one handle against the oracle run slice by slice, on every solve path;
3. own stream and start pose on external messages (pins the per-instance PriorFactor and BetweenFactor);
4. truth0 and per-instance maps in the device simulator against the EKF engine's simulator;
5. a closed-loop EKF batch feeding the pose graph tick by tick;
6. shard invariance, marginals, argument errors.

The bar against the oracle is test_parity_pgs_gpu._compare's (copied below): equal flags, LM iterations and lambda trials, initial poses
bit-exact, result within 1e-7 m, objective within 1e-9 relative."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import load_golden
from live_ekf_slam_amd.config import default_config
from live_ekf_slam_amd.scenario import make_scenario

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-7
OBJ_RTOL = 1e-9
SEED = 8


def _compare(pg, r, B, check_init=True, first=0):
    """test_parity_pgs_gpu._compare for the instances [first, first + B) of the handle against the oracle run r of those B."""
    st = {k: v[first:first + B] for k, v in pg.stats().items()}
    assert np.array_equal(st["flags"], r["flags"])
    assert np.array_equal(st["iterations"], r["iterations"]), (st["iterations"], r["iterations"])
    assert np.array_equal(st["trials"], r["trials"]), (st["trials"], r["trials"])
    assert np.allclose(st["err_init"], r["err_init"], rtol=1e-12, atol=0)
    assert np.allclose(st["err_final"], r["err_final"], rtol=OBJ_RTOL, atol=0)
    assert np.allclose(st["lam"], r["lam"], rtol=1e-12)
    for b in range(B):
        g0, g1 = pg.get_graph(first + b, 0), pg.get_graph(first + b, 1)
        M = r["M"][b]
        assert g0["M"] == M and np.array_equal(g0["ids"], r["ids"][b, :M])
        if check_init:
            assert np.array_equal(g0["poses"], r["pose_init"][b])          # bit-exact graph building
        assert np.abs(g1["poses"] - r["pose_res"][b]).max() < POSE_TOL
        assert np.abs(g1["landmarks"] - r["lm_res"][b, :M]).max() < POSE_TOL


def _snapshot(pg):
    B = pg.batch
    return dict(graphs=[[pg.get_graph(b, w) for w in (0, 1)] for b in range(B)], stats=pg.stats(), conn=[pg.connections(b) for b in range(B)],
                err=[pg.error_stats(0), pg.error_stats(1)])


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same(a, b, what):
    """Two snapshots agree bit for bit."""
    for i, (ga, gb) in enumerate(zip(a["graphs"], b["graphs"])):
        for w in (0, 1):
            assert ga[w]["M"] == gb[w]["M"] and np.array_equal(ga[w]["ids"], gb[w]["ids"]), (what, i, w)
            for key in ("poses", "landmarks"):
                assert np.array_equal(_bits(ga[w][key]), _bits(gb[w][key])), f"{what}: instance {i} which {w} {key}"
        assert np.array_equal(a["conn"][i], b["conn"][i]), (what, i)
    for key in a["stats"]:
        assert np.array_equal(_bits(a["stats"][key]), _bits(b["stats"][key])), f"{what}: stats {key}"
    for w in (0, 1):
        assert np.array_equal(_bits(a["err"][w]), _bits(b["err"][w])), f"{what}: error_stats({w})"


def _pg(S, B, T, L_max, KP, cfg=None, **kw):
    return S.BatchedPoseGraph(B, num_iterations=T + 1, L_max=L_max, k_per_pose=KP).readParams(cfg or default_config(), **kw)


# ---- 1. broadcast identity -------------------------------------------------------------------------------------------------------------
def _shared_run(S, lm, cmds, B, L, KP):
    T = cmds.shape[0]
    pg = _pg(S, B, T, L, KP)
    pg.set_map(lm); pg.set_seed(SEED); pg.init(0.0, 0.0, 0.0)
    pg.run_sim(cmds); pg.solvePoseGraph()
    out = _snapshot(pg)
    pg.close()
    return out


@pytest.mark.parametrize("L,T,B,KP", [(8, 33, 5, 8), (20, 150, 12, 8)])
def test_equal_rows_give_the_bits_of_the_shared_calls(L, T, B, KP):
    import live_ekf_slam_amd as S
    lm, cmds = make_scenario(155 + L, L, T)
    ref = _shared_run(S, lm, cmds, B, L, KP)
    each = np.ascontiguousarray(np.broadcast_to(cmds[:, None, :], (T, B, 2)))
    pg = _pg(S, B, T, L, KP)
    pg.set_map(np.broadcast_to(lm, (B, L, 2)), np.full(B, L, np.int32)); pg.set_seed(SEED)
    pg.init(np.zeros((B, 3), np.float32), truth0=np.zeros((B, 3)))
    pg.run_sim(each); pg.solvePoseGraph()
    _same(ref, _snapshot(pg), "simulator, all rows equal")
    pg.close()
    # shared calls up to T // 2, per-instance calls up to 3 T // 4, shared calls again; the per-instance maps come and go with them
    t1, t2 = T // 2, 3 * T // 4
    pg = _pg(S, B, T, L, KP)
    pg.set_map(lm); pg.set_seed(SEED); pg.init(0.0, 0.0, 0.0)
    pg.run_sim(cmds[:t1])
    pg.set_map(np.broadcast_to(lm, (B, L, 2)))
    pg.run_sim(each[t1:t2])
    pg.set_map(lm)
    pg.run_sim(cmds[t2:]); pg.solvePoseGraph()
    assert pg.timestep == T
    _same(ref, _snapshot(pg), "shared -> per instance -> shared")
    pg.close()


@pytest.mark.parametrize("L,T,B,KP", [(8, 33, 5, 8), (20, 150, 12, 8)])
def test_equal_rows_give_the_bits_of_the_shared_update(oracle, L, T, B, KP):
    """Host-fed streams (the oracle runner's messages and secondary poses): update((2,)) against update((B, 2)) with equal rows, and a
    handle that switches at T // 2 and back at 3 T // 4."""
    import live_ekf_slam_amd as S
    lm, cmds = make_scenario(155 + L, L, T)
    r = oracle.run_pgs_batch(lm, cmds, B, L, KP=KP, seed=SEED, want_streams=True)
    cnt = np.minimum(r["cnt"], KP)
    t1, t2 = T // 2, 3 * T // 4
    snaps = []
    for mode in ("shared", "each", "mixed"):
        pg = _pg(S, B, T, L, KP)
        if mode == "each":
            pg.init(np.zeros((B, 3), np.float32))
        else:
            pg.init(0.0, 0.0, 0.0)
        for t in range(T):
            pg.updateNaiveVehPoseEstimate(r["pose_init"][:, t + 1])
            per = mode == "each" or (mode == "mixed" and t1 <= t < t2)
            pg.update(np.tile(cmds[t], (B, 1)) if per else cmds[t], r["meas"][:, t], cnt[:, t])
        pg.solvePoseGraph()
        snaps.append(_snapshot(pg))
        pg.close()
    _same(snaps[0], snaps[1], "update, all rows equal")
    _same(snaps[0], snaps[2], "update, shared -> per instance -> shared")


# ---- 2. independent scenarios against the oracle ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scenarios(Ls, T):
    """Scenario s = make_scenario(100 + s, Ls[s], T): (maps [S][L_max][2], counts [S], cmds [S][T][2])."""
    L_max = max(Ls)
    maps = np.zeros((len(Ls), L_max, 2)); cmds = np.zeros((len(Ls), T, 2), np.float32)
    for s, L in enumerate(Ls):
        lm, c = make_scenario(100 + s, L, T)
        maps[s, :L] = lm; cmds[s] = c
    return maps, np.array(Ls, np.int32), cmds


@functools.lru_cache(maxsize=None)
def _oracle_slices(Ls, T, R, KP, every_iteration=False, want_streams=False):
    from oracle import oracle as O
    maps, counts, cmds = _scenarios(Ls, T)
    return [O.run_pgs_batch(maps[s, :counts[s]], cmds[s], R, max(Ls), KP=KP, seed=SEED, inst0=s * R, nthreads=8, every_iteration=every_iteration,
                            want_streams=want_streams) for s in range(len(Ls))]


def _hetero_handle(S, Ls, T, R, KP, B=None, offset=0, **kw):
    """Instances [s R, (s + 1) R) of the GLOBAL batch run scenario s; the handle holds the B instances from `offset` on."""
    maps, counts, cmds = _scenarios(Ls, T)
    B = len(Ls) * R if B is None else B
    sc = (offset + np.arange(B)) // R
    pg = _pg(S, B, T, max(Ls), KP, **kw)
    pg.set_map(maps[sc], counts[sc]); pg.set_seed(SEED)
    if offset:
        pg.set_instance_offset(offset)
    pg.init(np.zeros((B, 3), np.float32))
    return pg, np.ascontiguousarray(cmds[sc].transpose(1, 0, 2))


VARIANTS = [("32", None), ("32", "0"), ("0", None), ("0", "0")]     # (SLAM_PGS_SEG, SLAM_PGS_FUSED; None = default)
SHAPES = [((8, 20, 8, 20), T, 4, 8) for T in (31, 32, 33, 65, 150)] + [((40, 100, 40, 100), 250, 2, 24)]


@pytest.mark.parametrize("seg,fused", VARIANTS, ids=[f"seg{a}-fused{b or 'default'}" for a, b in VARIANTS])
@pytest.mark.parametrize("Ls,T,R,KP", SHAPES, ids=[f"L{max(s[0])}-T{s[1]}" for s in SHAPES])
def test_independent_scenarios_match_the_oracle(monkeypatch, oracle, Ls, T, R, KP, seg, fused):
    """Four scenarios (their own map, map size and command sequence) side by side in one handle; every slice equals the oracle run of that
    scenario alone with the slice's global instance numbers.  T around the 32-pose segment boundaries; the L 100 case is the size the
    two-launch and fused chain + SYRK paths are tested at."""
    import live_ekf_slam_amd as S
    monkeypatch.setenv("SLAM_PGS_SEG", seg)
    if fused is None:
        monkeypatch.delenv("SLAM_PGS_FUSED", raising=False)
    else:
        monkeypatch.setenv("SLAM_PGS_FUSED", fused)
    pg, cmds = _hetero_handle(S, Ls, T, R, KP)
    pg.run_sim(cmds); pg.solvePoseGraph()
    if seg == "0" or max(Ls) == 20:   # the path under test really ran (the wide maps may send a 32-pose segment to the sequential chain)
        assert pg.last_solve_paths()["segmented"] == (seg != "0"), pg.last_solve_paths()
    for s, r in enumerate(_oracle_slices(Ls, T, R, KP)):
        _compare(pg, r, R, first=s * R)
        assert np.allclose(pg.error_stats(0)[s * R:(s + 1) * R], r["avg_err_init"], rtol=1e-12)
        assert np.allclose(pg.error_stats(1)[s * R:(s + 1) * R], r["avg_err_result"], rtol=1e-6)
    pg.close()


def test_independent_scenarios_solved_every_iteration(oracle):
    """run_sim_every_iteration((T, B, 2)): the reference's default mode with one command per instance; the LM iterations and lambda trials
    summed over the ticks equal the oracle's tick counts."""
    import live_ekf_slam_amd as S
    Ls, T, R, KP = (6, 10, 6, 10), 60, 2, 6
    pg, cmds = _hetero_handle(S, Ls, T, R, KP, solve_graph_every_iteration=True)
    counts = pg.run_sim_every_iteration(cmds)
    assert pg.timestep == T and pg.solved_pose_graph
    for s, r in enumerate(_oracle_slices(Ls, T, R, KP, every_iteration=True)):
        sl = slice(s * R, (s + 1) * R)
        assert np.array_equal(counts[sl], r["tick_counts"].sum(axis=1)), (s, counts[sl], r["tick_counts"].sum(axis=1))
        assert np.array_equal(counts[sl, 0], r["iterations"]) and np.array_equal(counts[sl, 1], r["trials"])
        assert np.all(pg.stats()["flags"][sl] == 0)
        for b in range(R):
            g1 = pg.get_graph(s * R + b, 1); M = r["M"][b]
            assert g1["M"] == M and np.array_equal(g1["ids"], r["ids"][b, :M])
            assert np.abs(g1["poses"] - r["pose_res"][b]).max() < POSE_TOL
            assert np.abs(g1["landmarks"] - r["lm_res"][b, :M]).max() < POSE_TOL
    pg.close()


# ---- 3. own stream and start pose on external messages ---------------------------------------------------------------------------------
def _oracle_bar(pg, b, g, so, check_init=True):
    """Item 2's bar for instance b against one oracle graph g whose solve returned so."""
    st = pg.stats()
    assert st["flags"][b] == so["flags"] and st["iterations"][b] == so["iterations"] and st["trials"][b] == so["trials"], \
        (b, st["flags"][b], st["iterations"][b], st["trials"][b], so)
    assert np.isclose(st["err_init"][b], so["err_init"], rtol=1e-12, atol=0) and np.isclose(st["err_final"][b], so["err_final"], rtol=OBJ_RTOL, atol=0)
    v0, v1, g0, g1 = g.values(0), g.values(1), pg.get_graph(b, 0), pg.get_graph(b, 1)
    assert g0["M"] == v0["M"] and np.array_equal(g0["ids"], v0["ids"])
    if check_init:
        assert np.array_equal(g0["poses"], v0["poses"]) and np.array_equal(g0["landmarks"], v0["landmarks"])
    assert np.abs(g1["poses"] - v1["poses"]).max() < POSE_TOL
    assert np.abs(g1["landmarks"] - v1["landmarks"]).max() < POSE_TOL
    assert np.array_equal(pg.connections(b), g.connections())


def test_each_robot_its_own_stream_and_pose(oracle):
    """Instance b follows golden stream b % 4 (its commands and detections) from its own start pose, a host NaiveFilter per instance as
    the secondary filter == one oracle graph per instance started there and fed that stream.  An instance that read row 0 of the prior
    means or of the commands would solve another graph."""
    import live_ekf_slam_amd as S
    names = ["sim_seed0_L20_T1000.npz", "sim_seed1_L20_T400.npz", "sim_seed2_L50_T1000.npz", "sim_seed1234_L50_T400.npz"]
    gs = [load_golden(n) for n in names]
    B, L_max, T = 8, 50, 120
    ks = max(int(g["meas_count"][:T].max()) for g in gs)
    pose = np.array([[0.05 * b, -0.03 * b, 0.02 * b - 0.07] for b in range(B)], np.float32)
    cfg = default_config()
    pg = _pg(S, B, T, L_max, ks, cfg)
    pg.init(pose)
    orc, naive = [], []
    for b in range(B):
        o = oracle.OraclePoseGraph(cfg, N_max=T + 1, L_max=L_max, KP=ks); o.init(float(pose[b, 0]), float(pose[b, 1]), float(pose[b, 2]))
        n = S.NaiveFilter(); n.init(pose[b, 0], pose[b, 1], pose[b, 2])
        orc.append(o); naive.append(n)
    for t in range(T):
        meas = np.zeros((B, ks, 3), np.float32); cnt = np.zeros(B, np.int32); cmds = np.zeros((B, 2), np.float32); sec = np.zeros((B, 3))
        for b in range(B):
            g = gs[b % 4]; k = int(g["meas_count"][t])
            meas[b, :k] = g["meas"][t, :k]; cnt[b] = k; cmds[b] = g["cmds"][t]
            naive[b].update(cmds[b]); sec[b] = naive[b].getStateVector()
            orc[b].updateNaiveVehPoseEstimate(sec[b])
            orc[b].update(cmds[b, 0], cmds[b, 1], g["meas"][t, :k])
        pg.updateNaiveVehPoseEstimate(sec)
        pg.update(cmds, meas, cnt)
    pg.solvePoseGraph()
    for b in range(B):
        _oracle_bar(pg, b, orc[b], orc[b].solve())
    pg.close()


# ---- 4. truth0 and maps in the simulator -----------------------------------------------------------------------------------------------
def test_truth0_and_maps_in_the_simulator_against_the_ekf_engine(oracle):
    """An EKF handle and a pose-graph handle with the same seed, instance offset, maps, true start poses and commands generate the same
    messages (both simulators are sim_wave with the keys seed, global instance, step): the pose graph built by run_sim((1, B, 2)) tick by
    tick equals per-instance oracle graphs fed the EKF handle's dumped messages.  The secondary filter of the device simulator is the
    NaiveFilter from pose0[b]: its poses are compared with the host NaiveFilter's (libm sincos against the device's deterministic one:
    1e-12), and the oracle graphs are fed the device's poses, so that landmarks, ids and connections compare exactly."""
    import live_ekf_slam_amd as S
    B, L_max, T, off, seed = 6, 20, 40, 5, 21
    Ls = (8, 20, 12)
    maps = np.zeros((B, L_max, 2)); counts = np.zeros(B, np.int32); cmds = np.zeros((T, B, 2), np.float32)
    for b in range(B):
        lm, c = make_scenario(300 + b % 3, Ls[b % 3], T)
        maps[b, :Ls[b % 3]] = lm; counts[b] = Ls[b % 3]; cmds[:, b] = c
    pose0 = np.array([[0.02 * b, -0.01 * b, 0.03 * b] for b in range(B)], np.float32)
    truth0 = np.array([[0.1 * b, 0.2 - 0.05 * b, 0.05 * b - 0.1] for b in range(B)])
    cfg = default_config()
    ekf = S.BatchedEKF(B, L_max).readParams(cfg)
    ekf.set_map(maps, counts); ekf.set_seed(seed); ekf.set_instance_offset(off); ekf.init(pose0, truth0=truth0)
    ekf.last_meas(L_max)                                   # switch the measurement dump on
    pg = _pg(S, B, T, L_max, L_max, cfg)
    pg.set_map(maps, counts); pg.set_seed(seed); pg.set_instance_offset(off); pg.init(pose0, truth0=truth0)
    msgs, truth = [], np.zeros((B, T, 2))
    for t in range(T):
        ekf.run_sim(cmds[t][None])
        msgs.append(ekf.last_meas(L_max))
        truth[:, t] = ekf.truth()[:, :2]
        pg.run_sim(cmds[t][None])
    assert max(int(c.max()) for _, c in msgs) > 0 and len({int(c.sum()) for _, c in msgs}) > 1
    for b in range(B):
        g0 = pg.get_graph(b, 0)
        n = S.NaiveFilter(); n.init(pose0[b, 0], pose0[b, 1], pose0[b, 2])
        o = oracle.OraclePoseGraph(cfg, N_max=T + 1, L_max=L_max, KP=L_max); o.init(float(pose0[b, 0]), float(pose0[b, 1]), float(pose0[b, 2]))
        for t in range(T):
            n.update(cmds[t, b])
            assert np.abs(g0["poses"][t + 1] - n.getStateVector()).max() < 1e-12, (b, t)
            o.updateNaiveVehPoseEstimate(g0["poses"][t + 1])
            o.update(cmds[t, b, 0], cmds[t, b, 1], msgs[t][0][b, :msgs[t][1][b]])
        v = o.values(0)
        assert g0["M"] == v["M"] and np.array_equal(g0["ids"], v["ids"]), b
        assert np.array_equal(g0["poses"], v["poses"]) and np.array_equal(g0["landmarks"], v["landmarks"]), b
        assert np.array_equal(pg.connections(b), o.connections()), b
    # the recorded truth starts at truth0: pgs_error_stats against the EKF handle's truth (float32 wire values as plotting_node.py reads them)
    est = np.stack([pg.get_graph(b, 0)["poses"][:T, :2] for b in range(B)]).astype(np.float32).astype(np.float64)
    want = np.mean(np.hypot(est[..., 0] - truth[..., 0], est[..., 1] - truth[..., 1]), axis=1)
    assert np.allclose(pg.error_stats(0), want, rtol=1e-12), (pg.error_stats(0), want)
    ekf.close(); pg.close()


# ---- 5. closed loop feeding the pose graph ---------------------------------------------------------------------------------------------
def test_closed_loop_ekf_batch_feeds_the_pose_graph(oracle):
    """`filter: pose_graph` with `filter_to_compare: ekf_slam` in closed loop, the reference's default launch: per tick slam_nav_run(1) on an
    EKF handle whose instances follow their own paths, its commands, measurement dump and poses into update((B, 2), ...), which solves and
    adopts (solve_graph_every_iteration).  Against per-instance oracle graphs fed the same arrays and solved after every tick: flags at every
    tick, the LM iterations and lambda trials summed over the ticks (the bar of the every-iteration tests of test_parity_pgs_gpu.py), the
    objective of the last tick's solve, and the final graphs."""
    import live_ekf_slam_amd as S
    B, L, T, KS = 6, 20, 80, 20
    lm = make_scenario(47, L, 2)[0]
    paths = [lm[b % 3: b % 3 + 1 + b % 4].copy() for b in range(B)]
    cfg = default_config()
    ekf = S.BatchedEKF(B, L).readParams(cfg)
    ekf.set_map(lm); ekf.set_seed(11); ekf.init(0.0, 0.0, 0.0)
    ekf.set_paths(paths)
    ekf.last_meas(KS)                                      # switch the measurement dump on
    pg = _pg(S, B, T, L, KS, cfg, solve_graph_every_iteration=True)
    pg.init(0.0, 0.0, 0.0)
    orc = []
    for b in range(B):
        o = oracle.OraclePoseGraph(cfg, N_max=T + 1, L_max=L, KP=KS); o.init(0.0, 0.0, 0.0); orc.append(o)
    seen, sums, osums = 0, np.zeros((B, 2), np.int64), np.zeros((B, 2), np.int64)
    for t in range(T):
        cmds = ekf.run_nav(1, return_cmds=True)[0]
        meas, cnt = ekf.last_meas(KS)
        sec = ekf.poses()
        seen += int(cnt.sum())
        pg.updateNaiveVehPoseEstimate(sec)
        pg.update(cmds, meas, cnt)                          # solves and adopts
        st = pg.stats()
        for b, o in enumerate(orc):
            o.updateNaiveVehPoseEstimate(sec[b])
            o.update(cmds[b, 0], cmds[b, 1], meas[b, :cnt[b]])
            so = o.solve()
            assert st["flags"][b] == so["flags"], (t, b, st["flags"][b], so)
            sums[b] += (st["iterations"][b], st["trials"][b]); osums[b] += (so["iterations"], so["trials"])
            if t == T - 1:
                assert np.isclose(st["err_final"][b], so["err_final"], rtol=OBJ_RTOL, atol=0), (b, st["err_final"][b], so["err_final"])
            o.adopt()
    assert np.array_equal(sums, osums), (sums, osums)
    assert seen > 0, "the measurement dump stayed empty during the closed-loop ticks"
    assert len({tuple(c) for c in cmds.tolist()}) > 1, "the instances were meant to drive different commands"
    for b, o in enumerate(orc):
        v, g1 = o.values(1), pg.get_graph(b, 1)
        assert g1["M"] == v["M"] and np.array_equal(g1["ids"], v["ids"])
        assert np.abs(g1["poses"] - v["poses"]).max() < POSE_TOL and np.abs(g1["landmarks"] - v["landmarks"]).max() < POSE_TOL
        assert np.abs(pg.get_graph(b, 0)["poses"] - v["poses"]).max() < POSE_TOL      # adopted
        assert np.array_equal(pg.connections(b), o.connections())
    ekf.close(); pg.close()


# ---- 6. shard invariance, marginals, arguments -----------------------------------------------------------------------------------------
def test_a_shard_reproduces_its_rows_of_the_batch():
    import live_ekf_slam_amd as S
    Ls, T, R, KP = (8, 20, 8, 20), 65, 4, 8
    whole, cmds = _hetero_handle(S, Ls, T, R, KP)
    whole.run_sim(cmds); whole.solvePoseGraph()
    shard, cs = _hetero_handle(S, Ls, T, R, KP, B=4, offset=8)
    assert np.array_equal(cs, cmds[:, 8:12])
    shard.run_sim(cs); shard.solvePoseGraph()
    a, b = _snapshot(whole), _snapshot(shard)
    rows = dict(graphs=a["graphs"][8:12], conn=a["conn"][8:12], stats={k: v[8:12] for k, v in a["stats"].items()}, err=[e[8:12] for e in a["err"]])
    _same(rows, b, "instances 8..11 of 16 against the shard at offset 8")
    whole.close(); shard.close()


def test_marginals_of_two_scenarios(oracle):
    """marginals() on a heterogeneous batch: one instance of each of two scenarios against tests/pgs_marginals_reference.py at the device's
    result values, under that module's bar (the oracle graphs are rebuilt from the oracle runner's streams)."""
    import live_ekf_slam_amd as S
    import pgs_marginals_reference as MR
    import pgs_step_reference as R_
    Ls, T, R, KP = (8, 20, 8, 20), 65, 4, 8
    maps, counts, sc_cmds = _scenarios(Ls, T)
    pg, cmds = _hetero_handle(S, Ls, T, R, KP)
    pg.run_sim(cmds); pg.solvePoseGraph()
    pg.marginals(1)
    cfg = default_config()
    fails = []
    for s, b in ((0, 1), (1, 6)):
        r = _oracle_slices(Ls, T, R, KP, want_streams=True)[s]
        i = b - s * R
        assert r["cnt"].max() <= KP
        st = dict(cmds=sc_cmds[s], meas=r["meas"][i:i + 1], cnt=r["cnt"][i:i + 1], sec=r["pose_init"][i:i + 1, 1:])
        g = R_.build_oracle_graphs(oracle, cfg, st, T + 1, max(Ls), KP)[0]
        g1, m = pg.get_graph(b, 1), pg.get_marginals(b)
        j = MR.judge(g, g1["poses"], g1["landmarks"])
        assert "singular" not in j and m["status"] == 0, (b, m["status"])
        fom = MR.figure_of_merit(m["pose_cov"], m["lm_cov"], j["pose_cov"], j["lm_cov"])
        print(f"instance {b} (scenario {s}): N {j['N']} M {j['M']} figure {fom:.3g} spread {j['spread']:.3g} bar {j['bar']:.3g} bound {j['bound']:.3g}")
        if not fom <= j["bar"]:
            fails.append(f"instance {b}: figure {fom:.3g} above the bar {j['bar']:.3g}")
    pg.close()
    assert not fails, "; ".join(fails)


def test_errors_leave_the_handle_usable():
    """SLAM_ERR_STATE before an init and for the simulator calls without a map, SLAM_ERR_ARG for NULL or non-finite inputs, L[b] out of
    range and T <= 0 - and the handle then runs item 1's small case to the bits of a fresh one."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    ARG, STATE = -1, -4
    L, T, B, KP = 8, 33, 5, 8
    lm, cmds = make_scenario(155 + L, L, T)
    ref = _shared_run(S, lm, cmds, B, L, KP)
    lib = _lib.lib()
    fp, dp, ip = (lambda a: a.ctypes.data_as(C.POINTER(C.c_float))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_double))), (lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)))
    each = np.ascontiguousarray(np.broadcast_to(cmds[:, None, :], (T, B, 2)))
    bad_cmds = each.copy(); bad_cmds[3, 2, 1] = np.nan
    pose = np.zeros((B, 3), np.float32); bad_pose = pose.copy(); bad_pose[1, 2] = np.inf
    truth = np.zeros((B, 3)); bad_truth = truth.copy(); bad_truth[4, 0] = np.nan
    maps = np.ascontiguousarray(np.broadcast_to(lm, (B, L, 2))); bad_maps = maps.copy(); bad_maps[2, 1, 0] = np.nan
    cnt = np.full(B, L, np.int32); meas = np.zeros((B, 1, 3), np.float32); zero = np.zeros(B, np.int32)
    counts = np.zeros((B, 2), np.int32)
    pg = _pg(S, B, T, L, KP)
    h = pg.h
    # before an init
    assert lib.pgs_update_each(h, fp(each[0]), fp(meas), ip(zero), 1, None) == STATE
    assert lib.pgs_update_each_dev(h, fp(each[0]), None, None, 0, None) == STATE
    assert lib.pgs_run_sim_each(h, fp(each), T) == STATE
    assert lib.pgs_run_sim_every_iteration_each(h, fp(each), T, ip(counts)) == STATE
    # init_each
    assert lib.pgs_init_each(h, None, None) == ARG
    assert lib.pgs_init_each(h, fp(bad_pose), None) == ARG
    assert lib.pgs_init_each(h, fp(pose), dp(bad_truth)) == ARG
    assert lib.pgs_update_each(h, fp(each[0]), fp(meas), ip(zero), 1, None) == STATE     # a refused init is no init
    assert lib.pgs_init_each(h, fp(pose), dp(truth)) == 0
    # the simulator without a map
    assert lib.pgs_run_sim_each(h, fp(each), T) == STATE
    assert lib.pgs_run_sim_every_iteration_each(h, fp(each), T, ip(counts)) == STATE
    # set_maps
    assert lib.pgs_set_maps(h, None, ip(cnt), L) == ARG and lib.pgs_set_maps(h, dp(maps), None, L) == ARG
    assert lib.pgs_set_maps(h, dp(maps), ip(cnt), 0) == ARG and lib.pgs_set_maps(h, dp(maps), ip(cnt), 256) == ARG
    for k, v in ((0, 0), (B - 1, L + 1), (2, -3)):
        c = cnt.copy(); c[k] = v
        assert lib.pgs_set_maps(h, dp(maps), ip(c), L) == ARG
    assert lib.pgs_set_maps(h, dp(bad_maps), ip(cnt), L) == ARG
    assert lib.pgs_run_sim_each(h, fp(each), T) == STATE                                  # refused maps are no maps
    assert lib.pgs_set_maps(h, dp(maps), ip(cnt), L) == 0
    # commands
    assert lib.pgs_run_sim_each(h, None, T) == ARG and lib.pgs_run_sim_each(h, fp(each), 0) == ARG and lib.pgs_run_sim_each(h, fp(each), -2) == ARG
    assert lib.pgs_run_sim_each(h, fp(bad_cmds), T) == ARG
    assert lib.pgs_run_sim_every_iteration_each(h, None, T, None) == ARG and lib.pgs_run_sim_every_iteration_each(h, fp(each), 0, None) == ARG
    assert lib.pgs_run_sim_every_iteration_each(h, fp(bad_cmds), T, None) == ARG
    assert lib.pgs_update_each(h, None, fp(meas), ip(zero), 1, None) == ARG
    assert lib.pgs_update_each(h, fp(bad_cmds[3]), fp(meas), ip(zero), 1, None) == ARG
    assert lib.pgs_update_each(h, fp(each[0]), None, ip(zero), 1, None) == ARG and lib.pgs_update_each(h, fp(each[0]), fp(meas), ip(zero), -1, None) == ARG
    assert lib.pgs_update_each_dev(h, None, None, None, 0, None) == ARG
    assert lib.pgs_run_sim_each(h, fp(np.zeros((T + 1, B, 2), np.float32)), T + 1) == STATE     # beyond the pose capacity
    assert lib.pgs_timestep(h) == 0
    # ... and the handle runs the small case as if nothing had happened
    pg.set_seed(SEED)
    pg.run_sim(each); pg.solvePoseGraph()
    _same(ref, _snapshot(pg), "after the refused calls")
    pg.close()
