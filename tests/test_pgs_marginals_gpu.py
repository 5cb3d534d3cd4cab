"""Marginal covariances of the pose-graph solver on the device (pgs_marginals) against the extended-precision reference
(tests/pgs_marginals_reference.py).

Graphs are built through pgs_update from the host streams of tests/test_pgs_step_gpu.py's scenario table (its _device), solved with a
full solvePoseGraph(), then marginals(1); the reference is evaluated at the DEVICE's result values through the oracle graph's Jacobian.
Per instance the figure of merit is max over diagonal blocks of max|S - S_ref| / max|S_ref| and the bar 10 x the rounding spread of two
double routes on the CPU at the same values, never above the derived forward bound (pgs_marginals_reference.judge).  Every figure is
printed before it is asserted (pytest -s)."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import pgs_marginals_reference as MR
import pgs_step_reference as R
import test_pgs_step_gpu as T
from conftest import ROOT
from live_ekf_slam_amd.config import default_config
from live_ekf_slam_amd.scenario import make_scenario

pytestmark = pytest.mark.gpu

SMALL = [f"n{n}" for n in (2, 7, 8, 9, 31, 32, 33, 34)]
NAMES = ["ragged", "configs4", "ld512", "long", "ill", "fusable"] + SMALL
# The structurally singular instances of those scenarios (a landmark that was created but has no stored factor), evaluated on the CPU from
# the oracle graphs (test_pgs_marginals_reference.test_the_singular_instances_are_the_two_known_ones): the comparison leaves out these
# two instances and no other.
SINGULAR = {("n2", 4), ("fusable", 13)}


def _blocks_bits(m):
    return m["pose_cov"].tobytes(), m["lm_cov"].tobytes(), m["status"]


def _all_marginals(pg, B):
    return [pg.get_marginals(b) for b in range(B)]


@functools.lru_cache(maxsize=None)
def solved(name):
    """One device run of a scenario: solve, marginals at the result; per instance the result values, the blocks and the reference's
    verdict at those values."""
    sc = MR.scenario(name)
    pg = T._device(sc)
    B = len(sc["graphs"])
    pg.solvePoseGraph()
    pg.marginals()   # default: the result, as get_graph
    out = []
    for b in range(B):
        gr = pg.get_graph(b, 1)
        out.append((gr, pg.get_marginals(b), MR.judge(sc["graphs"][b], gr["poses"], gr["landmarks"])))
    flop, ms = pg.last_marginals_work()
    stats = pg.stats()
    pg.close()
    return dict(inst=out, flop=flop, ms=ms, stats=stats)


def _check_instance(tag, m, j):
    """Status and figure of merit of one instance against its verdict; returns (line to print, failure or None)."""
    if "singular" in j:
        ok = m["status"] == 1 and np.isnan(m["pose_cov"]).all() and np.isnan(m["lm_cov"]).all()
        return f"{tag}: singular (landmarks {j['singular'].tolist()} without a factor), status {m['status']}", None if ok else f"{tag}: singular graph, status {m['status']}"
    fom = MR.figure_of_merit(m["pose_cov"], m["lm_cov"], j["pose_cov"], j["lm_cov"])
    line = (f"{tag}: N {j['N']} M {j['M']} figure {fom:.3g} spread {j['spread']:.3g} (chol {j['spread_chol']:.3g}, lu {j['spread_lu']:.3g}) "
            f"figure/spread {fom / j['spread']:.2f} bar {j['bar']:.3g} bound {j['bound']:.3g} kappa_1 {j['kappa']:.3g} ref corr {j['last_correction']:.2g}")
    bad = None
    if m["status"] != 0:
        bad = f"{tag}: status {m['status']} on a regular graph"
    elif not fom <= j["bar"]:
        bad = f"{tag}: figure {fom:.3g} above the bar {j['bar']:.3g} (spread {j['spread']:.3g})"
    return line, bad


@pytest.mark.parametrize("name", NAMES)
def test_every_instance_within_the_bar_at_the_result(name):
    """Test 3: every instance of the scenario; the singular ones - predicted on the CPU from the oracle graph - have status 1 and NaN
    blocks, and the device's status vector equals the prediction exactly."""
    run = solved(name)
    fails, predicted, status = [], set(), []
    for b, (gr, m, j) in enumerate(run["inst"]):
        line, bad = _check_instance(f"{name}[{b}]", m, j)
        print(line)
        if bad:
            fails.append(bad)
        if "singular" in j:
            predicted.add(b)
        status.append(m["status"])
    print(f"{name}: marginals of {len(status)} instances {run['ms']:.3f} ms, model {run['flop']:.4g} FLOP")
    assert predicted == {b for s, b in SINGULAR if s == name}, (name, predicted)
    assert [int(b in predicted) for b in range(len(status))] == status, (name, status)
    assert not fails, "; ".join(fails)


def test_the_comparison_leaves_out_exactly_two_instances():
    """Of all instances test 3 runs, exactly two are structurally singular (a scenario change cannot quietly turn the comparison off)."""
    n = sum(1 for name in NAMES for (_, _, j) in solved(name)["inst"] if "singular" in j)
    total = sum(len(solved(name)["inst"]) for name in NAMES)
    print(f"{n} singular of {total} instances")
    assert n == 2 and n == len(SINGULAR)


def test_marginals_at_the_initial_estimate():
    """Test 4: which = 0 on `ragged`, before any solve; the device's initial estimate is the oracle's bit for bit."""
    sc = MR.scenario("ragged")
    pg = T._device(sc)
    with pytest.raises(Exception, match="no result yet"):
        pg.marginals(1)
    pg.marginals(0)
    fails = []
    for b, g in enumerate(sc["graphs"]):
        v = g.values(0)
        g0 = pg.get_graph(b, 0)
        assert np.array_equal(g0["poses"], v["poses"]) and np.array_equal(g0["landmarks"], v["landmarks"])
        line, bad = _check_instance(f"ragged[{b}] initial", pg.get_marginals(b), MR.judged_at_initial("ragged", b))
        print(line)
        if bad:
            fails.append(bad)
    pg.close()
    assert not fails, "; ".join(fails)


@pytest.mark.parametrize("name", NAMES)
def test_invariants_of_every_block(name):
    """Test 5: exactly symmetric, positive definite, and pose_cov[0] below the prior's covariance diag(1.3^2, 1.3^2, 1.2^2) up to the bar
    (information only adds)."""
    prior = np.diag(np.square(MR.PRIOR_SIGMAS))
    for b, (gr, m, j) in enumerate(solved(name)["inst"]):
        if "singular" in j:
            continue
        for blocks in (m["pose_cov"], m["lm_cov"]):
            assert np.array_equal(blocks, np.swapaxes(blocks, 1, 2)), (name, b)
            if blocks.shape[0]:
                assert np.linalg.eigvalsh(blocks).min() > 0.0, (name, b)
        gap = np.linalg.eigvalsh(prior - m["pose_cov"][0]).min()
        print(f"{name}[{b}]: smallest eigenvalue of prior - pose_cov[0] {gap:.3g}")
        assert gap >= -j["bar"] * prior.max(), (name, b, gap)


def test_determinism_isolation_and_chunks(monkeypatch):
    """Test 6: the call twice gives bit-identical buffers; an instance of the 17-instance `ragged` batch equals the same graph computed
    alone in a batch of 1; a chunked run equals the unchunked one.  (At the initial estimate, which graph building leaves bit-identical
    whatever the batch; a solve's launch shape follows the batch size.)"""
    sc = MR.scenario("ragged")
    B = len(sc["graphs"])
    pg = T._device(sc)
    pg.marginals(0)
    first = [_blocks_bits(m) for m in _all_marginals(pg, B)]
    pg.marginals(0)
    assert first == [_blocks_bits(m) for m in _all_marginals(pg, B)]
    pg.solvePoseGraph(); pg.marginals(1)
    res1 = [_blocks_bits(m) for m in _all_marginals(pg, B)]
    pg.marginals(1)
    assert res1 == [_blocks_bits(m) for m in _all_marginals(pg, B)]
    monkeypatch.setenv("SLAM_PGS_MARG_CHUNK", "5")
    pg.marginals(1)
    assert res1 == [_blocks_bits(m) for m in _all_marginals(pg, B)], "chunks of 5 instances"
    pg.marginals(0)
    assert first == [_blocks_bits(m) for m in _all_marginals(pg, B)], "chunks of 5 instances, initial estimate"
    monkeypatch.delenv("SLAM_PGS_MARG_CHUNK")
    pg.close()
    for b in (0, 5, 16):
        st = sc["st"]
        one = dict(sc, st=dict(cmds=st["cmds"], meas=st["meas"][b:b + 1], cnt=st["cnt"][b:b + 1], sec=st["sec"][b:b + 1]))
        p1 = T._device(one)
        p1.marginals(0)
        assert _blocks_bits(p1.get_marginals(0)) == first[b], f"instance {b} alone"
        p1.close()


def test_nothing_else_moves(monkeypatch):
    """Test 7: get_graph, stats() and a second solve after marginals() are bit-identical to the same sequence without the call;
    get_marginals after a following update / solve / adopt_result raises."""
    sc = MR.scenario("ragged")
    B = len(sc["graphs"])

    def snapshot(pg):
        st = pg.stats()
        return ([(g["poses"].tobytes(), g["landmarks"].tobytes()) for g in (pg.get_graph(b, w) for b in range(B) for w in (0, 1))],
                {k: v.tobytes() for k, v in st.items()})

    seqs = []
    for with_call in (False, True):
        pg = T._device(sc)
        if with_call:
            pg.marginals(0)
        pg.solvePoseGraph()
        if with_call:
            pg.marginals(1)
        a = snapshot(pg)
        pg.solvePoseGraph()
        c = snapshot(pg)
        seqs.append((a, c))
        if with_call:
            pg.marginals(1); pg.get_marginals(0)
            pg.solvePoseGraph()
            with pytest.raises(Exception, match="no marginals"):
                pg.get_marginals(0)
            pg.marginals(1); pg.get_marginals(0)
            pg.adopt_result()
            with pytest.raises(Exception, match="no marginals"):
                pg.marginalCovariance(0, pose=0)
            with pytest.raises(Exception, match="which"):
                pg.marginals(2)
            pg.marginals(0)
            with pytest.raises(Exception, match="out of range"):
                pg.get_marginals(B)
            with pytest.raises(IndexError):
                pg.marginalCovariance(0, pose=sc["N"])
            assert pg.marginalCovariance(3, landmark=0).shape == (2, 2) and pg.marginalCovariance(3, pose=sc["N"] - 1).shape == (3, 3)
        pg.close()
    assert seqs[0] == seqs[1]
    import live_ekf_slam_amd as S
    pg = S.BatchedPoseGraph(2, num_iterations=10, L_max=4, k_per_pose=4).readParams(default_config())
    pg.init(0.0, 0.0, 0.0)
    with pytest.raises(Exception, match="no marginals"):
        pg.get_marginals(0)
    meas = np.array([[7, 2.0, 0.3]], dtype=np.float32)
    pg.update(np.array([0.1, 0.0], dtype=np.float32), meas)
    pg.marginals(0); assert pg.get_marginals(1)["status"] == 0
    pg.update(np.array([0.1, 0.0], dtype=np.float32), meas)
    with pytest.raises(Exception, match="no marginals"):
        pg.get_marginals(1)
    pg.init(0.0, 0.0, 0.0)
    with pytest.raises(Exception, match="no result yet"):
        pg.marginals(1)
    pg.close()


def test_run_sim_at_the_baseline_shape(oracle):
    """Test 8: pgs_run_sim at BASELINE configs[4] shape (batch 64, 1000 poses x 200 landmarks, k_per_pose 32): status 0 everywhere, three
    instances against the reference (their oracle graphs rebuilt from the oracle runner's streams of the same noise streams)."""
    import live_ekf_slam_amd as S
    L, Tn, B, KP, seed = 200, 999, 64, 32, 11
    lm, cmds = make_scenario(321 + L, L, Tn)
    cfg = default_config()
    pg = S.BatchedPoseGraph(B, num_iterations=Tn + 1, L_max=L, k_per_pose=KP).readParams(cfg)
    pg.set_map(lm); pg.set_seed(seed); pg.init(0.0, 0.0, 0.0)
    pg.run_sim(cmds)
    pg.solvePoseGraph()
    pg.marginals(1)
    flop, ms = pg.last_marginals_work()
    print(f"batch {B}, 1000 x 200: marginals {ms:.2f} ms, model {flop:.4g} FLOP")
    status = [pg.get_marginals(b)["status"] for b in range(B)]
    assert status == [0] * B, status
    fails = []
    for b in (0, 31, 63):
        r = oracle.run_pgs_batch(lm, cmds, 1, L, KP=KP, seed=seed, inst0=b, cfg=cfg, want_streams=True)
        assert r["cnt"].max() <= KP
        st = dict(cmds=np.ascontiguousarray(cmds, dtype=np.float32), meas=r["meas"], cnt=r["cnt"], sec=r["pose_init"][:, 1:])
        g = R.build_oracle_graphs(oracle, cfg, st, Tn + 1, L, KP)[0]
        v, g0, g1 = g.values(0), pg.get_graph(b, 0), pg.get_graph(b, 1)
        assert g0["M"] == v["M"] and np.array_equal(g0["poses"], v["poses"]) and np.array_equal(g0["landmarks"], v["landmarks"]), b
        line, bad = _check_instance(f"run_sim[{b}]", pg.get_marginals(b), MR.judge(g, g1["poses"], g1["landmarks"]))
        print(line)
        if bad:
            fails.append(bad)
    pg.close()
    assert not fails, "; ".join(fails)


def test_cpp_mirror_marginal_covariance(oracle, tmp_path):
    """Test 9: BatchedPoseGraph::marginals / marginalCovariance / landmarkCovariance of include/slam_filter.hpp through the C++ driver
    (`filter_driver pose_graph ... dump`): the blocks of its first and last instance against the reference at the driver's own result
    values, on the oracle graph of the driver's messages (the Jacobian depends on the factors, not on the secondary filter's poses)."""
    exe = os.path.join(ROOT, "live_ekf_slam_amd", "filter_driver")
    assert os.path.exists(exe), "build the extension first (__graft_entry__.build())"
    B, L, Tn = 8, 10, 90
    dump = str(tmp_path / "marg.bin")
    out = subprocess.run([exe, "pose_graph", str(B), str(L), str(Tn), dump], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "marginals dumped" in out.stdout, out.stderr + out.stdout
    assert re.search(r"poses=90 solved=1", out.stdout), out.stdout
    # the driver's messages (filter_driver.cpp run_pose_graph): updates 0 .. Tn - 2 build the graph, the last tick solves
    import live_ekf_slam_amd as S
    _, cmds = make_scenario(7, L, Tn)
    cfg = default_config()
    g = oracle.OraclePoseGraph(cfg, N_max=Tn, L_max=L, KP=8)
    naive = S.NaiveFilter()
    g.init(0.0, 0.0, 0.0); naive.init(0.0, 0.0, 0.0)
    for t in range(Tn - 1):
        naive.update(cmds[t])
        g.updateNaiveVehPoseEstimate(naive.getStateVector())
        meas = np.array([[t // 30, np.float32(2.0) + np.float32(0.01) * np.float32(t % 7), np.float32(0.3) - np.float32(0.01) * np.float32(t % 5)]],
                        dtype=np.float32) if t % 3 == 0 else np.zeros((0, 3), dtype=np.float32)
        g.update(cmds[t, 0], cmds[t, 1], meas)
    raw = open(dump, "rb").read()
    off, fails = 0, []
    for inst in (0, B - 1):
        N, M = (int(v) for v in np.frombuffer(raw, np.int64, 2, off)); off += 16
        assert N == Tn and M == g.values(0)["M"] == 3
        poses = np.frombuffer(raw, np.float64, 3 * N, off).reshape(N, 3); off += 24 * N
        lms = np.frombuffer(raw, np.float64, 2 * M, off).reshape(M, 2); off += 16 * M
        pc = np.frombuffer(raw, np.float64, 9 * N, off).reshape(N, 3, 3); off += 72 * N
        lc = np.frombuffer(raw, np.float64, 4 * M, off).reshape(M, 2, 2); off += 32 * M
        line, bad = _check_instance(f"C++ mirror[{inst}]", dict(pose_cov=pc, lm_cov=lc, status=0), MR.judge(g, poses, lms))
        print(line)
        if bad:
            fails.append(bad)
    assert off == len(raw)
    assert not fails, "; ".join(fails)
