"""Absolute fixes (unary position / heading factors) of the pose graph on the device, against tests/pgs_fix_reference.py.

Graphs are built through pgs_update from the streams of tests/test_pgs_step_gpu.py's scenario table, with pgs_fix called as the graph grows:
fixes sit at pose 0 (with the prior), at separators of the solve path's segmentation, at segment-interior poses and at the last pose,
position-only, heading-only and both, and the last instance of every batch carries none.  One LM step on every solve path against the
extended-precision reference of the system with the appended rows; no fixes is the same code, byte for byte; whole solves against the dense
Python LM; the fix weights; the marginals; the simulated source; pgs_run_sim_fix against the loop of single calls; the every-iteration mode;
what fixes are for; and a graph that follows an EKF handle on the device."""
import ctypes as C
import functools

import numpy as np
import pytest

import pgs_fix_reference as F
import pgs_marginals_reference as MR
import pgs_robust_reference as RR
import pgs_step_reference as R
import test_pgs_step_gpu as T
from test_gate_gpu import _Dev
from test_pgs_robust_gpu import POSE_TOL, SOLVE_CASES, STEP_CASES, _bits, _Env

pytestmark = pytest.mark.gpu

FIX_LOSSES = {"gauss": (F.NONE, 0.0), "huber": (F.HUBER, 1.345), "gm": (F.GEMAN_MCCLURE, 3.0)}
LM_LOSSES = {"plain": (RR.NONE, 0.0), "lmhuber": (RR.HUBER, 1.345)}


def _device(sc, fix=None, kinds=None):
    """The handle of test_pgs_step_gpu._device with pgs_fix called for every pose that carries a fix, as the graph grows.  Returns (handle,
    verdicts per call)."""
    import live_ekf_slam_amd as S
    st = sc["st"]
    B, Tn = st["cnt"].shape
    pg = S.BatchedPoseGraph(B, num_iterations=sc["N"], L_max=sc["L_max"], k_per_pose=sc["KP"]).readParams(sc["cfg"])
    pg.init(0.0, 0.0, 0.0)
    verdicts = {}
    for i in range(Tn + 1):
        if i:
            pg.updateNaiveVehPoseEstimate(st["sec"][:, i - 1])
            pg.update(st["cmds"][i - 1], st["meas"][:, i - 1], st["cnt"][:, i - 1])
        if kinds is not None and kinds[:, i].any():
            verdicts[i] = pg.fix(fix[:, i], kinds[:, i])
    assert pg.timestep == sc["N"] - 1
    return pg, verdicts


def _expected_verdicts(kinds_col):
    return np.array([(F.STORED if k & 1 else 0) | ((F.STORED if k & 2 else 0) << 4) for k in kinds_col], dtype=np.int32)


@functools.lru_cache(maxsize=None)
def step_reference(name, path, loss):
    sc = F.case(name)
    fix, kinds = F.place_fixes(sc, path)
    refs = []
    for b, g in enumerate(sc["graphs"]):
        v = g.values(0)
        fg = F.FixGraph(g, fix[b], kinds[b], fix_loss=FIX_LOSSES[loss])
        S, W = F.system(fg, v["poses"], v["landmarks"], T.LAM0)
        d_ref, kappa, _ = R.reference_step(S)
        refs.append((v, S, W, d_ref, kappa, F.lm_solve(fg, max_trials=1), R.factor_pairs(g, v["poses"], v["landmarks"])))
    return fix, kinds, refs


@pytest.mark.parametrize("loss", ["gauss", "huber"])
@pytest.mark.parametrize("name,path", STEP_CASES, ids=[f"{n}-{p}" for n, p in STEP_CASES])
def test_one_lm_step_with_fixes_against_the_extended_precision_reference(name, path, loss):
    """Test 1.  The bounds of test_pgs_robust_gpu.py (eta <= 8 n u + eta_rec; forward with kappa_1) against the system with the appended
    fix rows, on every path.  A build that stored fixes but missed a solve path's linearisation would solve the oracle's system instead:
    the premise below says that step lies outside the forward bound."""
    sc = F.case(name)
    fix, kinds, refs = step_reference(name, path, loss)
    assert not kinds[-1].any() and kinds[:-1].any(axis=1).all()      # one instance carries none, every other some
    assert {int(k) for k in np.unique(kinds)} >= ({0, 1, 2, 3} if sc["N"] > 2 else {0, 1, 2})
    with _Env(path, {"SLAM_PGS_MAX_TRIALS": "1"}):
        pg, verdicts = _device(sc, fix, kinds)
        pg.set_fix_robust(*FIX_LOSSES[loss])
        assert pg.fix_robust == FIX_LOSSES[loss]
        B = len(refs)
        runs = []
        for _ in range(2):
            pg.solvePoseGraph()
            runs.append(_bits(pg, B))
        res = [pg.get_graph(b, 1) for b in range(B)]
        st = pg.stats()
        plan = pg.last_solve_paths()
        stored = [pg.fixes(b) for b in range(B)]
        pg.close()
    for i, v in verdicts.items():
        assert np.array_equal(v, _expected_verdicts(kinds[:, i])), (i, v)
    for b in range(B):   # pgs_get_fixes round-trips the rows
        assert np.array_equal(stored[b]["kinds"], kinds[b]) and stored[b]["fix"].tobytes() == fix[b].tobytes(), (name, b)
    assert runs[0] == runs[1], "the same solve twice differs"
    assert np.all(st["trials"] == 1)
    fused = T.SEG[path].get("SLAM_PGS_FUSED")
    if fused in ("2", "3", "4") and max(sc["Ms"]) <= 176:
        assert plan["flop_fused"] > 0 and plan["flop_separate"] == 0, plan
    want = 0 if T.SEG[path].get("SLAM_PGS_SEG") == "0" else R.predict_plan([r[6] for r in refs], sc["N"], int(T.SEG[path].get("SLAM_PGS_SEG", "32")))
    assert (plan["segment_length"] if plan["segmented"] else 0) == want, (plan, want)   # the path the case names really ran
    fails, accepted = [], 0
    for b, (v, S, W, d_ref, kappa, first, _) in enumerate(refs):
        assert st["iterations"][b] == first["iterations"], f"{name}/{path}/{loss} instance {b}: device accepted {st['iterations'][b]}, reference {first['iterations']}"
        assert first["margin"] >= 1e-6, (name, b, first["margin"])
        if not first["iterations"]:
            assert np.array_equal(res[b]["poses"], v["poses"]) and np.array_equal(res[b]["landmarks"], v["landmarks"]), (name, b)
            continue
        accepted += 1
        delta, eps = R.recover_step(v["poses"], v["landmarks"], res[b]["poses"], res[b]["landmarks"])
        eta = S.eta(delta)
        bound = R.BOUND_C * S.n * R.U + S.eta_of_error(eps, delta)
        dref = np.asarray(d_ref, dtype=np.float64)
        fwd = float(np.abs(delta - dref).max(initial=0.0))
        fbound = R.BOUND_C * S.n * R.U * kappa * float(np.abs(dref).max(initial=0.0)) + float(eps.max(initial=0.0))
        if kinds[b].any():   # premise: without the fix rows the step is another one
            d_plain = np.asarray(R.reference_step(R.system_of(sc["graphs"][b], v["poses"], v["landmarks"], T.LAM0))[0], dtype=np.float64)
            assert float(np.abs(d_plain - dref).max()) > fbound, (name, b)
        print(f"{name}/{path}/{loss}[{b}]: n {S.n} eta {eta:.3g} bound {bound:.3g}; |d_dev - d_ref| {fwd:.3g} bound {fbound:.3g}; kappa_1 {kappa:.3g}")
        if not (eta <= bound and fwd <= fbound):
            fails.append(f"instance {b} (n {S.n}): eta {eta:.3g} vs {bound:.3g}; |d_dev - d_ref| {fwd:.3g} vs {fbound:.3g}; kappa_1 {kappa:.3g}")
    assert accepted > 0, "no instance accepted its first trial: the step was not compared"
    assert not fails, f"{name}/{path}/{loss}: " + "; ".join(fails[:8])


@pytest.mark.parametrize("name,path", [("n34", "default"), ("ragged", "chain_fused3_list1")])
def test_no_fixes_is_the_same_code(name, path):
    """Test 2.  A handle that never calls the new interface (today's behaviour), one with pgs_set_fix_robust alone, and one whose only
    pgs_fix carries kinds 0 everywhere (it allocates the arrays and runs the kernels built with fixes, on no stored part): results, every
    array of the statistics and the marginals, byte for byte."""
    sc = F.case(name)
    B, N = len(sc["graphs"]), sc["N"]
    seen = []
    for setting in ("untouched", "loss only", "empty fix"):
        with _Env(path):
            pg, _ = _device(sc)
            if setting == "loss only":
                pg.set_fix_robust(F.GEMAN_MCCLURE, 3.0)
            if setting == "empty fix":
                v = pg.fix(np.full((B, 5), 7.0), np.zeros(B, dtype=np.int32))
                assert not v.any()
                pg.set_fix_robust(F.HUBER, 1.345)
            pg.solvePoseGraph()
            bits = _bits(pg, B)
            pg.marginals(1)
            for b in range(B):
                m = pg.get_marginals(b)
                bits += [m["pose_cov"].tobytes(), m["lm_cov"].tobytes(), bytes([m["status"]])]
            assert not pg.fixes(0)["kinds"].any() and np.isnan(pg.fix_weights(1)).all()
            assert pg.fix_weights(1).shape == (B, N, 2)
            pg.close()
        seen.append(bits)
    assert seen[0] == seen[1], "pgs_set_fix_robust on a handle without fixes changed a result"
    assert seen[0] == seen[2], "the kernels built with fixes differ on a graph that stores none"


@functools.lru_cache(maxsize=None)
def solve_reference(name, loss, lm):
    """The Python LM of every instance with the placement fixes, with pgs_robust_gpu's fairness checks."""
    sc = F.case(name)
    fix, kinds = F.place_fixes(sc, "seg5")
    out = []
    for b, g in enumerate(sc["graphs"]):
        fg = F.FixGraph(g, fix[b], kinds[b], fix_loss=FIX_LOSSES[loss], lm_loss=LM_LOSSES[lm])
        a, q = F.lm_solve(fg, "chol"), F.lm_solve(fg, "qr")
        assert a["margin"] >= 1e-6, (name, loss, lm, b, a["margin"])
        assert (a["iterations"], a["trials"]) == (q["iterations"], q["trials"]), (name, loss, lm, b)
        moved = max(float(np.abs(a["poses"] - q["poses"]).max()), float(np.abs(a["landmarks"] - q["landmarks"]).max(initial=0.0)))
        assert moved < 1e-8, (name, loss, lm, b, moved)
        assert a["flags"] == 0, (name, loss, lm, b)
        out.append((fg, a))
    return fix, kinds, out


@functools.lru_cache(maxsize=None)
def solved(name, path, loss, lm):
    sc = F.case(name)
    fix, kinds, _ = solve_reference(name, loss, lm)
    B = len(sc["graphs"])
    with _Env(path):
        pg, _ = _device(sc, fix, kinds)
        pg.set_fix_robust(*FIX_LOSSES[loss])
        pg.set_robust(*LM_LOSSES[lm])
        pg.solvePoseGraph()
        res = [pg.get_graph(b, 1) for b in range(B)]
        before = _bits(pg, B)
        w = pg.fix_weights(1)
        after = _bits(pg, B)
        st = pg.stats()
        pg.close()
    return dict(res=res, stats=st, w=w, before=before, after=after)


@pytest.mark.parametrize("lm", list(LM_LOSSES))
@pytest.mark.parametrize("loss", ["huber", "gm"])
@pytest.mark.parametrize("name,path", SOLVE_CASES, ids=[f"{n}-{p}" for n, p in SOLVE_CASES])
def test_whole_solves_with_fixes_against_the_python_lm(name, path, loss, lm):
    """Test 3.  Iteration and trial counts equal, results within POSE_TOL, no flag.  (The same fixes - seg5's placement - on every path.)"""
    _, kinds, ref = solve_reference(name, loss, lm)
    run = solved(name, path, loss, lm)
    st = run["stats"]
    assert np.all(st["flags"] == 0), st["flags"]
    for b, (_, a) in enumerate(ref):
        print(f"{name}/{path}/{loss}/{lm}[{b}]: device {st['iterations'][b]} iterations / {st['trials'][b]} trials, reference {a['iterations']} / {a['trials']}; "
              f"cost {st['err_init'][b]:.6g} -> {st['err_final'][b]:.6g} (reference {a['err_init']:.6g} -> {a['err_final']:.6g})")
    for b, (_, a) in enumerate(ref):
        assert (st["iterations"][b], st["trials"][b]) == (a["iterations"], a["trials"]), (name, path, loss, lm, b)
        d = max(float(np.abs(run["res"][b]["poses"] - a["poses"]).max()), float(np.abs(run["res"][b]["landmarks"] - a["landmarks"]).max(initial=0.0)))
        assert d <= POSE_TOL, (name, path, loss, lm, b, d)
        assert abs(st["err_final"][b] - a["err_final"]) <= 1e-9 * max(a["err_final"], 1e-12) + 1e-12, (b, st["err_final"][b], a["err_final"])
        assert abs(st["err_init"][b] - a["err_init"]) <= 1e-9 * max(a["err_init"], 1e-12) + 1e-12, (b, st["err_init"][b], a["err_init"])


@pytest.mark.parametrize("loss", ["gauss", "huber", "gm"])
@pytest.mark.parametrize("name,path", SOLVE_CASES[:3], ids=[f"{n}-{p}" for n, p in SOLVE_CASES[:3]])
def test_fix_weights_at_the_result(name, path, loss):
    """Test 4.  Against the reference's w from the reference's residuals at the DEVICE's result: relative difference at most 8 u; NaN where
    no part is stored; exactly 1.0 without a fix loss; the handle's results untouched by the call."""
    sc = F.case(name)
    fix, kinds, ref = solve_reference(name, loss, "plain")
    run = solved(name, path, loss, "plain")
    assert run["before"] == run["after"], "pgs_fix_weights changed a result or a statistic"
    for b, (fg, _) in enumerate(ref):
        w = run["w"][b]
        stored = np.stack([(kinds[b] & 1) > 0, (kinds[b] & 2) > 0], axis=1)
        assert np.isnan(w[~stored]).all() and not np.isnan(w[stored]).any(), (name, b)
        if loss == "gauss":
            assert np.all(w[stored] == 1.0)
            continue
        want = fg.weigh(run["res"][b]["poses"], run["res"][b]["landmarks"])["fix_w"]
        assert np.array_equal(np.isnan(want), ~stored)
        rel = np.abs(w[stored] - want[stored]) / want[stored]
        print(f"{name}/{path}/{loss}[{b}]: {int(stored.sum())} parts, w in [{w[stored].min(initial=1.0):.3g}, 1], largest relative difference {rel.max(initial=0.0) / R.U:.2f} u")
        assert np.all(rel <= 8 * R.U), (name, b, rel.max())
    assert sc["N"] == run["w"].shape[1]


def test_marginals_with_fixes():
    """Test 5.  pgs_marginals(1) on n34 with the placement fixes (Huber on them) against pgs_marginals_reference.judge fed the graph with
    the appended rows at the device's result, at test_pgs_marginals_gpu.py's bar; and at the initial estimate - the same values with and
    without the fixes - a pose with a position part has a strictly smaller position variance than in the graph without it."""
    sc = F.case("n34")
    fix, kinds = F.place_fixes(sc, "default")
    pg, _ = _device(sc, fix, kinds)
    pg.set_fix_robust(F.HUBER, 1.345)
    pg.solvePoseGraph()
    pg.marginals(1)
    fails = []
    for b, g in enumerate(sc["graphs"]):
        gr, m = pg.get_graph(b, 1), pg.get_marginals(b)
        j = MR.judge(F.FixGraph(g, fix[b], kinds[b], fix_loss=(F.HUBER, 1.345)), gr["poses"], gr["landmarks"])
        assert "singular" not in j and m["status"] == 0, (b, m["status"])
        fom = MR.figure_of_merit(m["pose_cov"], m["lm_cov"], j["pose_cov"], j["lm_cov"])
        print(f"n34[{b}] with fixes: figure {fom:.3g} spread {j['spread']:.3g} bar {j['bar']:.3g} bound {j['bound']:.3g} kappa_1 {j['kappa']:.3g}")
        if not fom <= j["bar"]:
            fails.append(f"instance {b}: figure {fom:.3g} above the bar {j['bar']:.3g}")
        if kinds[b].any():   # and they are not the graph's without fixes: that one fails the same bar
            plain = MR.judge(g, gr["poses"], gr["landmarks"])
            assert MR.figure_of_merit(m["pose_cov"], m["lm_cov"], plain["pose_cov"], plain["lm_cov"]) > j["bar"], b
    pg.marginals(0)
    with_fix = [pg.get_marginals(b)["pose_cov"] for b in range(len(sc["graphs"]))]
    pg.close()
    pg0, _ = _device(sc)
    pg0.marginals(0)
    hit = 0
    for b in range(len(sc["graphs"])):
        without = pg0.get_marginals(b)["pose_cov"]
        for i in np.flatnonzero(kinds[b] & 1):
            hit += 1
            assert with_fix[b][i, 0, 0] + with_fix[b][i, 1, 1] < without[i, 0, 0] + without[i, 1, 1], (b, i)
        if not kinds[b].any():
            assert with_fix[b].tobytes() == without.tobytes(), b
    pg0.close()
    assert hit >= 8
    assert not fails, "; ".join(fails)


def _sim_handle(B, L, Tmax, seed=5, scenario=905, each=False):
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(scenario, L, Tmax)
    pg = S.BatchedPoseGraph(B, num_iterations=Tmax + 1, L_max=L, k_per_pose=8).readParams()
    pg.set_map(lm); pg.set_seed(seed); pg.init(0.0, 0.0, 0.0)
    if each:
        cmds = np.ascontiguousarray(np.tile(cmds[:, None, :], (1, B, 1)) * (1.0 + 0.01 * np.arange(B))[None, :, None], dtype=np.float32)
    return pg, lm, cmds


def _sensor_rows(B):
    from live_ekf_slam_amd.config import default_fix_sensor_config as Rw
    rows = [Rw(pos_halfwidth=0.05, yaw_halfwidth=0.02, sigma_pos=0.1, sigma_yaw=0.05, kinds=3),
            Rw(pos_halfwidth=0.05, yaw_halfwidth=0.02, sigma_pos=0.1, sigma_yaw=0.05, kinds=3, p_miss_pos=1.0),     # a missed part
            Rw(pos_halfwidth=0.05, yaw_halfwidth=0.02, sigma_pos=0.1, sigma_yaw=0.05, kinds=3, p_miss_yaw=1.0),
            Rw(pos_halfwidth=0.05, sigma_pos=0.1, kinds=1, p_jump=1.0, jump_lo=1.0, jump_hi=3.0),                     # a jump
            Rw(),                                                                                                     # the all-zero row
            Rw(yaw_halfwidth=0.02, sigma_yaw=0.05, kinds=2),
            Rw(pos_halfwidth=0.05, yaw_halfwidth=0.02, sigma_pos=0.1, sigma_yaw=0.05, kinds=3, p_jump=0.5, jump_lo=1.0, jump_hi=3.0, p_miss_pos=0.3)]
    return [rows[b % len(rows)] for b in range(B)]


def test_the_simulated_source_is_the_ekf_batchs_and_advances_nothing():
    """Test 6.  pgs_fix_sense equals slam_fix_sense_instance_host bit for bit for every instance - the truth from the oracle's simulator
    stepped with the same seed -, a missed part, a jump and the all-zero row among them; and the truth and the RNG step are untouched: a
    following pgs_run_sim gives the bytes it gives without the sense."""
    from live_ekf_slam_amd.filters import fix_sense_instance_host
    from oracle import oracle as O
    B, L, Tn, seed, inst0 = 9, 17, 8, 5, 3
    rows = _sensor_rows(B)
    a, lm, cmds = _sim_handle(B, L, Tn, seed)
    a.set_instance_offset(inst0)
    a.set_fix_sensor(rows)
    a.run_sim(cmds[:5])
    s = a.fix_sense()
    s2 = a.fix_sense()
    assert all(s[k].tobytes() == s2[k].tobytes() for k in s), "two emissions at the same tick differ: the source advanced something"
    seen = set()
    for b in range(B):
        sim = O.OracleSim(lm)
        for t in range(5):
            truth, _ = sim.step_philox(cmds[t, 0], cmds[t, 1], seed, inst0 + b, t)
        want = fix_sense_instance_host(seed, inst0 + b, 5, truth, rows[b])
        assert s["fix"][b].tobytes() == want["fix"].tobytes() and s["kinds"][b] == want["kinds"] and s["jumped"][b] == want["jumped"], (b, s["fix"][b], want)
        seen.add((int(want["kinds"]), int(want["jumped"])))
    assert {(3, 0), (2, 0), (1, 0), (1, 1), (0, 0)} <= seen, seen
    a.run_sim(cmds[5:])
    c, _, _ = _sim_handle(B, L, Tn, seed)
    c.set_instance_offset(inst0)
    c.run_sim(cmds)
    for b in range(B):
        ga, gc = a.get_graph(b, 0), c.get_graph(b, 0)
        assert ga["poses"].tobytes() == gc["poses"].tobytes() and ga["landmarks"].tobytes() == gc["landmarks"].tobytes(), b
    assert a.error_stats(0).tobytes() == c.error_stats(0).tobytes()
    # the all-zero rows emit nothing
    a.set_fix_sensor(None)
    z = a.fix_sense()
    assert not z["kinds"].any() and not z["fix"].any() and not z["jumped"].any()
    a.close(); c.close()


def _graph_bits(pg, B):
    out = []
    for b in range(B):
        g, fx = pg.get_graph(b, 0), pg.fixes(b)
        out += [g["poses"].tobytes(), g["landmarks"].tobytes(), fx["fix"].tobytes(), fx["kinds"].tobytes(), pg.connections(b).tobytes()]
    return out


@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("fix_every", [1, 3, 20])
def test_run_sim_fix_is_the_loop_of_the_single_calls(each, fix_every):
    """Test 7.  pgs_run_sim_fix = chunks of pgs_run_sim[_each], pgs_fix_sense, pgs_fix: the graphs, the stored fixes and the solve, byte for
    byte; fix_every = 20 > T attaches nothing."""
    B, L, Tn = 9, 17, 8
    a, _, cmds = _sim_handle(B, L, Tn, each=each)
    a.set_fix_sensor(_sensor_rows(B))
    a.run_sim_fix(cmds, fix_every)
    h, _, _ = _sim_handle(B, L, Tn, each=each)
    h.set_fix_sensor(_sensor_rows(B))
    t = 0
    while t < Tn:
        n = min(fix_every - t % fix_every, Tn - t)
        h.run_sim(cmds[t:t + n])
        t += n
        if t % fix_every == 0:
            s = h.fix_sense()
            h.fix(s["fix"], s["kinds"])
    assert a.timestep == h.timestep == Tn
    assert _graph_bits(a, B) == _graph_bits(h, B)
    stored = sum(int(a.fixes(b)["kinds"].astype(bool).sum()) for b in range(B))
    assert (stored > 0) == (fix_every <= Tn), stored
    a.set_fix_robust(F.HUBER, 1.345); h.set_fix_robust(F.HUBER, 1.345)
    a.solvePoseGraph(); h.solvePoseGraph()
    assert _bits(a, B) == _bits(h, B)
    a.close(); h.close()


def test_every_iteration_mode_honours_the_fixes_in_the_graph():
    """Test 8.  With fixes attached, pgs_run_sim_every_iteration = the host loop of one simulator tick, pgs_solve, pgs_adopt_result, byte for
    byte; and the fixes matter there (the run without them differs)."""
    B, L, Tn = 5, 17, 8

    def handle(fixes):
        pg, _, cmds = _sim_handle(B, L, Tn)
        pg.set_fix_sensor(_sensor_rows(B))
        pg.set_fix_robust(F.HUBER, 1.345)
        if fixes:
            pg.run_sim_fix(cmds[:4], 2)
        else:
            pg.run_sim(cmds[:4])
        return pg, cmds

    def bits(pg):
        out = _bits(pg, B)
        for b in range(B):
            g = pg.get_graph(b, 0)
            out += [g["poses"].tobytes(), g["landmarks"].tobytes()]
        return out

    a, cmds = handle(True)
    counts = a.run_sim_every_iteration(cmds[4:])
    ba = bits(a)
    a.close()
    h, _ = handle(True)
    tot = np.zeros((B, 2), dtype=np.int64)
    for t in range(4, Tn):
        h.run_sim(cmds[t:t + 1])
        h.solvePoseGraph()
        st = h.stats()
        tot[:, 0] += st["iterations"]; tot[:, 1] += st["trials"]
        h.adopt_result()
    bh = bits(h)
    h.close()
    assert ba == bh and np.array_equal(counts, tot)
    g, _ = handle(False)
    g.run_sim_every_iteration(cmds[4:])
    bg = bits(g)
    g.close()
    assert bg != ba, "the run with fixes equals the run without: the fixes never acted"


def test_fixes_do_what_they_are_for():
    """Test 9.  The effect inputs of tests/test_pgs_fix_cpu.py on the device: (a) the mean position error against the truth with fixes is
    below the error without, on every instance; (b) with 3 m jumps on every seventh fix, Geman-McClure k = 3 ends nearer the clean-fix result
    than the Gaussian solve; (c) every jumped part has w < 0.5 and every clean part w >= 0.5.  Every fix row is judged."""
    ec = F.effect_case()
    truth, B = ec["st"]["truth"], len(ec["graphs"])
    runs = {}
    for key, fx, loss in (("none", None, None), ("clean", ec["fix"], None), ("gauss", ec["fix_jump"], None), ("gm", ec["fix_jump"], (F.GEMAN_MCCLURE, F.EFFECT_GM_K))):
        pg, _ = _device(ec, fx, None if fx is None else ec["kinds"])
        if loss:
            pg.set_fix_robust(*loss)
        pg.solvePoseGraph()
        assert np.all(pg.stats()["flags"] == 0), key
        runs[key] = dict(res=[pg.get_graph(b, 1)["poses"] for b in range(B)], w=pg.fix_weights(1) if fx is not None else None)
        pg.close()
    for b in range(B):
        e_none, e_fix = F.position_error(runs["none"]["res"][b], truth), F.position_error(runs["clean"]["res"][b], truth)
        d_gauss = float(np.abs(runs["gauss"]["res"][b][:, :2] - runs["clean"]["res"][b][:, :2]).max())
        d_gm = float(np.abs(runs["gm"]["res"][b][:, :2] - runs["clean"]["res"][b][:, :2]).max())
        w, j, stored = runs["gm"]["w"][b][:, 0], ec["jumped"][b], ec["kinds"][b] > 0
        print(f"effect[{b}]: mean position error {e_none:.4f} m without fixes, {e_fix:.4f} m with; jumps: {d_gauss:.4f} m (Gaussian) / {d_gm:.4f} m "
              f"(Geman-McClure) from the clean-fix result; w jumped <= {w[j & stored].max():.3g}, clean >= {w[~j & stored].min():.3g}")
        assert e_fix < e_none, (b, e_fix, e_none)
        assert d_gm < d_gauss, (b, d_gm, d_gauss)
        assert np.all(w[j & stored] < 0.5) and np.all(w[~j & stored] >= 0.5), (b, w)
        assert np.isnan(w[~stored]).all() and np.isnan(runs["gm"]["w"][b][:, 1]).all()
        assert np.all(runs["gauss"]["w"][b][stored, 0] == 1.0)


def test_a_graph_follows_an_ekf_handle_on_the_device():
    """Test 10.  The rows slam_fix_sense_dev of a slam_batch.h handle emits go into pgs_fix_dev unchanged, beside pgs_update_each_dev: device
    pointers read in the order of the pose graph's stream once the EKF handle's stream has written them.  The stored parts equal the emitted ones."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.scenario import make_scenario
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]
    dev = _Dev(hip)
    B, L, Tn = 7, 17, 6
    lm, cmds = make_scenario(905, L, Tn)
    f = S.BatchedEKF(B, L, device=0).readParams()
    f.set_map(lm); f.set_seed(5); f.init(0.0, 0.0, 0.0)
    f.set_fix_sensor(_sensor_rows(B))
    pg = S.BatchedPoseGraph(B, num_iterations=Tn + 1, L_max=L, k_per_pose=8).readParams()
    pg.init(0.0, 0.0, 0.0)
    dfix, dkinds = dev.put(np.zeros((B, 5))), dev.put(np.zeros(B, np.int32))
    Lb = _lib.lib()
    emitted = []
    for t in range(Tn):
        f.run_sim(cmds[t:t + 1])
        dcmd = dev.put(np.tile(cmds[t], (B, 1)).astype(np.float32))
        assert f.fix_sense(dev=(dfix, dkinds, None)) is None
        f.sync()
        assert Lb.pgs_update_each_dev(pg.h, C.c_void_p(dcmd), None, None, 0, None) == 0, Lb.slam_last_error()
        pg.timestep += 1
        assert pg.fix(dfix, dkinds, dev=True) is None
        pg.sync()
        emitted.append((dev.get(dfix, np.zeros((B, 5))), dev.get(dkinds, np.zeros(B, np.int32))))
    some = 0
    for b in range(B):
        st = pg.fixes(b)
        assert not st["kinds"][0]
        for t, (fx, kd) in enumerate(emitted):
            assert st["kinds"][t + 1] == kd[b], (b, t)
            if kd[b] & 1:
                assert st["fix"][t + 1, [0, 1, 3]].tobytes() == fx[b, [0, 1, 3]].tobytes(), (b, t)
            if kd[b] & 2:
                assert st["fix"][t + 1, [2, 4]].tobytes() == fx[b, [2, 4]].tobytes(), (b, t)
            some += int(kd[b] != 0)
    assert some >= 3 * Tn
    pg.solvePoseGraph()
    assert not np.any(pg.stats()["flags"] & 16)
    pg.close(); f.close(); dev.close()
