"""Robust loss (Huber, Geman-McClure) on the pose graph's landmark factors, on the device, against tests/pgs_robust_reference.py.

Graphs are built through pgs_update from the streams of tests/test_pgs_step_gpu.py's scenario table with outliers put in
(pgs_robust_reference.corrupt: every seventh non-first detection of an instance 3 m / 0.5 rad off).  One weighted LM step on every
solve path against the extended-precision reference of the weighted system; the loss switched off three ways, byte for byte; whole solves
against a dense Python LM with the device's decision logic; the factor weights; the marginals of the weighted graph; what the loss is for;
the every-iteration mode.  Every premise a test rests on is asserted on the reference first."""
import functools
import os

import numpy as np
import pytest

import pgs_marginals_reference as MR
import pgs_robust_reference as RR
import pgs_step_reference as R
import test_pgs_step_gpu as T

pytestmark = pytest.mark.gpu

POSE_TOL = 1e-7
LOSSES = {"huber": (RR.HUBER, 1.345), "gm": (RR.GEMAN_MCCLURE, 3.0)}
SMALL = ("n2", "n9", "n33", "n34")
# (`ragged` holds graphs of up to 223 landmarks: beyond the fused chain + SYRK kernel's 176, so its chain_fused3_list1 solve takes the separate
# launches - `fusable`, the step test's scenario for that kernel, is added so that the fused kernel does read weighted blocks)
STEP_CASES = [(n, p) for n in SMALL for p in ("default", "seg5", "seg2", "chain")] + [("ragged", "default"), ("ragged", "chain_fused3_list1"),
                                                                                      ("fusable", "chain_fused3_list1")]
# 128 separators, the most the separator kernel stages (the step test's sep258): the reweighted blocks - and, through test_pgs_fix_gpu.py, the
# appended rows of fixes at separators, the last among them - in every row of what it reads from A
STEP_CASES += [("sep258", "seg2")]
SOLVE_CASES = [(n, p) for n in ("n33", "n34") for p in ("default", "seg5", "chain")]


class _Env:
    """Environment of one solve path (test_pgs_step_gpu.SEG) around the creation of a handle."""

    def __init__(self, path, extra=None):
        self.set = dict(T.SEG[path], **(extra or {}))

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.set}
        os.environ.update(self.set)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _bits(pg, B):
    """Everything a solve leaves: the results and every array of the statistics, as bytes."""
    out = []
    for b in range(B):
        g = pg.get_graph(b, 1)
        out += [g["poses"].tobytes(), g["landmarks"].tobytes()]
    st = pg.stats()
    return out + [st[k].tobytes() for k in sorted(st)]


@functools.lru_cache(maxsize=None)
def step_reference(name, loss):
    """Per instance of the outlier case: (x0, weighted StepSystem, its linearisation, delta_ref, kappa_1, the reference's verdict on
    the first trial, the factors' (pose, landmark) pairs)."""
    kind, k = LOSSES[loss]
    sc = RR.case(name)
    refs = []
    for g in sc["graphs"]:
        v = g.values(0)
        S, L = RR.weighted_system(g, v["poses"], v["landmarks"], T.LAM0, kind, k)
        d_ref, kappa, _ = R.reference_step(S)
        first = RR.lm_solve(g, kind, k, max_trials=1)
        refs.append((v, S, L, d_ref, kappa, first, R.factor_pairs(g, v["poses"], v["landmarks"])))
    return refs


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("name,path", STEP_CASES, ids=[f"{n}-{p}" for n, p in STEP_CASES])
def test_one_weighted_lm_step_against_the_extended_precision_reference(name, path, loss):
    """Test 5.  The bounds of test_pgs_step_gpu.py (eta <= 8 n u + eta_rec; forward with kappa_1) against the WEIGHTED system.  The
    reference says which instances accept their first trial (with oldLin = error instead of the weighted linearised cost the verdicts
    differ); an instance that rejects it keeps x0."""
    kind, k = LOSSES[loss]
    sc, refs = RR.case(name), step_reference(name, loss)
    w_all = np.concatenate([L["w"] for _, _, L, _, _, _, _ in refs])
    r_all = np.concatenate([L["r"] for _, _, L, _, _, _, _ in refs])
    # premises, on the reference: outliers are down-weighted, inliers are not, nothing sits on the branch point.  (n2 has one update:
    # every detection is a landmark's first and stays clean, so it has no outlier to down-weight - asserted.)
    if name == "n2":
        assert not sc["bad"].any()
    else:
        assert (w_all < 0.5).any(), (name, loss)
    if kind == RR.HUBER:
        assert (w_all == 1.0).any(), (name, loss)
    assert not (np.abs(r_all - k) < 1e-9 * k).any()
    with _Env(path, {"SLAM_PGS_MAX_TRIALS": "1"}):
        pg = T._device(sc)
        pg.set_robust(kind, k)
        assert pg.robust == (kind, k)
        B = len(refs)
        runs = []
        for _ in range(2):
            pg.solvePoseGraph()
            runs.append(_bits(pg, B))
        res = [pg.get_graph(b, 1) for b in range(B)]
        st = pg.stats()
        plan = pg.last_solve_paths()
        pg.close()
    assert runs[0] == runs[1], "the same solve twice differs"
    assert np.all(st["trials"] == 1)
    fused = T.SEG[path].get("SLAM_PGS_FUSED")
    if fused in ("2", "3", "4") and max(sc["Ms"]) <= 176:
        assert plan["flop_fused"] > 0 and plan["flop_separate"] == 0, plan
    want = 0 if T.SEG[path].get("SLAM_PGS_SEG") == "0" else R.predict_plan([r[6] for r in refs], sc["N"], int(T.SEG[path].get("SLAM_PGS_SEG", "32")))
    assert (plan["segment_length"] if plan["segmented"] else 0) == want, (plan, want)   # the path the case names really ran
    fails, accepted = [], 0
    for b, (v, S, L, d_ref, kappa, first, _) in enumerate(refs):
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
        print(f"{name}/{path}/{loss}[{b}]: n {S.n} eta {eta:.3g} bound {bound:.3g}; |d_dev - d_ref| {fwd:.3g} bound {fbound:.3g}; kappa_1 {kappa:.3g}; min w {L['w'].min(initial=1.0):.3g}")
        if not (eta <= bound and fwd <= fbound):
            fails.append(f"instance {b} (n {S.n}): eta {eta:.3g} vs {bound:.3g}; |d_dev - d_ref| {fwd:.3g} vs {fbound:.3g}; kappa_1 {kappa:.3g}")
    assert accepted > 0, "no instance accepted its first trial: the step was not compared"
    assert not fails, f"{name}/{path}/{loss}: " + "; ".join(fails[:8])


@pytest.mark.parametrize("name,path", [("n34", "default"), ("ragged", "default"), ("ragged", "chain_fused3_list1")])
def test_the_loss_switched_off_is_the_same_code(name, path):
    """Test 6.  A handle never touched, one after set_robust(NONE, 0) and one with a Huber loss no residual reaches: results, every
    array of the statistics and the marginals, byte for byte."""
    sc = RR.case(name)
    B = len(sc["graphs"])
    seen = []
    for setting in (None, (RR.NONE, 0.0), (RR.HUBER, 1e300)):
        with _Env(path):
            pg = T._device(sc)
            if setting:
                pg.set_robust(*setting)
            pg.solvePoseGraph()
            bits = _bits(pg, B)
            pg.marginals(1)
            for b in range(B):
                m = pg.get_marginals(b)
                bits += [m["pose_cov"].tobytes(), m["lm_cov"].tobytes(), bytes([m["status"]])]
            pg.close()
        seen.append(bits)
    assert seen[0] == seen[1], "set_robust(NONE, 0) changed a result"
    assert seen[0] == seen[2], "Huber with k = 1e300 is not the Gaussian solve"


@functools.lru_cache(maxsize=None)
def solve_reference(name, loss):
    """The Python LM of every instance of the outlier case, with its own fairness checks: no accept / stop comparison within a relative
    1e-6 of its threshold, and a result that moves by less than 1e-8 m when QR replaces the normal equations."""
    kind, k = LOSSES[loss]
    out = []
    for b, g in enumerate(RR.case(name)["graphs"]):
        a, q = RR.lm_solve(g, kind, k, "chol"), RR.lm_solve(g, kind, k, "qr")
        assert a["margin"] >= 1e-6, (name, loss, b, a["margin"])
        assert (a["iterations"], a["trials"]) == (q["iterations"], q["trials"]), (name, loss, b)
        moved = max(float(np.abs(a["poses"] - q["poses"]).max()), float(np.abs(a["landmarks"] - q["landmarks"]).max(initial=0.0)))
        assert moved < 1e-8, (name, loss, b, moved)
        assert a["flags"] == 0, (name, loss, b)
        out.append(a)
    return out


@functools.lru_cache(maxsize=None)
def solved(name, path, loss, corrupted=True):
    """One device solve of the case with the loss (None: never set): per instance the result, then the statistics, the factor weights at the
    result, and the bytes of results and statistics before and after the weights were asked for."""
    sc = RR.case(name)
    if not corrupted:
        sc = dict(sc, st=sc["clean"])
    B = len(sc["graphs"])
    with _Env(path):
        pg = T._device(sc)
        if loss:
            pg.set_robust(*LOSSES[loss])
        pg.solvePoseGraph()
        res = [pg.get_graph(b, 1) for b in range(B)]
        before = _bits(pg, B)
        w = pg.factor_weights(1)
        after = _bits(pg, B)
        conn = [pg.connections(b) for b in range(B)]
        st = pg.stats()
        pg.close()
    return dict(res=res, stats=st, w=w, before=before, after=after, conn=conn)


@pytest.mark.parametrize("loss", list(LOSSES))
@pytest.mark.parametrize("name,path", SOLVE_CASES, ids=[f"{n}-{p}" for n, p in SOLVE_CASES])
def test_whole_solves_with_outliers_against_the_python_lm(name, path, loss):
    """Test 7.  Iteration and trial counts equal, results within POSE_TOL, every instance converged with no flag."""
    ref, run = solve_reference(name, loss), solved(name, path, loss)
    st = run["stats"]
    assert np.all(st["flags"] == 0), st["flags"]
    for b, a in enumerate(ref):
        print(f"{name}/{path}/{loss}[{b}]: device {st['iterations'][b]} iterations / {st['trials'][b]} trials, reference {a['iterations']} / {a['trials']}; "
              f"cost {st['err_init'][b]:.6g} -> {st['err_final'][b]:.6g} (reference {a['err_init']:.6g} -> {a['err_final']:.6g})")
    for b, a in enumerate(ref):
        assert (st["iterations"][b], st["trials"][b]) == (a["iterations"], a["trials"]), (name, path, loss, b)
        d = max(float(np.abs(run["res"][b]["poses"] - a["poses"]).max()), float(np.abs(run["res"][b]["landmarks"] - a["landmarks"]).max(initial=0.0)))
        assert d <= POSE_TOL, (name, path, loss, b, d)
        assert abs(st["err_final"][b] - a["err_final"]) <= 1e-9 * max(a["err_final"], 1e-12) + 1e-12, (b, st["err_final"][b], a["err_final"])


@pytest.mark.parametrize("loss", list(LOSSES) + [None])
@pytest.mark.parametrize("name,path", SOLVE_CASES, ids=[f"{n}-{p}" for n, p in SOLVE_CASES])
def test_factor_weights_at_the_result(name, path, loss):
    """Test 8.  Against the reference's w from the oracle's residuals at the DEVICE's result: relative difference at most 8 u; NaN where
    no factor is stored; exactly 1.0 without a loss; the handle's results untouched by the call."""
    sc, run = RR.case(name), solved(name, path, loss)
    kind, k = LOSSES[loss] if loss else (RR.NONE, 0.0)
    assert run["before"] == run["after"], "pgs_factor_weights changed a result or a statistic"
    N, KP = sc["N"], sc["KP"]
    assert run["w"].shape == (len(sc["graphs"]), N, KP)
    for b, g in enumerate(sc["graphs"]):
        cnt = np.r_[0, np.minimum(sc["st"]["cnt"][b], KP)]          # pose 0 stores no factor
        stored = np.arange(KP)[None, :] < cnt[:, None]
        w = run["w"][b]
        assert np.isnan(w[~stored]).all() and not np.isnan(w[stored]).any(), (name, b)
        assert np.array_equal(run["conn"][b][:, 0], np.nonzero(stored)[0]), (name, b)   # slot order = the order of the connections
        if kind == RR.NONE:
            assert np.all(w[stored] == 1.0), (name, b)
            continue
        L = RR.weigh(g, run["res"][b]["poses"], run["res"][b]["landmarks"], kind, k)
        rel = np.abs(w[stored] - L["w"]) / L["w"]
        print(f"{name}/{path}/{loss}[{b}]: {int(stored.sum())} factors, w in [{w[stored].min(initial=1.0):.3g}, 1], largest relative difference {rel.max(initial=0.0) / R.U:.2f} u")
        assert np.all(rel <= 8 * R.U), (name, b, rel.max())
        bad = RR.bad_factors(sc, b)
        if bad.any():   # the corrupted detections are the ones the solve believed least
            assert w[stored][bad].max() < w[stored][~bad].min(), (name, b, w[stored][bad].max(), w[stored][~bad].min())


def test_marginals_of_the_weighted_graph():
    """Test 9.  pgs_marginals(1) with Huber on n34 against pgs_marginals_reference.judge fed the weighted Jacobian at the device's result,
    with test_pgs_marginals_gpu.py's rule: the figure of merit within min(10 x the CPU's own rounding spread, the forward bound)."""
    kind, k = LOSSES["huber"]
    sc = RR.case("n34")
    pg = T._device(sc)
    pg.set_robust(kind, k)
    pg.solvePoseGraph()
    pg.marginals(1)
    plain = None
    fails = []
    for b, g in enumerate(sc["graphs"]):
        gr, m = pg.get_graph(b, 1), pg.get_marginals(b)
        j = MR.judge(RR.WeightedGraph(g, kind, k), gr["poses"], gr["landmarks"])
        assert "singular" not in j and m["status"] == 0, (b, m["status"])
        fom = MR.figure_of_merit(m["pose_cov"], m["lm_cov"], j["pose_cov"], j["lm_cov"])
        print(f"n34[{b}] huber: figure {fom:.3g} spread {j['spread']:.3g} bar {j['bar']:.3g} bound {j['bound']:.3g} kappa_1 {j['kappa']:.3g}")
        if not fom <= j["bar"]:
            fails.append(f"instance {b}: figure {fom:.3g} above the bar {j['bar']:.3g}")
        if RR.bad_factors(sc, b).any():   # and they are not the Gaussian graph's: that one fails the same bar
            plain = MR.judge(g, gr["poses"], gr["landmarks"])
            assert MR.figure_of_merit(m["pose_cov"], m["lm_cov"], plain["pose_cov"], plain["lm_cov"]) > j["bar"], b
    pg.close()
    assert plain is not None
    assert not fails, "; ".join(fails)


def test_the_loss_does_what_it_is_for():
    """Test 10.  One log of n34 with outliers: the landmarks of the Huber and the Geman-McClure result lie nearer the clean log's result
    than the Gaussian result's do, for every instance with a corrupted factor - and the Gaussian result is really off."""
    sc = RR.case("n34")
    clean = solved("n34", "default", None, corrupted=False)
    runs = {loss: solved("n34", "default", loss) for loss in (None, "huber", "gm")}
    hit = 0
    for b in range(len(sc["graphs"])):
        if not RR.bad_factors(sc, b).any():
            continue
        hit += 1
        err = {loss: float(np.linalg.norm(run["res"][b]["landmarks"] - clean["res"][b]["landmarks"], axis=1).max()) for loss, run in runs.items()}
        print(f"n34[{b}]: largest landmark distance from the clean log's result: Gaussian {err[None]:.4g} m, Huber {err['huber']:.4g} m, Geman-McClure {err['gm']:.4g} m")
        assert err[None] > 10 * POSE_TOL, (b, err)
        assert err["huber"] < err[None] and err["gm"] < err[None], (b, err)
    assert hit >= 3


def test_every_iteration_mode_with_a_loss():
    """Test 11.  pgs_run_sim_every_iteration with Huber on 9 poses = a host loop of one simulator tick, pgs_solve, pgs_adopt_result with the
    same setting, byte for byte; and the loss matters there (the Gaussian run differs)."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd.scenario import make_scenario
    B, L, Tn = 5, 17, 8
    lm, cmds = make_scenario(905, L, Tn)
    kind, k = RR.HUBER, 0.01   # (the simulator's detections are clean and the default configuration whitens by sigma = 1: a k inside the noise of a few cm, so that the loss reweights them)

    def handle(setting):
        pg = S.BatchedPoseGraph(B, num_iterations=Tn + 1, L_max=L, k_per_pose=8).readParams()
        pg.set_map(lm); pg.set_seed(5); pg.init(0.0, 0.0, 0.0)
        if setting:
            pg.set_robust(*setting)
        return pg

    def bits(pg):
        out = _bits(pg, B)
        for b in range(B):
            g = pg.get_graph(b, 0)
            out += [g["poses"].tobytes(), g["landmarks"].tobytes()]
        return out

    a = handle((kind, k))
    counts = a.run_sim_every_iteration(cmds)
    ba = bits(a)
    a.close()
    h = handle((kind, k))
    tot = np.zeros((B, 2), dtype=np.int64)
    for t in range(Tn):
        h.run_sim(cmds[t:t + 1])
        h.solvePoseGraph()
        st = h.stats()
        tot[:, 0] += st["iterations"]; tot[:, 1] += st["trials"]
        h.adopt_result()
    bh = bits(h)
    h.close()
    assert ba == bh and np.array_equal(counts, tot)
    g = handle(None)
    g.run_sim_every_iteration(cmds)
    bg = bits(g)
    g.close()
    assert bg != ba, "the Huber run equals the Gaussian run: the loss never acted"
