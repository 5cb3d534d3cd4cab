"""One LM step of every pose-graph solve path against the extended-precision reference (tests/pgs_step_reference.py).

The parity tests (test_parity_pgs_gpu.py) check whole solves: LM corrects its own errors, so a damped system solved wrongly by 1e-6
relative usually still reaches the same minimiser in the same number of iterations.  Here each path solves exactly ONE trial
(SLAM_PGS_MAX_TRIALS = 1, lambda = 1e-5) from graphs built through pgs_update out of host streams; the same streams build one oracle graph
per instance, whose Jacobian at x0 (bit-identical to the device's x0) defines A = J^T J + lam I and b = -J^T e.  Every instance accepts
its first trial (asserted), so its result is x0 (+) delta_dev, and per instance (n unknowns):

    eta(delta_dev) <= 8 n u + eta_rec                          (normwise backward error, independent of kappa(A))
    |delta_dev - delta_ref|_inf <= 8 n u kappa_1 |delta_ref|_inf + |eps_rec|_inf

eps_rec bounds the rounding of the retraction and of its inverse (pgs_step_reference.recover_step), eta_rec the same pushed through the
norm of eta; the constant 8 is calibrated in test_pgs_step_reference.py.  The same solve twice gives bit-identical results.  The
largest eta of each case and of each path, its bound, the largest kappa_1 and the plan taken are printed (pytest -s).  The `sep{N}`
scenarios put the segmented elimination at its separator-count edges (63 .. 129 separators, capacity 128), `lds1365` | `long` at the pose
count up to which the pose step keeps its chains in LDS; their premises are asserted without a GPU in test_pgs_step_reference.py.  Every case asserts that the path it names really ran:
the segment length the solve took (predicted from the factors with the plan kernel's rule, pgs_step_reference.predict_plan), and for the
sequential chain whether the fused chain + SYRK launch or the separate SYRK launches formed the Schur complement."""
import functools

import numpy as np
import pytest

import pgs_step_reference as R
from live_ekf_slam_amd.config import default_config
from live_ekf_slam_amd.scenario import make_scenario

LAM0 = 1e-5
M_EDGES = [0, 1, 7, 8, 15, 16, 17, 31, 32, 33, 63, 64, 65, 176, 177, 200, 223]

# name -> (N, Ms, detections per message, k_per_pose, L_max, make_streams options)
SCENARIOS = {
    "ragged": (300, M_EDGES, 8, 8, 223, dict(window=24, at_last=2, sep_only=3, SL=32, empty_every=11)),
    # every M <= 176 (the fused kernel's bound) and messages longer than the 32 factor slots, yet no 32-pose segment over 63 landmarks
    "fusable": (353, M_EDGES[:14], 40, 32, 176, dict(window=70, new_last=True, at_last=1, sep_only=2, SL=16)),
    # every M <= 207: the largest graphs the instance-resident SYRK holds (2 M + 1 <= 416 columns, 96 tiles of 32 x 32)
    "ragged207": (300, M_EDGES[:16] + [207], 8, 8, 207, dict(window=24, at_last=2, sep_only=3, SL=32, empty_every=11)),
    "ld512": (300, [240, 223, 100], 32, 32, 240, dict(window=24, at_last=2)),
    "configs4": (1000, [200, 177, 64], 32, 32, 200, dict(window=40, at_last=1, sep_only=2, SL=32)),
    "long": (1366, [0, 17, 64], 8, 8, 64, dict(window=60, at_last=1)),
    "ill": (1000, [30, 12], 8, 8, 30, dict(window=30, quiet=((60, 480), (520, 990)), far_once=8, radius=60.0)),
    "wide16": (160, [159], 64, 64, 159, dict(window=40)),
    "wide8": (160, [159], 64, 64, 159, dict(window=52)),
    "widechain": (160, [159], 64, 64, 159, dict(window=66)),
}
for _N, _kp in ((2, 8), (7, 8), (8, 8), (9, 8), (31, 1), (32, 8), (33, 33), (34, 32)):
    SCENARIOS[f"n{_N}"] = (_N, [0, 1, 7, 8, 17], max(8, -(-17 // max(_N - 1, 1))), _kp, 17, dict(window=6, at_last=1, sep_only=1, SL=5))

# The separator-count edges of the segmented elimination (pgs_seg_impl.h; capacity kPgsSegMaxSep = 128 separators, NS = (N - 2) / SL):
# NS = 63, 64, 65 put the last segment (nseg = NS + 1 of them, one lane each in pgs_seg_chain_kernel) in the last lane of wavefront 0 and the
# first of wavefront 1, with NS % 4 = 3, 0, 1 for the separator kernel's batches of four; NS = 127, 128 reach the last rows of every array
# staged per separator and lane 128, alone in wavefront 2, with a last segment of one pose (N = 258, 642) and of more; NS = 129 is over
# the capacity: the solve must take the sequential chain.  Segments of 2 poses (an interior of one pose), of 5 (real chains in every lane)
# and of 8 (the shortest the host's own search tries).  A landmark seen from the last three separators only (sep_last) wherever NS is 127 or
# 128.  The instance without landmarks keeps the gradient-only column of the separator kernel in every case.
SEP_EDGES = {}     # name -> (path, NS)
for _N, _sl, _Ms in ([(n, 2, [0, 1, 17, 40]) for n in (128, 130, 132, 256, 258, 259, 260)] + [(n, 5, [0, 17, 64]) for n in (637, 642, 646, 647)]
                     + [(1026, 8, [0, 17, 64]), (1034, 8, [17])]):
    _ns = (_N - 2) // _sl
    # (a landmark stays in view for 12 poses, for 24 / 32 in the longer chains, whose landmarks start 10 / 16 poses apart: the segments 64, 127
    # and 128 of the largest instance must hold factors - test_pgs_step_reference.py asserts it)
    SCENARIOS[f"sep{_N}"] = (_N, _Ms, 8, 8, max(_Ms), dict(window={2: 12, 5: 24, 8: 32}[_sl], at_last=1, sep_only=2, SL=_sl, sep_last=_ns in (127, 128)))
    SEP_EDGES[f"sep{_N}"] = (f"seg{_sl}", _ns)
FALLBACK = {n for n, (_, ns) in SEP_EDGES.items() if ns > 128}   # more separators than the capacity: the plan is the sequential chain
# `long` with one pose fewer: N = 1365 = kSegBackLdsPoses, the most poses whose chains the LDS pose step holds (12 N doubles of dynamic LDS)
SCENARIOS["lds1365"] = (1365, [0, 17, 64], 8, 8, 64, dict(window=60, at_last=1))

SEG = {"default": {}, "seg16": {"SLAM_PGS_SEG": "16"}, "seg8": {"SLAM_PGS_SEG": "8"}, "seg5": {"SLAM_PGS_SEG": "5"},
       "seg2": {"SLAM_PGS_SEG": "2"}, "back_global": {"SLAM_PGS_SEG_BACK_GLOBAL": "1"}, "chain": {"SLAM_PGS_SEG": "0"},
       "seg5_back_global": {"SLAM_PGS_SEG": "5", "SLAM_PGS_SEG_BACK_GLOBAL": "1"}}
for _f in ("0", "2", "3", "4"):
    for _l in ("0", "1"):
        SEG[f"chain_fused{_f}_list{_l}"] = {"SLAM_PGS_SEG": "0", "SLAM_PGS_FUSED": _f, "SLAM_PGS_LIST": _l}
for _s in ("0", "1000000000"):
    SEG[f"chain_syrk_switch{_s}"] = {"SLAM_PGS_SEG": "0", "SLAM_PGS_FUSED": "0", "SLAM_PGS_SYRK_INST_SWITCH": _s}

CASES = [("ragged", p) for p in ("default", "seg16", "seg8", "seg5", "back_global", "chain_syrk_switch0", "chain_syrk_switch1000000000")]
CASES += [("fusable", p) for p in ("default", "seg16", "seg8", "seg5") + tuple(k for k in SEG if k.startswith("chain_fused"))
          + ("chain_syrk_switch0", "chain_syrk_switch1000000000")]
CASES += [("ragged207", p) for p in ("chain_syrk_switch0", "chain_syrk_switch1000000000")]
CASES += [("ld512", "default"), ("ld512", "chain"), ("configs4", "default"), ("configs4", "chain"), ("long", "default"), ("long", "back_global"),
          ("ill", "default"), ("ill", "chain"), ("wide16", "default"), ("wide8", "default"), ("widechain", "default"),
          ("soak", "default"), ("soak", "chain_fused3_list1")]
CASES += [(f"n{n}", p) for n in (2, 7, 8, 9, 31, 32, 33, 34) for p in ("default", "seg5", "seg2", "chain")]
# 128 separators with the pose step's chains read from global memory (s_ds[129] of pgs_seg_backsolve_kernel), and the LDS pose step at its
# largest N against the global one
CASES += [(n, p) for n, (p, _) in SEP_EDGES.items()] + [("sep642", "seg5_back_global"), ("lds1365", "default"), ("lds1365", "back_global")]
# the plan each wide-sensor graph makes the default solve take: segment length (0 = the sequential chain)
EXPECT_SL = {"wide16": 16, "wide8": 8, "widechain": 0}
# graphs whose largest M the instance-resident SYRK holds (M <= 207): SYRK_INST_SWITCH=0 runs that kernel on them; on `ragged` (M up to 223)
# the host must give the solve to the tile kernel
INST_SYRK_OK = {"fusable", "ragged207"}

REPORT = {}
BITS = {}      # (scenario, path) -> the bytes of every instance's result (test_the_pose_count_boundary_of_the_lds_pose_step)


@functools.lru_cache(maxsize=None)
def scenario(name):
    """Streams, oracle graphs and per-instance references (delta_ref, kappa_1, the StepSystem) of one scenario, computed once."""
    from oracle import oracle as O
    cfg = default_config()
    if name == "soak":   # test_parity_pgs_gpu.test_the_ill_conditioned_instance_of_the_round_4_soak, instance 9, replayed through pgs_update
        L, T, KP, B, seed, sc = 40, 846, 32, 11, 1058182634, 1043562854
        lm, cmds = make_scenario(sc, L, T)
        r = O.run_pgs_batch(lm, cmds, B, L, KP=KP, seed=seed, cfg=cfg, nthreads=8, want_streams=True)
        assert r["cnt"][9].max() <= KP
        st = dict(cmds=np.ascontiguousarray(cmds, dtype=np.float32), meas=r["meas"][9:10], cnt=r["cnt"][9:10], sec=r["pose_init"][9:10, 1:])
        N, L_max, Ms = T + 1, L, [int(r["M"][9])]
    else:
        N, Ms, per_pose, KP, L_max, opt = SCENARIOS[name]
        st = R.make_streams(N, Ms, per_pose, 1000 + len(name) * 7 + N, **opt)
    gs = R.build_oracle_graphs(O, cfg, st, N, L_max, KP)
    refs = []
    for b, g in enumerate(gs):
        v = g.values(0)
        assert v["M"] == Ms[b], (name, b, v["M"], Ms[b])
        S = R.system_of(g, v["poses"], v["landmarks"], LAM0)
        d_ref, kappa, _ = R.reference_step(S)
        refs.append((v, S, d_ref, kappa, R.factor_pairs(g, v["poses"], v["landmarks"])))
    return dict(st=st, N=N, KP=KP, L_max=L_max, cfg=cfg, refs=refs, graphs=gs)


def expected_plan(sc, name, path):
    """Segment length the solve of `path` must take on scenario `name` (0: the sequential chain)."""
    env = SEG[path]
    if env.get("SLAM_PGS_SEG") == "0":
        return 0
    start = int(env.get("SLAM_PGS_SEG", "32"))
    return R.predict_plan([r[4] for r in sc["refs"]], sc["N"], start)


def _device(sc):
    import live_ekf_slam_amd as S
    st = sc["st"]
    B, T = st["cnt"].shape
    pg = S.BatchedPoseGraph(B, num_iterations=sc["N"], L_max=sc["L_max"], k_per_pose=sc["KP"]).readParams(sc["cfg"])
    pg.init(0.0, 0.0, 0.0)
    for t in range(T):
        pg.updateNaiveVehPoseEstimate(st["sec"][:, t])
        pg.update(st["cmds"][t], st["meas"][:, t], st["cnt"][:, t])
    assert pg.timestep == sc["N"] - 1
    return pg


@pytest.mark.gpu
@pytest.mark.parametrize("name,path", CASES, ids=[f"{n}-{p}" for n, p in CASES])
def test_one_lm_step_against_the_extended_precision_reference(monkeypatch, name, path):
    sc = scenario(name)
    monkeypatch.setenv("SLAM_PGS_MAX_TRIALS", "1")
    for k, v in SEG[path].items():
        monkeypatch.setenv(k, v)
    pg = _device(sc)
    B = len(sc["refs"])
    for b, (v, _, _, _, _) in enumerate(sc["refs"]):   # graph building is bit-exact
        g0 = pg.get_graph(b, 0)
        assert g0["M"] == v["M"] and np.array_equal(g0["poses"], v["poses"]) and np.array_equal(g0["landmarks"], v["landmarks"]), (name, b)
    runs = []
    for _ in range(2):
        pg.solvePoseGraph()
        runs.append(([pg.get_graph(b, 1) for b in range(B)], pg.stats()))
    plan = pg.last_solve_paths()
    pg.close()
    (res, st), (res2, st2) = runs
    BITS[(name, path)] = b"".join(res[b][key].tobytes() for b in range(B) for key in ("poses", "landmarks"))
    for b in range(B):   # determinism: the same solve twice, bit for bit
        assert np.array_equal(res[b]["poses"], res2[b]["poses"]) and np.array_equal(res[b]["landmarks"], res2[b]["landmarks"]), (path, name, b)
    assert np.array_equal(st["trials"], st2["trials"]) and np.array_equal(st["iterations"], st2["iterations"])
    assert np.all(st["trials"] == 1), (path, name, st["trials"])
    accepted = st["iterations"] == 1
    for b in np.flatnonzero(~accepted):   # a rejected trial leaves x0
        v = sc["refs"][b][0]
        assert np.array_equal(res[b]["poses"], v["poses"]) and np.array_equal(res[b]["landmarks"], v["landmarks"]), (path, name, b)
    assert accepted.all(), f"{path} / {name}: instances {np.flatnonzero(~accepted).tolist()} rejected their first trial (the test needs every one)"
    # the path the case names really ran: the segment length (a forced length that re-planned would duplicate another case), the chain's
    # launch shape (the solve's SYRK FLOP by path: separate SYRK launches / fused chain + SYRK)
    want = EXPECT_SL[name] if name in EXPECT_SL else expected_plan(sc, name, path)
    if name in FALLBACK:   # over the separator capacity: the plan kernel says so and the host takes the sequential chain
        assert want == 0 and not plan["segmented"], (path, name, plan, want)
    elif name not in EXPECT_SL and "SLAM_PGS_SEG" in SEG[path] and SEG[path]["SLAM_PGS_SEG"] != "0":
        assert want == int(SEG[path]["SLAM_PGS_SEG"]), f"{name}: SLAM_PGS_SEG={SEG[path]['SLAM_PGS_SEG']} would re-plan to {want}"
    if name not in EXPECT_SL and path in ("default", "back_global"):
        assert want == 32, f"{name}: the default solve would re-plan to {want}"
    got = plan["segment_length"] if plan["segmented"] else 0
    assert got == want, (path, name, plan, want)
    asked = int(SEG[path].get("SLAM_PGS_SEG", "32"))   # the length the search for the plan starts from (0: the chain was asked for)
    fused = SEG[path].get("SLAM_PGS_FUSED")
    if fused in ("2", "3", "4"):
        assert plan["flop_fused"] > 0 and plan["flop_separate"] == 0, (path, name, plan)
    if fused == "0":
        assert plan["flop_separate"] > 0 and plan["flop_fused"] == 0, (path, name, plan)
    if path.startswith("chain_syrk_switch"):
        assert (name in INST_SYRK_OK) == (max(r[0]["M"] for r in sc["refs"]) <= 207), name
    worst = REPORT.setdefault(path, [0.0, 0.0, 0.0, ""])
    fails, case_eta = [], (0.0, 0.0)
    for b, (v, S, d_ref, kappa, _) in enumerate(sc["refs"]):
        delta, eps = R.recover_step(v["poses"], v["landmarks"], res[b]["poses"], res[b]["landmarks"])
        eta = S.eta(delta)
        bound = R.BOUND_C * S.n * R.U + S.eta_of_error(eps, delta)
        dref = np.asarray(d_ref, dtype=np.float64)
        fwd = float(np.abs(delta - dref).max(initial=0.0))
        fbound = R.BOUND_C * S.n * R.U * kappa * float(np.abs(dref).max(initial=0.0)) + float(eps.max(initial=0.0))
        N, M = v["poses"].shape[0], v["M"]
        if eta >= case_eta[0]:
            case_eta = (eta, bound)
        if eta > worst[0]:
            worst[0], worst[1], worst[3] = eta, bound, f"{name} instance {b}"
        worst[2] = max(worst[2], kappa)
        if not (eta <= bound and fwd <= fbound):
            fails.append(f"path {path} / {name}: instance {b} (N {N}, M {M}, n {S.n}): eta {eta:.3g} vs bound {bound:.3g}; "
                         f"|d_dev - d_ref| {fwd:.3g} vs {fbound:.3g}; kappa_1 {kappa:.3g}")
    print(f"\n{path:28s} {name:10s} largest eta {case_eta[0]:.3g} (bound {case_eta[1]:.3g}); on this path so far {worst[0]:.3g} (bound {worst[1]:.3g}, {worst[3]}), largest kappa_1 {worst[2]:.3g}, "
          f"plan {'seg ' + str(plan['segment_length']) if plan['segmented'] else 'chain'}"
          + (f", NS {(sc['N'] - 2) // asked} at {asked} poses per segment" if asked else ""))
    assert not fails, f"{len(fails)} instance(s) off the reference: " + "; ".join(fails[:8])


def _result_bits(monkeypatch, name, path):
    """The bytes of every instance's result of one solve of `path` on scenario `name` (from the case above when it ran in this process)."""
    if (name, path) not in BITS:
        sc = scenario(name)
        monkeypatch.setenv("SLAM_PGS_MAX_TRIALS", "1")
        for k, v in SEG[path].items():
            monkeypatch.setenv(k, v)
        pg = _device(sc)
        pg.solvePoseGraph()
        BITS[(name, path)] = b"".join(pg.get_graph(b, 1)[key].tobytes() for b in range(len(sc["refs"])) for key in ("poses", "landmarks"))
        pg.close()
        for k in SEG[path]:
            monkeypatch.delenv(k)
    return BITS[(name, path)]


@pytest.mark.gpu
def test_the_pose_count_boundary_of_the_lds_pose_step(monkeypatch):
    """The pose step of the segmented elimination keeps its chains in LDS up to N = 1365 poses (kSegBackLdsPoses) unless
    SLAM_PGS_SEG_BACK_GLOBAL = 1 asks for the kernel that reads them from global memory.  At N = 1366 (`long`) both settings run that same
    kernel: their results are equal byte for byte.  At N = 1365 (`lds1365`) the two kernels run, each held to the bounds by the cases above;
    the LDS kernel associates differently by design, so whether their bits differ is printed, not asserted."""
    assert SCENARIOS["long"][0] == 1366 and SCENARIOS["lds1365"][0] == 1365
    assert _result_bits(monkeypatch, "long", "default") == _result_bits(monkeypatch, "long", "back_global"), \
        "N = 1366: SLAM_PGS_SEG_BACK_GLOBAL changed a result (the LDS pose step ran beyond its pose count?)"
    same = _result_bits(monkeypatch, "lds1365", "default") == _result_bits(monkeypatch, "lds1365", "back_global")
    print(f"\nN = 1365: the LDS pose step and the global one give {'the same' if same else 'different'} bits")


def test_the_ill_conditioned_scenario_is_ill_conditioned():
    """(CPU only.)  The premise of the `ill` scenario: long stretches without detections and landmarks seen once, far away: kappa_1 >= 1e10."""
    kappas = [r[3] for r in scenario("ill")["refs"]]
    assert max(kappas) >= 1e10, kappas
