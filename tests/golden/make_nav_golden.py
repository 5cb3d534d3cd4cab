#!/usr/bin/env python3
"""Generate the controller fixtures nav_*.npz by IMPORTING the reference's pure_pursuit.py (nothing is copied).

Runs only where the reference tree is available (REF below); the tests read the .npz files, which hold data only.

For each case a kinematic closed loop is run: the true pose follows the simulator's motion model (sim_node.py:222) under the reference
controller's own commands, and the controller sees the true pose plus Gaussian noise, rounded to float32 as the state message does
(EKFState.msg:5-7).  The loop calls the reference exactly as goal_pursuit_node.py:42-50 does: PurePursuit.get_next_cmd(cur) for "pp"
with get_control = cmd_loose or cmd_tight, PurePursuit.direct_nav(cur) for "direct".  Recorded per tick: the float32 estimate, the
float32 command (Command.msg), the queue length after the tick, integ and err_prev.

One substitution, as everywhere in this project (csrc/slam_math.h): the module's `atan2` is replaced by det_atan2, the library's
deterministic atan2 - device and host must agree bit for bit, and libm's atan2 is not available on the device.  The estimates of every
case are replayed through a second, untouched import of the module (libm atan2); `libm_cmd_mismatch` records how many float32 commands
differ (the two atan2 agree to an ulp of fp64, far below float32).

The reference takes `**4`, `**12`, `**3` and `**(1/2)` through libm's pow, the restatement multiplies and takes sqrt; glibc's pow(x, 2.0)
differs from the exact product x * x in the last bit for about one x in a thousand, and a pure-pursuit tick evaluates some ten squares
per segment and radius.  So in about one pure-pursuit seed in three (10 of the 30 tried; none of the 10 `direct` seeds) integ or err_prev
of the reference leaves the restatement's by a few ulp somewhere in the run, while every float32 command and queue length still agrees.
classify() checks exactly that - commands and queue lengths bit for bit, the fp64 state within 1e-12 - and raises for anything larger.
Such a seed cannot serve the bit-for-bit test of the fp64 state and is not offered to it: it is stored under `cases_cmd_only` and tested for
its commands and queue lengths.  Seeds are tried in order until two cases per path and controller are exact (`cases`).
"""
import importlib.util, math, os, sys, types
import numpy as np
import yaml

REF = "/root/reference/ekf_ws/src"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from live_ekf_slam_amd import navigation as N  # noqa: E402


class _Msg:
    def __init__(self, **kw):
        self.__dict__.update(kw)


def _load(name):
    m = types.ModuleType("base_pkg"); sys.modules["base_pkg"] = m
    mm = types.ModuleType("base_pkg.msg"); mm.Command = _Msg; sys.modules["base_pkg.msg"] = mm
    spec = importlib.util.spec_from_file_location(name, REF + "/planning_pkg/src/pure_pursuit.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _setup(mod, cfg, path, control):
    PPc = mod.PurePursuit
    PPc.config = cfg
    PPc.goal_queue = [[float(x), float(y)] for x, y in path]
    PPc.integ = 0
    PPc.err_prev = 0.0
    PPc.get_control = PPc.cmd_tight if control == "tight" else PPc.cmd_loose
    return PPc


def _call(PPc, method, cur):
    return PPc.get_next_cmd(cur) if method == "pp" else PPc.direct_nav(cur)   # goal_pursuit_node.py:45-50


def run_case(cfg, path, method, control, T, seed, start, sigma):
    det = _load("ref_pp_det")
    det.atan2 = lambda y, x: float(N.det_atan2(y, x))
    libm = _load("ref_pp_libm")
    A, Bm = _setup(det, cfg, path, control), _setup(libm, cfg, path, control)
    rng = np.random.default_rng(seed)
    truth = np.array(start, dtype=np.float64)
    est = np.zeros((T, 3), np.float32); cmds = np.zeros((T, 2), np.float32); qlen = np.zeros(T, np.int32)
    integ = np.zeros(T); errp = np.zeros(T)
    mismatch = 0
    for t in range(T):
        e = (truth + rng.normal(0.0, sigma, 3)).astype(np.float32)            # the wire values
        cur = [float(e[0]), float(e[1]), float(e[2])]
        m = _call(A, method, cur)
        c = np.array([m.fwd, m.ang], dtype=np.float64).astype(np.float32)    # Command.msg: float32
        m2 = _call(Bm, method, cur)
        mismatch += int(np.any(np.array([m2.fwd, m2.ang], dtype=np.float64).astype(np.float32) != c))
        est[t], cmds[t], qlen[t], integ[t], errp[t] = e, c, len(A.goal_queue), float(A.integ), float(A.err_prev)
        truth = N.kinematic_step(truth, c.astype(np.float64))
    return dict(path=np.asarray(path, dtype=np.float64), est=est, cmds=cmds, qlen=qlen, integ=integ, err_prev=errp,
                method=np.int32(N.PP if method == "pp" else N.DIRECT), control=np.int32(N.TIGHT if control == "tight" else N.LOOSE),
                dt=np.float64(cfg["dt"]), la_init=np.float64(cfg["path_planning"]["lookahead_dist_init"]),
                la_max=np.float64(cfg["path_planning"]["lookahead_dist_max"]),
                d_max=np.float64(cfg["constraints"]["commands"]["d_max"]), th_max=np.float64(cfg["constraints"]["commands"]["th_max"]),
                libm_cmd_mismatch=np.int32(mismatch))


ULP_BOUND = 1e-12   # fp64 state of a case that is kept for its commands only; see classify()


def classify(c):
    """"exact": navigation.py reproduces every tick bit for bit.  "ulp": every float32 command and queue length is reproduced and integ /
    err_prev stay within ULP_BOUND of the reference's - what an ulp of pow(x, 2.0) against x * x does (2e-16 relative on values of order
    one, through a sqrt, a division and an atan2 of modest condition; six orders of magnitude below a float32 command's resolution).
    Anything else is a defect of the restatement, not of pow: AssertionError."""
    pp = N.PurePursuitBatch(1, c["path"], dt=float(c["dt"]), lookahead_dist_init=float(c["la_init"]), lookahead_dist_max=float(c["la_max"]),
                            method=int(c["method"]), control=int(c["control"]), d_max=float(c["d_max"]), th_max=float(c["th_max"]))
    exact = True
    for t in range(c["est"].shape[0]):
        cmd = pp.next_cmds(c["est"][t][None])[0]
        assert np.array_equal(cmd.view(np.uint32), c["cmds"][t].view(np.uint32)) and pp.remaining[0] == c["qlen"][t], f"tick {t}: command or queue differs"
        di, de = abs(pp.integ[0] - c["integ"][t]), abs(pp.err_prev[0] - c["err_prev"][t])
        assert di <= ULP_BOUND and de <= ULP_BOUND, f"tick {t}: integ / err_prev off by {di:g} / {de:g}, more than an ulp of pow explains"
        exact = exact and di == 0.0 and de == 0.0
    return "exact" if exact else "ulp"


PATHS = {
    "zigzag": [[1.0, 0.3], [2.0, -0.4], [3.0, 0.5], [3.5, 2.0], [2.0, 3.0], [0.0, 2.5]],
    "single": [[2.5, 1.0]],                                                    # choose_lookahead_pt returns the only point
    # passes within 0.15 m of its own later leg near (1, 0): pare_path cuts the loop in between away
    "selfapproach": [[0.5, 0.0], [1.0, 0.05], [2.0, 0.0], [2.5, 1.0], [1.5, 1.2], [1.02, 0.1], [1.0, -1.0], [0.0, -1.5]],
    "unreachable": [[6.0, 6.0], [7.0, 6.0], [7.0, 7.5]],                        # farther than lookahead_dist_max from the start: the head
    "dense": [[0.2 * i, 0.3 * math.sin(0.5 * i)] for i in range(1, 40)],
}

if __name__ == "__main__":
    with open(REF + "/base_pkg/config/params.yaml") as f:
        base = yaml.safe_load(f)
    total = tried = ulp = 0
    for ctl_name, method, control in (("pp_loose", "pp", "loose"), ("pp_tight", "pp", "tight"), ("direct", "direct", "loose")):
        out, kept, cmd_only = {}, [], []
        for k, (pname, path) in enumerate(PATHS.items()):
            T = 600 if control == "tight" else 300
            got = 0
            for rep in range(40):                                               # seeds in order until two cases of this path match exactly
                sigma, start = ((0.02, [0.0, 0.0, 0.0]), (0.05, [0.3, -0.4, 2.0]))[rep % 2]
                c = run_case(base, path, method, control, T, 100 * k + rep + 7, start, sigma)
                name = f"{pname}{rep}"
                kind = classify(c)
                for key, v in c.items():
                    out[f"{name}__{key}"] = v
                print(f"{ctl_name}/{name}: {kind}, T {T}, queue {len(path)} -> {int(c['qlen'][-1])}, libm mismatches {int(c['libm_cmd_mismatch'])}")
                if kind == "ulp":                                               # kept for its commands and queue lengths only
                    cmd_only.append(name)
                    continue
                kept.append(name)
                got += 1
                if got == 2:
                    break
            assert got == 2, f"no two exact cases for {ctl_name}/{pname}"
        out["cases"] = np.array(kept)
        out["cases_cmd_only"] = np.array(cmd_only, dtype="U32")
        tried += len(kept) + len(cmd_only); ulp += len(cmd_only)
        p = os.path.join(HERE, f"nav_{ctl_name}.npz")
        np.savez_compressed(p, **out)
        total += os.path.getsize(p)
        print(p, os.path.getsize(p), "bytes,", len(kept), "exact cases,", len(cmd_only), "for commands only")
    print("total bytes", total, "-", ulp, "of", tried, "seeds kept for commands only")
