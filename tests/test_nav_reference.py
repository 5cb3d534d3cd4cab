"""The controller restatement against the reference's pure_pursuit.py, tick by tick and bit for bit (no GPU).

tests/golden/nav_*.npz were recorded by tests/golden/make_nav_golden.py from the reference module itself: for every case the float32
estimates it was fed and, per tick, its float32 command, the length of its goal_queue, integ and err_prev.  Both restatements -
live_ekf_slam_amd.navigation (numpy) and csrc/nav_kernel.h compiled for the host (slam_nav_tick_host; the device kernel compiles the
same function) - must reproduce every tick of every case exactly.  No miss is allowed."""
import ctypes as C
import os

import numpy as np
import pytest

from live_ekf_slam_amd import navigation as N

GOLD = os.path.join(os.path.dirname(__file__), "golden")
FILES = ["nav_pp_loose.npz", "nav_pp_tight.npz", "nav_direct.npz"]


def _cases():
    out = []
    for f in FILES:
        z = np.load(os.path.join(GOLD, f))
        for name in z["cases"]:
            out.append((f, str(name)))
    return out


def _cmd_only_cases():
    """Seeds in which the reference's fp64 state leaves the restatement's by an ulp of libm's pow somewhere (make_nav_golden.py: classify):
    their float32 commands and queue lengths are still the reference's, and are checked; integ / err_prev to the generator's 1e-12."""
    out = []
    for f in FILES:
        z = np.load(os.path.join(GOLD, f))
        out += [(f, str(n)) for n in z["cases_cmd_only"]]
    return out


def _case(f, name):
    z = np.load(os.path.join(GOLD, f))
    return {k.split("__", 1)[1]: z[k] for k in z.files if k.startswith(name + "__")}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else np.uint64)


def test_fixture_set_covers_what_it_should():
    names = _cases()
    assert len(names) >= 24 and len(_cmd_only_cases()) >= 1
    for f, method, control in zip(FILES, (N.PP, N.PP, N.DIRECT), (N.LOOSE, N.TIGHT, N.LOOSE)):
        mine = [n for ff, n in names if ff == f]
        for path in ("zigzag", "single", "selfapproach", "unreachable", "dense"):
            assert any(n.startswith(path) for n in mine), (f, path)
        for n in mine:
            c = _case(f, n)
            assert int(c["method"]) == method and int(c["control"]) == control
            assert c["est"].dtype == np.float32 and c["cmds"].dtype == np.float32
            assert int(c["libm_cmd_mismatch"]) == 0       # det_atan2 in place of libm's atan2 changed no float32 command
    # pure pursuit on the self-approaching path pares a waypoint that is not the head (the queue drops by more than one point at once)
    drops = []
    for f in FILES[:2]:
        for ff, n in names:
            if ff == f and n.startswith("selfapproach"):
                q = np.concatenate([[8], _case(f, n)["qlen"]])
                drops.append(int((q[:-1] - q[1:]).max()))
    assert max(drops) > 1
    # the unreachable-lookahead cases start farther from every segment than lookahead_dist_max
    c = _case(FILES[0], [n for ff, n in names if ff == FILES[0] and n.startswith("unreachable")][0])
    d = np.hypot(*(c["path"] - c["est"][0, :2].astype(np.float64)).T)
    assert d.min() > float(c["la_max"]) * 1.25


@pytest.mark.parametrize("f,name", _cases())
def test_navigation_py_reproduces_the_reference(f, name):
    c = _case(f, name)
    pp = N.PurePursuitBatch(1, c["path"], dt=float(c["dt"]), lookahead_dist_init=float(c["la_init"]), lookahead_dist_max=float(c["la_max"]),
                            method=int(c["method"]), control=int(c["control"]), d_max=float(c["d_max"]), th_max=float(c["th_max"]))
    T = c["est"].shape[0]
    cmds = np.zeros((T, 2), np.float32); qlen = np.zeros(T, np.int32); integ = np.zeros(T); errp = np.zeros(T)
    for t in range(T):
        cmds[t] = pp.next_cmds(c["est"][t][None])[0]
        qlen[t], integ[t], errp[t] = pp.remaining[0], pp.integ[0], pp.err_prev[0]
    assert np.array_equal(_bits(cmds), _bits(c["cmds"]))
    assert np.array_equal(qlen, c["qlen"])
    assert np.array_equal(_bits(integ), _bits(c["integ"])) and np.array_equal(_bits(errp), _bits(c["err_prev"]))
    # finish_tick: the first tick whose command was issued with an empty queue
    empty_at_cmd = np.concatenate([[False], c["qlen"][:-1] == 0]) if int(c["method"]) == N.DIRECT else c["qlen"] == 0
    want = int(np.argmax(empty_at_cmd)) if empty_at_cmd.any() else (T if int(c["method"]) == N.DIRECT and c["qlen"][-1] == 0 else -1)
    assert int(pp.finish_tick[0]) == want
    if 0 <= want < T:
        assert not cmds[want:].any()


def test_navigation_py_batch_equals_single_instances():
    """All cases of one file as ONE batch with per-instance paths: every instance as on its own (the masks do not leak between lanes)."""
    for f in FILES:
        names = [n for ff, n in _cases() if ff == f]
        cs = [_case(f, n) for n in names]
        T = min(c["est"].shape[0] for c in cs)
        c0 = cs[0]
        pp = N.PurePursuitBatch(len(cs), [c["path"] for c in cs], method=int(c0["method"]), control=int(c0["control"]))
        for t in range(T):
            cmd = pp.next_cmds(np.stack([c["est"][t] for c in cs]))
            assert np.array_equal(_bits(cmd), _bits(np.stack([c["cmds"][t] for c in cs]))), (f, t)
            assert np.array_equal(pp.remaining, [c["qlen"][t] for c in cs])
        assert np.array_equal(_bits(pp.integ), _bits(np.array([c["integ"][T - 1] for c in cs])))


def test_guards():
    pp = N.PurePursuitBatch(3, [[1.0, 0.0], [2.0, 0.5]])
    est = np.array([[0.0, 0.0, 0.0], [np.nan, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    cmd = pp.next_cmds(est, frozen=[False, False, True])
    assert cmd[0].any() and not cmd[1:].any()
    assert pp.integ[0] != 0.0 and not pp.integ[1:].any() and not pp.err_prev[1:].any() and np.all(pp.head == 0)
    with pytest.raises(ValueError):
        N.PurePursuitBatch(1, [[1.0, 0.0], [1.0, 0.0], [2.0, 0.0]])
    with pytest.raises(ValueError):
        N.PurePursuitBatch(1, np.zeros((N.MAX_WAYPOINTS + 1, 2)) + np.arange(N.MAX_WAYPOINTS + 1)[:, None])
    with pytest.raises(ValueError):
        N.PurePursuitBatch(1, [[1.0, 0.0]], lookahead_dist_init=1e-30)


def test_det_atan2_port_matches_libm_to_an_ulp():
    rng = np.random.default_rng(0)
    y, x = rng.normal(size=20000), rng.normal(size=20000)
    got, ref = N.det_atan2(y, x), np.arctan2(y, x)
    assert np.all(np.abs(got - ref) <= np.spacing(np.abs(ref)))
    assert N.det_atan2(0.0, -1.0) == np.pi and N.det_atan2(-0.0, -1.0) == -np.pi and N.det_atan2(1.0, 0.0) == np.pi / 2
    v = rng.uniform(-30, 30, 5000)
    import math
    assert np.array_equal(N.rem2pi(v), [math.remainder(a, N.TAU) for a in v])


@pytest.mark.parametrize("f,name", _cases())
def test_compiled_tick_reproduces_the_reference(f, name):
    """csrc/nav_kernel.h's nav_tick, the function the device kernel compiles, built for the host."""
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.config import NavConfig
    L = _lib.lib()
    c = _case(f, name)
    cfg = NavConfig(float(c["dt"]), float(c["la_init"]), float(c["la_max"]), int(c["method"]), int(c["control"]))
    path = np.ascontiguousarray(c["path"])
    P = path.shape[0]
    head, fin = C.c_int32(0), C.c_int32(-1)
    integ, errp = C.c_double(0.0), C.c_double(0.0)
    cmd = np.zeros(2, np.float32)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    for t in range(c["est"].shape[0]):
        est = np.ascontiguousarray(c["est"][t])
        rc = L.slam_nav_tick_host(C.byref(cfg), float(c["d_max"]), float(c["th_max"]), path.ctypes.data_as(dp), P, est.ctypes.data_as(fp), 0, t,
                                  C.byref(head), C.byref(fin), C.byref(integ), C.byref(errp), cmd.ctypes.data_as(fp))
        assert rc == 0
        assert np.array_equal(_bits(cmd), _bits(c["cmds"][t])), t
        assert P - head.value == c["qlen"][t], t
        assert np.float64(integ.value).tobytes() == c["integ"][t].tobytes() and np.float64(errp.value).tobytes() == c["err_prev"][t].tobytes(), t


@pytest.mark.parametrize("f,name", _cmd_only_cases())
def test_commands_and_queue_of_the_seeds_with_an_ulp_of_pow(f, name):
    """Both restatements on the seeds kept for their commands only: every float32 command and queue length exact, the fp64 state within
    1e-12 (the generator's bound for what an ulp of pow(x, 2.0) against x * x can do), and the two restatements equal to each other
    bit for bit."""
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.config import NavConfig
    L = _lib.lib()
    c = _case(f, name)
    kw = dict(dt=float(c["dt"]), lookahead_dist_init=float(c["la_init"]), lookahead_dist_max=float(c["la_max"]))
    pp = N.PurePursuitBatch(1, c["path"], method=int(c["method"]), control=int(c["control"]), d_max=float(c["d_max"]), th_max=float(c["th_max"]), **kw)
    cfg = NavConfig(kw["dt"], kw["lookahead_dist_init"], kw["lookahead_dist_max"], int(c["method"]), int(c["control"]))
    path = np.ascontiguousarray(c["path"]); P = path.shape[0]
    head, fin, integ, errp = C.c_int32(0), C.c_int32(-1), C.c_double(0.0), C.c_double(0.0)
    cmd = np.zeros(2, np.float32)
    dp, fp = C.POINTER(C.c_double), C.POINTER(C.c_float)
    for t in range(c["est"].shape[0]):
        est = np.ascontiguousarray(c["est"][t])
        got = pp.next_cmds(est[None])[0]
        assert L.slam_nav_tick_host(C.byref(cfg), float(c["d_max"]), float(c["th_max"]), path.ctypes.data_as(dp), P, est.ctypes.data_as(fp), 0, t,
                                    C.byref(head), C.byref(fin), C.byref(integ), C.byref(errp), cmd.ctypes.data_as(fp)) == 0
        assert np.array_equal(_bits(got), _bits(c["cmds"][t])) and np.array_equal(_bits(cmd), _bits(c["cmds"][t])), t
        assert pp.remaining[0] == c["qlen"][t] and P - head.value == c["qlen"][t], t
        assert abs(pp.integ[0] - c["integ"][t]) <= 1e-12 and abs(pp.err_prev[0] - c["err_prev"][t]) <= 1e-12, t
        assert pp.integ[0] == integ.value and pp.err_prev[0] == errp.value, t
