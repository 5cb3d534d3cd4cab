"""Closed-loop runs on the GPU (slam_nav_run): the device route against the host route, bit for bit, on every instance.

Device route: handle A runs slam_nav_run(T, cmds_out) - per tick the controller kernel (csrc/nav_kernel.hip) and one simulator timestep.
Host route: handle B, same seed, runs per tick  nav_estimates -> live_ekf_slam_amd.navigation.PurePursuitBatch -> run_sim_each(., 1).
The two must agree in every bit of x, P, M, ids, truth, error statistics, status, all T x B commands and the controller state.

The scenario: make_scenario(47, L, .)'s map; the shared path is its first three landmarks (4.2 m of legs), per-instance paths are one to
four consecutive landmarks starting at landmark 0, 1 or 2.  Every instance starts (filter and simulator alike) one metre before its first
waypoint, heading at it along the line of its first leg, so that every head advances within the first ticks and, with per-instance paths,
a part of the batch finishes within 300 ticks under every controller while the instances whose paths run to the far landmarks 3 and 4 do
not (a dry run of navigation.py with the simulator's motion model and noise levels: every head advances; 30 to 59 of 64 finish)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from batch_state import describe, differing_instances
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCEN_SEED, B_TEST, T_TEST = 47, 256, 300
CONFIGS = ["ekf64_L20", "ekf64_L50", "ekf32_L20", "ukf_slam_L20", "ukf_loc"]
CONTROLS = {"pp_loose": (0, 0), "pp_tight": (0, 1), "direct": (1, 0)}


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _map(L):
    from live_ekf_slam_amd.scenario import make_scenario
    return make_scenario(SCEN_SEED, L, 2)[0]


def _starts(paths, B):
    """(B, 3) float32 start poses: one metre before the first waypoint on the line of the first leg (a single waypoint: on the line from
    the origin), heading at the waypoint."""
    out = np.zeros((B, 3), np.float32)
    for b in range(B):
        p = np.asarray(paths if isinstance(paths, np.ndarray) else paths[b])
        d = p[0] - p[1] if len(p) > 1 else -p[0]
        d = d / np.hypot(*d)
        out[b] = [p[0, 0] + d[0], p[0, 1] + d[1], np.arctan2(-d[1], -d[0])]
    return out


def _make(S, config, B, seed=11, offset=0, starts=None):
    L = 50 if config.endswith("L50") else 20
    if config.startswith("ekf"):
        f = S.BatchedEKF(B, L, dtype=S.F32 if config.startswith("ekf32") else S.F64)
    elif config == "ukf_slam_L20":
        f = S.BatchedUKF(B, L)
    else:
        f = S.BatchedUKFLoc(B)
    f.readParams()
    lm = _map(L)
    f.set_map(lm); f.set_seed(seed)
    if offset:
        f.set_instance_offset(offset)
    if starts is None:
        f.init(0.0, 0.0, 0.0)
    else:
        f.init(starts, truth0=starts.astype(np.float64))
    return f, lm


def _paths(lm, B, each, first=0):
    """shared: the first three landmarks; each: instance g (global index) gets 1 .. 4 landmarks starting at landmark g % 3."""
    if not each:
        return lm[:3].copy()
    out = []
    for b in range(B):
        g = first + b
        out.append(lm[g % 3: g % 3 + 1 + g % 4].copy())
    return out


def _nav(method, control):
    return dict(method=method, control=control)


def _set(f, paths, each, nav):
    (f.set_paths if each else f.set_path)(paths, nav=nav)


def _host_controller(f, paths, nav):
    from live_ekf_slam_amd.navigation import PurePursuitBatch
    return PurePursuitBatch(f.batch, paths, method=nav["method"], control=nav["control"], d_max=f.cfg.d_max, th_max=f.cfg.th_max)


def _host_route(f, pp, T):
    cmds = np.zeros((T, f.batch, 2), np.float32)
    for t in range(T):
        frozen = (f.status() & 4) != 0
        cmds[t] = pp.next_cmds(f.nav_estimates(), frozen)
        f.run_sim(cmds[t][None])                     # slam_run_sim_each(cmds, 1)
    return cmds


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_nav_state(sa, sb, what):
    for k in ("remaining", "finish_tick", "integ", "err_prev"):
        assert np.array_equal(_bits(sa[k]), _bits(sb[k])), f"{what}: {k} differs in {(np.asarray(_bits(sa[k])) != _bits(sb[k])).sum()} instances"


def _same_handles(fa, fb, what, count=None, b_offset=0):
    d = differing_instances(fa, fb, count=count, b_offset=b_offset)
    assert not d, f"{what}: {describe(d)}"


@pytest.mark.parametrize("each", [False, True], ids=["shared", "each"])
@pytest.mark.parametrize("control", list(CONTROLS))
@pytest.mark.parametrize("config", CONFIGS)
def test_device_route_equals_host_route(S, config, control, each):
    nav = _nav(*CONTROLS[control])
    paths = _paths(_map(20), B_TEST, each)      # (the first landmarks of the L = 20 and L = 50 maps of one seed are the same)
    st = _starts(paths, B_TEST)
    fa, lm = _make(S, config, B_TEST, starts=st)
    fb, _ = _make(S, config, B_TEST, starts=st)
    assert np.array_equal(lm[:6], _map(20)[:6])
    _set(fa, paths, each, nav); _set(fb, paths, each, nav)
    ca = fa.run_nav(T_TEST, return_cmds=True)
    pp = _host_controller(fb, paths, nav)
    cb = _host_route(fb, pp, T_TEST)
    diff = _bits(ca) != _bits(cb)
    assert not diff.any(), f"{diff.any(axis=2).sum()} of {T_TEST * B_TEST} commands differ, first at tick {int(np.argmax(diff.any(axis=(1, 2))))}"
    _same_handles(fa, fb, f"{config}/{control}")
    sa = fa.nav_state()
    _same_nav_state(sa, dict(remaining=pp.remaining, finish_tick=pp.finish_tick, integ=pp.integ, err_prev=pp.err_prev), "device vs host controller")
    assert np.array_equal(fa.status(), fb.status())
    assert ca.any() and np.isfinite(ca).all()
    assert (sa["remaining"] < pp.plen).mean() > 0.5, "few heads advanced: the scenario does not exercise the queue"
    if each:   # (per-instance paths of one to four landmarks: a part of the batch finishes, the rest is still under way)
        assert (sa["finish_tick"] >= 0).any() and (sa["finish_tick"] < 0).any(), "the scenario should finish a part of the batch"
    assert fa.timestep == T_TEST and fa.get_state(0)["timestep"] == T_TEST
    fa.close(); fb.close()


@pytest.mark.parametrize("config", ["ekf64_L20", "ekf32_L20", "ukf_slam_L20"])
def test_replay_of_the_issued_commands(S, config):
    """cmds_out fed to slam_run_sim_each(cmds, T) (multi-step launches for the EKF) on a fresh handle: the same final bits."""
    nav = _nav(*CONTROLS["pp_loose"])
    paths = _paths(_map(20), B_TEST, True)
    st = _starts(paths, B_TEST)
    fa, lm = _make(S, config, B_TEST, starts=st)
    _set(fa, paths, True, nav)
    cmds = fa.run_nav(T_TEST, return_cmds=True)
    fr, _ = _make(S, config, B_TEST, starts=st)
    fr.run_sim(cmds)
    _same_handles(fa, fr, f"replay {config}")
    fa.close(); fr.close()


@pytest.mark.parametrize("config", ["ekf64_L20", "ukf_slam_L20"])
def test_chunking_changes_nothing(S, config, monkeypatch):
    """slam_nav_run cuts its ticks into chunks by the rule of every per-tick run (SLAM_MONITOR_LOG_BYTES over the 8 * batch bytes a tick
    of the command log holds): the chunk size changes no bit of the commands, of the handle or of the controller state."""
    Bn, T = 5, 10
    nav = _nav(*CONTROLS["pp_loose"])
    paths = _paths(_map(20), Bn, True)
    st = _starts(paths, Bn)

    def run(budget, timing=False):
        if budget is None:
            monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
        else:
            monkeypatch.setenv("SLAM_MONITOR_LOG_BYTES", str(budget))
        f, _ = _make(S, config, Bn, starts=st)
        _set(f, paths, True, nav)
        if timing:
            f.set_nav_timing(True)
        return f, f.run_nav(T, return_cmds=True)
    three = 3 * 8 * Bn + 7                       # three ticks per chunk: four chunks, the last of one tick
    ref, cmds = run(None)
    assert cmds.any() and np.isfinite(cmds).all()
    for budget, timing in ((three, False), (1, False), (three, True)):
        f, c = run(budget, timing)
        what = f"{config}, SLAM_MONITOR_LOG_BYTES={budget}, timing {timing}"
        assert np.array_equal(_bits(c), _bits(cmds)), what
        _same_handles(f, ref, what)
        _same_nav_state(f.nav_state(), ref.nav_state(), what)
        if timing:
            ctrl, total = f.last_nav_work()
            assert 0.0 < ctrl < total
        f.close()
    monkeypatch.delenv("SLAM_MONITOR_LOG_BYTES", raising=False)
    fr, _ = _make(S, config, Bn, starts=st)
    fr.run_sim(cmds)
    _same_handles(ref, fr, f"replay {config}")
    ref.close(); fr.close()


def test_more_ticks_than_one_chunk_holds(S):
    """T = 4100 crosses the cap of 4096 ticks per chunk: the commands of both chunks land in their rows (the replay of what was returned
    ends in the same bits) and the rows of the second chunk are written."""
    Bn, T = 2, 4100
    paths = [np.array([[3.0, 0.5], [1.0e5, -1.0]]), np.array([[0.3, 0.0]])]     # instance 0 is under way to the end, instance 1 finishes at once
    fa, _ = _make(S, "ekf64_L20", Bn)
    _set(fa, paths, True, _nav(*CONTROLS["pp_loose"]))
    cmds = fa.run_nav(T, return_cmds=True)
    assert cmds.shape == (T, Bn, 2) and fa.timestep == T and fa.get_state(0)["timestep"] == T
    fr, _ = _make(S, "ekf64_L20", Bn)
    fr.run_sim(cmds)
    _same_handles(fa, fr, "replay of 4100 ticks")
    finish = fa.nav_state()["finish_tick"]
    assert finish[0] == -1 and 0 <= finish[1] < 4096
    assert np.isfinite(cmds).all()
    for t in range(T - 4, T):
        for b in range(Bn):
            done = 0 <= finish[b] <= t
            assert cmds[t, b].any() != done, (t, b, cmds[t, b], finish[b])
    assert cmds[4095, 0].any() and cmds[4096, 0].any()
    fa.close(); fr.close()


@pytest.mark.parametrize("config", ["ekf64_L20", "ukf_slam_L20"])
def test_batch_independence_and_split_calls(S, config):
    nav = _nav(*CONTROLS["pp_loose"])
    paths = _paths(_map(20), B_TEST, True)
    st = _starts(paths, B_TEST)
    fa, lm = _make(S, config, B_TEST, starts=st)
    _set(fa, paths, True, nav)
    ca = fa.run_nav(T_TEST, return_cmds=True)
    sa = fa.nav_state()
    # a sub-batch: instances 128 .. 191 on a handle of their own
    off, n = 128, 64
    fs, _ = _make(S, config, n, offset=off, starts=st[off:off + n])
    _set(fs, paths[off:off + n], True, nav)
    cs = fs.run_nav(T_TEST, return_cmds=True)
    assert np.array_equal(_bits(cs), _bits(ca[:, off:off + n]))
    _same_handles(fs, fa, "sub-batch", count=n, b_offset=off)
    _same_nav_state(fs.nav_state(), {k: v[off:off + n] for k, v in sa.items()}, "sub-batch")
    # T split over two calls
    fc, _ = _make(S, config, B_TEST, starts=st)
    _set(fc, paths, True, nav)
    c1 = fc.run_nav(120, return_cmds=True); c2 = fc.run_nav(T_TEST - 120, return_cmds=True)
    assert np.array_equal(_bits(np.concatenate([c1, c2])), _bits(ca))
    _same_handles(fc, fa, "split calls")
    _same_nav_state(fc.nav_state(), sa, "split calls")
    fa.close(); fs.close(); fc.close()


@pytest.mark.parametrize("control", list(CONTROLS))
def test_properties(S, control):
    nav = _nav(*CONTROLS[control])
    paths = _paths(_map(20), B_TEST, True)
    plen = np.array([len(p) for p in paths])
    st = _starts(paths, B_TEST)
    st_est = st.copy(); st_est[2, 0] = np.nan      # instance 2: the filter starts from a non-finite estimate (the simulator's pose is finite)
    f, lm = _make(S, "ekf64_L20", B_TEST)
    f.init(st_est, truth0=st.astype(np.float64))
    # freeze instance 1 first: a message that repeats a NEW id (ekf.cpp:115 would index out of range); everybody else gets no detections
    meas = np.zeros((B_TEST, 2, 3), np.float32); cnt = np.zeros(B_TEST, np.int32)
    meas[1] = [[8, 1.0, 0.0], [8, 1.0, 0.0]]; cnt[1] = 2
    f.update((0.0, 0.0), meas, cnt)
    assert f.status()[1] & 4
    truth0 = f.truth()[1].copy()
    f.set_paths(paths, nav=nav)
    cmds = f.run_nav(T_TEST, return_cmds=True)
    s = f.nav_state()
    assert np.array_equal(s["remaining"] == 0, s["finish_tick"] >= 0)
    assert np.all(s["remaining"] >= 0) and np.all(s["remaining"] <= plen) and np.all(s["finish_tick"] <= T_TEST)
    assert (s["finish_tick"] >= 0).any() and (s["finish_tick"] < 0).any(), "the scenario should finish a part of the batch"
    for b in np.nonzero((s["finish_tick"] >= 0) & (s["finish_tick"] < T_TEST))[0]:
        assert not cmds[s["finish_tick"][b]:, b].any(), b
        assert cmds[:s["finish_tick"][b], b].any(), b
    assert np.all(cmds[:, :, 0] >= 0) and np.all(cmds[:, :, 0] <= np.float32(f.cfg.d_max)) and np.all(np.abs(cmds[:, :, 1]) <= np.float32(f.cfg.th_max))
    # the frozen instance: (0, 0) throughout, controller state and truth untouched
    assert not cmds[:, 1].any()
    assert s["remaining"][1] == plen[1] and s["finish_tick"][1] == -1 and s["integ"][1] == 0.0 and s["err_prev"][1] == 0.0
    assert np.array_equal(f.truth()[1], truth0)
    # the instance with a non-finite estimate: (0, 0) throughout, controller state untouched; its neighbours are not affected
    assert np.isnan(f.nav_estimates()[2, 0])
    assert not cmds[:, 2].any()
    assert s["remaining"][2] == plen[2] and s["finish_tick"][2] == -1 and s["integ"][2] == 0.0 and s["err_prev"][2] == 0.0
    assert cmds[:, 3].any() and cmds[:, 0].any()
    # slam_init resets the controller state and keeps the path
    f.init(0.0, 0.0, 0.0)
    s = f.nav_state()
    assert np.array_equal(s["remaining"], plen) and np.all(s["finish_tick"] == -1) and not s["integ"].any() and not s["err_prev"].any()
    again = f.run_nav(5, return_cmds=True)
    assert again[:, 1].any()        # no longer frozen
    f.close()


def test_untouched_behaviour(S):
    """A handle that never calls slam_nav_* and one that set a path but ran slam_run_sim: identical bits."""
    from live_ekf_slam_amd.scenario import make_scenario
    for config in ("ekf64_L20", "ukf_slam_L20"):
        _, cmds = make_scenario(SCEN_SEED, 20, 120)
        fx, lm = _make(S, config, 64)
        fy, _ = _make(S, config, 64)
        fy.set_path(lm[:3])
        fx.run_sim(cmds); fy.run_sim(cmds)
        _same_handles(fx, fy, f"untouched {config}")
        s = fy.nav_state()
        assert np.all(s["remaining"] == 3) and np.all(s["finish_tick"] == -1)
        fx.close(); fy.close()


def test_error_codes(S):
    from live_ekf_slam_amd import _lib
    from live_ekf_slam_amd.config import default_nav_config
    L = _lib.lib()
    OK, ARG, STATE = 0, -1, -4
    dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    lm = _map(20)
    path = np.ascontiguousarray(lm[:3])
    cfg = default_nav_config()

    def set_path(f, pts=path, c=cfg):
        pts = np.ascontiguousarray(pts, dtype=np.float64)
        return L.slam_nav_set_path(f.h, C.byref(c), pts.ctypes.data_as(dp), pts.shape[0])

    # before init
    f = S.BatchedEKF(8, 20).readParams(); f.set_map(lm)
    assert set_path(f) == OK
    assert L.slam_nav_run(f.h, 3, None) == STATE
    f.close()
    # before a path is set
    f = S.BatchedEKF(8, 20).readParams(); f.set_map(lm); f.init(0.0, 0.0, 0.0)
    assert L.slam_nav_run(f.h, 3, None) == STATE
    assert L.slam_nav_state(f.h, None, None, None, None) == STATE
    assert L.slam_last_nav_work(f.h, None, None) == STATE
    # bad config, bad path, bad T
    bad = default_nav_config(); bad.dt = 0.0
    assert set_path(f, c=bad) == ARG
    bad = default_nav_config(); bad.method = 7
    assert set_path(f, c=bad) == ARG
    assert set_path(f, pts=[[1.0, 0.0], [1.0, 0.0]]) == ARG
    assert set_path(f, pts=np.stack([np.arange(1025.0), np.zeros(1025)], axis=1)) == ARG
    assert set_path(f, pts=[[np.nan, 0.0]]) == ARG
    pts = np.zeros((8, 2, 2)); pts[:, 1, 0] = 1.0
    cnt = np.full(8, 2, np.int32); cnt[3] = 3
    assert L.slam_nav_set_paths(f.h, C.byref(cfg), pts.ctypes.data_as(dp), cnt.ctypes.data_as(ip), 2) == ARG
    cnt[3] = 0
    assert L.slam_nav_set_paths(f.h, C.byref(cfg), pts.ctypes.data_as(dp), cnt.ctypes.data_as(ip), 2) == ARG
    assert L.slam_nav_run(f.h, 3, None) == STATE       # none of the refused paths was installed
    assert set_path(f) == OK
    assert L.slam_nav_run(f.h, -1, None) == ARG
    assert L.slam_nav_run(f.h, 0, None) == OK
    # while slam_track_instance is on
    f.track_instance(2)
    assert L.slam_nav_run(f.h, 3, None) == STATE
    f.track_instance(-1)
    assert L.slam_nav_run(f.h, 3, None) == OK
    ctrl, total = f.last_nav_work()
    assert ctrl == -1.0 and total > 0.0           # per-tick timing is off by default
    f.set_nav_timing(True)
    assert L.slam_nav_run(f.h, 3, None) == OK
    ctrl, total = f.last_nav_work()
    assert 0.0 < ctrl < total
    f.close()
    # while a prediction stage is pending (UKF): refused before anything moves
    u = S.BatchedUKF(8, 20).readParams(); u.set_map(lm); u.init(0.0, 0.0, 0.0)
    assert L.slam_nav_set_path(u.h, C.byref(cfg), path.ctypes.data_as(dp), path.shape[0]) == OK
    assert L.slam_nav_run(u.h, 2, None) == OK
    before = u.nav_state()
    u.predictionStage(np.tile(np.array([0.05, 0.01], np.float32), (8, 1)))      # slam_predict_each: the update stage will read dcmd_each
    assert L.slam_nav_run(u.h, 2, None) == STATE
    _same_nav_state(u.nav_state(), before, "refused run")
    u.updateStage()
    assert L.slam_nav_run(u.h, 2, None) == OK
    u.close()
    # without a map
    f = S.BatchedEKF(8, 20).readParams(); f.init(0.0, 0.0, 0.0)
    assert set_path(f) == OK
    assert L.slam_nav_run(f.h, 3, None) == STATE
    f.close()


def test_per_instance_maps(S):
    """slam_set_maps: every instance steers through its own map (device route against host route)."""
    nav = _nav(*CONTROLS["pp_loose"])
    B = 64
    lm = _map(20)
    maps = np.stack([lm + 0.01 * b for b in range(B)])
    paths = [maps[b, :3] for b in range(B)]
    fa, _ = _make(S, "ekf64_L20", B); fb, _ = _make(S, "ekf64_L20", B)
    for f in (fa, fb):
        f.set_map(maps); f.init(0.0, 0.0, 0.0); f.set_paths(paths, nav=nav)
    ca = fa.run_nav(150, return_cmds=True)
    pp = _host_controller(fb, paths, nav)
    cb = _host_route(fb, pp, 150)
    assert np.array_equal(_bits(ca), _bits(cb))
    _same_handles(fa, fb, "per-instance maps")
    fa.close(); fb.close()


def test_cpp_mirror_equals_the_python_mirror(S, tmp_path):
    """setPath / runNav / navState of include/slam_filter.hpp (through the host driver) against set_path / run_nav / nav_state."""
    from live_ekf_slam_amd.scenario import make_scenario
    B, L, T = 16, 20, 120
    dump = str(tmp_path / "nav.bin")
    out = subprocess.run([os.path.join(ROOT, "live_ekf_slam_amd", "filter_driver"), "nav", str(B), str(L), str(T), dump, str(SCEN_SEED)],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "driver ok: nav" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    assert int(np.frombuffer(raw[:8], dtype=np.int64)[0]) == B and len(raw) == 8 + T * B * 8 + B * (4 + 4 + 8 + 8)
    lm, _ = make_scenario(SCEN_SEED, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_map(lm)
    f.set_path(lm[:3])
    cmds = f.run_nav(T, return_cmds=True)
    s = f.nav_state()
    assert raw[8:] == cmds.tobytes() + s["remaining"].tobytes() + s["finish_tick"].tobytes() + s["integ"].tobytes() + s["err_prev"].tobytes()
    assert cmds.any()
    f.close()
