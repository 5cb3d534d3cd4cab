"""SLAM_INST_NONFINITE and SLAM_INST_S_SINGULAR as the step kernels raise them on the MI355X, against the CPU oracle: the crafted cases of
failure_flags_reference.py (checked on the oracle alone by test_failure_flags_reference.py) in batches of 64 - the crafted instances at
0, 63 and in between, at least three quarters of the batch healthy neighbours with ordinary messages - through every step-kernel path:

  EKF, one step per launch (slam_step_each: a command per instance)     L_max 20, 50 (both storage types) and 100: ekf_step_kernel<43 | 103 |
        203, .., false> (the barrier-synchronised step of ekf_step_lockstep.h; bulk stream, write_vehicle and the x copy of ekf_kernel_impl.h);
        L_max 201 fp64 and 60 fp32: ekf_big_step_kernel (ekf_big_kernel.hip checks every entry it stores).  Case H (P alone overflows, empty
        message) hangs on write_vehicle, case L (nine detections) on the last pass of a step of several groups (mid_pass)
  EKF, eight queued steps per launch (slam_set_lazy_steps(8) + slam_step)  L_max 20, 50 (both storage types), 100 and 200:
        ekf_step_kernel<43 | 103 | 203 | 403, .., true>: a step of 0 .. 2 updates runs in the
        decoupled control / streamer loop (ekf_step_decoupled.h; `fastable` takes EMPTY messages too, so case C's step stays in that loop -
        its vehicle rows and columns are checked when the loop ends, write_vehicle), an insertion (case E) goes through the lockstep step
  UKF (slam_step_each)  L_max 20, 50: ukf_step_kernel in its LDS classes; 100: ukf_big_step_kernel; ukf_loc with a map of 20

After EVERY launch: status == the oracle's flags for every instance; an instance without bit 1 equals the oracle bit for bit in x, P, M, ids
and timestep; an instance with bit 1 equals it in M, ids and timestep, and bit 1 is set iff the device's own get_state shows a non-finite
entry (the header calls that state undefined: its values are not compared); bits 4 and 32 never appear.

The step queue of slam_step carries ONE command per step for the batch, so a bad command cannot be given to some instances of a multi-step
launch only.  The queued cases with a bad command (C: forward +inf, D: angular NaN) therefore give it to the whole batch at the fourth step:
every instance is then flagged, the crafted ones being those with the empty message (C) or one update (D); the queue of bad MESSAGES (A, B,
E, F, H) keeps its healthy neighbours.  The UKF kinds do have a per-instance command entry (slam_step_each), so case C sits in the same batch."""
import os
import re

import numpy as np
import pytest

import failure_flags_reference as FF
from test_consistency_gpu import _write

pytestmark = pytest.mark.gpu

_REF = {}     # the oracle's walks, computed once per batch of scripts and shared by the tests that use it


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _reference(key, make_scripts, walk):
    if key not in _REF:
        scripts = make_scripts()
        _REF[key] = (scripts, [walk(s) for s in scripts])
    return _REF[key]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check(f, walks, t, what):
    """the device after the launch that ends with step t against the oracle after step t"""
    status = f.status()
    want = np.array([w[t][0] for w in walks], dtype=status.dtype)
    print(f"{what}, step {t}: status of the flagged instances {dict((int(b), int(status[b])) for b in np.nonzero(status)[0][:12])}")
    assert np.array_equal(status, want), f"{what}, step {t}: status differs from the oracle at {[(int(b), int(status[b]), int(want[b])) for b in np.nonzero(status != want)[0]]}"
    assert not (status & (FF.INDEX_OOR | FF.WATCHDOG)).any(), (what, t, status)
    for b in range(f.batch):
        sd, so = f.get_state(b), walks[b][t][1]
        where = f"{what}, step {t}, instance {b}"
        assert sd["M"] == so["M"] and np.array_equal(sd["ids"], so["ids"]) and sd["timestep"] == so["timestep"] == t + 1, where
        if status[b] & FF.NONFINITE:
            assert FF.nonfinite(sd), f"{where}: bit 1 without a non-finite entry of x or P"
        else:
            assert not FF.nonfinite(sd), f"{where}: a non-finite entry of x or P without bit 1"
            assert np.array_equal(_bits(sd["x"]), _bits(so["x"])), f"{where}: x differs from the oracle, max {np.abs(sd['x'] - so['x']).max()}"
            assert np.array_equal(_bits(sd["P"]), _bits(so["P"])), f"{where}: P differs from the oracle, max {np.abs(sd['P'] - so['P']).max()}"
    return status


def _step(f, scripts, t, shared_cmd=False):
    cmds, meas, cnt = FF.pack_step(scripts, t)
    if shared_cmd:      # slam_step: one command for the batch
        assert (cmds.view(np.uint32) == cmds[0].view(np.uint32)).all()
        f.update(cmds[0], meas, cnt)
    else:               # slam_step_each
        f.update(cmds, meas, cnt)


def _ekf_handle(S, scripts, L_max, f32, tmp_path):
    """the start states by checkpoint, the crafted noise rows by slam_set_noise_each"""
    cfg = FF.config()
    dt = S.F32 if f32 else S.F64
    insts = [dict(P=s["st"]["P"], x=s["st"]["x"], M=s["st"]["M"], ids=s["st"]["ids"], truth=np.zeros(3), status=0) for s in scripts]
    path = tmp_path / "failure_flags.ckpt"
    _write(S, L_max, dt, insts, path, tmp_path)
    f = S.BatchedEKF(len(scripts), L_max, dtype=dt).readParams(cfg)
    f.load_state(path); os.remove(path)
    rows = S.config.noise_rows(cfg, len(scripts))
    for b, s in enumerate(scripts):
        if s["noise"] is not None:
            rows[b] = s["noise"]
    f.set_noise(rows)
    return f


def _kernel(f, multi, L_max, f32):
    """the step kernel slam_kernel_info names for this handle, checked against the size class the parametrisation is meant to hit"""
    name = f.kernel_info(multi_step=multi)["name"]
    streamed = L_max > (50 if f32 else 200)
    if streamed:
        assert name == "ekf_big_step_kernel", name
    else:
        m = re.match(r"ekf_step_kernel<(\d+),(\d+),.*,(double|float),\d+,(true|false),\d+>", name)
        nmax = 3 + 2 * (20 if L_max <= 20 else 50 if L_max <= 50 else 100 if L_max <= 100 else 200)
        assert m and int(m.group(1)) == nmax and m.group(3) == ("float" if f32 else "double") and m.group(4) == ("true" if multi else "false"), name
        if multi:
            assert int(m.group(2)) >= 2, f"{name}: the decoupled loop needs a control wavefront and a streamer"
    return name


def _flag_summary(scripts, status):
    return {s["case"] + str(b): int(status[b]) for b, s in enumerate(scripts) if s["case"]}


# ---- EKF, one step per launch ------------------------------------------------------------------------------------------------------------
EKF_SINGLE = [(20, False), (20, True), (50, False), (50, True), (100, False), (201, False), (60, True)]


@pytest.mark.parametrize("L_max,f32", EKF_SINGLE, ids=["L20_f64_lds43", "L20_f32_lds43", "L50_f64_lds103", "L50_f32_lds103", "L100_f64_lds203",
                                                        "L201_f64_streamed", "L60_f32_streamed"])
def test_ekf_single_step_launches(S, oracle, tmp_path, L_max, f32):
    """cases A - F, H and L at the first step (a command per instance: slam_step_each), then three ordinary steps (case G)"""
    T = 4
    scripts, walks = _reference(("ekf", L_max, f32, T, 0), lambda: FF.ekf_batch(7 + L_max, L_max, f32, T, 0),
                                lambda s: FF.walk_ekf(oracle, s, L_max, f32))
    f = _ekf_handle(S, scripts, L_max, f32, tmp_path)
    what = f"EKF L_max={L_max} {'f32' if f32 else 'f64'} {_kernel(f, False, L_max, f32)}"
    for t in range(T):
        _step(f, scripts, t)
        status = _check(f, walks, t, what)
        got = _flag_summary(scripts, status)
        assert got == {s["case"] + str(b): FF.expected_flags(s["case"], f32) for b, s in enumerate(scripts) if s["case"]}, (what, t, got)
    assert (status == 0).sum() >= 3 * FF.B // 4
    f.close()


# ---- EKF, eight queued steps per launch --------------------------------------------------------------------------------------------------
QUEUES = {"messages": dict(cases=("A", "B", "E", "F", "A", "H", "B")), "fwd_inf": dict(cases=("C",) * 7, shared_bad_cmd="C"),
          "ang_nan": dict(cases=("D",) * 7, shared_bad_cmd="D")}


@pytest.mark.parametrize("queue", list(QUEUES))
@pytest.mark.parametrize("L_max,f32", [(20, False), (20, True), (50, False), (50, True), (100, False), (200, False)],
                         ids=["L20_f64", "L20_f32", "L50_f64", "L50_f32", "L100_f64", "L200_f64"])
def test_ekf_multi_step_launch(S, oracle, tmp_path, monkeypatch, L_max, f32, queue):
    """eight slam_step calls queued into ONE launch, the failing step the fourth; the same calls with the queue off (one launch each, checked
    after every one); the two handles agree in status everywhere and in state where bit 1 is not set"""
    T, bad_at = 8, 3
    kw = QUEUES[queue]
    scripts, walks = _reference(("ekf", L_max, f32, T, bad_at, queue), lambda: FF.ekf_batch(9 + L_max, L_max, f32, T, bad_at, **kw),
                                lambda s: FF.walk_ekf(oracle, s, L_max, f32))
    monkeypatch.setenv("SLAM_EAGER_FLUSH", "0")      # (read at slam_create: the queue is launched when it is full, not when the GPU idles)
    lazy, plain = _ekf_handle(S, scripts, L_max, f32, tmp_path), _ekf_handle(S, scripts, L_max, f32, tmp_path)
    what = f"EKF L_max={L_max} {'f32' if f32 else 'f64'} queue '{queue}' {_kernel(lazy, True, L_max, f32)}"
    lazy.set_lazy_steps(T); plain.set_lazy_steps(0)
    from live_ekf_slam_amd import _lib
    for t in range(T):
        _step(lazy, scripts, t, shared_cmd=True)
        assert _lib.lib().slam_queued_steps(lazy.h) == (t + 1) % T, (what, t)       # all eight in one launch
        _step(plain, scripts, t, shared_cmd=True)
        _check(plain, walks, t, what + ", queue off")
    status = _check(lazy, walks, T - 1, what)
    assert np.array_equal(status, plain.status())
    for b in np.nonzero((status & FF.NONFINITE) == 0)[0]:
        a, c = lazy.get_state(int(b)), plain.get_state(int(b))
        assert np.array_equal(_bits(a["x"]), _bits(c["x"])) and np.array_equal(_bits(a["P"]), _bits(c["P"])), (what, b)
    got = _flag_summary(scripts, status)
    print(what, got)
    if "shared_bad_cmd" in kw:
        assert np.all(status == FF.NONFINITE)        # one command per step for the batch: nobody stays healthy (module docstring)
    else:
        assert got == {s["case"] + str(b): FF.expected_flags(s["case"], f32) for b, s in enumerate(scripts) if s["case"]}, (what, got)
        assert (status == 0).sum() >= 3 * FF.B // 4
    lazy.close(); plain.close()


# ---- UKF ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,L_max,M_cap", [("ukf_slam", 20, None), ("ukf_slam", 50, None), ("ukf_slam", 100, 40), ("ukf_loc", 20, None)],
                         ids=["ukf_slam_L20_lds", "ukf_slam_L50_lds", "ukf_slam_L100_ukf_big_kernel", "ukf_loc_map20_lds"])
def test_ukf_steps(S, oracle, kind, L_max, M_cap):
    """cases A, B, C at the fourth step of seven (the first inserts the map), a command per instance (slam_step_each)"""
    from live_ekf_slam_amd.scenario import make_scenario
    T, bad_at = 7, 3
    loc_map = make_scenario(77, L_max, 4)[0] if kind == "ukf_loc" else None
    scripts, walks = _reference((kind, L_max, T, bad_at), lambda: FF.ukf_batch(3 + L_max, L_max, T, bad_at, loc_map=loc_map, M_cap=M_cap),
                                lambda s: FF.walk_ukf(oracle, s, L_max, loc_map))
    if kind == "ukf_loc":
        f = S.BatchedUKFLoc(FF.B).readParams(); f.set_map(loc_map)
    else:
        f = S.BatchedUKF(FF.B, L_max).readParams()
    f.init(0.0, 0.0, 0.0)
    what = f"{kind} L_max={L_max}"
    for t in range(T):
        _step(f, scripts, t)
        status = _check(f, walks, t, what)
        got = _flag_summary(scripts, status)
        assert all(v == (FF.NONFINITE if t >= bad_at else 0) for v in got.values()) and len(got) == 6, (what, t, got)
    assert (status == 0).sum() >= 3 * FF.B // 4
    f.close()


# ---- the producer of the flag and its consumers, once ------------------------------------------------------------------------------------
def test_flagged_instances_reach_consistency_monitor_and_nav(S, oracle, tmp_path):
    """EKF, L_max 20, fp64, after case A (and the other cases of the batch): slam_consistency and slam_monitor_now report INSTANCE_FAILED
    for exactly the instances whose status carries bit 1, and slam_nav_run issues (0, 0) to those of them whose pose is not finite (all but
    case H: the controller looks at the estimate it steers by, as the header says, not at the status)."""
    L_max, f32, T = 20, False, 4
    scripts, walks = _reference(("ekf", L_max, f32, T, 0), lambda: FF.ekf_batch(7 + L_max, L_max, f32, T, 0),
                                lambda s: FF.walk_ekf(oracle, s, L_max, f32))
    f = _ekf_handle(S, scripts, L_max, f32, tmp_path)
    _step(f, scripts, 0)
    status = _check(f, walks, 0, "end to end")
    flagged = (status & FF.NONFINITE) != 0
    assert flagged[0] and scripts[0]["case"] == "A" and flagged.sum() == 6      # A, B, C, D, H, F (E stays finite in fp64)
    rng = np.random.default_rng(5)
    f.set_map(rng.uniform(-8.0, 8.0, (L_max, 2)))
    c = f.consistency()
    assert np.array_equal((c["flags"] & f.INSTANCE_FAILED) != 0, flagged), (c["flags"], status)
    assert np.isnan(c["nees_pose"][flagged]).all() and np.isnan(c["nees_full"][flagged]).all()
    m = f.monitor_now()
    assert np.array_equal((m["flags"] & f.INSTANCE_FAILED) != 0, flagged), (m["flags"], status)
    f.set_paths([np.array([[3.0, 0.5], [5.0, -1.0]])] * FF.B)
    # slam_nav_run reads the ESTIMATE, not the status (slam_batch.h: "an instance whose estimate is not finite, or which is frozen, gets the
    # command (0, 0)"): every flagged instance of cases A - D and F has a non-finite pose; case H (P alone is not finite) is driven on
    pose_bad = ~np.isfinite(f.poses()).all(axis=1)
    is_H = np.array([s["case"] == "H" for s in scripts])
    assert np.array_equal(pose_bad, flagged & ~is_H) and (flagged & is_H).sum() == 1
    cmds = f.run_nav(2, return_cmds=True)
    assert not cmds[:, pose_bad].any(), "slam_nav_run: (0, 0) for the instances with a non-finite estimate"
    assert cmds[0, ~pose_bad].any(axis=1).all(), "slam_nav_run: everybody else is driven"
    assert ((f.status() & FF.NONFINITE) != 0)[flagged].all()
    f.close()
