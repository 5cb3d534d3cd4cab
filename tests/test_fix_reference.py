"""The absolute position and heading fix without a GPU: the host hook (slam_fix_instance_host, compiled from csrc/fix_kernel.h, the source
the kernel compiles) against the independent numpy reference of tests/fix_reference.py in bits, against the information-form posterior
in mpmath, the simulated source against its restatement, and the behaviour - dead reckoning bounded by fixes - driven with the oracle
EKF and the reference alone."""
import math

import numpy as np
import pytest

import fix_reference as FR
from merge_reference import as_stored

L_MAXES = (20, 50)
HOWS = ("near", "far_pos", "far_yaw", "nan_sigma", "inf_z", "neg_sigma", "zero_block", "skip")


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes()


def _state(rng, M, f32, scale=0.02):
    """An SPD P that is symmetric only to rounding, and an x of a few units."""
    n = 3 + 2 * M
    A = rng.uniform(-0.5, 0.5, (n, n)) * scale
    P = A @ A.T + 1.6e-5 * np.eye(n)
    P = P * (1.0 + 1e-9 * (np.arange(n)[:, None] - np.arange(n)[None, :]))
    x = np.concatenate([rng.uniform(-0.5, 0.5, 3), rng.uniform(-4.0, 4.0, 2 * M)])
    return as_stored(x, f32), as_stored(P, f32)


def _case(rng, how, x, P):
    """(row, status, P) of one verdict scenario on the state."""
    row = np.array([x[0] + 0.01, x[1] - 0.015, x[2] + 0.01, 0.05, 0.02])
    status = 0
    if how == "far_pos":
        row[1] += 30.0
    elif how == "far_yaw":
        row[2] += 2.0
    elif how == "nan_sigma":
        row[3] = math.nan; row[4] = math.inf
    elif how == "inf_z":
        row[0] = math.inf; row[2] = math.nan
    elif how == "neg_sigma":
        row[3] = -0.05; row[4] = -1e-300
    elif how == "zero_block":
        P = P.copy(); P[0:2, :] = 0.0; P[:, 0:2] = 0.0
        row[3] = 0.0
    elif how == "skip":
        status = int(rng.choice([1, 4, 32, 5]))
    return row, status, P


def _expected(how, kinds):
    vp = {"near": 1, "far_pos": 2, "far_yaw": 1, "nan_sigma": 4, "inf_z": 4, "neg_sigma": 4, "zero_block": 3, "skip": 0}[how] if kinds & 1 else 0
    vy = {"near": 1, "far_pos": 1, "far_yaw": 2, "nan_sigma": 4, "inf_z": 4, "neg_sigma": 4, "zero_block": 1, "skip": 0}[how] if kinds & 2 else 0
    return 0 if how == "skip" else vp | (vy << 4)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", L_MAXES)
def test_hook_equals_the_reference_in_bits(S, L_max, f32):
    rng = np.random.default_rng(300 + L_max + int(f32))
    seen = set()
    for M in (0, 1, 2, 7, L_max - 1, L_max):
        x0, P0 = _state(rng, M, f32)
        for how in HOWS:
            row, status, P = _case(rng, how, x0, P0)
            for kinds in (0, 1, 2, 3, 3 | 8):
                h = S.fix_instance_host(x0, P, L_max, row, kinds, status=status, f32_storage=f32)
                r = FR.reference_fix(x0, P, row, kinds, status=status, f32=f32)
                what = (M, how, kinds)
                assert h["verdict"] == r["verdict"] == _expected(how, kinds), (what, h["verdict"], r["verdict"])
                assert _bits(h["nis"]) == _bits(r["nis"]) and _bits(h["rec"]) == _bits(r["rec"]), (what, h["nis"], r["nis"], h["rec"], r["rec"])
                assert _bits(h["x"]) == _bits(r["x"]) and _bits(h["P"]) == _bits(r["P"]), what
                if not r["written"]:                  # an instance without an applied part keeps its bytes
                    assert _bits(h["x"]) == _bits(x0) and _bits(h["P"]) == _bits(P), what
                else:
                    assert _bits(h["P"]) != _bits(P), what
                seen.add(h["verdict"])
    assert {0x00, 0x01, 0x10, 0x11, 0x02, 0x12, 0x21, 0x20, 0x44, 0x04, 0x40, 0x13, 0x03} <= seen, sorted(hex(v) for v in seen)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_a_nis_equal_to_the_gate_is_accepted_and_the_next_smaller_gate_rejects(S, f32):
    rng = np.random.default_rng(17)
    x, P = _state(rng, 7, f32)
    row = np.array([x[0] + 0.03, x[1] - 0.02, x[2] + 0.04, 0.05, 0.02])
    open_cfg = S.FixConfig(math.inf, math.inf, 10)
    nis_p = S.fix_instance_host(x, P, 20, row, 1, f32_storage=f32, cfg=open_cfg)["nis"][0]
    nis_y = S.fix_instance_host(x, P, 20, row, 2, f32_storage=f32, cfg=open_cfg)["nis"][1]
    assert nis_p > 0 and nis_y > 0
    for kinds, nis, field in ((1, nis_p, "gate_pos"), (2, nis_y, "gate_yaw")):
        at = S.default_fix_config(); setattr(at, field, nis)
        below = S.default_fix_config(); setattr(below, field, math.nextafter(nis, 0.0))
        a = S.fix_instance_host(x, P, 20, row, kinds, f32_storage=f32, cfg=at)
        b = S.fix_instance_host(x, P, 20, row, kinds, f32_storage=f32, cfg=below)
        sh = 0 if kinds == 1 else 4
        assert a["verdict"] == FR.APPLIED << sh and b["verdict"] == FR.REJECTED << sh
        gates = lambda c: (c.gate_pos, c.gate_yaw)
        for got, c in ((a, at), (b, below)):
            r = FR.reference_fix(x, P, row, kinds, gates=gates(c), f32=f32)
            assert got["verdict"] == r["verdict"] and _bits(got["P"]) == _bits(r["P"]) and _bits(got["nis"]) == _bits(r["nis"])
        assert _bits(b["P"]) == _bits(P) and _bits(b["nis"]) == _bits(a["nis"]), "a rejected part reports its nis and writes nothing"


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_both_parts_in_one_call_equal_position_then_heading(S, f32):
    rng = np.random.default_rng(23)
    for L_max in L_MAXES:
        for M in (0, 2, 7, L_max):
            x, P = _state(rng, M, f32)
            row = np.array([x[0] - 0.02, x[1] + 0.01, x[2] - 0.015, 0.03, 0.01])
            both = S.fix_instance_host(x, P, L_max, row, 3, f32_storage=f32)
            a = S.fix_instance_host(x, P, L_max, row, 1, f32_storage=f32)
            b = S.fix_instance_host(a["x"], a["P"], L_max, row, 2, f32_storage=f32)
            assert both["verdict"] == 0x11 and a["verdict"] == 0x01 and b["verdict"] == 0x10
            assert _bits(both["x"]) == _bits(b["x"]) and _bits(both["P"]) == _bits(b["P"]), (L_max, M)
            assert _bits(both["nis"]) == _bits([a["nis"][0], b["nis"][1]])


def test_an_input_that_is_not_representable_in_fp32_is_untouched_when_nothing_applies(S):
    rng = np.random.default_rng(5)
    x, P = _state(rng, 3, False)
    row = np.array([x[0] + 40.0, x[1], x[2] + 2.5, 0.05, 0.02])
    h = S.fix_instance_host(x, P, 20, row, 3, f32_storage=True)
    assert h["verdict"] == 0x22 and _bits(h["x"]) == _bits(x) and _bits(h["P"]) == _bits(P)
    assert _bits(as_stored(P, True)) != _bits(P)


def test_against_the_information_form_posterior_in_mpmath(S):
    """(P^-1 + H^T R^-1 H)^-1 and x + P' H^T R^-1 (z - H x) at 50 digits.  The bound is 4 x the numpy reference's own error against mpmath
    on the same inputs (the hook differs from the reference by nothing but storage rounding in fp64).  Measured on these inputs: the
    reference's largest error is 2.74e-19 in P (entries below 1e-3) and 4.05e-16 in x (entries up to 4), so the bounds come to 1.1e-18
    and 1.6e-15; the hook's errors are the reference's, 2.74e-19 and 4.05e-16, since the two agree in bits."""
    mpmath = pytest.importorskip("mpmath")
    mpmath.mp.dps = 50
    rng = np.random.default_rng(41)
    worst = [0.0, 0.0, 0.0, 0.0]
    for M in (0, 2, 7, 20):
        x, P = _state(rng, M, False)
        P = 0.5 * (P + P.T)
        n = 3 + 2 * M
        row = np.array([x[0] + 0.01, x[1] - 0.015, x[2] + 0.01, 0.05, 0.02])
        for kinds in (1, 2, 3):
            sel = [i for i, bit in ((0, 1), (1, 1), (2, 2)) if kinds & bit]
            H = mpmath.zeros(len(sel), n)
            for a, i in enumerate(sel):
                H[a, i] = 1
            Rinv = mpmath.diag([1 / mpmath.mpf(float(row[3] if i < 2 else row[4])) ** 2 for i in sel])
            Pm = mpmath.matrix(P.tolist())
            post = mpmath.inverse(mpmath.inverse(Pm) + H.T * Rinv * H)
            z = mpmath.matrix([mpmath.mpf(float(row[i])) for i in sel])
            xm = mpmath.matrix([mpmath.mpf(float(v)) for v in x])
            xpost = xm + post * H.T * Rinv * (z - H * xm)
            exactP = np.array([[post[r, c] for c in range(n)] for r in range(n)], dtype=object)
            exactx = np.array([xpost[r] for r in range(n)], dtype=object)
            r = FR.reference_fix(x, P, row, kinds)
            h = S.fix_instance_host(x, P, 50, row, kinds)
            errs = []
            for got in (r, h):
                eP = max(abs(mpmath.mpf(float(got["P"][i, j])) - exactP[i, j]) for i in range(n) for j in range(n))
                ex = max(abs(mpmath.mpf(float(got["x"][i])) - exactx[i]) for i in range(n))
                errs += [float(eP), float(ex)]
            print(f"M={M} kinds={kinds}: reference |dP| {errs[0]:.3g} |dx| {errs[1]:.3g}; hook |dP| {errs[2]:.3g} |dx| {errs[3]:.3g}")
            assert errs[0] > 0 and errs[1] > 0
            assert errs[2] <= 4 * errs[0] and errs[3] <= 4 * errs[1], (M, kinds, errs)
            worst = [max(a, b) for a, b in zip(worst, errs)]
    print(f"largest errors: reference |dP| {worst[0]:.3g} |dx| {worst[1]:.3g}; hook |dP| {worst[2]:.3g} |dx| {worst[3]:.3g}")


def test_the_simulated_source_equals_its_restatement_in_bits(S, oracle):
    import ctypes as C
    R = S.default_fix_sensor_config
    rows = [R(), R(kinds=3), R(pos_halfwidth=0.5, yaw_halfwidth=0.1, sigma_pos=0.3, sigma_yaw=0.06, kinds=3),
            R(pos_halfwidth=0.5, sigma_pos=0.3, kinds=1), R(yaw_halfwidth=0.1, sigma_yaw=0.06, kinds=2),
            R(pos_halfwidth=0.2, yaw_halfwidth=0.05, sigma_pos=0.1, sigma_yaw=0.03, p_jump=1.0, jump_lo=2.0, jump_hi=5.0, kinds=3),
            R(pos_halfwidth=0.2, yaw_halfwidth=0.05, sigma_pos=0.1, sigma_yaw=0.03, p_miss_pos=0.5, p_miss_yaw=0.5, p_jump=0.5, jump_lo=1.0, jump_hi=1.0, kinds=3),
            R(pos_halfwidth=0.2, sigma_pos=0.1, p_miss_pos=1.0, p_miss_yaw=1.0, p_jump=1.0, jump_hi=3.0, kinds=3)]
    rng = np.random.default_rng(9)
    kinds_seen, jumps = set(), 0
    for k, row in enumerate(rows):
        for trial in range(24):
            seed, inst, step = int(rng.integers(0, 2 ** 63)), int(rng.integers(0, 2 ** 40)), int(rng.integers(0, 2 ** 31))
            truth = np.array([rng.uniform(-5, 5), rng.uniform(-5, 5), rng.uniform(-3.1, 3.1)])
            got = S.fix_sense_instance_host(seed, inst, step, truth, row)
            ref = FR.reference_sense(seed, inst, step, truth, row)
            assert got["kinds"] == ref["kinds"] and got["jumped"] == ref["jumped"] and _bits(got["fix"]) == _bits(ref["fix"]), (k, trial, got, ref)
            kinds_seen.add((k, got["kinds"])); jumps += got["jumped"]
            if k == 0:                                # the all-zero row emits nothing
                assert got["kinds"] == 0 and not got["fix"].any() and got["jumped"] == 0
            if k == 7:
                assert got["kinds"] == 0 and got["jumped"] == 0 and not got["fix"][:3].any()
    assert {(6, 0), (6, 1), (6, 2), (6, 3)} <= kinds_seen and jumps > 24
    assert _bits(S.fix_sense_instance_host(1, 2, 3, [1.0, 2.0, 0.5], None)["fix"]) == _bits(np.zeros(5))
    # the restated generator is the oracle's
    out = np.zeros(2)
    for p in (FR.PAIR_G, FR.PAIR_G + 3):
        oracle.lib().orc_noise_pair(77, 2 ** 33 + 5, 12, p, out.ctypes.data_as(C.POINTER(C.c_double)))
        assert tuple(out) == FR.noise_pair(77, 2 ** 33 + 5, 12, p)


def test_position_fixes_bound_dead_reckoning_and_keep_the_pose_consistent(S, oracle):
    """64 instances, every landmark out of range for the whole run, with the oracle EKF and the reference alone: the batch-mean position
    error at the end is lower with position fixes every 10 ticks than without, and the mean pose NEES with fixes lies inside the band
    consistency_summary gives for 3 degrees of freedom per instance."""
    from live_ekf_slam_amd.filters import consistency_summary
    O = oracle
    B, T, every = 64, 120, 10
    a_d, a_th, a_fix = 0.01, 0.002, 0.03                 # half-widths of the motion noise and of the position fix
    cfg = S.default_config()
    cfg.replicate_vw_quirk = 0
    cfg.v_d = cfg.v_th = 0.0
    cfg.V_00, cfg.V_11 = a_d * a_d / 3.0, a_th * a_th / 3.0     # the variance of a uniform draw of half-width a
    sigma = a_fix / math.sqrt(3.0)
    rng = np.random.default_rng(64)
    cmds = np.stack([np.full(T, 0.05), 0.02 * np.sin(np.arange(T) / 9.0)], axis=1).astype(np.float32)
    err = {False: [], True: []}
    nees = []
    for b in range(B):
        dd = cmds[:, 0].astype(np.float64) + rng.uniform(-a_d, a_d, T)
        hh = cmds[:, 1].astype(np.float64) + rng.uniform(-a_th, a_th, T)
        zs = rng.uniform(-a_fix, a_fix, (T, 2))
        for fixes in (False, True):
            ekf = O.OracleEKF(cfg, L_max=20)
            ekf.init(0.0, 0.0, 0.0)
            truth = np.zeros(3)
            for t in range(T):
                truth = np.array([truth[0] + dd[t] * math.cos(truth[2]), truth[1] + dd[t] * math.sin(truth[2]), truth[2] + hh[t]])
                assert ekf.update(cmds[t, 0], cmds[t, 1], np.zeros((0, 3), np.float32)) == 0
                if fixes and (t + 1) % every == 0:
                    st = ekf.state()
                    row = np.array([truth[0] + zs[t, 0], truth[1] + zs[t, 1], 0.0, sigma, 0.0])
                    r = FR.reference_fix(st["x"], st["P"], row, FR.POS)
                    assert r["verdict"] == FR.APPLIED, (b, t, r["verdict"], r["nis"])
                    ekf.set_state(r["x"], r["P"], st["ids"], timestep=st["timestep"])
            st = ekf.state()
            e = np.array([st["x"][0] - truth[0], st["x"][1] - truth[1], math.remainder(st["x"][2] - truth[2], FR.TWO_PI)])
            err[fixes].append(math.hypot(e[0], e[1]))
            if fixes:
                nees.append(float(e @ np.linalg.solve(st["P"][:3, :3], e)))
    free, fixed = float(np.mean(err[False])), float(np.mean(err[True]))
    s = consistency_summary(np.array(nees), np.full(B, 3), np.zeros(B, dtype=np.int32))
    print(f"mean position error after {T} ticks: {free:.4f} m without fixes, {fixed:.4f} m with; pose NEES / dof {s['normalised']:.3f} in [{s['lower']:.3f}, {s['upper']:.3f}]")
    assert fixed < free
    assert s["count"] == B and s["lower"] <= s["normalised"] <= s["upper"], s
