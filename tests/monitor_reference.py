"""The reference of the run monitor (slam_monitor_now / slam_monitor_run, include/slam_batch.h) on the host.  A helper: no tests in here.

Per instance (the operations of csrc/monitor_kernel.h, one by one, in fp64):
  err_pos   sqrt(wx wx + wy wy), wx = float64(float32(x)) - x_true, wy likewise (the summand of the handle's error sum) - bit for bit
  err_yaw   remainder(yaw - yaw_true, 2 pi); UKF kinds: yaw = remainder(det_atan2(x_t(3), x_t(2)), 2 pi) - bit for bit
  nees_pose e^T S^-1 e in np.longdouble (consistency_reference.solve_hp) with S = (P3 + P3^T) / 2 and e = (x - x_true, y - y_true, err_yaw)
            formed in fp64 exactly as the device forms them, so the reference differs from the device in the factorisation alone
  flags     POSE_NOT_PD, INSTANCE_FAILED by the rules of slam_consistency_flags
Records from per-instance arrays: the 16 entries by plain numpy sums (the device's sums run in another order: the tests allow
B 2^-53 relative on sums of non-negative terms; counts and maxima are exact)."""
import math

import numpy as np

import consistency_reference as R
from live_ekf_slam_amd.navigation import det_atan2

POSE_NOT_PD, INSTANCE_FAILED = R.POSE_NOT_PD, R.INSTANCE_FAILED
NEES_LO, NEES_HI = 0.21579528262389785, 9.348403604496148    # chi-square quantiles at 0.025 / 0.975, 3 degrees of freedom (scipy, recorded)
(N_OK, N_FAILED, N_NEES, N_POSE_NOT_PD, SUM_POS, SUM_POS2, MAX_POS, SUM_YAW2, MAX_YAW, SUM_NEES, N_BELOW, N_ABOVE, SUM_M, N_FULL, SUM_FULL,
 SUM_DOF) = range(16)
SUMS = (SUM_POS, SUM_POS2, SUM_YAW2, SUM_NEES, SUM_FULL)      # the entries whose order of summation differs from numpy's
EXACT = tuple(i for i in range(16) if i not in SUMS)          # counts, maxima and the integer sums (M, dof)


def _rem(v):
    return math.remainder(v, R.TWO_PI) if math.isfinite(v) else math.nan


def instance(x, P3, truth, status=0, ukf=False):
    """dict(err_pos, err_yaw [float], nees_pose [longdouble or NaN], flags, S, e, z) for one instance; x [3] (EKF) or [4] (UKF kinds),
    P3 the leading 3 x 3 block of P as stored, truth [3]."""
    nan = float("nan")
    out = dict(err_pos=nan, err_yaw=nan, nees_pose=np.longdouble("nan"), flags=INSTANCE_FAILED, S=None, e=None, z=None)
    if status & (R.NONFINITE | R.WATCHDOG):
        return out
    x = np.asarray(x, dtype=np.float64); truth = np.asarray(truth, dtype=np.float64)
    with np.errstate(all="ignore"):
        e0, e1 = float(x[0] - truth[0]), float(x[1] - truth[1])
        yaw = _rem(float(det_atan2(x[3], x[2]))) if ukf else float(x[2])
        e2 = _rem(yaw - float(truth[2]))
        if not (math.isfinite(e0) and math.isfinite(e1) and math.isfinite(e2)):
            return out
        wx = np.float64(np.float32(x[0])) - truth[0]
        wy = np.float64(np.float32(x[1])) - truth[1]
        out.update(err_pos=float(np.sqrt(wx * wx + wy * wy)), err_yaw=e2, flags=0)
    if ukf:
        return out
    S = R.symmetric_part(np.asarray(P3, dtype=np.float64).reshape(3, 3))
    e = np.array([e0, e1, e2])
    out["S"], out["e"] = S, e
    y, z, bad = R.solve_hp(S, e)
    if bad is not None:
        out["flags"] = POSE_NOT_PD
    else:
        out["nees_pose"], out["z"] = y @ y, z
    return out


def errors(x, truth, status, ukf=False):
    """err_pos, err_yaw [B] of a whole batch, bit for bit: x [B][3] (EKF: x, y, yaw) or [B][4] (UKF kinds: x, y, cos yaw, sin yaw),
    truth [B][3], status [B].  NaN for the instances that are INSTANCE_FAILED."""
    x, truth = np.asarray(x, dtype=np.float64), np.asarray(truth, dtype=np.float64)
    rem = np.frompyfunc(_rem, 1, 1)
    with np.errstate(all="ignore"):
        yaw = rem(det_atan2(x[:, 3], x[:, 2])).astype(np.float64) if ukf else x[:, 2]
        e0, e1 = x[:, 0] - truth[:, 0], x[:, 1] - truth[:, 1]
        e2 = rem(yaw - truth[:, 2]).astype(np.float64)
        wx = x[:, 0].astype(np.float32).astype(np.float64) - truth[:, 0]
        wy = x[:, 1].astype(np.float32).astype(np.float64) - truth[:, 1]
        pos = np.sqrt(wx * wx + wy * wy)
    failed = ((np.asarray(status) & (R.NONFINITE | R.WATCHDOG)) != 0) | ~(np.isfinite(e0) & np.isfinite(e1) & np.isfinite(e2))
    return np.where(failed, np.nan, pos), np.where(failed, np.nan, e2)


def record(err_pos, err_yaw, nees_pose, flags, M, nees_lo=NEES_LO, nees_hi=NEES_HI, nees_full=None, dof=None):
    """The 16 entries of one record from the per-instance arrays of one tick (M: landmark counts, clamped by the caller)."""
    err_pos, err_yaw, nees_pose = (np.asarray(a, dtype=np.float64) for a in (err_pos, err_yaw, nees_pose))
    flags, M = np.asarray(flags), np.asarray(M)
    ok = (flags & INSTANCE_FAILED) == 0
    fin = ok & np.isfinite(nees_pose)
    r = np.zeros(16)
    r[N_OK], r[N_FAILED], r[N_NEES] = ok.sum(), (~ok).sum(), fin.sum()
    r[N_POSE_NOT_PD] = (ok & ((flags & POSE_NOT_PD) != 0)).sum()
    p, a = err_pos[ok], err_yaw[ok]
    r[SUM_POS], r[SUM_POS2], r[SUM_YAW2] = p.sum(), (p * p).sum(), (a * a).sum()
    r[MAX_POS] = p.max() if p.size else 0.0
    r[MAX_YAW] = np.abs(a).max() if a.size else 0.0
    v = nees_pose[fin]
    r[SUM_NEES], r[N_BELOW], r[N_ABOVE] = v.sum(), (v < nees_lo).sum(), (v > nees_hi).sum()
    r[SUM_M] = M[ok].sum()
    if nees_full is not None:
        full = np.isfinite(np.asarray(nees_full, dtype=np.float64))
        r[N_FULL], r[SUM_FULL], r[SUM_DOF] = full.sum(), np.asarray(nees_full)[full].sum(), np.asarray(dof)[full].sum()
    return r


def flags_from(nees_pose, err_pos, ukf=False):
    """The flags a per-instance SERIES implies (slam_monitor_run returns no flags): all NaN = INSTANCE_FAILED; EKF with a NaN nees_pose
    and a finite error = POSE_NOT_PD."""
    nees_pose, err_pos = np.asarray(nees_pose), np.asarray(err_pos)
    failed = np.isnan(err_pos)
    fl = np.where(failed, INSTANCE_FAILED, 0)
    if not ukf:
        fl = np.where(~failed & np.isnan(nees_pose), POSE_NOT_PD, fl)
    return fl.astype(np.int32)


def assert_record(dev, ref, B, what=""):
    """Counts, maxima and integer sums exactly; each floating sum within B 2^-53 relative (non-negative terms)."""
    dev, ref = np.asarray(dev), np.asarray(ref)
    for i in EXACT:
        assert dev[i] == ref[i], (what, "entry", i, dev[i], ref[i])
    for i in SUMS:
        assert abs(dev[i] - ref[i]) <= B * 2.0 ** -53 * abs(ref[i]), (what, "entry", i, dev[i], ref[i])
