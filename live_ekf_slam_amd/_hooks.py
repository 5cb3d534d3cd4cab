"""TEST HOOKS: the per-instance functions of the kernels compiled for the host (slam_*_instance_host, include/slam_batch.h), one
instance at a time and without a handle or a GPU.  filters.py re-exports them; they are not part of the drop-in surface."""
import ctypes as C

import numpy as np

from . import _lib
from ._marshal import _d, _f, _i, ptr, opt, config_from, JOINT
from .config import INNOV_MAX_DET, default_innovation_config, default_gate_config, default_assoc_config, default_map_config
from .config import default_merge_config, default_fix_config


def _i32s(n):
    return [C.c_int32(0) for _ in range(n)]


def _detection_inputs(x, P, ids, cmd, meas):
    """The state, the ids, the message (k, 3) and the command of the four detection hooks: (x, P, ids, M, c, m)."""
    x = np.ascontiguousarray(x, dtype=np.float64); P = np.ascontiguousarray(P, dtype=np.float64)
    ids = np.ascontiguousarray(ids, dtype=np.int32); M = ids.shape[0]
    m = np.ascontiguousarray(meas, dtype=np.float32).reshape(-1, 3)
    c = np.ascontiguousarray(cmd, dtype=np.float32).reshape(2)
    if x.shape != (3 + 2 * M,) or P.shape != (3 + 2 * M, 3 + 2 * M):
        raise ValueError("x and P do not match the number of ids")
    return x, P, ids, M, c, m


def _message_row(m, count, k_stride):
    """The message padded to the capacity of its row: (row (k_stride, 3), count as given, k_stride)."""
    ks = max(m.shape[0], 1) if k_stride is None else int(k_stride)
    count = m.shape[0] if count is None else int(count)
    if ks < m.shape[0]:
        raise ValueError("k_stride is smaller than the message")
    row = np.zeros((ks, 3), dtype=np.float32); row[:m.shape[0]] = m
    return row, count, ks


def _map_inputs(x, P, ids, L_max, least):
    """The state of the map and merge hooks, copied because the call compacts it in place: (x, P flat, id row of at least `least`
    entries, M, L_max)."""
    x = np.array(x, dtype=np.float64); P = np.array(P, dtype=np.float64)
    ids_in = np.ascontiguousarray(ids, dtype=np.int32); M = ids_in.shape[0]
    if x.shape != (3 + 2 * M,) or P.shape != (3 + 2 * M, 3 + 2 * M):
        raise ValueError("x and P do not match the number of ids")
    L_max = int(L_max)
    row = np.zeros(max(L_max, M, least), dtype=np.int32); row[:M] = ids_in
    return x, np.ascontiguousarray(P).reshape(-1).copy(), row, M, L_max


def _map_outputs(x, Pf, row, Mk, L_max, **more):
    n2 = 3 + 2 * Mk
    return dict(x=x[:n2].copy(), P=Pf[:n2 * n2].reshape(n2, n2).copy(), ids=row[:Mk].copy(), M=Mk, **more, ids_row=row[:L_max].copy())


def sense_instance_host(seed, instance, step, truth, cmd, map_xy, cfg, vision=(3.0, -1.57, 1.57), sim_noise=None, row=None, k_stride=16, status=0):
    """TEST HOOK (slam_sense_instance_host): the sensor model of one instance compiled for the host; no GPU.  cfg: the SlamConfig (d_max,
    th_max and, without sim_noise, the simulator's half-widths V_00, V_11, W_00, W_11); vision: (range_max, fov_min, fov_max).  Returns
    dict(meas (k_stride, 3), count, origin, fault (k_stride,), truth_next (3,), flags, rec (16,))."""
    truth = np.ascontiguousarray(truth, dtype=np.float64)
    c = np.ascontiguousarray(cmd, dtype=np.float32)
    m = np.ascontiguousarray(map_xy, dtype=np.float64).reshape(-1, 2)
    sn = np.ascontiguousarray((cfg.V_00, cfg.V_11, cfg.W_00, cfg.W_11) if sim_noise is None else sim_noise, dtype=np.float64)
    ks = int(k_stride)
    out = dict(meas=np.zeros((max(ks, 0), 3), dtype=np.float32), origin=np.zeros(max(ks, 0), dtype=np.int32), fault=np.zeros(max(ks, 0), dtype=np.int32),
               truth_next=np.zeros(3), rec=np.zeros(16))
    count, flags = _i32s(2)
    _lib.check(_lib.lib().slam_sense_instance_host(int(seed), int(instance), int(step), _d(truth), _f(c), int(status), _d(m), m.shape[0],
                                                   float(cfg.d_max), float(cfg.th_max), float(vision[0]), float(vision[1]), float(vision[2]), _d(sn),
                                                   None if row is None else C.byref(row), ks, _f(out["meas"]), C.byref(count), _i(out["origin"]),
                                                   _i(out["fault"]), _d(out["truth_next"]), C.byref(flags), _d(out["rec"])))
    out["count"], out["flags"] = count.value, flags.value
    return out


def fix_instance_host(x, P, L_max, row, kinds, status=0, f32_storage=False, cfg=None):
    """TEST HOOK (slam_fix_instance_host): the fix of one instance compiled for the host, as two sequential passes; no GPU.  x (3 + 2 M,),
    P (n, n), row (5,), kinds.  Returns dict(x, P (the state after the fix; the input's bytes where no part applied), verdict, nis (2,),
    rec (16,))."""
    x = np.array(x, dtype=np.float64); P = np.array(P, dtype=np.float64)
    n = x.shape[0]; M = (n - 3) // 2
    if n < 3 or n != 3 + 2 * M or P.shape != (n, n):
        raise ValueError("x and P do not describe a state of 3 + 2 M entries")
    r = np.ascontiguousarray(row, dtype=np.float64)
    if r.shape != (5,):
        raise ValueError("a fix row has 5 entries")
    c_cfg = default_fix_config() if cfg is None else cfg
    Pf = np.ascontiguousarray(P).reshape(-1).copy()
    verdict = C.c_int32(0); nis = np.zeros(2); rec = np.zeros(16)
    _lib.check(_lib.lib().slam_fix_instance_host(_d(x), _d(Pf), M, int(L_max), int(status), int(bool(f32_storage)), C.byref(c_cfg), _d(r), int(kinds),
                                                 C.byref(verdict), _d(nis), _d(rec)))
    return dict(x=x, P=Pf.reshape(n, n), verdict=verdict.value, nis=nis, rec=rec)


def fix_sense_instance_host(seed, instance, step, truth, row=None):
    """TEST HOOK (slam_fix_sense_instance_host): the simulated source of fixes of one instance on the host; no GPU.  Returns dict(fix (5,),
    kinds, jumped)."""
    t = np.ascontiguousarray(truth, dtype=np.float64)
    fix = np.zeros(5); kinds, jumped = _i32s(2)
    _lib.check(_lib.lib().slam_fix_sense_instance_host(int(seed), int(instance), int(step), _d(t), None if row is None else C.byref(row), _d(fix),
                                                       C.byref(kinds), C.byref(jumped)))
    return dict(fix=fix, kinds=kinds.value, jumped=jumped.value)


def merge_instance_host(x, P, ids, L_max, status=0, f32_storage=False, cfg=None, seen=None, expected=None, partner=None, fuse=True):
    """TEST HOOK (slam_merge_instance_host): the find, the fusion and the compaction of one instance compiled for the host; no GPU.
    x (3 + 2 M,), P (n, n), ids (M,); seen / expected (L_max,) or None (no counters); partner (L_max,) caller pairs or None (the pairs
    found); fuse=False: the decision alone.  Returns dict(x, P, ids (the merged state), M, partner, d2 (L_max,: the find on the state
    given), rec (16,), seen, expected (L_max,) or None)."""
    x, Pf, row, M, L_max = _map_inputs(x, P, ids, L_max, least=1)
    if (seen is None) != (expected is None):
        raise ValueError("seen and expected come together")
    se = None if seen is None else np.array(seen, dtype=np.int32)
    ex = None if expected is None else np.array(expected, dtype=np.int32)
    pin = None if partner is None else np.ascontiguousarray(partner, dtype=np.int32)
    if pin is not None and pin.shape != (L_max,):
        raise ValueError("partner does not have L_max entries")
    pout = np.zeros(max(L_max, 1), dtype=np.int32); dout = np.zeros(max(L_max, 1)); rec = np.zeros(16); Mo = C.c_int32(0)
    c_cfg = default_merge_config() if cfg is None else cfg
    _lib.check(_lib.lib().slam_merge_instance_host(_d(x), _d(Pf), _i(row), M, L_max, int(status), int(bool(f32_storage)), C.byref(c_cfg),
                                                   ptr(se), ptr(ex),
                                                   ptr(pin), int(bool(fuse)), _i(pout), _d(dout), _d(rec), C.byref(Mo)))
    return _map_outputs(x, Pf, row, Mo.value, L_max, partner=pout[:L_max].copy(), d2=dout[:L_max].copy(), rec=rec,
                        seen=None if se is None else se[:L_max].copy(), expected=None if ex is None else ex[:L_max].copy())


def map_instance_host(x, P, ids, L_max, status=0, meas=None, count=None, k_stride=None, assoc_flag=0, vision=(3.0, -1.57, 1.57), f32_storage=False,
                      cfg=None, seen=None, expected=None, remove=None, prune=False):
    """TEST HOOK (slam_map_instance_host): the tally, the prune decision and the compaction of one instance compiled for the host; no GPU.
    x (3 + 2 M,), P (n, n), ids (M,); meas (k, 3) float32 or None (no tally); vision = (range_max, fov_min, fov_max); seen / expected
    (L_max,) or None (zeros); remove (M,) mask or None; prune: decide by the rule.  Returns dict(x, P, ids (the compacted state), M, mask
    (L_max,), seen, expected (L_max,))."""
    x, Pf, row, M, L_max = _map_inputs(x, P, ids, L_max, least=0)
    se = np.zeros(max(L_max, 1), dtype=np.int32) if seen is None else np.array(seen, dtype=np.int32)
    ex = np.zeros(max(L_max, 1), dtype=np.int32) if expected is None else np.array(expected, dtype=np.int32)
    mp, cnt, ks = None, 0, 1
    if meas is not None:
        mrow, cnt, ks = _message_row(np.ascontiguousarray(meas, dtype=np.float32).reshape(-1, 3), count, k_stride)
        mp = _f(mrow)
    rm = None if remove is None else np.ascontiguousarray(remove, dtype=np.int32)
    if rm is not None and rm.shape != (M,):
        raise ValueError("remove does not match the number of ids")
    if rm is not None and M == 0:
        rm = np.zeros(1, dtype=np.int32)
    mask = np.zeros(max(L_max, 1), dtype=np.int32); Mo = C.c_int32(0)
    c_cfg = default_map_config() if cfg is None else cfg
    _lib.check(_lib.lib().slam_map_instance_host(_d(x), _d(Pf), _i(row), M, L_max, int(status), mp, cnt, ks, int(assoc_flag), float(vision[0]),
                                                 float(vision[1]), float(vision[2]), int(bool(f32_storage)), C.byref(c_cfg), _i(se), _i(ex),
                                                 ptr(rm), int(bool(prune)), _i(mask), C.byref(Mo)))
    return _map_outputs(x, Pf, row, Mo.value, L_max, mask=mask[:L_max].copy(), seen=se[:L_max].copy(), expected=ex[:L_max].copy())


def innovation_instance_host(x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred=False, f32_storage=False, cfg=None):
    """TEST HOOK (slam_innovation_instance_host): the per-instance function of the innovation kernel compiled for the host; no GPU.
    x (3 + 2 M,), P (n, n), ids (M,), meas (k, 3) float32, noise a config.Noise row.  Returns the dict of innovation() for one instance."""
    x, P, ids, M, c, m = _detection_inputs(x, P, ids, cmd, meas)
    out = dict(rec=np.zeros(16), det=np.zeros((INNOV_MAX_DET, 6)), post=np.zeros(12))
    s = C.c_double(0); nu, nn, fl = _i32s(3)
    c_cfg = default_innovation_config() if cfg is None else cfg
    _lib.check(_lib.lib().slam_innovation_instance_host(_d(x), _d(P), opt(ids), M, int(L_max), int(status), _f(c), opt(m), m.shape[0],
                                                        C.byref(noise), int(bool(lm_from_pred)), int(bool(f32_storage)), C.byref(c_cfg),
                                                        _d(out["rec"]), C.byref(s), C.byref(nu), C.byref(nn), C.byref(fl), _d(out["det"]),
                                                        _d(out["post"])))
    out.update(nis_sum=s.value, n_upd=nu.value, n_new=nn.value, flags=fl.value)
    return out


def gate_instance_host(x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred=False, f32_storage=False, cfg=None, count=None, k_stride=None):
    """TEST HOOK (slam_gate_instance_host): the per-instance function of the gate kernel compiled for the host; no GPU.  Arguments as
    innovation_instance_host; count (default: the rows of meas) is the count as given and k_stride (default: max(rows, 1)) the capacity
    of the message row.  Returns the dict of gate() for one instance: meas_out (k_stride, 3) starts as a copy of the input row."""
    x, P, ids, M, c, m = _detection_inputs(x, P, ids, cmd, meas)
    row, count, ks = _message_row(m, count, k_stride)
    out = dict(rec=np.zeros(16), det=np.zeros((INNOV_MAX_DET, 6)), post=np.zeros(12), meas_out=row.copy(), verdict=np.zeros(INNOV_MAX_DET, dtype=np.int32))
    s = C.c_double(0); nu, nn, fl, co, nr = _i32s(5)
    c_cfg = default_gate_config() if cfg is None else cfg
    _lib.check(_lib.lib().slam_gate_instance_host(_d(x), _d(P), opt(ids), M, int(L_max), int(status), _f(c), _f(row), count, ks,
                                                  C.byref(noise), int(bool(lm_from_pred)), int(bool(f32_storage)), C.byref(c_cfg),
                                                  _d(out["rec"]), C.byref(s), C.byref(nu), C.byref(nn), C.byref(fl), _d(out["det"]),
                                                  _d(out["post"]), _f(out["meas_out"]), C.byref(co), C.byref(nr), _i(out["verdict"])))
    out.update(nis_sum=s.value, n_upd=nu.value, n_new=nn.value, flags=fl.value, count_out=co.value, n_rej=nr.value)
    return out


def _associate_host(symbol, c_cfg, x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred, f32_storage, count, k_stride, joint):
    """associate_instance_host and its joint twin, whose call ends in three more outputs: d2_joint, nodes, ncand."""
    x, P, ids, M, c, m = _detection_inputs(x, P, ids, cmd, meas)
    row, count, ks = _message_row(m, count, k_stride)
    k_in = min(max(count, 0), ks)
    out = dict(rec=np.zeros(16), cost=np.full((k_in if k_in <= INNOV_MAX_DET else 0, M), np.nan), verdict=np.zeros(INNOV_MAX_DET, dtype=np.int32),
               slot=np.zeros(INNOV_MAX_DET, dtype=np.int32), det=np.zeros((INNOV_MAX_DET, 4)), meas_out=row.copy())
    nm, nn, nd, fl, co, no = _i32s(6); d2 = C.c_double(0)
    tail = ()
    if joint:
        out["ncand"] = np.zeros(INNOV_MAX_DET, dtype=np.int32)
        tail = (C.byref(d2), C.byref(no), _i(out["ncand"]))
    _lib.check(getattr(_lib.lib(), symbol)(_d(x), _d(P), opt(ids), M, int(L_max), int(status), _f(c), _f(row), count, ks, C.byref(noise),
                      int(bool(lm_from_pred)), int(bool(f32_storage)), C.byref(c_cfg), _d(out["rec"]), C.byref(nm), C.byref(nn), C.byref(nd), C.byref(fl),
                      opt(out["cost"]), _i(out["verdict"]), _i(out["slot"]), _d(out["det"]), _f(out["meas_out"]), C.byref(co), *tail))
    out.update(n_match=nm.value, n_new=nn.value, n_drop=nd.value, flags=fl.value, count_out=co.value)
    if joint:
        out.update(d2_joint=d2.value, nodes=no.value)
    return out


def associate_instance_host(x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred=False, f32_storage=False, cfg=None, count=None, k_stride=None):
    """TEST HOOK (slam_associate_instance_host): the per-instance function of the association kernel compiled for the host; no GPU.
    Arguments as gate_instance_host (the id column of meas is not read).  Returns the dict of associate() for one instance, plus cost
    (count_in, M), the full matrix; meas_out (k_stride, 3) starts as a copy of the input row."""
    c_cfg = default_assoc_config() if cfg is None else cfg
    return _associate_host("slam_associate_instance_host", c_cfg, x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred, f32_storage,
                           count, k_stride, joint=False)


def associate_joint_instance_host(x, P, ids, L_max, status, cmd, meas, noise, lm_from_pred=False, f32_storage=False, cfg=None, count=None,
                                  k_stride=None):
    """TEST HOOK (slam_associate_joint_instance_host): the per-instance function of the joint association kernel compiled for the host; no
    GPU.  Arguments as associate_instance_host (cfg: a JointConfig, a dict of its fields, or None).  Returns its dict plus d2_joint, nodes
    and ncand (INNOV_MAX_DET,)."""
    return _associate_host("slam_associate_joint_instance_host", config_from(cfg, *JOINT), x, P, ids, L_max, status, cmd, meas, noise,
                           lm_from_pred, f32_storage, count, k_stride, joint=True)
