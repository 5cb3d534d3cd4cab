"""An independent reference of the sensor fault model (slam_sense*, the *_run_sim calls; include/slam_batch.h) in numpy.  A helper: no tests
in here.  The draws come from the oracle library's orc_noise_pair, the clean message and the advanced true pose from the oracle simulator
(OracleSim.step_philox); what is restated here is the model: dropout, range spike, clutter, order, erased ids, the output row, the labels
and the record."""
import ctypes as C

import numpy as np

from oracle import oracle as O

MAX_DET, MAX_CLUTTER, F = 64, 8, 0x40000000
FROZEN, TOO_LONG = 1, 2
INDEX_OOR = 4
NAN_BITS = 0x7FC00000


def noise_pair(seed, g, step, pair):
    out = np.zeros(2)
    O.lib().orc_noise_pair(int(seed), int(g), int(step), int(pair), out.ctypes.data_as(C.POINTER(C.c_double)))
    return float(out[0]), float(out[1])


def clean(seed, g, step, truth, cmd, map_xy, cfg, vision, sim_noise):
    """(truth_next (3,), clean message (c_vis, 3) float32) of the oracle simulator with the instance's half-widths and vision limits."""
    c = cfg.copy()
    c.V_00, c.V_11, c.W_00, c.W_11 = (float(v) for v in sim_noise)
    c.range_max, c.fov_min, c.fov_max = (float(v) for v in vision)
    sim = O.OracleSim(map_xy, c)
    O.lib().orc_sim_reset(sim.h, float(truth[0]), float(truth[1]), float(truth[2]))
    return sim.step_philox(cmd[0], cmd[1], int(seed), int(g), int(step))


def reference(seed, g, step, truth, cmd, map_xy, cfg, vision, sim_noise, row, k_stride, status=0):
    """Every per-instance output of the model as a dict like live_ekf_slam_amd.sense_instance_host returns."""
    ks = int(k_stride)
    meas = np.zeros((ks, 3), dtype=np.float32)
    origin = np.full(ks, -1, dtype=np.int32); fault = np.zeros(ks, dtype=np.int32)
    rec = np.zeros(16)
    if status & INDEX_OOR:
        rec[1] = 1.0
        return dict(meas=meas, count=0, origin=origin, fault=fault, truth_next=np.array(truth, dtype=np.float64), flags=FROZEN, rec=rec)
    truth_next, msg = clean(seed, g, step, truth, cmd, map_xy, cfg, vision, sim_noise)
    L = np.asarray(map_xy).reshape(-1, 2).shape[0]
    c_vis = msg.shape[0]
    c = min(c_vis, MAX_DET)
    range_max, fov_min, fov_max = (float(v) for v in vision)
    items = []          # (key, position in the shuffle = 0 order, id, r, b, origin, fault)
    n_miss = n_spike = n_clutter = 0
    spike_sum = 0.0
    for v in range(c):
        a_v, b_v = noise_pair(seed, g, step, F + v)
        m_v, k_v = noise_pair(seed, g, step, F + 64 + v)
        if a_v < row.p_miss:
            n_miss += 1
            continue
        r = msg[v, 1]
        spiked = 0
        if b_v < row.p_spike:
            amount = row.spike_lo + (row.spike_hi - row.spike_lo) * m_v
            r = np.float32(np.float64(r) + amount)
            spike_sum = spike_sum + amount
            n_spike += 1
            spiked = 1
        items.append((k_v, len(items), msg[v, 0], r, msg[v, 2], int(msg[v, 0]), spiked))
    for j in range(int(row.n_clutter)):
        ur, ub = noise_pair(seed, g, step, F + 128 + j)
        e_j, kc_j = noise_pair(seed, g, step, F + 136 + j)
        if not e_j < row.p_clutter:
            continue
        n_clutter += 1
        r = np.float32(row.clutter_r_min + (range_max - row.clutter_r_min) * ur)
        beta = np.float32(fov_min + (fov_max - fov_min) * ub)
        items.append((kc_j, len(items), np.float32(L + j), r, beta, -1, 0))
    if row.shuffle:
        items.sort(key=lambda it: (it[0], it[1]))
    n_out = len(items)
    for p, it in enumerate(items[:ks]):
        meas[p] = (it[2], it[3], it[4])
        if row.erase_ids:
            meas[p:p + 1, 0:1].view(np.uint32)[...] = NAN_BITS
        origin[p], fault[p] = it[5], it[6]
    rec[0] = 1.0
    rec[2] = 1.0 if c_vis > MAX_DET else 0.0
    rec[3], rec[4], rec[5], rec[6], rec[7], rec[8], rec[9] = c, n_miss, n_spike, n_clutter, n_out, max(n_out - ks, 0), spike_sum
    return dict(meas=meas, count=n_out, origin=origin, fault=fault, truth_next=truth_next, flags=TOO_LONG if c_vis > MAX_DET else 0, rec=rec)


def same(a, b):
    """Every output of two result dicts equal in bits (floats compared as their bit patterns, so an erased id equals an erased id)."""
    ok = a["count"] == b["count"] and a["flags"] == b["flags"]
    ok = ok and np.asarray(a["meas"], np.float32).tobytes() == np.asarray(b["meas"], np.float32).tobytes()
    ok = ok and np.array_equal(a["origin"], b["origin"]) and np.array_equal(a["fault"], b["fault"])
    ok = ok and np.asarray(a["truth_next"], np.float64).tobytes() == np.asarray(b["truth_next"], np.float64).tobytes()
    return bool(ok and np.asarray(a["rec"], np.float64).tobytes() == np.asarray(b["rec"], np.float64).tobytes())
