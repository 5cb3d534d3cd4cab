"""The sensor fault model (csrc/sense_kernel.h) without a GPU: the host hook - the kernel's own per-instance function compiled for the
host - against the oracle simulator with the all-off row, against the independent numpy reference (tests/sense_reference.py) with the faults
on, in every output bit, and the rates of its draws against their probabilities."""
import math

import numpy as np
import pytest

import sense_reference as SR
from live_ekf_slam_amd import default_config, default_sensor_config, sense_instance_host

VISION = (3.0, -1.57, 1.57)


def _case(rng, L=None, spread=3.0):
    """A random (seed, instance, step, pose, command, map, simulator half-widths)."""
    L = int(rng.integers(1, 31)) if L is None else L
    truth = np.array([rng.uniform(-2, 2), rng.uniform(-2, 2), rng.uniform(-3.5, 3.5)])
    lm = truth[:2] + rng.uniform(-spread, spread, (L, 2))
    cmd = np.array([rng.uniform(-0.02, 0.13), rng.uniform(-0.08, 0.08)], dtype=np.float32)      # beyond d_max, th_max and below 0 too
    sn = (rng.uniform(0, 0.05), rng.uniform(0, 0.01), rng.uniform(0, 0.05), rng.uniform(0, 0.05))
    return dict(seed=int(rng.integers(0, 2 ** 63)), g=int(rng.integers(0, 2 ** 40)), step=int(rng.integers(0, 2 ** 31)), truth=truth, cmd=cmd,
                map_xy=lm, sim_noise=sn)


def _crowd(rng, n):
    """n landmarks on an arc in front of the pose, all in view."""
    c = _case(rng, L=1)
    ang = c["truth"][2] + np.linspace(-1.2, 1.2, n)
    rad = rng.uniform(0.8, 2.5, n)
    c["map_xy"] = c["truth"][:2] + np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1)
    c["cmd"] = np.array([0.05, 0.01], dtype=np.float32)
    return c


def _behind(rng):
    """landmarks behind the vehicle or out of range: an empty view"""
    c = _case(rng, L=1)
    th = c["truth"][2]
    back = c["truth"][:2] - 1.5 * np.array([math.cos(th), math.sin(th)])
    far = c["truth"][:2] + 9.0 * np.array([math.cos(th), math.sin(th)])
    c["map_xy"] = np.stack([back, far, back + 0.2])
    c["cmd"] = np.array([0.05, 0.0], dtype=np.float32)
    return c


def _hook(c, cfg, row, ks, status=0):
    return sense_instance_host(c["seed"], c["g"], c["step"], c["truth"], c["cmd"], c["map_xy"], cfg, vision=VISION, sim_noise=c["sim_noise"],
                               row=row, k_stride=ks, status=status)


def _ref(c, cfg, row, ks, status=0):
    return SR.reference(c["seed"], c["g"], c["step"], c["truth"], c["cmd"], c["map_xy"], cfg, VISION, c["sim_noise"], row, ks, status)


def test_the_default_row_is_the_oracle_simulator_bit_for_bit(oracle):
    rng = np.random.default_rng(20261020)
    cfg = default_config()
    cases = [_crowd(rng, 80), _crowd(rng, 65), _crowd(rng, 64), _behind(rng)] + [_case(rng) for _ in range(196)]
    seen_long = seen_empty = 0
    for c in cases:
        truth_next, msg = SR.clean(c["seed"], c["g"], c["step"], c["truth"], c["cmd"], c["map_xy"], cfg, VISION, c["sim_noise"])
        ks = max(msg.shape[0], 1) + 2
        for row in (None, default_sensor_config()):
            got = _hook(c, cfg, row, ks)
            kept = min(msg.shape[0], SR.MAX_DET)
            assert got["count"] == kept
            assert got["truth_next"].tobytes() == truth_next.tobytes()
            assert got["meas"][:kept].tobytes() == msg[:kept].tobytes()
            assert not got["meas"][kept:].any() and (got["origin"][kept:] == -1).all() and not got["fault"].any()
            assert np.array_equal(got["origin"][:kept], msg[:kept, 0].astype(np.int32))
            assert got["flags"] == (SR.TOO_LONG if msg.shape[0] > SR.MAX_DET else 0)
        seen_long += msg.shape[0] > SR.MAX_DET
        seen_empty += msg.shape[0] == 0
    assert len(cases) == 200 and seen_long >= 2 and seen_empty >= 1


def _rows(rng):
    """The edge rows of the issue, then random ones: 500 in all, shuffle and erase in all four combinations."""
    R = default_sensor_config
    rows = [R(), R(p_miss=1.0), R(p_spike=1.0, spike_lo=0.5, spike_hi=0.5), R(p_spike=1.0, spike_lo=-0.4, spike_hi=1.5),
            R(p_clutter=1.0, n_clutter=8), R(p_clutter=1.0, n_clutter=0), R(p_clutter=0.0, n_clutter=8), R(p_miss=1.0, p_clutter=1.0, n_clutter=8),
            R(p_clutter=1.0, n_clutter=8, clutter_r_min=VISION[0]), R(p_clutter=1.0, n_clutter=3, clutter_r_min=1.0)]
    rows = [R(**dict({k: getattr(r, k) for k, _ in r._fields_}, shuffle=s, erase_ids=e)) for r in rows for s in (0, 1) for e in (0, 1)]
    while len(rows) < 500:
        lo = rng.uniform(-1.0, 1.0)
        rows.append(R(p_miss=rng.choice([0.0, 1.0, rng.uniform()]), p_spike=rng.choice([0.0, 1.0, rng.uniform()]), spike_lo=lo,
                      spike_hi=lo + rng.choice([0.0, rng.uniform(0, 2.0)]), p_clutter=rng.choice([0.0, 1.0, rng.uniform()]),
                      clutter_r_min=rng.uniform(0, VISION[0]), n_clutter=int(rng.integers(0, 9)), shuffle=int(rng.integers(0, 2)),
                      erase_ids=int(rng.integers(0, 2))))
    return rows


def test_faults_on_the_hook_equals_the_reference_in_every_bit(oracle):
    rng = np.random.default_rng(77)
    cfg = default_config()
    rows = _rows(rng)
    assert len(rows) == 500
    short = long_ = 0
    for i, row in enumerate(rows):
        c = _crowd(rng, int(rng.choice([5, 12, 64, 70]))) if i % 3 == 0 else _case(rng)
        ks = int(rng.choice([1, 3, 16, 80]))
        status = SR.INDEX_OOR if i % 41 == 7 else (1 if i % 41 == 8 else 0)     # frozen; another status bit alone does not freeze
        got, want = _hook(c, cfg, row, ks, status), _ref(c, cfg, row, ks, status)
        assert SR.same(got, want), (i, {k: getattr(row, k) for k, _ in row._fields_}, ks, got["count"], want["count"], got["rec"], want["rec"])
        if row.erase_ids and got["count"]:
            assert (got["meas"][:min(got["count"], ks), 0].view(np.uint32) == SR.NAN_BITS).all()
        short += got["count"] > ks
        long_ += got["flags"] == SR.TOO_LONG
    assert short >= 20 and long_ >= 5       # k_stride smaller than n_out, and more than 64 in view, both occur


def test_rates_of_the_draws():
    """One row over 20 000 instance-ticks with exactly one landmark in view, so the dropout share is a share of 20 000 trials."""
    cfg = default_config()
    row = default_sensor_config(p_miss=0.3, p_spike=0.2, spike_lo=0.5, spike_hi=1.5, p_clutter=0.5, n_clutter=8, clutter_r_min=0.5)
    truth = np.zeros(3); lm = np.array([[1.5, 0.2]]); cmd = np.array([0.05, 0.0], dtype=np.float32)
    N = 20000
    rec = np.zeros(16)
    cl_r, cl_b = [], []
    for g in range(N):
        out = sense_instance_host(2025, g, g % 7, truth, cmd, lm, cfg, vision=VISION, row=row, k_stride=9)
        rec += out["rec"]
        k = min(out["count"], 9)
        clutter = out["origin"][:k] == -1
        cl_r.append(out["meas"][:k][clutter, 1]); cl_b.append(out["meas"][:k][clutter, 2])
    assert rec[0] == N and rec[3] == N and rec[8] == 0            # one clean detection per tick, no row overflows
    sd = (lambda p, n: math.sqrt(p * (1 - p) / n))
    assert abs(5 * sd(0.3, N) - 0.0162) < 5e-5
    survivors = N - rec[4]
    shares = dict(miss=(rec[4] / N, 0.3, N), spike=(rec[5] / survivors, 0.2, survivors), clutter=(rec[6] / (8 * N), 0.5, 8 * N))
    for name, (share, p, n) in shares.items():
        assert abs(share - p) <= 5 * sd(p, n), (name, share, p, n)
    cl_r, cl_b = np.concatenate(cl_r).astype(np.float64), np.concatenate(cl_b).astype(np.float64)
    assert cl_r.size == rec[6]
    # the float32 rounding is monotone, so a value of the open fp64 interval lands within the float32 images of its ends
    for v, lo, hi in ((cl_r, 0.5, VISION[0]), (cl_b, VISION[1], VISION[2])):
        assert (v >= np.float32(lo)).all() and (v <= np.float32(hi)).all()
        assert abs(v.mean() - 0.5 * (lo + hi)) <= 5 * (hi - lo) / math.sqrt(12 * v.size)
    # the spike amounts are uniform in [spike_lo, spike_hi)
    assert abs(rec[9] / rec[5] - 1.0) <= 5 * 1.0 / math.sqrt(12 * rec[5])


def test_a_frozen_instance_senses_nothing():
    rng = np.random.default_rng(5)
    cfg = default_config()
    c = _crowd(rng, 6)
    got = _hook(c, cfg, default_sensor_config(p_clutter=1.0, n_clutter=8), 4, status=SR.INDEX_OOR | 8)
    assert got["count"] == 0 and got["flags"] == SR.FROZEN and not got["meas"].any() and (got["origin"] == -1).all()
    assert got["truth_next"].tobytes() == c["truth"].tobytes() and got["rec"][1] == 1 and got["rec"].sum() == 1
