"""An independent reference of map management (slam_remove_landmarks, slam_map_tally, slam_map_prune; include/slam_batch.h) in plain
numpy: np.delete on x, P and ids, np.hypot / np.arctan2 / math.remainder for the view test, integer counters.  It shares no code with
live_ekf_slam_amd/csrc/map_kernel.h.  The view test is compared in bits only where every r and beta stays MARGIN away from each
threshold (check_margins asserts it): libm and the library's own atan2 agree to an ulp, not to the bit."""
import math

import numpy as np

from live_ekf_slam_amd import map_instance_host
from live_ekf_slam_amd.config import default_map_config

TWO_PI = 2 * 3.14159265358979323846
VISION = (3.0, -1.57, 1.57)          # range_max, fov_min, fov_max of the default config
MARGIN = 1e-6
SKIP_STATUS = 1 | 4 | 32             # NONFINITE, INDEX_OOR (frozen), WATCHDOG
REMOVAL_SETS = ("none", "slot 0", "the last slot", "all", "alternating", "a single survivor")


def as_stored(a, f32):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if f32 else a


def limits(cfg, vision=VISION):
    return vision[0] * cfg.range_shrink, vision[1] + cfg.fov_margin, vision[2] - cfg.fov_margin


def view(x, M):
    """r and beta of every estimated landmark from the estimated pose."""
    lm = np.asarray(x[3:3 + 2 * M]).reshape(M, 2)
    dx, dy = lm[:, 0] - x[0], lm[:, 1] - x[1]
    r = np.hypot(dx, dy)
    beta = np.array([math.remainder(v, TWO_PI) for v in (np.arctan2(dy, dx) - x[2])]) if M else np.zeros(0)
    return r, beta


def check_margins(x, M, cfg, name, vision=VISION):
    r, beta = view(x, M)
    r_lim, lo, hi = limits(cfg, vision)
    assert (np.abs(r - r_lim) >= MARGIN).all(), (name, "a range within the margin of range_max * range_shrink")
    assert (np.abs(beta - lo) >= MARGIN).all() and (np.abs(beta - hi) >= MARGIN).all(), (name, "a bearing within the margin of the field of view")
    assert (np.abs(np.abs(beta) - math.pi) >= MARGIN).all(), (name, "a bearing within the margin of the wrap")


def message_ids(meas, count, k_stride):
    """The ids of the first clamp(count, 0, k_stride) triplets that are int32 values (NaN and out-of-range ids match nothing)."""
    k = min(max(int(count), 0), int(k_stride))
    out = set()
    for v in np.asarray(meas, dtype=np.float32).reshape(-1, 3)[:k, 0]:
        if not np.isnan(v) and -2.0 ** 31 <= float(v) < 2.0 ** 31:
            out.add(int(v))              # (truncation towards zero, as a C cast)
    return out


def reference_tally(x, ids, meas, count, k_stride, status, assoc_flag, seen, expected, cfg, f32=False, vision=VISION):
    """The counters after the tally of one message: (seen, expected), new arrays."""
    seen, expected = np.array(seen, dtype=np.int32), np.array(expected, dtype=np.int32)
    if (status & SKIP_STATUS) or assoc_flag != 0:
        return seen, expected
    M = len(ids)
    xs = as_stored(x, f32)
    r, beta = view(xs, M)
    r_lim, lo, hi = limits(cfg, vision)
    got = message_ids(meas, count, k_stride)
    for j in range(M):
        seen_now = int(ids[j]) in got
        in_view = (not r[j] > r_lim) and beta[j] > lo and beta[j] < hi
        seen[j] += int(seen_now)
        expected[j] += int(seen_now or in_view)
    return seen, expected


def reference_decide(seen, expected, M, L_max, cfg):
    mask = np.zeros(L_max, dtype=np.int32)
    for j in range(M):
        mask[j] = int(expected[j] >= cfg.min_expected and float(seen[j]) < cfg.min_ratio * float(expected[j]))
    return mask


def reference_remove(x, P, ids, mask, L_max, seen=None, expected=None, f32=False):
    """np.delete of the dropped slots: dict(x, P, ids, M, ids_row, seen, expected) with the rows zeroed from M' up."""
    M = len(ids)
    drop = [j for j in range(M) if mask[j]]
    idx = [i for j in drop for i in (3 + 2 * j, 4 + 2 * j)]
    x2 = np.delete(as_stored(x, f32), idx)
    P2 = np.delete(np.delete(as_stored(P, f32), idx, axis=0), idx, axis=1)
    ids2 = np.delete(np.asarray(ids, dtype=np.int32), drop)
    out = dict(x=x2, P=P2, ids=ids2, M=M - len(drop))
    if not drop:     # an untouched instance is not written at all: the rows keep what they held
        return dict(out, ids_row=None, seen=None if seen is None else np.array(seen), expected=None if expected is None else np.array(expected))

    def row(a):
        r = np.zeros(L_max, dtype=np.int32)
        kept = np.delete(np.asarray(a, dtype=np.int32)[:M], drop)
        r[:len(kept)] = kept
        return r
    out["ids_row"] = row(ids)
    out["seen"] = None if seen is None else row(seen)
    out["expected"] = None if expected is None else row(expected)
    return out


def removal_mask(kind, M, rng=None):
    m = np.zeros(M, dtype=np.int32)
    if kind == "slot 0":
        m[:1] = 1
    elif kind == "the last slot":
        m[M - 1:] = 1
    elif kind == "all":
        m[:] = 1
    elif kind == "alternating":
        m[::2] = 1
    elif kind == "a single survivor":
        m[:] = 1
        if M:
            m[M // 2] = 0
    elif kind == "random":
        m[:] = rng.integers(0, 2, M)
    else:
        assert kind == "none", kind
    return m


def crafted_state(rng, M, f32=False, nan_at=None):
    """Pose near the origin; landmarks 0.5 - 3.4 m away at bearings of -1.9 .. 1.9 rad, so that some lie beyond the shrunk range, some
    outside the shrunk field of view and most inside; P symmetric positive definite with distinct entries everywhere; ids a permutation of
    100 .. 100 + M - 1."""
    n = 3 + 2 * M
    pose = np.array([0.3, -0.2, 0.4]) + 0.01 * rng.standard_normal(3)
    rr = rng.uniform(0.5, 3.4, M); bb = rng.uniform(-1.9, 1.9, M)
    lm = np.stack([pose[0] + rr * np.cos(pose[2] + bb), pose[1] + rr * np.sin(pose[2] + bb)], axis=1)
    G = rng.standard_normal((n, n)) * 0.01
    P = G @ G.T + 1e-4 * np.eye(n)
    x = np.concatenate([pose, lm.ravel()])
    if nan_at is not None:
        P[nan_at, :] = np.nan; P[:, nan_at] = np.nan; x[nan_at] = np.nan
    x, P = as_stored(x, f32), as_stored(P, f32)
    return dict(x=x, P=P, ids=(100 + rng.permutation(M)).astype(np.int32), M=M)


def crafted_message(rng, st, k, hits=0.6):
    """k triplets: ids of mapped slots with probability `hits` (repeats allowed), else ids that are not in the map, NaN, +-inf or far
    outside int32; r and b arbitrary (the tally does not read them)."""
    M = st["M"]
    m = np.zeros((k, 3), dtype=np.float32)
    odd = [np.nan, np.inf, -np.inf, 3e9, -3e9, 7.0, 1e6, 99.5, -0.5]
    for l in range(k):
        if M and rng.uniform() < hits:
            m[l, 0] = float(st["ids"][rng.integers(0, M)])
        else:
            m[l, 0] = odd[rng.integers(0, len(odd))]
        m[l, 1:] = rng.uniform(0.5, 3.0), rng.uniform(-1.5, 1.5)
    return m


def hook(st, L_max, f32=False, cfg=None, **kw):
    return map_instance_host(st["x"], st["P"], st["ids"], L_max, f32_storage=f32, cfg=cfg or default_map_config(), **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()
