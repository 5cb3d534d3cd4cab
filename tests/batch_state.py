"""Helpers shared by the GPU tests that compare whole batches: a streaming per-instance state comparator and the byte layout of a
checkpoint (slam_save_state)."""
import numpy as np


def _bits_equal(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _maxdiff(a, b):
    if a.shape != b.shape:
        return float("inf")
    d = np.abs(np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64))
    return float(np.nanmax(d)) if d.size and not np.isnan(d).all() else (0.0 if d.size == 0 else float("nan"))


def state_diff(sa, sb):
    """max |delta| over x and P of two get_state() dicts, or None when they agree bit for bit (M, ids, timestep, x, P)."""
    if sa["M"] != sb["M"] or sa["timestep"] != sb["timestep"] or not _bits_equal(sa["ids"], sb["ids"]):
        return float("inf")
    if _bits_equal(sa["x"], sb["x"]) and _bits_equal(sa["P"], sb["P"]):
        return None
    return max(_maxdiff(sa["x"], sb["x"]), _maxdiff(sa["P"], sb["P"]), 5e-324)


def differing_instances(fa, fb, count=None, b_offset=0):
    """Instances i < count whose state in handle fa differs from instance b_offset + i of handle fb: [(i, max |delta|)].
    Streams one instance at a time, so two batch-sized slabs never sit on the host together.  Compared bit for bit: x, P, M, ids
    and timestep of every instance, its truth pose, its error sum and its status word."""
    count = fa.batch if count is None else count
    sl = slice(b_offset, b_offset + count)
    ta, tb = fa.truth()[:count], fb.truth()[sl]
    ea, eb = fa.error_stats()[:count], fb.error_stats()[sl]
    fla, flb = fa.status()[:count], fb.status()[sl]
    out = []
    for i in range(count):
        d = state_diff(fa.get_state(i), fb.get_state(b_offset + i))
        for u, v in ((ta[i], tb[i]), (ea[i:i + 1], eb[i:i + 1]), (fla[i:i + 1], flb[i:i + 1])):
            if not _bits_equal(u, v):   # a difference in bits alone (-0.0 against 0.0) still counts: the smallest nonzero delta
                d = max(d or 0.0, _maxdiff(u, v), 5e-324)
        if d is not None:
            out.append((i, d))
    return out


def describe(diffs, base=0, first=20):
    """The first `first` differing instances (ids shifted by `base`) and their max |delta|, for an assertion message."""
    head = ", ".join(f"{base + i}: {d:.3g}" for i, d in diffs[:first])
    return f"{len(diffs)} instance(s) differ; first {min(first, len(diffs))} (instance: max |delta|): {head}"


def ckpt_layout(path):
    """Byte layout of a checkpoint (slam_save_state: a header, then P, x, M, ids, flags, timestep, truth, err and, for the UKF
    kinds, sqtP, n_sq, x_prev, V^T, age; every item batch-major).  Returns (header bytes, dict of item -> (byte offset, bytes),
    header fields)."""
    with open(path, "rb") as fh:
        raw = fh.read(40)
        fh.seek(0, 2)
        size = fh.tell()
    kind, B, L_max, dtype, n_max, ps, xs, esz = (int(v) for v in np.frombuffer(raw[8:40], dtype=np.int32))
    items = [("P", esz * B * ps), ("x", esz * B * xs), ("M", 4 * B), ("ids", 4 * B * L_max), ("flags", 4 * B), ("timestep", 4 * B),
             ("truth", 24 * B), ("err", 8 * B)]
    if kind != 1:   # the UKF kinds (SLAM_EKF_SLAM = 1)
        items += [("sqtP", 8 * B * ps), ("n_sq", 4 * B), ("x_prev", 8 * B * xs), ("VT", 8 * B * ps), ("age", 4 * B)]
    head = size - sum(nb for _, nb in items)
    assert 0 < head <= 128, head
    off, pos = {}, head
    for name, nb in items:
        off[name] = (pos, nb)
        pos += nb
    return head, off, dict(kind=kind, B=B, L_max=L_max, dtype=dtype, n_max=n_max, pstride=ps, xstride=xs, esz=esz)
