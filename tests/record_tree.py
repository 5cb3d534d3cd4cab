"""The fixed-order reduction of the per-instance records (live_ekf_slam_amd/csrc/record_kernel.h: record_block_tree, record_reduce_kernel
and record_sum_kernel) restated in numpy, for every GPU test that checks a record in bits."""
import numpy as np

MAX_ENTRY_8 = (8,)   # the join mask of the innovation, gate, association, joint association, map and merge records
ALL_SUMS = ()        # ... of the sense and fix records


def _join(a, b, max_entries):
    r = a + b
    for i in max_entries:
        r[..., i] = np.where(b[..., i] > a[..., i], b[..., i], a[..., i])   # (the kernel's b > a ? b : a)
    return r


def fixed_order_record(inst, max_entries):
    """inst [n][16] -> the record [16].  Per 256 instances the shuffle tree of each wavefront of 64 lanes (lane i joins lane i + off for
    off = 32 .. 1; a lane without a partner joins itself, which only lanes that lane 0 never reads do), the four wavefronts in order, then
    the blocks in ascending order.  Instances past the batch contribute zeros.  max_entries: the entries joined by a maximum (the record's
    join mask); every other is a sum."""
    n = inst.shape[0]
    blocks = (n + 255) // 256
    pad = np.zeros((blocks * 256, 16)); pad[:n] = inst
    rec = None
    for blk in range(blocks):
        part = None
        for wv in range(4):
            r = pad[blk * 256 + wv * 64: blk * 256 + (wv + 1) * 64].copy()
            for off in (32, 16, 8, 4, 2, 1):
                partner = np.concatenate([r[off:], r[64 - off:]])
                r = _join(r, partner, max_entries)
            part = r[0] if part is None else _join(part, r[0], max_entries)
        rec = part if rec is None else _join(rec, part, max_entries)
    return rec
