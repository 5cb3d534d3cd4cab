"""An independent reference of landmark merging (slam_map_duplicates, slam_merge_landmarks, slam_map_merge; include/slam_batch.h) in
plain numpy and Python floats: the cost of every pair, the mutual nearest neighbours, the sequential fusion and np.delete.  It shares
no code with live_ekf_slam_amd/csrc/merge_kernel.h but keeps its ORDER OF OPERATIONS, with elementwise numpy only (one ufunc per IEEE
operation), so no fused multiply-add can occur and the comparison with the hook is in bits.  A helper: no tests in here."""
import math

import numpy as np

from live_ekf_slam_amd import merge_instance_host
from live_ekf_slam_amd.config import default_merge_config

TWO_PI = 2 * 3.14159265358979323846
SKIP_STATUS = 1 | 4 | 32             # NONFINITE, INDEX_OOR (frozen), WATCHDOG
REC_TOUCHED, REC_FUSED, REC_NOT_MUTUAL, REC_SINGULAR, REC_UPDATED, REC_SUM_D2, REC_MAX_D2 = 0, 1, 2, 3, 4, 7, 8


def as_stored(a, f32):
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if f32 else a


def inv2x2(S):
    """The 2 x 2 inverse by LU with partial pivoting, column by column (what MatrixXd::inverse() does): (Si, ok)."""
    s00, s01, s10, s11 = (float(v) for v in S)
    sw = abs(s10) > abs(s00)
    a00, a01, a10, a11 = (s10, s11, s00, s01) if sw else (s00, s01, s10, s11)
    with np.errstate(all="ignore"):
        l = float(np.float64(a10) / np.float64(a00))
        u11 = a11 - l * a01
        ok = a00 != 0.0 and u11 != 0.0
        cols = []
        for r0, r1 in (((0.0, 1.0) if sw else (1.0, 0.0)), ((1.0, 0.0) if sw else (0.0, 1.0))):
            y1 = r1 - l * r0
            x1 = float(np.float64(y1) / np.float64(u11))
            cols.append((float(np.float64(r0 - a01 * x1) / np.float64(a00)), x1))
    return (cols[0][0], cols[1][0], cols[0][1], cols[1][1]), ok


def d2_of(d0, d1, S):
    """(d2 or NaN, Si, usable)"""
    Si, ok = inv2x2(S)
    ok = ok and all(math.isfinite(v) for v in S)
    with np.errstate(all="ignore"):
        d2 = float(np.float64(d0) * (np.float64(Si[0]) * d0 + np.float64(Si[1]) * d1) + np.float64(d1) * (np.float64(Si[2]) * d0 + np.float64(Si[3]) * d1))
    if not (ok and math.isfinite(d0) and math.isfinite(d1)):
        d2 = math.nan
    return d2, Si, ok


def pair_S(P, ii, jj, sigma2):
    A = (P[ii:ii + 2, ii:ii + 2] - P[ii:ii + 2, jj:jj + 2]) - (P[jj:jj + 2, ii:ii + 2] - P[jj:jj + 2, jj:jj + 2])
    return (float(A[0, 0] + sigma2), float(A[0, 1]), float(A[1, 0]), float(A[1, 1] + sigma2))


def cost_matrix(x, P, M, sigma=0.0):
    """d2 of every unordered pair, (M, M) symmetric with NaN on the diagonal."""
    D = np.full((M, M), np.nan)
    with np.errstate(all="ignore"):
        for i in range(M):
            for j in range(i + 1, M):
                ii, jj = 3 + 2 * i, 3 + 2 * j
                D[i, j] = D[j, i] = d2_of(float(x[ii] - x[jj]), float(x[ii + 1] - x[jj + 1]), pair_S(P, ii, jj, sigma * sigma))[0]
    return D


def reference_find(x, P, M, L_max, cfg, status=0, f32=False):
    """dict(partner, d2 (L_max,), nn (M,), D): the decision on the stored state."""
    partner = np.full(L_max, -1, dtype=np.int32); d2 = np.full(L_max, np.nan)
    nn = np.full(M, -1, dtype=np.int64)
    if (status & SKIP_STATUS) or M < 2:
        return dict(partner=partner, d2=d2, nn=nn, D=None)
    D = cost_matrix(as_stored(x, f32), as_stored(P, f32), M, cfg.sigma)
    for s in range(M):
        ok = np.isfinite(D[s]) & (D[s] <= cfg.gate_merge)
        if ok.any():
            best = np.where(ok, D[s], np.inf)
            nn[s] = int(np.argmin(best))          # (the first minimum: ties to the lowest slot)
            d2[s] = D[s, nn[s]]
    for s in range(M):
        if nn[s] >= 0 and nn[nn[s]] == s:
            partner[s] = nn[s]
    return dict(partner=partner, d2=d2, nn=nn, D=D)


def honoured_pairs(partner, M, L_max, status=0):
    """(pairs ascending i, entries that are neither -1 nor honoured)"""
    pairs, ignored = [], 0
    for s in range(L_max):
        e = int(partner[s])
        hon = not (status & SKIP_STATUS) and s < M and 0 <= e < M and e != s and int(partner[e]) == s
        if hon and e > s:
            pairs.append((s, e))
        if not hon and e != -1:
            ignored += 1
    return pairs, ignored


def fuse_pair(x, P, i, j, sigma2, f32):
    """One fusion on (x, P), new arrays as stored: (x, P, d2, fused)."""
    ii, jj = 3 + 2 * i, 3 + 2 * j
    with np.errstate(all="ignore"):
        c = P[:, ii:ii + 2] - P[:, jj:jj + 2]
        g = P[ii:ii + 2, :] - P[jj:jj + 2, :]
        d0, d1 = float(x[ii] - x[jj]), float(x[ii + 1] - x[jj + 1])
        S = (float((c[ii, 0] - c[jj, 0]) + sigma2), float(c[ii, 1] - c[jj, 1]), float(c[ii + 1, 0] - c[jj + 1, 0]),
             float((c[ii + 1, 1] - c[jj + 1, 1]) + sigma2))
        d2, Si, ok = d2_of(d0, d1, S)
        if not ok:
            return x, P, d2, False
        K0 = c[:, 0] * Si[0] + c[:, 1] * Si[2]
        K1 = c[:, 0] * Si[1] + c[:, 1] * Si[3]
        x2 = x + (K0 * (-d0) + K1 * (-d1))
        x2[2] = math.remainder(x2[2], TWO_PI) if math.isfinite(x2[2]) else x2[2]
        P2 = P - (K0[:, None] * g[0][None, :] + K1[:, None] * g[1][None, :])
    return as_stored(x2, f32), as_stored(P2, f32), d2, True


def reference_merge(x, P, ids, L_max, cfg, status=0, f32=False, seen=None, expected=None, partner=None):
    """Find (partner None) or the caller's pairs, the sequential fusion, np.delete: dict(x, P, ids, M, rec, seen, expected, ids_row,
    partner) with the rows zeroed from M' up; an instance without a fused pair keeps everything it held."""
    M = len(ids)
    xs, Ps = as_stored(x, f32), as_stored(P, f32)
    found = reference_find(x, P, M, L_max, cfg, status, f32)
    lonely = 0 if partner is not None else int(sum(1 for s in range(M) if found["nn"][s] >= 0 and found["partner"][s] < 0))
    pairs, ignored = honoured_pairs(found["partner"] if partner is None else partner, M, L_max, status)
    rec = np.zeros(16)
    rec[REC_NOT_MUTUAL] = ignored + lonely
    se = None if seen is None else np.array(seen, dtype=np.int32)
    ex = None if expected is None else np.array(expected, dtype=np.int32)
    drop = []
    n = 3 + 2 * M
    for i, j in pairs:
        xs, Ps, d2, fused = fuse_pair(xs, Ps, i, j, cfg.sigma * cfg.sigma, f32)
        if not fused:
            rec[REC_SINGULAR] += 1
            continue
        drop.append(j)
        rec[REC_FUSED] += 1; rec[REC_UPDATED] += n * n
        if math.isfinite(d2):
            rec[REC_SUM_D2] += d2; rec[REC_MAX_D2] = max(rec[REC_MAX_D2], d2)
        if se is not None:
            e2 = max(int(ex[i]), int(ex[j]))
            se[i] = min(int(se[i]) + int(se[j]), e2); ex[i] = e2
    out = dict(partner=found["partner"], d2=found["d2"], rec=rec, D=found["D"])
    if not drop:
        return dict(out, x=np.asarray(x, dtype=np.float64), P=np.asarray(P, dtype=np.float64), ids=np.asarray(ids, dtype=np.int32), M=M, ids_row=None,
                    seen=None if seen is None else np.array(seen), expected=None if expected is None else np.array(expected))
    rec[REC_TOUCHED] = 1
    idx = [k for j in drop for k in (3 + 2 * j, 4 + 2 * j)]

    def row(a):
        r = np.zeros(L_max, dtype=np.int32)
        kept = np.delete(np.asarray(a, dtype=np.int32)[:M], drop)
        r[:len(kept)] = kept
        return r
    return dict(out, x=np.delete(xs, idx), P=np.delete(np.delete(Ps, idx, axis=0), idx, axis=1), ids=np.delete(np.asarray(ids, dtype=np.int32), drop),
                M=M - len(drop), ids_row=row(ids), seen=None if se is None else row(se), expected=None if ex is None else row(ex))


# ---- crafted states ----------------------------------------------------------------------------------------------------------------------
def crafted_state(rng, layout, f32=False, noise=0.004, nan_slot=None):
    """layout: one entry per slot, ("new",) a physical landmark of its own or ("copy", s, (ex, ey), noisy) a duplicate of the earlier slot
    s displaced by (ex, ey) * noise, with independent noise of variance noise^2 on its own block and on its source's when `noisy`
    (so S of the pair is 2 noise^2 I and its d2 = (ex^2 + ey^2) / 2).  The physical landmarks sit
    on a jittered 0.5 m grid and P0 = A A^T is small against that spacing, so every pair of DIFFERENT landmarks costs far more than any
    gate (the tests assert the margins); the state is P = T P0 T^T + N for the copy transform T."""
    phys = [k for k, e in enumerate(layout) if e[0] == "new"]
    n0 = 3 + 2 * len(phys)
    side = int(math.ceil(math.sqrt(max(len(phys), 1))))
    pose = np.array([0.3, -0.2, 0.4]) + 0.01 * rng.standard_normal(3)
    order = rng.permutation(side * side)[:len(phys)]
    lm0 = np.stack([0.5 * (order % side) - 1.0, 0.5 * (order // side) - 1.0], axis=1) + rng.uniform(-0.05, 0.05, (len(phys), 2))
    x0 = np.concatenate([pose, lm0.ravel()])
    A = rng.standard_normal((n0, n0)) * (0.02 / math.sqrt(n0))
    P0 = A @ A.T + 1e-5 * np.eye(n0)
    M = len(layout)
    n = 3 + 2 * M
    T = np.zeros((n, n0)); T[:3, :3] = np.eye(3)
    off = np.zeros(n); N = np.zeros((n, n))
    base = {}
    for s, e in enumerate(layout):
        b = phys.index(s) if e[0] == "new" else base[e[1]]
        base[s] = b
        T[3 + 2 * s, 3 + 2 * b] = T[4 + 2 * s, 4 + 2 * b] = 1.0
        if e[0] == "copy":
            off[3 + 2 * s:5 + 2 * s] = np.asarray(e[2], dtype=np.float64) * noise
            if e[3]:                       # independent noise on the copy AND on its source: the fusion has something to average
                for q in (s, e[1]):
                    N[3 + 2 * q, 3 + 2 * q] = N[4 + 2 * q, 4 + 2 * q] = noise * noise
    x = T @ x0 + off
    P = T @ P0 @ T.T + N
    if nan_slot is not None:
        k = 3 + 2 * nan_slot
        P[k, :] = np.nan; P[:, k] = np.nan; x[k] = np.nan
    return dict(x=as_stored(x, f32), P=as_stored(P, f32), ids=(100 + rng.permutation(M)).astype(np.int32), M=M, base=base)


def layout_with(M, copies):
    """M slots, all physical but the listed copies {slot: (source slot, offset, noisy)}."""
    return [("copy",) + tuple(copies[s]) if s in copies else ("new",) for s in range(M)]


def check_margins(D, pairs, gate, name, factor=2.0):
    """Every listed pair costs less than gate / factor, every other pair more than factor * gate (or is not finite)."""
    M = D.shape[0]
    want = {(min(a, b), max(a, b)) for a, b in pairs}
    for i in range(M):
        for j in range(i + 1, M):
            if (i, j) in want:
                assert np.isfinite(D[i, j]) and D[i, j] < gate / factor, (name, i, j, D[i, j])
            else:
                assert not np.isfinite(D[i, j]) or D[i, j] > gate * factor, (name, i, j, D[i, j])


def hook(st, L_max, f32=False, cfg=None, **kw):
    return merge_instance_host(st["x"], st["P"], st["ids"], L_max, f32_storage=f32, cfg=cfg or default_merge_config(), **kw)


def same_bits(a, b):
    return np.ascontiguousarray(a, dtype=np.float64).tobytes() == np.ascontiguousarray(b, dtype=np.float64).tobytes()


def same_values(a, b):
    """The same bits wherever either is a number; a NaN matches any NaN (the sign and payload a NaN operand leaves behind depend on the
    order in which a compiler feeds it to a commutative instruction, which no language fixes)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    if a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return bool(((a.view(np.uint64) == b.view(np.uint64)) | both).all())
