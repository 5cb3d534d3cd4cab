"""slam_map_score (include/slam_batch.h, "map score") restated in numpy, independently of live_ekf_slam_amd/csrc/score_kernel.h: the distance
table of all slots against all true rows at once, the claims resolved PER TRUE ROW (the kernel resolves them per slot), and the summary in
the order the header states.  Every operation is an IEEE fp64 operation in the order of the definition, so the integers, lm_err, lm_nees and
map_rms are compared in bits.  Also here: the ctypes plumbing of the host hook and of the device call (the package has no mirror method for
them yet: tests and tools go through _lib.lib()), the crafted states the CPU and the GPU tests share, and the per-instance record."""
import ctypes as C
import math

import numpy as np

TWO_PI = 2 * 3.14159265358979323846
NONE, MATCHED, DUPLICATE, SPURIOUS = 0, 1, 2, 3
MATCHED_NOT_PD, LM_NOT_PD, INSTANCE_FAILED = 1, 4, 8
NONFINITE, WATCHDOG = 1, 32
LM_LO, LM_HI = -2.0 * math.log(0.975), -2.0 * math.log(0.025)
MAX_ENTRY_7 = (7,)   # the join mask of the score record (record_tree.fixed_order_record)

PER_INSTANCE = ("n_matched", "n_duplicate", "n_spurious", "map_rms", "max_err", "flags")
PER_SLOT = ("row", "role", "lm_err", "lm_nees")
BITWISE = PER_INSTANCE + PER_SLOT


def stored(a, f32):
    """The values as the handle stores them, widened."""
    a = np.asarray(a, dtype=np.float64)
    return a.astype(np.float32).astype(np.float64) if f32 else a


def reference(x, P, M, L_max, status, truth, map_xy, radius=math.inf, lo=LM_LO, hi=LM_HI, f32=False):
    """One instance: dict of the per-instance outputs, the per-slot outputs [L_max], and for the record: sum_d2, lm_n, lm_sum, lm_below,
    lm_above; sel = the MATCHED slots in ascending order."""
    M = min(max(int(M), 0), L_max)
    n = 3 + 2 * M
    x = stored(x, f32)[:n]
    P = stored(P, f32).reshape(-1, n)[:n] if np.ndim(P) == 1 else stored(P, f32)[:n, :n]
    map_xy = np.asarray(map_xy, dtype=np.float64).reshape(-1, 2)
    nan = float("nan")
    out = dict(n_matched=0, n_duplicate=0, n_spurious=0, map_rms=nan, max_err=nan, flags=0, row=np.full(L_max, -1, np.int32),
               role=np.zeros(L_max, np.int32), lm_err=np.full(L_max, nan), lm_nees=np.full(L_max, nan), sum_d2=nan, lm_n=0, lm_sum=0.0,
               lm_below=0, lm_above=0, sel=np.zeros(0, np.int64), M=M)
    with np.errstate(all="ignore"):
        e = (x[0] - truth[0], x[1] - truth[1], x[2] - truth[2])
        e2 = math.remainder(e[2], TWO_PI) if math.isfinite(e[2]) else nan
        if (status & (NONFINITE | WATCHDOG)) or not (math.isfinite(e[0]) and math.isfinite(e[1]) and math.isfinite(e2)):
            out["flags"] = INSTANCE_FAILED
            return out
        out.update(map_rms=0.0, max_err=0.0, sum_d2=0.0)
        if M == 0:
            return out
        lm = x[3:].reshape(M, 2)
        dx = lm[:, None, 0] - map_xy[None, :, 0]
        dy = lm[:, None, 1] - map_xy[None, :, 1]
        d2 = dx * dx + dy * dy                                    # [M][Lb]
        masked = np.where(np.isfinite(d2), d2, np.inf)
        near = np.argmin(masked, axis=1)                          # (the first of equal values: the lowest row)
        best = d2[np.arange(M), near]
        r2 = radius * radius
        has = np.isfinite(best) & (best <= r2)
        row = np.where(has, near, -1)
        role = np.where(has, DUPLICATE, SPURIOUS)
        for r in np.unique(row[has]):                             # per true row: the claimant of least d2, ties to the lowest slot
            claim = np.flatnonzero(row == r)
            role[claim[np.lexsort((claim, best[claim]))[0]]] = MATCHED
        i = 3 + 2 * np.arange(M)
        a, c = P[i, i], P[i + 1, i + 1]
        b = 0.5 * (P[i + 1, i] + P[i, i + 1])
        ex, ey = dx[np.arange(M), near], dy[np.arange(M), near]
        s0 = np.sqrt(a)
        y0 = ex / s0
        l = b / s0
        d = c - l * l
        y1 = (ey - y0 * l) / np.sqrt(d)
        ok = (a > 0) & np.isfinite(a) & (d > 0) & np.isfinite(d)
        nees = np.where(has & ok, y0 * y0 + y1 * y1, nan)
        err = np.where(has, np.sqrt(best), nan)
    out["row"][:M] = row; out["role"][:M] = role; out["lm_err"][:M] = err; out["lm_nees"][:M] = nees
    if np.any(has & ~ok):
        out["flags"] |= LM_NOT_PD
    out["n_matched"], out["n_duplicate"], out["n_spurious"] = (int((role == k).sum()) for k in (MATCHED, DUPLICATE, SPURIOUS))
    sel = np.flatnonzero(role == MATCHED)
    out["sel"] = sel
    total, lm_sum = np.float64(0.0), np.float64(0.0)
    for j in sel:                                                 # ascending j, one addition per slot
        total = total + best[j]
        if np.isfinite(nees[j]):
            out["lm_n"] += 1
            lm_sum = lm_sum + nees[j]
            out["lm_below"] += int(nees[j] < lo); out["lm_above"] += int(nees[j] > hi)
    out["sum_d2"], out["lm_sum"] = float(total), float(lm_sum)
    if sel.size:
        out["map_rms"] = float(np.sqrt(total / np.float64(sel.size)))
        out["max_err"] = float(err[sel].max())
    return out


def instance_record(r, nees_matched=float("nan"), dof_matched=0):
    """What one instance adds to the record [16], from reference() and the instance's nees_matched / dof_matched."""
    rec = np.zeros(16)
    if r["flags"] & INSTANCE_FAILED:
        rec[1] = 1.0
        return rec
    rec[0] = 1.0; rec[2] = r["M"]; rec[3] = r["n_matched"]; rec[4] = r["n_duplicate"]; rec[5] = r["n_spurious"]
    rec[6] = r["sum_d2"]; rec[7] = r["max_err"]; rec[8] = r["lm_n"]; rec[9] = r["lm_sum"]; rec[10] = r["lm_below"]; rec[11] = r["lm_above"]
    if np.isfinite(nees_matched):
        rec[12] = 1.0; rec[13] = nees_matched; rec[14] = dof_matched
    rec[15] = 1.0 if r["n_duplicate"] + r["n_spurious"] > 0 else 0.0
    return rec


def selected_state(x, P, M, sel, rows):
    """(x, P, ids) of the state that holds the pose and the slots `sel` only, for consistency_reference.reference: the principal submatrix
    nees_matched factors, with the true rows as ids."""
    n = 3 + 2 * M
    src = np.concatenate([[0, 1, 2], np.stack([3 + 2 * sel, 4 + 2 * sel], axis=1).ravel()]).astype(np.int64)
    P = np.asarray(P, dtype=np.float64).reshape(-1, n)[:n]
    return np.asarray(x, dtype=np.float64)[src], P[np.ix_(src, src)], np.asarray(rows, dtype=np.int32)


# ---- ctypes plumbing ---------------------------------------------------------------------------------------------------------------------

def config(radius=math.inf, lo=LM_LO, hi=LM_HI, full=0):
    from live_ekf_slam_amd import _lib
    return _lib.ScoreConfig(radius, lo, hi, full)


def _d(a):
    from live_ekf_slam_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib._dp)


def _i(a):
    from live_ekf_slam_amd import _lib
    return None if a is None else a.ctypes.data_as(_lib._ip)


def host_hook(x, P, M, L_max, status, truth, map_xy, cfg=None, f32=False):
    """slam_map_score_instance_host on arrays of exactly the stated sizes -> (rc, dict as reference())."""
    from live_ekf_slam_amd import _lib
    n = 3 + 2 * M
    x = np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:n]).copy()
    P = np.ascontiguousarray(np.asarray(P, dtype=np.float64).reshape(-1)[:n * n]).copy()
    truth = np.ascontiguousarray(truth, dtype=np.float64).copy()
    map_xy = np.ascontiguousarray(map_xy, dtype=np.float64).reshape(-1, 2).copy()
    ints = {k: np.full(1, -7, np.int32) for k in ("n_matched", "n_duplicate", "n_spurious", "flags")}
    vals = {k: np.full(1, -7.0) for k in ("map_rms", "max_err")}
    row, role = np.full(max(L_max, 1), -7, np.int32), np.full(max(L_max, 1), -7, np.int32)
    err, nees = np.full(max(L_max, 1), -7.0), np.full(max(L_max, 1), -7.0)
    rc = _lib.lib().slam_map_score_instance_host(_d(x), _d(P), M, L_max, status, _d(truth), _d(map_xy), map_xy.shape[0], int(f32),
                                                 None if cfg is None else C.byref(cfg), _i(ints["n_matched"]), _i(ints["n_duplicate"]),
                                                 _i(ints["n_spurious"]), _d(vals["map_rms"]), _d(vals["max_err"]), _i(ints["flags"]), _i(row),
                                                 _i(role), _d(err), _d(nees))
    out = {k: int(v[0]) for k, v in ints.items()}
    out.update({k: float(v[0]) for k, v in vals.items()})
    out.update(row=row[:L_max], role=role[:L_max], lm_err=err[:L_max], lm_nees=nees[:L_max])
    return rc, out


def device_score(f, cfg=None, want=None):
    """slam_map_score on the handle of the mirror object f -> dict of arrays ([B] and [B][L_max]; rec [16]).  want: the outputs asked for
    (the others are passed as NULL)."""
    from live_ekf_slam_amd import _lib
    B, L_max = f.batch, f.L_max
    out = dict(rec=np.zeros(16), n_matched=np.zeros(B, np.int32), n_duplicate=np.zeros(B, np.int32), n_spurious=np.zeros(B, np.int32),
               map_rms=np.zeros(B), max_err=np.zeros(B), nees_matched=np.zeros(B), dof_matched=np.zeros(B, np.int32), flags=np.zeros(B, np.int32),
               row=np.zeros((B, L_max), np.int32), role=np.zeros((B, L_max), np.int32), lm_err=np.zeros((B, L_max)), lm_nees=np.zeros((B, L_max)))
    if want is not None:
        out = {k: v for k, v in out.items() if k in want}
    p = (lambda k: None if k not in out else (_d(out[k]) if out[k].dtype == np.float64 else _i(out[k])))
    _lib.check(_lib.lib().slam_map_score(f.h, None if cfg is None else C.byref(cfg), p("rec"), p("n_matched"), p("n_duplicate"), p("n_spurious"),
                                         p("map_rms"), p("max_err"), p("nees_matched"), p("dof_matched"), p("flags"), p("row"), p("role"),
                                         p("lm_err"), p("lm_nees")))
    return out


def last_score_work(f):
    from live_ekf_slam_amd import _lib
    by, ms = C.c_double(), C.c_double()
    _lib.check(_lib.lib().slam_last_score_work(f.h, C.byref(by), C.byref(ms)))
    return by.value, ms.value


def same_bits(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def differences(got, want, keys=BITWISE):
    """The keys whose bits differ between two results of one instance (NaN payloads aside: both sides produce the default NaN)."""
    bad = []
    for k in keys:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        if g.dtype.kind == "f" or w.dtype.kind == "f":
            g = g.astype(np.float64); w = w.astype(np.float64)
            if not (np.array_equal(np.isnan(g), np.isnan(w)) and same_bits(np.where(np.isnan(g), 0.0, g), np.where(np.isnan(w), 0.0, w))):
                bad.append(k)
        elif not np.array_equal(g, w):
            bad.append(k)
    return bad


# ---- crafted states ----------------------------------------------------------------------------------------------------------------------
# The true map is a grid of spacing 4 with exactly representable coordinates (also in fp32), the radius of the crafted cases 2.5
# (r2 = 6.25 exactly): a slot half way between two rows ties at d2 = 4, a slot at (+2, +2) from a row is sqrt(8) from four rows (SPURIOUS
# under the radius, a four-way tie without it), and left of the grid's first column a slot can sit at exactly 2.5 from one row.
RADIUS = 2.5
TRUTH = np.array([0.5, -0.25, 0.125 + 2 * TWO_PI])   # (the simulator's heading is not wrapped)


def grid_map(L):
    r = np.arange(L)
    return np.stack([4.0 * (r % 8), 4.0 * (r // 8)], axis=1)


def spd(rng, n, asym=True):
    """A well-conditioned covariance of the size of real ones, slightly asymmetric as the filter leaves it."""
    v = rng.standard_normal((n, 3)) * 0.02
    P = np.diag(rng.uniform(0.5e-2, 2e-2, n)) + v @ v.T
    if asym:
        K = np.triu(rng.standard_normal((n, n)), 1) * 1e-12
        P = P + K - K.T
    return P


def make(rng, M, map_xy, slots, status=0, pose_err=(0.01, -0.02, 0.005)):
    """One state with M slots: slots = {j: (x, y)} placed exactly, every other slot at a random true row plus noise below 0.3."""
    n = 3 + 2 * M
    x = np.zeros(n)
    x[:3] = TRUTH + np.asarray(pose_err)
    for j in range(M):
        if j in slots:
            x[3 + 2 * j: 5 + 2 * j] = slots[j]
        else:
            x[3 + 2 * j: 5 + 2 * j] = map_xy[rng.integers(map_xy.shape[0])] + rng.uniform(-0.3, 0.3, 2)
    return dict(x=x, P=spd(rng, n), M=M, status=status, truth=TRUTH.copy(), ids=np.arange(M, dtype=np.int32) % max(map_xy.shape[0], 1))


def edge_cases(rng, L_max, map_xy):
    """name -> state, each with 0 < M <= L_max slots unless the name says otherwise (L_max >= 8, the map at least 9 rows)."""
    m = map_xy
    two = 2.0 ** -25
    cases = {
        "M = 0": make(rng, 0, m, {}),
        "full": make(rng, L_max, m, {}),
        "tie between two true rows": make(rng, 4, m, {1: m[2] + (2.0, 0.0), 3: m[8] + (0.0, -2.0)}),       # rows 2 / 3 and 0 / 8: the lower wins
        "tie between two slots": make(rng, 5, m, {0: m[5] + (0.25, 0.0), 3: m[5] + (-0.25, 0.0)}),
        "two claimants": make(rng, 4, m, {1: m[6] + (0.5, 0.0), 2: m[6] + (0.25, 0.0)}),
        "three claimants": make(rng, 6, m, {0: m[1] + (0.75, 0.0), 2: m[1] + (0.0, 0.25), 5: m[1] + (0.5, 0.0)}),
        "d2 at the bound and one ulp above": make(rng, 4, m, {0: m[8] + (-2.5, 0.0), 2: m[0] + (-2.5, two)}),
        "beyond the radius": make(rng, 5, m, {1: m[0] + (2.0, 2.0), 4: m[7] + (30.0, 0.0)}),
        "NaN and inf coordinates": make(rng, 6, m, {0: (float("nan"), 1.0), 2: (1.0, float("inf")), 5: (float("-inf"), float("nan"))}),
        "status NONFINITE": make(rng, 3, m, {}, status=NONFINITE),
        "status WATCHDOG": make(rng, 3, m, {}, status=WATCHDOG),
        "pose not finite": make(rng, 3, m, {}, pose_err=(float("nan"), 0.0, 0.0)),
        "other status bits": make(rng, 3, m, {}, status=2 | 4 | 8),
    }
    s = make(rng, 5, m, {})
    s["P"][3 + 2 * 1, 3 + 2 * 1] = -1e-3                     # first pivot of slot 1
    s["P"][4 + 2 * 3, 4 + 2 * 3] = 0.0                       # second pivot of slot 3
    s["P"][3 + 2 * 4, 3 + 2 * 4] = float("inf")              # not finite
    cases["2 x 2 blocks that are not PD"] = s
    assert 2.5 * 2.5 == 6.25 and 6.25 + two * two == np.nextafter(6.25, 7.0)
    return cases
