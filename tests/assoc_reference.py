"""Helpers of the association tests (slam_associate_*, include/slam_batch.h): the host hook on a case, the INDEPENDENT reference built
from the UNGATED innovation hook alone (cost[l][j] = the nis slam_innovation_instance_host reports in slot 0 for the one-detection
message [(ids[j], r_l, b_l)]; the decisions of the header's steps 1 - 6 in plain Python), and the crafted states and messages the CPU and
the GPU tests share.  A helper: no tests in here.

Geometry.  innovation_reference.synthetic_state places landmarks at random, and two may coincide, so the verdict cases use a grid in
polar coordinates around the pose: slot j at range 1.5 + 1.0 (j // 5) m and bearing -1.0 + 0.5 (j % 5) rad, P = G G^T + 1e-5 I with
G = (0.02 / sqrt n) N(0, 1), the noise row and CMD of gate_reference (V = 1e-4, W = 2.5e-3), clean detections with a noise of standard
deviation 0.02 in range and bearing, "new" detections at the cell centres (+0.5 m, +0.25 rad).  Then a detection's own landmark costs less
than 1.4, every other landmark more than 60 and a new detection's best more than 78; the tests assert own < gate_match / 2, other and
new > 2 gate_new with the reference matrix, so no verdict of the main cases hangs on rounding."""
import math

import numpy as np

import innovation_reference as IR
from gate_reference import CMD, NOISE  # noqa: F401
from live_ekf_slam_amd.config import AssocConfig, Noise, default_assoc_config
from live_ekf_slam_amd.filters import associate_instance_host, innovation_instance_host

NONE, MATCHED, NEW, AMBIGUOUS, CONFLICT, NO_ROOM, INVALID = range(7)
FROZEN, TOO_LONG = IR.FROZEN, IR.TOO_LONG
MAX_DET = IR.MAX_DET
GATE_MATCH, GATE_NEW = default_assoc_config().gate_match, default_assoc_config().gate_new
ID_LIMIT = 1 << 24
SINGULAR_NOISE = Noise(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.01, 0.0, 0.0, 0.0, 0.0)


def assoc_cfg(gate_match=GATE_MATCH, gate_new=GATE_NEW):
    return AssocConfig(gate_match, gate_new)


# ---- crafted states and detections --------------------------------------------------------------------------------------------------------
def grid_state(rng, M, f32=False, ids=None):
    n = 3 + 2 * M
    pose = np.array([0.3, -0.2, 0.4]) + 0.01 * rng.standard_normal(3)
    j = np.arange(M)
    rr, bb = 1.5 + 1.0 * (j // 5), -1.0 + 0.5 * (j % 5)
    lm = np.stack([pose[0] + rr * np.cos(pose[2] + bb), pose[1] + rr * np.sin(pose[2] + bb)], axis=1)
    G = rng.standard_normal((n, n)) * (0.02 / math.sqrt(n))
    P = G @ G.T + 1e-5 * np.eye(n)
    x = np.concatenate([pose, lm.ravel()])
    if f32:
        x, P = x.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)
    ids = (100 + rng.permutation(M)).astype(np.int32) if ids is None else np.asarray(ids, dtype=np.int32)
    return dict(x=x, P=P, ids=ids, M=M)


def clean(rng, st, slot, id_col=0.0, dr=0.0):
    """A detection of landmark `slot` as the pose of the state sees it, with noise; dr: a range offset.  id_col: what the id column holds
    (it is not read)."""
    x = st["x"]
    dx, dy = x[3 + 2 * slot] - x[0], x[4 + 2 * slot] - x[1]
    r = math.hypot(dx, dy) + 0.02 * rng.standard_normal() + dr
    b = math.remainder(math.atan2(dy, dx) - x[2], IR.TWO_PI) + 0.02 * rng.standard_normal()
    return [id_col, r, b]


def fresh(cell, id_col=0.0):
    """A detection of something that is not in the map: the centre of grid cell `cell`."""
    return [id_col, 1.5 + 1.0 * (cell // 5) + 0.5, -1.0 + 0.5 * (cell % 5) + 0.25]


# ---- the hook and the reference ----------------------------------------------------------------------------------------------------------
def ahook(case, cmd=CMD, cfg=None, f32=False, meas=None, count=None, k_stride=None):
    st = case["st"]
    return associate_instance_host(st["x"], st["P"], st["ids"], case["L_max"], case["status"], cmd, case["meas"] if meas is None else meas,
                                   case["noise"], f32_storage=f32, cfg=cfg or case.get("cfg") or assoc_cfg(),
                                   count=case.get("count") if count is None else count, k_stride=case.get("k_stride") if k_stride is None else k_stride)


def reference_costs(case, cmd=CMD, f32=False):
    """cost [k][M] and nu [k][M][2] by the UNGATED innovation hook alone, one call per pair."""
    st = case["st"]
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    count = meas.shape[0] if case.get("count") is None else case["count"]
    ks = max(meas.shape[0], 1) if case.get("k_stride") is None else case["k_stride"]
    k = min(max(count, 0), ks)
    M = st["ids"].shape[0]
    cost = np.full((k, M), np.nan); nu = np.full((k, M, 2), np.nan)
    for l in range(min(k, 4 * MAX_DET)):
        for j in range(M):
            one = np.array([[float(st["ids"][j]), meas[l, 1], meas[l, 2]]], dtype=np.float32)
            r = innovation_instance_host(st["x"], st["P"], st["ids"], case["L_max"], 0, cmd, one, case["noise"], f32_storage=f32)
            assert r["n_upd"] == 1, "the one-detection message is an update of landmark j"
            cost[l, j] = r["det"][0, 0]; nu[l, j] = r["det"][0, 1:3]
    return cost, nu


def reference_associate(case, cost, nu, cfg=None):
    """The decisions of steps 1 - 6 in plain Python from the cost matrix: dict of verdict, slot [64], det [64][4], meas_out (the rows the
    kernel writes, as a list of (index, triplet)), count_out, n_match, n_new, n_drop, flags, rec."""
    cfg = cfg or case.get("cfg") or assoc_cfg()
    st = case["st"]
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    k, M = cost.shape
    L_max = case["L_max"]
    verdict = np.zeros(MAX_DET, np.int32); slot = np.full(MAX_DET, -1, np.int32); det = np.full((MAX_DET, 4), np.nan)
    rec = np.zeros(16)
    zero = np.zeros(3, np.float32)
    if case["status"] & IR.INST_INDEX_OOR or k > MAX_DET:
        flags = FROZEN if case["status"] & IR.INST_INDEX_OOR else TOO_LONG
        rec[1 if flags == FROZEN else 2] = 1.0
        return dict(verdict=verdict, slot=slot, det=det, rows=[(i, zero) for i in range(k)], count_out=0, n_match=0, n_new=0, n_drop=0, flags=flags,
                    rec=rec)
    cand = [NONE] * k
    for l in range(k):
        fin = [(cost[l, j], j) for j in range(M) if np.isfinite(cost[l, j])]
        fin.sort()
        if fin:
            slot[l] = fin[0][1]
            det[l] = (fin[0][0], fin[1][0] if len(fin) > 1 else np.nan, nu[l, fin[0][1], 0], nu[l, fin[0][1], 1])
        if M > 0 and not fin:
            cand[l] = INVALID
        elif M == 0 or fin[0][0] > cfg.gate_new:
            cand[l] = "new"
        elif fin[0][0] <= cfg.gate_match:
            cand[l] = "match"
        else:
            cand[l] = AMBIGUOUS
    base = 0 if M == 0 else 1 + int(max(st["ids"].tolist()))
    rank, ident = 0, {}
    for l in range(k):
        if cand[l] == "match":
            rivals = [(det[i, 0], i) for i in range(k) if cand[i] == "match" and slot[i] == slot[l]]
            verdict[l] = MATCHED if min(rivals) == (det[l, 0], l) else CONFLICT
            ident[l] = int(st["ids"][slot[l]])
        elif cand[l] == "new":
            ok = M + rank < L_max and base + rank < ID_LIMIT
            verdict[l] = NEW if ok else NO_ROOM
            ident[l] = base + rank
            rank += 1
        else:
            verdict[l] = cand[l]
    kept = [l for l in range(k) if verdict[l] in (MATCHED, NEW)]
    rows = [(p, np.array([np.float32(ident[l]), meas[l, 1], meas[l, 2]], dtype=np.float32)) for p, l in enumerate(kept)]
    rows += [(i, zero) for i in range(len(kept), k)]
    cnt = {v: int((verdict[:k] == v).sum()) for v in range(7)}
    s, mx = 0.0, 0.0
    for l in range(k):
        if verdict[l] == MATCHED:
            s = s + det[l, 0]; mx = max(mx, det[l, 0])
    rec[0] = 1.0; rec[3] = k; rec[4] = cnt[MATCHED]; rec[5] = cnt[NEW]; rec[6] = cnt[AMBIGUOUS]; rec[7] = s; rec[8] = mx
    rec[9] = cnt[CONFLICT]; rec[10] = cnt[NO_ROOM]; rec[11] = cnt[INVALID]
    return dict(verdict=verdict, slot=slot, det=det, rows=rows, count_out=len(kept), n_match=cnt[MATCHED], n_new=cnt[NEW],
                n_drop=cnt[AMBIGUOUS] + cnt[CONFLICT] + cnt[NO_ROOM] + cnt[INVALID], flags=0, rec=rec)


def model_work(M, k, flags, esz):
    """slam_last_associate_work's model restated in Python integers (assoc_traffic of csrc/assoc_kernel.h summed over the instances): per
    instance M landmarks, k = n_match + n_new + n_drop detections and its flags.  Returns (bytes, the same with the reads of P in
    128-byte lines).  An instance that emits an empty message (any flag) contributes (0, 8, 0): its counts."""
    p_elems = other = p_lines = 0
    for m, kk, fl in zip(M, k, flags):
        if int(fl):
            other += 8
            continue
        m, n = int(m), 3 + 2 * int(m)
        p_elems += 3 * n + 10 * m                                 # rows 0 - 2 whole; per landmark P[ii .. ii + 1][0 .. 2] and the 2 x 2 diagonal block
        other += n * esz + 4 * m + 24 * int(kk) + 8               # x, ids, the message in and out, the count in and out
        p_lines += 3 * ((n * esz + 127) // 128) + 4 * m
    return p_elems * esz + other, 128 * p_lines + other


def same_bits(a, b):
    a, b = np.ravel(np.asarray(a, dtype=np.float64)), np.ravel(np.asarray(b, dtype=np.float64))
    return a.shape == b.shape and not ((a.view(np.uint64) != b.view(np.uint64)) & ~(np.isnan(a) & np.isnan(b))).any()


def expected_row(ref, row_in):
    """The output row: the input row with the rows the kernel writes replaced."""
    out = np.array(row_in, dtype=np.float32, copy=True)
    for i, t in ref["rows"]:
        out[i] = t
    return out


def check_against_reference(g, ref, what, row_in=None, cost=None):
    """Every output of the hook or of the device for one instance (dict g) against the reference, bit for bit."""
    if cost is not None and not ref["flags"]:          # (an instance that emits an empty message computes no cost)
        assert same_bits(g["cost"], cost), (what, "cost")
    assert g["flags"] == ref["flags"], (what, g["flags"], ref["flags"])
    assert np.array_equal(g["verdict"], ref["verdict"]), (what, g["verdict"][:8], ref["verdict"][:8])
    assert np.array_equal(g["slot"], ref["slot"]), (what, g["slot"][:8], ref["slot"][:8])
    if "det" in g:
        assert same_bits(g["det"], ref["det"]), (what, "det")
    assert (g["count_out"], g["n_match"], g["n_new"], g["n_drop"]) == (ref["count_out"], ref["n_match"], ref["n_new"], ref["n_drop"]), what
    if "rec" in g:
        assert same_bits(g["rec"], ref["rec"]), (what, g["rec"], ref["rec"])
    if row_in is not None:
        assert np.asarray(g["meas_out"], dtype=np.float32).tobytes() == expected_row(ref, row_in).tobytes(), (what, "the labelled message")


def padded_row(case):
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    ks = max(meas.shape[0], 1) if case.get("k_stride") is None else case["k_stride"]
    row = np.zeros((ks, 3), np.float32); row[:meas.shape[0]] = meas
    return row


# ---- the crafted cases -------------------------------------------------------------------------------------------------------------------
def crafted_cases(seed, L_max, f32=False, M=None):
    """Dicts: name, st, status, meas [k][3] float32, noise, L_max, optional cfg / count / k_stride, and what to expect: verdicts (list over
    count_in; None = not stated), flags.  `main` cases state their verdicts through clean and fresh detections and must keep the margins
    of the module docstring.  M: landmarks of the main state (default min(18, L_max - 2))."""
    rng = np.random.default_rng(seed)
    M = min(18, L_max - 2) if M is None else M
    assert 5 <= M <= L_max - 2
    out = []
    garbage = [float("nan"), -7.0, 1e30, 3.5, float("inf")]

    def add(name, st, dets, verdicts=None, flags=0, status=0, noise=NOISE, main=True, **kw):
        out.append(dict(name=name, st=st, status=status, meas=np.asarray(dets, dtype=np.float32).reshape(-1, 3), noise=noise, L_max=L_max,
                        verdicts=verdicts, flags=flags, main=main and verdicts is not None, **kw))
    st = grid_state(rng, M, f32)
    add("empty message", st, [], [])
    none = grid_state(rng, 0, f32)
    add("M = 0, two detections", none, [fresh(1), fresh(7)], [NEW, NEW])
    order = rng.permutation(M)[:MAX_DET]
    add("every mapped landmark, shuffled, garbage ids", st, [clean(rng, st, int(j), garbage[i % 5]) for i, j in enumerate(order)], [MATCHED] * len(order))
    add("updates around two new detections", st, [clean(rng, st, 0), fresh(2), clean(rng, st, 3), fresh(M - 1), clean(rng, st, 1)],
        [MATCHED, NEW, MATCHED, NEW, MATCHED])
    add("two detections of one landmark", st, [clean(rng, st, 2), clean(rng, st, 4), clean(rng, st, 2)], None, main=False, conflict=(0, 2))
    twice = clean(rng, st, 3)
    add("an exact tie: the triplet repeated", st, [clean(rng, st, 1), twice, twice], [MATCHED, MATCHED, CONFLICT])
    add("ambiguous", st, [clean(rng, st, 0), clean(rng, st, 4, dr=0.3)], [MATCHED, AMBIGUOUS], cfg=assoc_cfg(2.0, 200.0), ambiguous=1)
    add("NaN range", st, [clean(rng, st, 0), [0.0, float("nan"), 0.1]], [MATCHED, INVALID])
    add("singular S: zero P, zero W", dict(st, P=np.zeros_like(st["P"])), [clean(rng, st, 2), clean(rng, st, 0)], [INVALID, INVALID],
        noise=SINGULAR_NOISE, main=False)
    full = grid_state(rng, L_max, f32)
    add("a full map", full, [clean(rng, full, 1), fresh(3), clean(rng, full, 0)], [MATCHED, NO_ROOM, MATCHED])
    nearly = grid_state(rng, L_max - 1, f32)
    add("room for one", nearly, [fresh(3), clean(rng, nearly, 2), fresh(6)], [NEW, MATCHED, NO_ROOM])
    top = grid_state(rng, 5, f32, ids=[ID_LIMIT - 4, 5, ID_LIMIT - 2, 9, 11])
    add("ids near 2^24", top, [fresh(0), clean(rng, top, 0), fresh(3), clean(rng, top, 2)], [NEW, MATCHED, NO_ROOM, MATCHED])
    add("65 detections", st, [clean(rng, st, l % M) for l in range(MAX_DET + 1)], None, flags=TOO_LONG)
    add("frozen status", st, [clean(rng, st, 2), fresh(1)], None, flags=FROZEN, status=IR.INST_INDEX_OOR)
    add("count beyond the row", st, [clean(rng, st, 1), fresh(2), clean(rng, st, 0)], [MATCHED, NEW, MATCHED], count=9, k_stride=3)
    add("negative count", st, [clean(rng, st, 1)], [], count=-3, k_stride=2)
    add("sentinels behind the count", st, [clean(rng, st, 1), fresh(2), clean(rng, st, 1), [7.0, 7.0, 7.0], [7.0, 7.0, 7.0]], None, main=False,
        count=3, k_stride=5)
    add("gate_new = +inf: only M = 0 inserts", st, [clean(rng, st, 0), fresh(2)], [MATCHED, AMBIGUOUS], cfg=assoc_cfg(GATE_MATCH, float("inf")),
        main=False)
    add("gate_new = +inf on an empty map", none, [fresh(2)], [NEW], cfg=assoc_cfg(GATE_MATCH, float("inf")), main=False)
    return out


def check_margins(case, cost, what):
    """own < gate_match / 2, every other landmark and every fresh detection > 2 gate_new, as the reference matrix has them."""
    if not case["main"] or cost.size == 0:
        return
    for l, v in enumerate(case["verdicts"]):
        fin = np.sort(cost[l][np.isfinite(cost[l])])
        if v in (MATCHED, CONFLICT):
            assert fin[0] < GATE_MATCH / 2 and (fin.size == 1 or fin[1] > 2 * GATE_NEW), (what, l, fin[:2])
        elif v in (NEW, NO_ROOM):
            assert fin[0] > 2 * GATE_NEW, (what, l, fin[0])
        elif v == AMBIGUOUS:
            assert 4 < fin[0] < 100, (what, l, fin[0])
