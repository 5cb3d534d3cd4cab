"""Helpers of the joint-association tests (slam_associate_joint_*, include/slam_batch.h): the host hook on a case and the INDEPENDENT
reference.  nu and the individual costs come from the UNGATED innovation hook, one call per pair (assoc_reference.reference_costs); H and
P_pred are restated in numpy (with the float truncations of the range, ekf.cpp:115); the joint distance of a hypothesis is a dense solve
nu^T S^-1 nu; the search is a plain Python depth-first walk with the node rule of the header, and - for small cases - an exhaustive
enumeration of every hypothesis.  A helper: no tests in here.

Crafted states ("wide yaw, tight landmarks").  Pose (0, 0, 0) with yaw variance 0.01 and position variance 1e-6, landmarks at range 5 m
with variance 1e-6, uncorrelated, W = 1e-4 (sigma 0.01), command (0, 0).  A yaw error shifts the bearing innovation of EVERY landmark
alike: individually a shift of 0.05 rad costs 0.05^2 / 0.0101 = 0.25, far inside the gate, so a detection sits inside the gate of every
landmark within some 0.3 rad; jointly two innovations that differ by 0.08 rad cost 0.08^2 / 2e-4 = 32, far outside gate_joint[1] = 13.3."""
import itertools
import math

import numpy as np

import assoc_reference as AR
import innovation_reference as IR
from live_ekf_slam_amd.config import Noise, default_joint_config
from live_ekf_slam_amd.filters import associate_joint_instance_host

NONE, MATCHED, NEW, AMBIGUOUS, CONFLICT, NO_ROOM, INVALID, UNPAIRED = range(8)
BUDGET, S_SINGULAR, LM_TABLE = 16, 32, 64
MAX_CAND, MAX_PAIR, MAX_DET = 4, 16, IR.MAX_DET
TIGHT = Noise(0.0, 0.0, 0.0, 0.0, 1e-6, 1e-6, 1e-4, 1e-4, 0.0, 0.0, 0.0, 0.0)
ZERO_CMD = (0.0, 0.0)


def joint_cfg(**kw):
    c = default_joint_config()
    for k, v in kw.items():
        if k == "gate_joint":
            for i, g in enumerate(v):
                c.gate_joint[i] = g
        else:
            setattr(c, k, v)
    return c


def jhook(case, cfg=None, f32=False, meas=None):
    st = case["st"]
    return associate_joint_instance_host(st["x"], st["P"], st["ids"], case["L_max"], case["status"], case.get("cmd", AR.CMD),
                                         case["meas"] if meas is None else meas, case["noise"], f32_storage=f32, cfg=cfg or case.get("cfg"),
                                         count=case.get("count"), k_stride=case.get("k_stride"))


# ---- crafted states -------------------------------------------------------------------------------------------------------------------------
def yaw_state(bearings, yaw_var=0.01, lm_var=1e-6, pos_var=1e-6, r=5.0, f32=False):
    M = len(bearings)
    n = 3 + 2 * M
    x = np.zeros(n)
    for j, b in enumerate(bearings):
        x[3 + 2 * j], x[4 + 2 * j] = r * math.cos(b), r * math.sin(b)
    P = np.diag([pos_var, pos_var, yaw_var] + [lm_var] * (2 * M))
    if f32:
        x, P = x.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)
    return dict(x=x, P=P, ids=(200 + np.arange(M)).astype(np.int32), M=M)


def seen(st, slot, shift=0.0, dr=0.0):
    """The detection of landmark `slot` from the state's pose with the bearing innovation `shift` and the range innovation dr."""
    x = st["x"]
    dx, dy = x[3 + 2 * slot] - x[0], x[4 + 2 * slot] - x[1]
    return [0.0, math.hypot(dx, dy) + dr, math.remainder(math.atan2(dy, dx) - x[2], IR.TWO_PI) + shift]


# ---- the reference ----------------------------------------------------------------------------------------------------------------------------
def predicted(case, f32=False):
    """x_pred (pose), P_pred and the stacked-row builder H_j in numpy."""
    st, nz = case["st"], case["noise"]
    x, P = np.array(st["x"], dtype=np.float64), np.array(st["P"], dtype=np.float64)
    if f32:
        x, P = x.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)
    fwd, ang = (np.float32(v) for v in case.get("cmd", AR.CMD))
    n = x.shape[0]
    th = x[2]
    dd = float(np.float32(fwd + np.float32(nz.v_d)))
    xp = x.copy()
    xp[0] += dd * math.cos(th); xp[1] += dd * math.sin(th)
    xp[2] = math.remainder(th + float(ang) + float(np.float32(nz.v_th)), IR.TWO_PI)
    F = np.eye(n); F[0, 2] = -float(fwd) * math.sin(th); F[1, 2] = float(fwd) * math.cos(th)
    Q = np.zeros((n, n)); u = np.array([math.cos(th), math.sin(th)])
    Q[:2, :2] = nz.V_00 * np.outer(u, u); Q[2, 2] = nz.V_11
    Pp = F @ P @ F.T + Q

    def H(j):
        ii = 3 + 2 * j
        dx, dy = xp[ii] - xp[0], xp[ii + 1] - xp[1]
        dist = np.float32(math.sqrt(dx * dx + dy * dy))
        d1, d2 = float(dist), float(np.float32(dist * dist))
        h = np.zeros((2, n))
        h[0, 0], h[0, 1], h[0, ii], h[0, ii + 1] = -dx / d1, -dy / d1, dx / d1, dy / d1
        h[1, 0], h[1, 1], h[1, 2], h[1, ii], h[1, ii + 1] = dy / d2, -dx / d2, -1.0, -dy / d2, dx / d2
        return h
    return Pp, H


def stacked(case, nu, pairs, Pp, H):
    """nu (2 m,) and S (2 m, 2 m) of the hypothesis [(l, j), ...]."""
    nz = case["noise"]
    Hs = np.vstack([H(j) for _, j in pairs])
    S = Hs @ Pp @ Hs.T + np.kron(np.eye(len(pairs)), np.diag([nz.W_00, nz.W_11]))
    v = np.concatenate([nu[l, j] for l, j in pairs])
    return v, S


def dense_d2(v, S):
    return float(v @ np.linalg.solve(S, v))


def mp_d2(case, nu, pairs, f32=False):
    """nu^T S^-1 nu with S = H P_pred H^T + W formed in mpmath (50 digits) from the hook's own double inputs: x, P (as the storage rounds
    them), the command, the noise row and the innovations nu.  H takes the float-truncated range of ekf.cpp:115, as the filter defines it."""
    import mpmath as mp
    mp.mp.dps = 50
    st, nz = case["st"], case["noise"]
    x, P = np.array(st["x"], dtype=np.float64), np.array(st["P"], dtype=np.float64)
    if f32:
        x, P = x.astype(np.float32).astype(np.float64), P.astype(np.float32).astype(np.float64)
    fwd, ang = (np.float32(v) for v in case.get("cmd", AR.CMD))
    n = x.shape[0]
    th = mp.mpf(float(x[2]))
    dd = mp.mpf(float(np.float32(fwd + np.float32(nz.v_d))))
    xp = [mp.mpf(float(t)) for t in x]
    xp[0] += dd * mp.cos(th); xp[1] += dd * mp.sin(th)
    F = mp.eye(n); F[0, 2] = -mp.mpf(float(fwd)) * mp.sin(th); F[1, 2] = mp.mpf(float(fwd)) * mp.cos(th)
    Pm = mp.matrix([[mp.mpf(float(t)) for t in row] for row in P])
    Pp = F * Pm * F.T
    u = [mp.cos(th), mp.sin(th)]
    for a in range(2):
        for b in range(2):
            Pp[a, b] += mp.mpf(nz.V_00) * u[a] * u[b]
    Pp[2, 2] += mp.mpf(nz.V_11)
    Hs = mp.zeros(2 * len(pairs), n)
    for p, (_, j) in enumerate(pairs):
        ii = 3 + 2 * j
        dx, dy = xp[ii] - xp[0], xp[ii + 1] - xp[1]
        dist = np.float32(float(mp.sqrt(dx * dx + dy * dy)))
        d1, d2 = mp.mpf(float(dist)), mp.mpf(float(np.float32(dist * dist)))
        Hs[2 * p, 0], Hs[2 * p, 1], Hs[2 * p, ii], Hs[2 * p, ii + 1] = -dx / d1, -dy / d1, dx / d1, dy / d1
        Hs[2 * p + 1, 0], Hs[2 * p + 1, 1], Hs[2 * p + 1, 2], Hs[2 * p + 1, ii], Hs[2 * p + 1, ii + 1] = dy / d2, -dx / d2, -1, -dy / d2, dx / d2
    S = Hs * Pp * Hs.T
    for p in range(len(pairs)):
        S[2 * p, 2 * p] += mp.mpf(nz.W_00); S[2 * p + 1, 2 * p + 1] += mp.mpf(nz.W_11)
    vm = mp.matrix([mp.mpf(float(t)) for l, j in pairs for t in nu[l, j]])
    return (vm.T * mp.lu_solve(S, vm))[0]


def candidates(case, cost, cfg):
    """Per detection the (d2, j) of its candidates, ascending, at most MAX_CAND."""
    out = []
    for l in range(cost.shape[0]):
        c = sorted((cost[l, j], j) for j in range(cost.shape[1]) if np.isfinite(cost[l, j]) and cost[l, j] <= cfg.gate_match)
        out.append(c[:MAX_CAND])
    return out


class Margin(Exception):
    pass


def reference_search(case, cost, nu, cfg, f32=False, rel=1e-6):
    """The depth-first walk of the header in plain Python with dense solves.  Returns dict(assign {l: j}, d2, nodes, flags, ncand, leaves
    [(pairs, d2, assign)]); raises Margin when a joint gate decision is closer than rel to its gate or a pivot decision is unclear."""
    Pp, H = predicted(case, f32)
    cand = candidates(case, cost, cfg)
    levels = [l for l in range(len(cand)) if cand[l]]
    nd = len(levels)
    gates = [cfg.gate_joint[i] for i in range(MAX_PAIR)]
    st = dict(nodes=0, flags=0, best=None, stop=False, leaves=[])

    def better(pairs, d2):
        b = st["best"]
        return b is None or len(pairs) > len(b[0]) or (len(pairs) == len(b[0]) and d2 < b[1])

    def walk(level, pairs, d2):
        if st["stop"]:
            return
        remaining = nd - level
        bound = len(pairs) + min(remaining, MAX_PAIR - len(pairs))
        if st["best"] is not None and (bound < len(st["best"][0]) or (bound == len(st["best"][0]) and d2 >= st["best"][1])):
            return
        if level == nd:
            st["leaves"].append((len(pairs), d2, dict(pairs)))
            st["best"] = (list(pairs), d2)
            return
        l = levels[level]
        for _, j in cand[l]:
            if len(pairs) == MAX_PAIR or any(j == q for _, q in pairs):
                continue
            if st["nodes"] == cfg.max_nodes:
                st["flags"] |= BUDGET; st["stop"] = True
                if better(pairs, d2):
                    st["best"] = (list(pairs), d2)
                return
            st["nodes"] += 1
            v, S = stacked(case, nu, pairs + [(l, j)], Pp, H)
            ev = np.linalg.eigvalsh(S)
            if ev[0] <= 1e-9 * ev[-1]:
                if ev[0] > 1e-13 * ev[-1]:
                    raise Margin(f"pivot decision unclear: eigenvalues {ev[0]} .. {ev[-1]}")
                st["flags"] |= S_SINGULAR
                continue
            dn = dense_d2(v, S)
            g = gates[len(pairs)]
            if np.isfinite(g) and abs(dn - g) <= rel * g:
                raise Margin(f"joint distance {dn} against gate {g}")
            if dn <= g:
                walk(level + 1, pairs + [(l, j)], dn)
                if st["stop"]:
                    return
        walk(level + 1, pairs, d2)
    walk(0, [], 0.0)
    pairs, d2 = st["best"]
    return dict(assign=dict(pairs), d2=d2, nodes=st["nodes"], flags=st["flags"], ncand=[len(c) for c in cand], leaves=st["leaves"], levels=levels,
                cand=cand, pairs=pairs)


def exhaustive(case, cost, nu, cfg, f32=False):
    """Every hypothesis (at most 6 detections with candidates, 3 candidates each): (pairs, d2, assign) of the compatible ones, every
    prefix compatible as the search requires."""
    Pp, H = predicted(case, f32)
    cand = candidates(case, cost, cfg)
    levels = [l for l in range(len(cand)) if cand[l]]
    assert len(levels) <= 6 and all(len(cand[l]) <= 3 for l in levels)
    out = []
    for choice in itertools.product(*[[j for _, j in cand[l]] + [None] for l in levels]):
        pairs = [(l, j) for l, j in zip(levels, choice) if j is not None]
        if len({j for _, j in pairs}) != len(pairs):
            continue
        ok, d2 = True, 0.0
        for m in range(1, len(pairs) + 1):
            v, S = stacked(case, nu, pairs[:m], Pp, H)
            if np.linalg.eigvalsh(S)[0] <= 0:
                ok = False
                break
            d2 = dense_d2(v, S)
            if not d2 <= cfg.gate_joint[m - 1]:
                ok = False
                break
        if ok:
            out.append((len(pairs), d2, dict(pairs)))
    return out


def reference_joint(case, cost, nu, cfg=None, f32=False):
    """Everything the hook reports, from the reference search: dict as assoc_reference.reference_associate plus d2_joint, nodes, ncand."""
    cfg = cfg or case.get("cfg") or joint_cfg()
    st = case["st"]
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    k, M = cost.shape
    L_max = case["L_max"]
    verdict = np.zeros(MAX_DET, np.int32); slot = np.full(MAX_DET, -1, np.int32); det = np.full((MAX_DET, 4), np.nan)
    ncand = np.zeros(MAX_DET, np.int32)
    rec = np.zeros(16)
    zero = np.zeros(3, np.float32)
    if case["status"] & IR.INST_INDEX_OOR or k > MAX_DET:
        flags = IR.FROZEN if case["status"] & IR.INST_INDEX_OOR else IR.TOO_LONG
        rec[1 if flags == IR.FROZEN else 2] = 1.0
        return dict(verdict=verdict, slot=slot, det=det, rows=[(i, zero) for i in range(k)], count_out=0, n_match=0, n_new=0, n_drop=0, flags=flags,
                    rec=rec, d2_joint=0.0, nodes=0, ncand=ncand, search=None)
    s = reference_search(case, cost, nu, cfg, f32)
    ncand[:k] = s["ncand"]
    base = 0 if M == 0 else 1 + int(max(st["ids"].tolist()))
    rank, ident, differ = 0, {}, 0
    for l in range(k):
        fin = sorted((cost[l, j], j) for j in range(M) if np.isfinite(cost[l, j]))
        if fin:
            slot[l] = fin[0][1]
            det[l] = (fin[0][0], fin[1][0] if len(fin) > 1 else np.nan, nu[l, fin[0][1], 0], nu[l, fin[0][1], 1])
        if s["ncand"][l]:
            if l in s["assign"]:
                j = s["assign"][l]
                verdict[l] = MATCHED; ident[l] = int(st["ids"][j])
                differ += int(j != slot[l])
                slot[l] = j; det[l, 0] = cost[l, j]; det[l, 2:] = nu[l, j]
            else:
                verdict[l] = UNPAIRED
        elif M > 0 and not fin:
            verdict[l] = INVALID
        elif M == 0 or fin[0][0] > cfg.gate_new:
            ok = M + rank < L_max and base + rank < AR.ID_LIMIT
            verdict[l] = NEW if ok else NO_ROOM
            ident[l] = base + rank
            rank += 1
        else:
            verdict[l] = AMBIGUOUS
    kept = [l for l in range(k) if verdict[l] in (MATCHED, NEW)]
    rows = [(p, np.array([np.float32(ident[l]), meas[l, 1], meas[l, 2]], dtype=np.float32)) for p, l in enumerate(kept)]
    rows += [(i, zero) for i in range(len(kept), k)]
    cnt = {v: int((verdict[:k] == v).sum()) for v in range(8)}
    rec[0] = 1.0; rec[3] = k; rec[4] = cnt[MATCHED]; rec[5] = cnt[NEW]; rec[6] = cnt[AMBIGUOUS]
    rec[9] = cnt[UNPAIRED]; rec[10] = cnt[NO_ROOM]; rec[11] = cnt[INVALID]; rec[12] = s["nodes"]
    rec[13] = float(bool(s["flags"] & BUDGET)); rec[14] = float(bool(s["flags"] & S_SINGULAR)); rec[15] = differ
    return dict(verdict=verdict, slot=slot, det=det, rows=rows, count_out=len(kept), n_match=cnt[MATCHED], n_new=cnt[NEW],
                n_drop=cnt[AMBIGUOUS] + cnt[UNPAIRED] + cnt[NO_ROOM] + cnt[INVALID], flags=s["flags"], rec=rec, d2_joint=s["d2"], nodes=s["nodes"],
                ncand=ncand, search=s)


def check_margins(case, cost, ref, cfg, rel_gate=1e-6, rel_best=1e-9):
    """Every individual gate decision at least rel_gate away from its gate (the joint ones are checked inside the search), and the best
    hypothesis at least rel_best away from the runner-up of equal size."""
    fin = cost[np.isfinite(cost)]
    for g in (cfg.gate_match, cfg.gate_new):
        if np.isfinite(g):
            assert (np.abs(fin - g) > rel_gate * g).all(), ("an individual cost at its gate", g)
    s = ref["search"]
    if s is None:
        return
    same = sorted(d for n, d, a in s["leaves"] if n == len(s["pairs"]) and a != s["assign"])
    if same and s["d2"] > 0:
        assert same[0] - s["d2"] > rel_best * s["d2"], ("the runner-up of equal size", s["d2"], same[0])


def check_against_reference(g, ref, what, row_in=None, d2_rel=1e-9):
    """Decisions, slots, verdicts, counts, node count and the output message of the hook (dict g) equal the reference's exactly; det and
    d2_joint come from the same nu and costs, so det in bits and d2_joint to d2_rel (its own test bounds it against mpmath)."""
    assert g["flags"] == ref["flags"], (what, "flags", g["flags"], ref["flags"])
    assert np.array_equal(g["verdict"], ref["verdict"]), (what, g["verdict"][:8], ref["verdict"][:8])
    assert np.array_equal(g["slot"], ref["slot"]), (what, g["slot"][:8], ref["slot"][:8])
    assert np.array_equal(g["ncand"], ref["ncand"]), (what, g["ncand"][:8], ref["ncand"][:8])
    assert AR.same_bits(g["det"], ref["det"]), (what, "det")
    assert (g["count_out"], g["n_match"], g["n_new"], g["n_drop"], g["nodes"]) == \
        (ref["count_out"], ref["n_match"], ref["n_new"], ref["n_drop"], ref["nodes"]), (what, g["nodes"], ref["nodes"])
    skip = (7, 8)
    assert all(g["rec"][i] == ref["rec"][i] for i in range(16) if i not in skip), (what, g["rec"], ref["rec"])
    assert g["rec"][7] == g["rec"][8] == g["d2_joint"] or g["flags"] & (IR.FROZEN | IR.TOO_LONG), what
    assert abs(g["d2_joint"] - ref["d2_joint"]) <= d2_rel * max(ref["d2_joint"], 1e-300), (what, g["d2_joint"], ref["d2_joint"])
    if row_in is not None:
        assert np.asarray(g["meas_out"], dtype=np.float32).tobytes() == AR.expected_row(ref, row_in).tobytes(), (what, "the labelled message")
