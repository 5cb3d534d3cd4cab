"""Helpers of the gate tests (slam_gate_*, include/slam_batch.h): the gated host hook on a case, the INDEPENDENT reference of the rejected
set built from the UNGATED hook alone, and the crafted messages the CPU and the GPU tests share.  A helper: no tests in here.

Noise and spikes.  The crafted states of innovation_reference have a pose covariance of some 1e-3 and detections drawn with a standard
deviation of 0.02 in range and bearing.  With W = diag(0.05^2) and the small command CMD a clean detection has a NIS of a few units at most
and a range spike of SPIKE = 1 m one of more than 100: the tests assert, with the ungated hook, nis < GATE / 2 for every clean and
nis > 2 GATE for every spiked detection they rely on, so no verdict of the main cases hangs on rounding."""
import numpy as np

import innovation_reference as IR
from live_ekf_slam_amd.config import GateConfig, Noise, default_gate_config
from live_ekf_slam_amd.filters import gate_instance_host

GATE = default_gate_config().gate
NOISE = Noise(0.0, 0.0, 0.0, 0.0, 1e-4, 1e-4, 2.5e-3, 2.5e-3, 0.0, 0.0, 0.0, 0.0)
CMD = np.array([0.01, 0.004], dtype=np.float32)
SPIKE = 1.0
NONE, ACCEPTED, REJECTED = 0, 1, 2
PASS = IR.FROZEN | IR.WOULD_FREEZE | IR.TOO_LONG


def gate_cfg(gate=GATE):
    c = default_gate_config()
    c.gate = gate
    return c


def ghook(case, cmd, gate=GATE, f32=False, L_max=None, meas=None, count=None, k_stride=None, lm_from_pred=False):
    """The gated host hook on a case dict (st, status, meas, noise)."""
    st = case["st"]
    return gate_instance_host(st["x"], st["P"], st["ids"], case["L_max"] if L_max is None else L_max, case["status"], cmd,
                              case["meas"] if meas is None else meas, case["noise"], lm_from_pred=lm_from_pred, f32_storage=f32,
                              cfg=gate_cfg(gate), count=count, k_stride=k_stride)


def uhook(case, cmd, meas, f32=False, lm_from_pred=False):
    """The UNGATED hook of the innovation statistics on the same case with another message."""
    cfg = IR.config_for(case["noise"])
    cfg.ekf_landmark_from_x_pred = int(lm_from_pred)
    return IR.hook(case["st"], cmd, meas, cfg, case["L_max"], f32, status=case["status"], noise=case["noise"])


def reference_gate(case, cmd, gate=GATE, f32=False, lm_from_pred=False):
    """The rejected set by the ungated hook alone: evaluate the message, delete the first slot with a finite nis > gate, repeat until there
    is none.  Earlier slots never depend on later ones, so this defines the set the gated replay rejects.  Returns dict(meas: the
    surviving message, orig: the original index of every survivor, rejected: [(original index, its six det values when it was
    deleted)], last: the ungated hook's result on the surviving message, nis: every finite nis the loop relied on)."""
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    orig = list(range(meas.shape[0]))
    rejected, seen = [], []
    while True:
        r = uhook(case, cmd, meas, f32, lm_from_pred)
        k = min(meas.shape[0], IR.MAX_DET)
        first = next((l for l in range(k) if np.isfinite(r["det"][l, 0]) and r["det"][l, 0] > gate), None)
        if first is None:
            seen += [float(v) for v in r["det"][:k, 0] if np.isfinite(v)]
            return dict(meas=meas, orig=orig, rejected=rejected, last=r, nis=seen)
        seen += [float(v) for v in r["det"][:first + 1, 0] if np.isfinite(v)]
        rejected.append((orig[first], r["det"][first].copy()))
        meas = np.delete(meas, first, axis=0)
        del orig[first]


def check_against_reference(g, ref, case, what):
    """Every output of the gated hook (dict g) against the reference loop, bit for bit."""
    meas = np.asarray(case["meas"], dtype=np.float32).reshape(-1, 3)
    k = meas.shape[0]
    last = ref["last"]
    assert g["flags"] == last["flags"], (what, g["flags"], last["flags"])
    if g["flags"] & PASS:
        assert not ref["rejected"], what
        assert g["n_rej"] == 0 and not g["verdict"].any() and g["count_out"] == k, what
        assert g["meas_out"][:k].tobytes() == meas.tobytes(), what
        assert np.isnan(g["post"]).all() and np.isnan(g["det"]).all() and np.isnan(g["nis_sum"]), what
        return
    surv = ref["meas"]
    assert g["count_out"] == surv.shape[0] and g["n_rej"] == len(ref["rejected"]) == k - surv.shape[0], (what, g["count_out"], g["n_rej"])
    assert g["meas_out"][:surv.shape[0]].tobytes() == surv.tobytes(), (what, "the surviving message")
    assert not g["meas_out"][surv.shape[0]:k].any(), (what, "the tail count_out .. count_in - 1 is zero")
    for l2, l in enumerate(ref["orig"]):            # survivors: what the ungated hook reports on the surviving message
        assert IR.bits(g["det"][l]) == IR.bits(last["det"][l2]) or (np.isnan(g["det"][l]).all() and np.isnan(last["det"][l2]).all()), (what, l)
        upd = int(meas[l, 0]) in case["st"]["ids"].tolist()       # an update slot is a found id
        assert g["verdict"][l] == (ACCEPTED if upd else NONE), (what, l, g["verdict"][l])
    for l, d in ref["rejected"]:                    # rejected: what the ungated hook reported when the loop deleted the slot
        assert IR.bits(g["det"][l]) == IR.bits(d) and g["verdict"][l] == REJECTED, (what, l)
    assert not g["verdict"][k:].any() and np.isnan(g["det"][k:]).all(), what
    assert IR.bits(g["post"]) == IR.bits(last["post"]), (what, "post")
    assert IR.bits(g["nis_sum"]) == IR.bits(last["nis_sum"]), (what, "nis_sum")
    assert g["n_upd"] == last["n_upd"] + g["n_rej"] and g["n_new"] == last["n_new"], what
    assert IR.bits(g["rec"][:15]) == IR.bits(last["rec"][:15]) and g["rec"][15] == g["n_rej"], (what, g["rec"], last["rec"])


def spiked(det, by=SPIKE):
    return [det[0], det[1] + by, det[2]]


def crafted_cases(seed, L_max, f32=False):
    """The crafted messages of the gate as dicts: name, st, status, meas [k][3] float32, noise (always a row), L_max, and what to expect:
    verdicts (list over the message; None = not stated), flags.  `main` cases state their verdicts through clean / spiked detections and
    must keep the margins of the module docstring.  L_max >= MAX_LM + 2."""
    assert L_max >= IR.MAX_LM + 2
    rng = np.random.default_rng(seed)
    out = []
    A, R, N = ACCEPTED, REJECTED, NONE

    def add(name, st, dets, verdicts=None, flags=0, status=0, noise=NOISE, main=True):
        out.append(dict(name=name, st=st, status=status, meas=np.asarray(dets, dtype=np.float32).reshape(-1, 3), noise=noise, L_max=L_max,
                        verdicts=verdicts, flags=flags, main=main and verdicts is not None))
    det = IR.detection
    st = IR.synthetic_state(rng, 5, f32)
    add("k = 0", st, [], [])
    add("k = 1, clean", st, [det(rng, st, 2)], [A])
    add("k = 1, spiked", st, [spiked(det(rng, st, 2))], [R])
    add("the first slot rejected", st, [spiked(det(rng, st, 0)), det(rng, st, 1), det(rng, st, 2)], [R, A, A])
    add("the last slot rejected", st, [det(rng, st, 0), det(rng, st, 1), spiked(det(rng, st, 2))], [A, A, R])
    add("every update rejected", st, [spiked(det(rng, st, j)) for j in (3, 1, 4)], [R, R, R])
    add("the same landmark twice, the first rejected", st, [spiked(det(rng, st, 1)), det(rng, st, 1)], [R, A])
    add("a negative spike in the middle", st, [det(rng, st, 4), spiked(det(rng, st, 0), -0.9), det(rng, st, 3)], [A, R, A])
    nearly = IR.synthetic_state(rng, L_max - 1, f32)
    add("an insertion and a capacity skip between updates", nearly,
        [spiked(det(rng, nearly, 0)), det(rng, nearly, new_id=7), det(rng, nearly, 1), det(rng, nearly, new_id=8), spiked(det(rng, nearly, 2)),
         det(rng, nearly, new_id=8), det(rng, nearly, 3)], [R, N, A, N, R, N, A])
    big = IR.synthetic_state(rng, IR.MAX_LM + 1, f32)
    # 64 detections over 8 landmarks; every fifth is spiked
    long64 = [spiked(det(rng, big, l % 8)) if l % 5 == 2 else det(rng, big, l % 8) for l in range(IR.MAX_DET)]
    add("64 detections", big, long64, [R if l % 5 == 2 else A for l in range(IR.MAX_DET)])
    add("65 detections", big, long64 + [spiked(det(rng, big, 0))], None, flags=IR.TOO_LONG)
    add("exactly MAX_LM distinct landmarks", big, [spiked(det(rng, big, j)) if j in (0, 9) else det(rng, big, j) for j in range(IR.MAX_LM)],
        [R if j in (0, 9) else A for j in range(IR.MAX_LM)])
    add("more than MAX_LM distinct landmarks", big, [spiked(det(rng, big, j)) if j == 3 else det(rng, big, j) for j in range(IR.MAX_LM + 1)], None,
        flags=IR.TOO_LONG)
    add("would freeze", st, [spiked(det(rng, st, 0)), det(rng, st, new_id=7), det(rng, st, new_id=7)], None, flags=IR.WOULD_FREEZE)
    add("frozen status", st, [spiked(det(rng, st, 2))], None, flags=IR.FROZEN, status=IR.INST_INDEX_OOR)
    zero = dict(st, P=np.zeros_like(st["P"]))
    add("singular S is never rejected", zero, [spiked(det(rng, st, 2)), det(rng, st, 0)], None, flags=IR.S_SINGULAR,
        noise=Noise(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.01, 0.0, 0.0, 0.0, 0.0))
    empty = IR.synthetic_state(rng, 0, f32)
    add("M = 0, two new ids", empty, [det(rng, empty, new_id=3), det(rng, empty, new_id=4)], [N, N])
    return out
