"""ukf_chol_kernel at every state size of both LDS classes against a high-precision factor (tests/test_cholesky_highprec.py).

On the bench scenario most instance-steps fall back to the eigen path, so the Cholesky kernel's large-n code (the packed-triangle row
recovery, trailing triangles larger than the workgroup, the byte-packed (row, column) table) is fed crafted matrices instead: a UKF
checkpoint is written with our own P (every M from 0 to L_max in one ragged batch), one update with no detections predicts only, and the
factor is read back from the stored square root sqtP = L^T of a checkpoint taken after the step.  Each factor must meet Higham's
componentwise backward-error bound and a forward-error bound against the longdouble factor.  The pivot rule is tested at its edge: an
exact pivot of 2e-8 must factor, one of 5e-9, a NaN or an Inf must take the cold eigen path, bit-identical to an eigen handle's step,
and leave the other instances of the batch untouched."""
import numpy as np
import pytest

from batch_state import ckpt_layout
from test_cholesky_highprec import EPS, cholesky_hp, gamma, spd_graded, spd_with_condition, spd_with_pivot

pytestmark = pytest.mark.gpu

# Forward error ||L - L_ref||_F / ||L_ref||_2 <= C_FWD * n * eps * kappa_2(Y).  First-order perturbation theory (Sun 1991; Higham, ASNA
# 2nd ed., sec. 10.1) bounds it by 2^-1/2 kappa_2 ||dY||_F / ||Y||_2, and the backward error ||dY||_F <= gamma_{n+1} trace(Y)
# <= gamma_{n+1} n ||Y||_2, so the worst case is about 0.7 (n + 1) n eps kappa; that needs every rounding error aligned.  LAPACK's
# factor of these same matrices (n = 4..104, kappa 1e1..1e8 and the graded ones) measured at most 0.017 n eps kappa, so C_FWD = 1 leaves
# a margin of 50 over a sound factorisation while a wrong or skipped element (an error of the order of |L| itself) is far outside it.
C_FWD = 1.0
PIVOT_FACTORS, PIVOT_FALLS_BACK = 2e-8, 5e-9     # either side of the kernel's floor of 1e-8


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _scale(M):
    return float(np.float32(2 * M + 4) / (np.float32(1) - np.float32(0.2)))   # ukf.cpp:114 in float, as both sqrt kernels form it


def _scaled(P, M):
    return 0.5 * (P + P.T) * _scale(M)


def _cases(L_max, seed):
    """[(name, M, P, expect)] for one handle: every M in 0..L_max with kappa 1e1, 1e4, 1e8 and a graded diagonal (expect "factor"),
    then the pivot-edge matrices at the class's largest n and a NaN and an Inf off-diagonal pair (expect "eigen")."""
    rng = np.random.default_rng(seed)
    cases = []
    for M in range(L_max + 1):
        n = 4 + 2 * M
        for kind in ("k1e1", "k1e4", "k1e8", "graded"):
            Y = spd_graded(rng, n) if kind == "graded" else spd_with_condition(rng, n, float(kind[1:]))
            cases.append((f"n={n} {kind}", M, Y / _scale(M), "factor"))
    M = L_max; n = 4 + 2 * M
    for k in sorted({0, n // 2, 43, min(44, n - 1), n - 1}):
        for p, expect in ((PIVOT_FACTORS, "factor"), (PIVOT_FALLS_BACK, "eigen")):
            cases.append((f"n={n} pivot {p:g} at column {k}", M, spd_with_pivot(rng, n, k, p) / _scale(M), expect))
    for bad, (i, j) in ((np.nan, (n - 1, 0)), (np.inf, (n // 2 + 1, n // 2))):
        P = spd_with_condition(rng, n, 1e2) / _scale(M)
        P[i, j] = P[j, i] = bad
        cases.append((f"n={n} {bad} at ({i}, {j})", M, P, "eigen"))
    for name, M, P, expect in cases:
        assert np.array_equal(P, P.T, equal_nan=True), name   # exactly symmetric: Y = P * scale, one rounding per element
        L, piv = cholesky_hp(_scaled(P, M))                   # the inputs themselves: which side of the floor the exact pivots lie
        factors = L is not None and float(np.min(piv)) >= 1.5e-8
        falls_back = L is None or not np.all(np.isfinite(piv.astype(np.float64))) or float(np.min(piv)) <= 0.6e-8
        assert (factors, falls_back) == ((True, False) if expect == "factor" else (False, True)), (name, np.min(piv))
    return [cases[i] for i in rng.permutation(len(cases))]   # ragged sizes, edges and all, mixed in one launch


def _write(S, L_max, Ps, Ms, path, tmp_path):
    """A checkpoint of a fresh handle with P, M, ids and x replaced: landmarks 0..M-1 at plausible positions, the vehicle at
    (0.5, -0.3) heading 0, every warm start marked cold (age -1)."""
    B = len(Ps)
    src = S.BatchedUKF(B, L_max).readParams(); src.init(0.0, 0.0, 0.0)
    base = tmp_path / "init.ckpt"
    src.save_state(base); src.close()
    head, off, hd = ckpt_layout(base)
    raw = bytearray(open(base, "rb").read())
    ps, xs = hd["pstride"], hd["xstride"]

    def view(item, dt):
        o, nb = off[item]
        return np.frombuffer(raw, dtype=dt, count=nb // np.dtype(dt).itemsize, offset=o)
    Pv, xv, Mv, idv, agev = view("P", np.float64), view("x", np.float64), view("M", np.int32), view("ids", np.int32), view("age", np.int32)
    rng = np.random.default_rng(3)
    for b, (P, M) in enumerate(zip(Ps, Ms)):
        n = 4 + 2 * M
        Pv[b * ps:b * ps + n * n] = P.ravel()
        Mv[b] = M
        idv[b * L_max:b * L_max + M] = np.arange(M)
        xv[b * xs:b * xs + n] = np.concatenate([[0.5, -0.3, 1.0, 0.0], rng.uniform(-5.0, 5.0, 2 * M)])
        agev[b] = -1
    open(path, "wb").write(bytes(raw))


def _step(S, L_max, B, path, mode, tmp_path, tag):
    """Load the checkpoint into a new handle, take one predict-only update; return the handle and sqtP of every instance."""
    f = S.BatchedUKF(B, L_max).readParams(); f.set_sqrt_mode(mode); f.load_state(path)
    f.update(S.Command(0.05, 0.01), [])
    after = tmp_path / f"after_{tag}.ckpt"
    f.save_state(after)
    _, off, hd = ckpt_layout(after)
    o, nb = off["sqtP"]
    sq = np.fromfile(after, dtype=np.float64, count=nb // 8, offset=o).reshape(B, hd["pstride"])
    return f, sq


@pytest.mark.parametrize("L_max", [20, 50])
def test_cholesky_kernel_at_every_size_against_a_high_precision_factor(S, L_max, tmp_path):
    cases = _cases(L_max, 950 + L_max)
    B = len(cases)
    names = [c[0] for c in cases]; Ms = [c[1] for c in cases]; Ps = [c[2] for c in cases]; expect = [c[3] for c in cases]
    edge = [i for i, c in enumerate(cases) if "pivot" in c[0] or "nan" in c[0] or "inf" in c[0]]
    # the same batch with every edge instance swapped for a well-conditioned matrix of its size: the neighbours' reference
    clean = list(Ps)
    for i in edge:
        clean[i] = spd_with_condition(np.random.default_rng(i), 4 + 2 * Ms[i], 1e2) / _scale(Ms[i])
    p_edge, p_clean = tmp_path / "edge.ckpt", tmp_path / "clean.ckpt"
    _write(S, L_max, Ps, Ms, p_edge, tmp_path)
    _write(S, L_max, clean, Ms, p_clean, tmp_path)

    c, sq = _step(S, L_max, B, p_edge, "cholesky", tmp_path, "c")
    status = c.status()
    e, _ = _step(S, L_max, B, p_edge, "eigen", tmp_path, "e")
    es = e.status()

    bad = []   # (n, message) of every instance that fails, so a failure names all the sizes affected
    for b in range(B):
        if expect[b] != "factor":
            continue
        M = Ms[b]; n = 4 + 2 * M
        Y = _scaled(Ps[b], M)
        L = sq[b, :n * n].reshape(n, n).T            # sqtP = L^T row-major
        why = []
        if status[b] != 0:
            why.append(f"status {status[b]}")
        if not (np.all(np.triu(L, 1) == 0.0) and np.all(np.diag(L) > 0)):
            why.append("not lower-triangular with a positive diagonal")
        Ll = L.astype(np.longdouble)                  # the check's own products: exact to far below gamma_{n+1}
        R = np.abs(Ll @ Ll.T - Y)
        bound = gamma(n + 1) * (np.abs(Ll) @ np.abs(Ll).T)
        if not np.all(R <= bound):
            r, q = np.unravel_index(np.argmax(R - bound), R.shape)
            why.append(f"backward error {float(R[r, q]):.3g} > {float(bound[r, q]):.3g} at ({r}, {q})")
        Lr, _ = cholesky_hp(Y)
        ev = np.linalg.eigvalsh(Y)
        fwd = float(np.linalg.norm((Ll - Lr).astype(np.float64)) / np.sqrt(ev[-1]))
        if not fwd <= C_FWD * n * EPS * (ev[-1] / ev[0]):
            why.append(f"forward error {fwd:.3g} > {C_FWD * n * EPS * ev[-1] / ev[0]:.3g}")
        X = c.sigma_points(b)                         # the offsets the step used are the columns of L
        x = X[:, 0]
        if not (X.shape == (n, 2 * n + 1) and np.array_equal(X[:, 1:n + 1], x[:, None] + L) and np.array_equal(X[:, n + 1:], x[:, None] - L)):
            why.append("sigma points are not x +- the columns of L")
        if why:
            bad.append((n, f"instance {b} ({names[b]}): " + "; ".join(why)))

    # the fallbacks: the cold eigen step of an eigen handle on the same checkpoint, bit for bit, and the same status word (0 for the
    # small pivots; a NaN or an Inf in P is SLAM_INST_NONFINITE in both modes)
    for b in range(B):
        if expect[b] == "eigen":
            sc, se = c.get_state(b), e.get_state(b)
            same = sc["M"] == se["M"] and sc["x"].tobytes() == se["x"].tobytes() and sc["P"].tobytes() == se["P"].tobytes()
            same = same and c.sigma_points(b).tobytes() == e.sigma_points(b).tobytes()
            if not same or status[b] != es[b] or ("pivot" in names[b] and status[b] != 0):
                bad.append((4 + 2 * Ms[b], f"instance {b} ({names[b]}): not the eigen handle's cold step "
                            f"(state equal {same}, status {status[b]} vs {es[b]})"))
    assert not bad, (f"{len(bad)} instance(s) wrong at n = {sorted({n for n, _ in bad})}:\n" + "\n".join(m for _, m in bad[:40]))
    n_fallback = expect.count("eigen")
    assert c.sqrt_stats().tolist() == [B - n_fallback, n_fallback], (c.sqrt_stats(), n_fallback)
    e.close()

    # the neighbours: the same bits as in the batch without the edge instances
    k, sqk = _step(S, L_max, B, p_clean, "cholesky", tmp_path, "k")
    assert int(k.sqrt_stats()[1]) == 0
    for b in range(B):
        if b in edge:
            continue
        n = 4 + 2 * Ms[b]
        sc, sk = c.get_state(b), k.get_state(b)
        assert sq[b, :n * n].tobytes() == sqk[b, :n * n].tobytes(), names[b]
        assert sc["x"].tobytes() == sk["x"].tobytes() and sc["P"].tobytes() == sk["P"].tobytes() and status[b] == k.status()[b], names[b]
    k.close(); c.close()
