"""slam_consistency on the MI355X against the longdouble reference (tests/consistency_reference.py) evaluated at the device's own state
(get_state, truth(), the map): crafted states at every size of both LDS classes and of the workspace class, real simulator runs, and
the promises of the header - nothing else moves, an instance's value does not depend on its batch, a second call or the chunking.

Judging (consistency_reference.judge): per pool of at least 30 instances of one kind, every instance's figure
g = |v_dev - v| / (n u ||S||_2 ||z||_2^2) must be <= 10 G and <= 4, G being the largest figure of the three fp64 host routes in that
pool.  dof and flags exactly, map_rms within (2 M + 4) u.  No instance is left out except those built to carry a flag, and those are
counted.  Every pool's G, the device's largest g and their ratio are printed (pytest -s)."""
import os
import subprocess

import numpy as np
import pytest

import consistency_reference as R
from batch_state import ckpt_layout, differing_instances
from conftest import ROOT
from test_cholesky_highprec import cholesky_hp, spd_graded, spd_with_condition

pytestmark = pytest.mark.gpu

FAMILIES = ("k1e1", "k1e4", "k1e8", "graded")
TRUTH = np.array([0.5, -0.3, 0.2 + 2 * R.TWO_PI])   # (the simulator's heading is not wrapped)


@pytest.fixture(scope="module")
def S():
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    _lib.lib()
    return S


def _family(rng, kind, n):
    return spd_graded(rng, n) if kind == "graded" else spd_with_condition(rng, n, float(kind[1:]))


def _instance(rng, Smat, M, lm, dtype32, kind, status=0):
    """One crafted instance: P = Smat, e drawn at the size of sqrt(diag S), x = truth + e with the landmarks at M distinct map rows."""
    n = 3 + 2 * M
    P = Smat.astype(np.float32).astype(np.float64) if dtype32 else Smat
    e = rng.standard_normal(n) * np.sqrt(np.abs(np.diag(Smat)))
    ids = rng.permutation(lm.shape[0])[:M].astype(np.int32)
    x = np.concatenate([TRUTH + e[:3], (lm[ids] + e[3:].reshape(M, 2)).ravel()])
    return dict(P=P, x=x, M=M, ids=ids, truth=TRUTH, status=status, kind=kind)


def _write(S, L_max, dtype, insts, path, tmp_path):
    """A checkpoint of a fresh EKF handle with P (pad columns of ekf_ld zero), x, M, ids, status and truth replaced."""
    B = len(insts)
    src = S.BatchedEKF(B, L_max, dtype=dtype).readParams(); src.init(0.0, 0.0, 0.0)
    base = tmp_path / "init.ckpt"
    src.save_state(base); src.close()
    _, off, hd = ckpt_layout(base)
    raw = bytearray(open(base, "rb").read())
    ps, xs, esz = hd["pstride"], hd["xstride"], hd["esz"]
    ft = np.float64 if esz == 8 else np.float32

    def view(item, dt):
        o, nb = off[item]
        return np.frombuffer(raw, dtype=dt, count=nb // np.dtype(dt).itemsize, offset=o)
    Pv, xv, Mv, idv, flv, tv = view("P", ft), view("x", ft), view("M", np.int32), view("ids", np.int32), view("flags", np.int32), view("truth", np.float64)
    for b, it in enumerate(insts):
        n = 3 + 2 * it["M"]
        ld = (n + 1) & ~1 if esz == 8 else (n + 3) & ~3
        slab = np.zeros((n, ld), dtype=ft)
        slab[:, :n] = it["P"]
        Pv[b * ps:b * ps + n * ld] = slab.ravel()
        xv[b * xs:b * xs + n] = it["x"]
        Mv[b] = it["M"]
        idv[b * L_max:b * L_max + it["M"]] = it["ids"]
        flv[b] = it["status"]
        tv[3 * b:3 * b + 3] = it["truth"]
    open(path, "wb").write(bytes(raw))


def _load(S, L_max, dtype, insts, lm, tmp_path, tag="a"):
    path = tmp_path / f"crafted_{tag}.ckpt"
    _write(S, L_max, dtype, insts, path, tmp_path)
    f = S.BatchedEKF(len(insts), L_max, dtype=dtype).readParams()
    f.load_state(path); f.set_map(lm)
    os.remove(path)
    return f


def _nan_pattern(c, b, r):
    return all(bool(np.isnan(c[k][b])) == bool(np.isnan(float(r[k]))) for k in ("nees_full", "nees_pose", "map_rms"))


def _collect(f, c, maps, kinds, id_known=True, only=None, pools=None):
    """Reference at the device's state for every instance (or those of `only`); asserts dof, flags, the NaN pattern and map_rms; files
    every finite NEES into pools[kind] / pools[kind + " pose"].  Returns (pools, instances that carry a flag)."""
    pools = {} if pools is None else pools
    truth, status = f.truth(), f.status()
    flagged, wrong = [], []
    for b in (range(f.batch) if only is None else only):
        st = f.get_state(b)
        m = maps[b] if isinstance(maps, (list, tuple)) or np.ndim(maps) == 3 else maps
        r = R.reference(st["x"], st["P"], st["M"], st["ids"], truth[b], m, int(status[b]), id_known)
        if c["dof"][b] != r["dof"] or c["flags"][b] != r["flags"] or not _nan_pattern(c, b, r):
            wrong.append((b, kinds[b], int(c["dof"][b]), r["dof"], int(c["flags"][b]), r["flags"]))
            continue
        if r["flags"]:
            flagged.append(b)
        if np.isfinite(float(r["map_rms"])):
            ref = float(r["map_rms"])
            if not abs(c["map_rms"][b] - ref) <= R.map_rms_bound(st["M"]) * ref:
                wrong.append((b, kinds[b], "map_rms", c["map_rms"][b], ref))
        if np.isfinite(float(r["nees_full"])):
            pools.setdefault(kinds[b], []).append((c["nees_full"][b], r["nees_full"], r["S"], r["e"], r["z_full"]))
        if np.isfinite(float(r["nees_pose"])):
            pools.setdefault(kinds[b] + " pose", []).append((c["nees_pose"][b], r["nees_pose"], r["S"][:3, :3], r["e"][:3], r["z_pose"]))
    assert not wrong, f"{len(wrong)} instance(s) with wrong dof / flags / NaN pattern / map_rms: {wrong[:20]}"
    return pools, flagged


def _judge(pools, label):
    bad = []
    for name in sorted(pools):
        pool = pools[name]
        assert len(pool) >= 30, (label, name, len(pool))
        G, gd, bar, over = R.judge(pool)
        print(f"[consistency] {label} pool {name!r}: {len(pool)} instances, G = {G:.3g}, device max g = {gd:.3g}, "
              f"ratio = {gd / G if G else float('inf'):.3g}, bar = {bar:.3g}")
        if over:
            bad.append((name, len(over), gd, bar))
    assert not bad, f"{label}: pools above their bar (name, instances over, device max g, bar): {bad}"


def _crafted_batch(L_max, dtype32, seed, Ms, per=1, with_edges=True):
    rng = np.random.default_rng(seed)
    lm = rng.uniform(-8.0, 8.0, (L_max, 2))
    fams = [k for k in FAMILIES if not (dtype32 and k == "k1e8")]   # rounding kappa 1e8 to float can make it indefinite
    insts = []
    for M in Ms:
        for kind in fams:
            for _ in range(per):
                Y = _family(rng, kind, 3 + 2 * M)
                if dtype32:
                    assert cholesky_hp(Y.astype(np.float32).astype(np.float64))[0] is not None, (kind, M)
                insts.append(_instance(rng, Y, M, lm, dtype32, kind))
    edges = 0
    if with_edges:
        # P asymmetric by a skew part of relative size 1e-10: the value is that of (P + P^T) / 2 (fp64 storage; a pool of its own)
        if not dtype32:
            for i in range(32):
                M = int(rng.integers(1, L_max + 1)); n = 3 + 2 * M
                Y = spd_with_condition(rng, n, 1e3)
                K = np.triu(rng.standard_normal((n, n)), 1) * 1e-10 * np.abs(Y)
                it = _instance(rng, Y, M, lm, False, "skew")
                it["P"] = Y + K - K.T
                assert not np.array_equal(it["P"], it["P"].T)
                insts.append(it)
        # one negative pivot (the matrices of the CPU test; fp32 storage: D_k = -1e-3, above the rounding to float)
        n = 3 + 2 * L_max
        for k in (0, 2, 3, n // 2, n - 1):
            insts.append(_instance(rng, R.not_pd_matrix(rng, n, k, -1e-3 if dtype32 else -1e-6), L_max, lm, dtype32, f"not PD at {k}"))
        it = _instance(rng, spd_with_condition(rng, 13, 1e2), 5, lm, dtype32, "status NONFINITE", status=R.NONFINITE)
        insts.append(it)
        it = _instance(rng, spd_with_condition(rng, 13, 1e2), 5, lm, dtype32, "NaN in P")
        it["P"] = it["P"].copy(); it["P"][7, 4] = np.nan
        insts.append(it)
        it = _instance(rng, spd_with_condition(rng, 13, 1e2), 5, lm, dtype32, "id outside the map")
        it["ids"] = it["ids"].copy(); it["ids"][2] = L_max
        insts.append(it)
        edges = 8
    order = rng.permutation(len(insts))
    return lm, [insts[i] for i in order], edges


@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("L_max", [20, 50])
def test_crafted_states_at_every_size(S, L_max, dtype32, tmp_path):
    dt = S.F32 if dtype32 else S.F64
    # (two matrices per size and family at L_max = 20, so that a family's pool has 42 instances; 51 at L_max = 50)
    lm, insts, edges = _crafted_batch(L_max, dtype32, 7000 + L_max, range(L_max + 1), per=2 if L_max == 20 else 1)
    kinds = [it["kind"] for it in insts]
    f = _load(S, L_max, dt, insts, lm, tmp_path)
    c = f.consistency()
    pools, flagged = _collect(f, c, lm, kinds)
    expect = {"status NONFINITE": R.INSTANCE_FAILED, "NaN in P": R.FULL_NOT_PD, "id outside the map": R.NO_TRUTH}
    n = 3 + 2 * L_max
    expect.update({f"not PD at {k}": R.FULL_NOT_PD | (R.POSE_NOT_PD if k < 3 else 0) for k in (0, 2, 3, n // 2, n - 1)})
    assert sorted(kinds[b] for b in flagged) == sorted(expect) and len(flagged) == edges
    for b in flagged:
        assert c["flags"][b] == expect[kinds[b]], (kinds[b], c["flags"][b])
    pools = {k: v for k, v in pools.items() if k.split(" pose")[0] in FAMILIES + ("skew",)}   # (the edge instances' poses: a handful each)
    _judge(pools, f"crafted L_max={L_max} {'f32' if dtype32 else 'f64'}")
    c2 = f.consistency()
    assert all(c[k].tobytes() == c2[k].tobytes() for k in c), "a second call gives other bits"
    # the neighbours of the flagged instances: the same bits in a batch where those are replaced by a plain matrix
    clean = list(insts)
    rng = np.random.default_rng(1)
    for b in flagged:
        clean[b] = _instance(rng, spd_with_condition(rng, 3 + 2 * insts[b]["M"], 1e2), insts[b]["M"], lm, dtype32, "clean")
    g = _load(S, L_max, dt, clean, lm, tmp_path, "clean")
    cg = g.consistency()
    keep = np.setdiff1d(np.arange(len(insts)), flagged)
    assert np.all(cg["flags"] == 0)
    assert all(c[k][keep].tobytes() == cg[k][keep].tobytes() for k in c), "a flagged instance changed its neighbours"
    f.close(); g.close()


@pytest.mark.parametrize("dtype32", [False, True], ids=["f64", "f32"])
def test_workspace_class_every_size_at_60_landmarks(S, dtype32, tmp_path):
    L_max = 60
    lm, insts, _ = _crafted_batch(L_max, dtype32, 7060, range(L_max + 1), with_edges=False)
    kinds = [it["kind"] for it in insts]
    f = _load(S, L_max, S.F32 if dtype32 else S.F64, insts, lm, tmp_path)
    c = f.consistency()
    pools, flagged = _collect(f, c, lm, kinds)
    assert not flagged
    _judge(pools, f"workspace L_max=60 {'f32' if dtype32 else 'f64'}")
    f.close()


def test_workspace_class_in_chunks_and_at_1000_landmarks(S, tmp_path, monkeypatch):
    L_max = 200
    lm, insts, _ = _crafted_batch(L_max, False, 7200, (0, 51, 100, 200), per=8, with_edges=False)
    kinds = [it["kind"] for it in insts]
    f = _load(S, L_max, S.F64, insts, lm, tmp_path)
    monkeypatch.delenv("SLAM_CONSISTENCY_WS_BYTES", raising=False)
    c = f.consistency()
    per_instance = 8 * (3 + 2 * L_max + 1) * (3 + 2 * L_max + 2) // 2
    budget = 25_000_000
    assert len(insts) == 128 and -(-len(insts) // (budget // per_instance)) >= 3   # at least three chunks
    monkeypatch.setenv("SLAM_CONSISTENCY_WS_BYTES", str(budget))
    cc = f.consistency()
    monkeypatch.setenv("SLAM_CONSISTENCY_WS_BYTES", "1")   # below one instance: one instance per chunk
    c1 = f.consistency()
    monkeypatch.delenv("SLAM_CONSISTENCY_WS_BYTES")
    assert all(c[k].tobytes() == cc[k].tobytes() == c1[k].tobytes() for k in c), "chunked differs from unchunked"
    pools, flagged = _collect(f, c, lm, kinds)
    assert not flagged
    f.close()
    # one instance at the largest state the EKF holds; it joins the kappa 1e4 pool (g is normalised by n)
    rng = np.random.default_rng(71000)
    lm_big = rng.uniform(-30.0, 30.0, (1000, 2))
    big = [_instance(rng, spd_with_condition(rng, 2003, 1e4), 1000, lm_big, False, "k1e4")]
    h = _load(S, 1000, S.F64, big, lm_big, tmp_path, "big")
    cb = h.consistency()
    print(f"[consistency] L_max=1000, M=1000: device time {h.last_consistency_work()[1]:.1f} ms")
    pools, flagged = _collect(h, cb, lm_big, ["k1e4"], pools=pools)
    assert not flagged and cb["dof"][0] == 2003 and len(pools["k1e4"]) == 33
    _judge(pools, "workspace L_max=200 (+ one instance at L_max=1000)")
    h.close()


def _run(S, L, T, B, dt, quirk=1, id_known=1, each=False, seed=2025):
    from live_ekf_slam_amd.scenario import make_scenario
    lm, cmds = make_scenario(321 + L, L, T)
    cfg = S.default_config()
    cfg.replicate_vw_quirk = quirk
    cfg.landmark_id_is_known = id_known
    f = S.BatchedEKF(B, L, dtype=dt).readParams(cfg)
    f.set_seed(seed)
    maps = lm
    if each:
        rng = np.random.default_rng(5)
        maps = lm[None] + rng.normal(0.0, 0.3, (B, L, 2))
        f.set_map(maps)
        f.init(rng.uniform(-0.005, 0.005, (B, 3)).astype(np.float32))
    else:
        f.set_map(lm)
        f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds)
    return f, maps


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("L,T,dtype32", [(20, 400, False), (50, 1000, False), (50, 1000, True)])
def test_real_runs(S, L, T, dtype32, quirk):
    B = 256
    f, lm = _run(S, L, T, B, S.F32 if dtype32 else S.F64, quirk)
    c = f.consistency()
    label = f"run L={L} T={T} {'f32' if dtype32 else 'f64'} quirk={quirk}"
    pools, flagged = _collect(f, c, lm, ["run"] * B)
    assert not flagged and not c["flags"].any() and not f.status().any(), (label, np.flatnonzero(c["flags"]), c["flags"][c["flags"] != 0])
    assert len(pools["run"]) == B and len(pools["run pose"]) == B
    _judge(pools, label)
    from live_ekf_slam_amd.filters import consistency_summary
    print(f"[consistency] {label}: full {consistency_summary(c['nees_full'], c['dof'], c['flags'])}, "
          f"pose {consistency_summary(c['nees_pose'], np.full(B, 3), c['flags'])}, map_rms mean {c['map_rms'].mean():.4g}")
    f.close()


def test_real_run_with_per_instance_maps_and_start_poses(S):
    B = 256
    f, maps = _run(S, 20, 400, B, S.F64, each=True)
    c = f.consistency()
    pools, flagged = _collect(f, c, maps, ["run"] * B)
    assert not flagged and not c["flags"].any()
    assert len(pools["run"]) == B and len(pools["run pose"]) == B
    _judge(pools, "run L=20 T=400 f64, per-instance maps and start poses")
    f.close()


def test_unknown_ids_report_the_pose_only(S):
    B = 256
    f, lm = _run(S, 20, 400, B, S.F64, id_known=0)
    c = f.consistency()
    M = f.landmark_counts()
    assert not f.status().any()
    pools, flagged = _collect(f, c, lm, ["run"] * B, id_known=False)
    assert len(flagged) == int((M > 0).sum()) and (M > 0).any()
    assert np.array_equal(c["flags"], np.where(M > 0, R.NO_TRUTH, 0)) and np.array_equal(c["dof"], 3 + 2 * M)
    assert np.all(np.isnan(c["nees_full"][M > 0])) and np.all(np.isnan(c["map_rms"][M > 0]))
    assert "run" not in pools or len(pools["run"]) == int((M == 0).sum())
    pools = {"run pose": pools["run pose"]}
    assert len(pools["run pose"]) == B
    _judge(pools, "run L=20 T=400 f64, unknown ids")
    f.close()


def _bits(c):
    return b"".join(np.ascontiguousarray(c[k]).tobytes() for k in ("nees_full", "nees_pose", "map_rms", "dof", "flags"))


def test_nothing_else_moves(S):
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 20, 120, 17
    lm, cmds = make_scenario(321 + L, L, T)

    def handle(batch=B, offset=0):
        f = S.BatchedEKF(batch, L).readParams(); f.set_seed(11); f.set_instance_offset(offset); f.set_map(lm); f.init(0.0, 0.0, 0.0)
        return f
    a, b = handle(), handle()
    seen = {}
    a.set_lazy_steps(0); b.set_lazy_steps(0)
    for t in range(21):
        if t in (0, 1, 7, 20):
            seen[t] = a.consistency()
            assert _bits(a.consistency()) == _bits(seen[t]), "a second call gives other bits"
            b.status()   # (any getter runs the queue: both handles launch the same steps together, b just never asks for the NEES)
        a.update_sim(cmds[t]); b.update_sim(cmds[t])
    a.set_lazy_steps(16); b.set_lazy_steps(16)
    for t in range(21, 60):
        if t == 30:
            from live_ekf_slam_amd import _lib
            assert _lib.lib().slam_queued_steps(a.h) > 0   # inside a queued stretch: the call runs the queue first
            seen[t] = a.consistency()
            b.status()
        a.update_sim(cmds[t]); b.update_sim(cmds[t])
    a.run_sim(cmds[60:]); b.run_sim(cmds[60:])
    seen[T] = a.consistency()
    assert differing_instances(a, b) == []
    assert np.array_equal(a.k_histogram(), b.k_histogram()) and np.array_equal(a.traffic_counters(), b.traffic_counters())
    assert _bits(b.consistency()) == _bits(seen[T])
    # the value of an instance does not depend on the batch it sits in
    for inst in (0, 5, 16):
        s = handle(1, inst)
        s.run_sim(cmds)
        cs = s.consistency()
        for k in cs:
            assert cs[k].tobytes() == seen[T][k][inst:inst + 1].tobytes(), (inst, k)
        s.close()
    # with an instance tracked in its shadow filter the call still answers for the batch
    t1, t2 = handle(), handle()
    t1.track_instance(3)
    for t in range(40):
        t1.update_sim(cmds[t]); t2.update_sim(cmds[t])
    assert _bits(t1.consistency()) == _bits(t2.consistency())
    for f in (a, b, t1, t2):
        f.close()


def test_errors_and_null_outputs(S):
    from live_ekf_slam_amd import _lib
    f = S.BatchedEKF(4, 20).readParams()
    with pytest.raises(S.SlamError, match="slam_init has not been called"):
        f.consistency()
    f.init(0.0, 0.0, 0.0)
    with pytest.raises(S.SlamError, match="slam_set_map"):
        f.consistency()
    f.set_map(np.array([[2.0, 1.0], [-3.0, 2.0], [4.0, -4.0]]))
    for _ in range(5):
        f.update_sim((0.1, 0.02))
    c = f.consistency()
    L = _lib.lib()
    assert L.slam_consistency(f.h, None, None, None, None, None) == 0
    pose = np.zeros(4)
    assert L.slam_consistency(f.h, None, pose.ctypes.data_as(_lib._dp), None, None, None) == 0
    assert pose.tobytes() == c["nees_pose"].tobytes()
    by, ms = f.last_consistency_work()
    assert by > 0 and ms > 0
    f.close()
    for u in (S.BatchedUKF(2, 20).readParams(), S.BatchedUKFLoc(2).readParams()):
        u.set_map(np.array([[2.0, 1.0], [-3.0, 2.0]])); u.init(0.0, 0.0, 0.0)
        with pytest.raises(S.SlamError, match="rank-deficient"):
            u.consistency()
        u.close()


def test_cpp_mirror_equals_the_python_mirror(S, tmp_path):
    from live_ekf_slam_amd.scenario import make_scenario
    B, L, T = 8, 10, 90
    dump = str(tmp_path / "consistency.bin")
    out = subprocess.run([os.path.join(ROOT, "live_ekf_slam_amd", "filter_driver"), "consistency", str(B), str(L), str(T), dump],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "driver ok: consistency" in out.stdout, out.stdout + out.stderr
    raw = open(dump, "rb").read()
    assert int(np.frombuffer(raw[:8], dtype=np.int64)[0]) == B and len(raw) == 8 + B * (3 * 8 + 2 * 4)
    lm, cmds = make_scenario(1234, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.init(0.0, 0.0, 0.0); f.set_map(lm); f.run_sim(cmds)
    c = f.consistency()
    assert raw[8:] == _bits(c) and not c["flags"].any() and np.all(c["nees_full"] > 0)
    f.close()


def test_full_size_once(S):
    from live_ekf_slam_amd.filters import consistency_summary
    from live_ekf_slam_amd.scenario import make_scenario
    L, T, B = 50, 100, 65536
    lm, cmds = make_scenario(321 + L, L, T)
    f = S.BatchedEKF(B, L).readParams(); f.set_map(lm); f.init(0.0, 0.0, 0.0)
    f.run_sim(cmds)
    c = f.consistency()
    by, ms = f.last_consistency_work()
    assert not c["flags"].any(), (np.flatnonzero(c["flags"])[:20], c["flags"][c["flags"] != 0][:20])
    assert all(np.all(np.isfinite(c[k])) for k in ("nees_full", "nees_pose", "map_rms")) and np.array_equal(c["dof"], 3 + 2 * f.landmark_counts())
    drawn = np.sort(np.random.default_rng(65536).choice(B, 256, replace=False))
    pools, flagged = _collect(f, c, lm, {int(b): "run" for b in drawn}, only=[int(b) for b in drawn])
    assert not flagged and len(pools["run"]) == 256
    _judge(pools, f"full size L={L} B={B} T={T}")
    print(f"[consistency] full size: {ms:.2f} ms on the device, model {by / 1e9:.3f} GB, summary {consistency_summary(c['nees_full'], c['dof'], c['flags'])}")
    f.close()
