"""Joint-compatibility association without a GPU: the host hook (slam_associate_joint_instance_host, the kernel's own per-instance
function) against the independent reference of joint_reference.py on crafted cases.  Every test asserts its margins with the reference
first (individual and joint gate decisions at least 1e-6 relative from their gates, the best hypothesis at least 1e-9 relative from the
runner-up of equal size), then the hook's decisions, slots, verdicts, counts, node count and output message must equal the reference's.

d2_joint.  The hook's value is compared with an mpmath evaluation (50 digits) of nu^T S^-1 nu in which S = H P_pred H^T + W is formed in
mpmath from the hook's own double inputs (x and P as the storage rounds them, the command, the noise row, the innovations nu); the bound is
10 x the error of numpy's dense solve (numpy's own S) against that same mpmath value on the same case, floor 64 ulp.  Largest error of the
hook seen: 12.0 ulp of d2_joint (four pairings, fp32 storage), where numpy's was 7.0 ulp and the bound 69.7 ulp; on the other cases the
64 ulp floor was the bound in force and the hook's error at most 2.9 ulp.  Largest ratio of the hook's error to its bound: 0.17."""
import numpy as np
import pytest

import assoc_reference as AR
import innovation_reference as IR
import joint_reference as JR
from live_ekf_slam_amd.config import default_joint_config
from live_ekf_slam_amd.filters import associate_instance_host

A1, A2, C = 0.50, 0.58, -0.80     # bearings: two neighbours 0.08 rad apart and an isolated landmark
SHIFT = 0.05                      # the bearing innovation a yaw error puts on every detection


def _case(st, dets, L_max=8, noise=JR.TIGHT, cmd=JR.ZERO_CMD, status=0, **kw):
    return dict(st=st, status=status, meas=np.asarray(dets, dtype=np.float32).reshape(-1, 3), noise=noise, L_max=L_max, cmd=cmd, **kw)


def _run(case, cfg=None, f32=False, exhaustive=True):
    cfg = cfg or JR.joint_cfg()
    cost, nu = AR.reference_costs(case, cmd=case["cmd"], f32=f32)
    ref = JR.reference_joint(case, cost, nu, cfg, f32)
    JR.check_margins(case, cost, ref, cfg)
    g = JR.jhook(case, cfg, f32)
    JR.check_against_reference(g, ref, case.get("name", ""), AR.padded_row(case))
    if exhaustive and ref["search"] is not None and not ref["flags"] & JR.BUDGET:
        hyp = JR.exhaustive(case, cost, nu, cfg, f32)
        top = max(n for n, _, _ in hyp)
        best = min((d, i) for i, (n, d, _) in enumerate(hyp) if n == top)
        assert hyp[best[1]][2] == ref["search"]["assign"], "the search against the exhaustive enumeration"
    return g, ref, cost, nu


def _nn(case, f32=False):
    st = case["st"]
    return associate_instance_host(st["x"], st["P"], st["ids"], case["L_max"], case["status"], case["cmd"], case["meas"], case["noise"], f32_storage=f32)


def test_a_separated_grid_equals_nearest_neighbour():
    rng = np.random.default_rng(3)
    st = AR.grid_state(rng, 12)
    dets = [AR.clean(rng, st, j) for j in (4, 0, 9, 2, 11)] + [AR.fresh(3)]
    case = _case(st, dets, L_max=20, noise=AR.NOISE, cmd=AR.CMD)
    g, ref, cost, _ = _run(case)
    nn = _nn(case)
    assert list(g["ncand"][:6]) == [1, 1, 1, 1, 1, 0] and g["nodes"] == 5 and g["flags"] == 0
    assert np.array_equal(g["verdict"], nn["verdict"]) and np.array_equal(g["slot"], nn["slot"]) and AR.same_bits(g["det"], nn["det"])
    assert g["meas_out"].tobytes() == nn["meas_out"].tobytes() and g["rec"][15] == 0
    assert AR.same_bits(g["cost"], nn["cost"]) and AR.same_bits(g["cost"], cost)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_b_nearest_neighbour_is_wrong_and_a_second_detection_pins_the_pose(f32):
    st = JR.yaw_state([A1, A2, C], f32=f32)
    case = _case(st, [JR.seen(st, 0, SHIFT), JR.seen(st, 2, SHIFT)])
    g, ref, cost, _ = _run(case, f32=f32)
    nn = _nn(case, f32)
    assert cost[0, 1] < cost[0, 0] < JR.joint_cfg().gate_match                 # individually the neighbour is nearer
    assert list(nn["verdict"][:2]) == [JR.MATCHED, JR.MATCHED] and list(nn["slot"][:2]) == [1, 2]     # nearest neighbour: the wrong slot
    assert list(g["verdict"][:2]) == [JR.MATCHED, JR.MATCHED] and list(g["slot"][:2]) == [0, 2]       # jointly: the true one
    assert g["nodes"] == 4 and g["rec"][15] == 1 and list(g["meas_out"][:, 0]) == [200.0, 202.0]
    leaves = ref["search"]["leaves"]
    assert leaves[0][0] == 1 and leaves[0][2] == {0: 1}, "the first dive holds the wrong pairing alone: with it, detection 1 is incompatible"


def test_c_two_detections_with_the_same_best_slot_are_both_paired():
    st = JR.yaw_state([A1, A2])
    case = _case(st, [JR.seen(st, 0, SHIFT), JR.seen(st, 1, SHIFT)])
    g, ref, _, _ = _run(case)
    nn = _nn(case)
    assert list(nn["slot"][:2]) == [1, 1] and list(nn["verdict"][:2]) == [JR.MATCHED, JR.CONFLICT]
    assert list(g["verdict"][:2]) == [JR.MATCHED, JR.MATCHED] and list(g["slot"][:2]) == [0, 1] and g["n_drop"] == 0


def test_d_a_spurious_detection_inside_an_individual_gate_is_left_unpaired():
    st = JR.yaw_state([A1, C])
    case = _case(st, [JR.seen(st, 1, SHIFT), JR.seen(st, 0, -0.04), JR.seen(st, 0, SHIFT)])
    g, ref, _, _ = _run(case)
    assert list(g["verdict"][:3]) == [JR.MATCHED, JR.UNPAIRED, JR.MATCHED] and g["n_drop"] == 1 and g["count_out"] == 2
    assert g["rec"][9] == 1 and list(g["meas_out"][:, 0]) == [201.0, 200.0, 0.0]
    nn = _nn(case)
    assert list(nn["verdict"][:3]) == [JR.MATCHED, JR.MATCHED, JR.CONFLICT]      # nearest neighbour keeps the spurious one


def test_e_a_budget_of_the_first_dive_returns_the_first_dive():
    st = JR.yaw_state([A1, A2, C])
    case = _case(st, [JR.seen(st, 0, SHIFT), JR.seen(st, 2, SHIFT)])
    full, _, _, _ = _run(case)
    g, ref, _, _ = _run(case, cfg=JR.joint_cfg(max_nodes=2))            # the first dive: 0 -> A2 compatible, 1 -> C incompatible
    assert g["flags"] == JR.BUDGET and g["nodes"] == 2 and g["rec"][13] == 1
    assert list(g["verdict"][:2]) == [JR.MATCHED, JR.UNPAIRED] and g["slot"][0] == 1
    assert full["flags"] == 0 and full["nodes"] == 4
    one, _, _, _ = _run(case, cfg=JR.joint_cfg(max_nodes=1))            # inside the first dive: the branch at hand competes
    assert one["flags"] == JR.BUDGET and one["nodes"] == 1 and one["n_match"] == 1


def test_f_more_than_sixteen_associable_detections_match_sixteen():
    rng = np.random.default_rng(5)
    st = AR.grid_state(rng, 18)
    case = _case(st, [AR.clean(rng, st, j) for j in range(18)], L_max=20, noise=AR.NOISE, cmd=AR.CMD)
    g, ref, _, _ = _run(case, exhaustive=False)
    assert g["n_match"] == 16 and g["n_drop"] == 2 and (g["verdict"][:18] == JR.UNPAIRED).sum() == 2 and g["count_out"] == 16
    from live_ekf_slam_amd.filters import innovation_instance_host
    inn = innovation_instance_host(st["x"], st["P"], st["ids"], 20, 0, AR.CMD, g["meas_out"][:16], AR.NOISE)
    assert inn["flags"] == 0 and inn["n_upd"] == 16, "the labelled message is not TOO_LONG for slam_innovation"


def test_g_a_singular_joint_S_is_flagged_and_the_search_goes_on():
    st = JR.yaw_state([A1, C, 0.1], yaw_var=0.0625, lm_var=0.0, pos_var=0.0)
    noise = JR.Noise(0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1e-4, 0.0, 0.0, 0.0, 0.0, 0.0)     # W_11 = 0: every bearing innovation is the yaw error alone
    case = _case(st, [JR.seen(st, 0, 0.01), JR.seen(st, 1, 0.01), JR.seen(st, 2, 0.01)], noise=noise)
    g, ref, _, _ = _run(case, exhaustive=False)
    assert g["flags"] == JR.S_SINGULAR and g["rec"][14] == 1 and g["n_match"] == 1 and g["nodes"] == ref["nodes"] >= 3
    assert list(g["verdict"][:3]) == [JR.MATCHED, JR.UNPAIRED, JR.UNPAIRED]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_h_the_edges_of_the_message(f32):
    rng = np.random.default_rng(9)
    st = AR.grid_state(rng, 10, f32)
    none = AR.grid_state(rng, 0, f32)
    grid = dict(L_max=20, noise=AR.NOISE, cmd=AR.CMD)
    cases = [_case(none, [AR.fresh(1), AR.fresh(7)], name="M = 0", **grid), _case(st, [], name="k = 0", **grid),
             _case(st, [AR.clean(rng, st, l % 10) for l in range(64)], name="64 detections", **grid),
             _case(st, [AR.clean(rng, st, l % 10) for l in range(65)], name="65 detections", **grid),
             _case(st, [AR.clean(rng, st, 2), AR.fresh(1)], name="frozen", status=IR.INST_INDEX_OOR, **grid),
             _case(st, [AR.clean(rng, st, 1), AR.fresh(2), AR.clean(rng, st, 1), [7.0, 7.0, 7.0]], name="sentinels", count=3, k_stride=4, **grid)]
    # (64 detections of 10 landmarks: six rivals per landmark, the default budget ends the search; the reference walks the same nodes)
    want = {"M = 0": (0, 2, 0), "k = 0": (0, 0, 0), "64 detections": (10, 0, JR.BUDGET), "65 detections": (0, 0, IR.TOO_LONG), "frozen": (0, 0, IR.FROZEN),
            "sentinels": (1, 1, 0)}
    for case in cases:
        g, ref, _, _ = _run(case, f32=f32, exhaustive=False)
        assert (g["n_match"], g["n_new"], g["flags"]) == want[case["name"]], case["name"]
        row = AR.padded_row(case)                       # in place: the output row is the input row
        st_ = case["st"]
        from live_ekf_slam_amd import _lib
        import ctypes as Ct
        co = Ct.c_int32(-1)
        cfg = default_joint_config()
        d = (lambda a, t: a.ctypes.data_as(t))
        x = np.ascontiguousarray(st_["x"]); P = np.ascontiguousarray(st_["P"]); ids = np.ascontiguousarray(st_["ids"])
        cmd = np.asarray(case["cmd"], np.float32)
        cnt = case["meas"].shape[0] if case.get("count") is None else case["count"]
        rc = _lib.lib().slam_associate_joint_instance_host(d(x, _lib._dp), d(P, _lib._dp), d(ids, _lib._ip) if ids.size else None, ids.size, 20,
                                                           case["status"], d(cmd, _lib._fp), d(row, _lib._fp), cnt, row.shape[0], Ct.byref(case["noise"]),
                                                           0, int(f32), Ct.byref(cfg), None, None, None, None, None, None, None, None, None,
                                                           d(row, _lib._fp), Ct.byref(co), None, None, None)
        assert rc == 0 and co.value == g["count_out"] and row.tobytes() == g["meas_out"].tobytes(), (case["name"], "in place")


def test_d2_joint_against_mpmath():
    """The bound and the figures: see the module docstring."""
    worst = 0.0
    for f32 in (False, True):
        st3 = JR.yaw_state([A1, A2, C, 0.1, -0.3], f32=f32)
        cases = [_case(JR.yaw_state([A1, A2, C], f32=f32), [JR.seen(st3, 0, SHIFT), JR.seen(st3, 2, SHIFT)]),
                 _case(st3, [JR.seen(st3, 0, SHIFT, 0.01), JR.seen(st3, 2, SHIFT + 0.004), JR.seen(st3, 3, SHIFT - 0.006, -0.01), JR.seen(st3, 4, SHIFT)])]
        for case in cases:
            cfg = JR.joint_cfg()
            cost, nu = AR.reference_costs(case, cmd=case["cmd"], f32=f32)
            ref = JR.reference_joint(case, cost, nu, cfg, f32)
            g = JR.jhook(case, cfg, f32)
            assert g["n_match"] == ref["n_match"] >= 2
            Pp, H = JR.predicted(case, f32)
            v, S = JR.stacked(case, nu, ref["search"]["pairs"], Pp, H)
            exact = JR.mp_d2(case, nu, ref["search"]["pairs"], f32)
            ulp = float(np.spacing(float(exact)))
            err_numpy = abs(float(JR.dense_d2(v, S) - exact))
            err_hook = abs(float(g["d2_joint"] - exact))
            bound = max(10.0 * err_numpy, 64.0 * ulp)
            print(f"d2_joint {float(exact):.17g}: hook {err_hook / ulp:.2f} ulp, numpy {err_numpy / ulp:.2f} ulp, bound {bound / ulp:.1f} ulp")
            worst = max(worst, err_hook / ulp)
            assert err_hook <= bound, (err_hook / ulp, bound / ulp)
    print("largest error of the hook:", worst, "ulp")


def test_default_joint_gates_are_the_chi_square_quantiles():
    import mpmath as mp
    mp.mp.dps = 50
    c = default_joint_config()
    for m in range(1, 17):
        x = mp.mpf(c.gate_joint[m - 1]) / 2
        cdf = 1 - mp.e ** (-x) * sum(x ** i / mp.factorial(i) for i in range(m))
        assert abs(cdf - mp.mpf("0.99")) < mp.mpf("1e-12"), (m, cdf)
    assert c.gate_joint[0] == c.gate_match and c.max_nodes == 2048
    assert all(c.gate_joint[i] < c.gate_joint[i + 1] for i in range(15))


def test_the_cpu_oracle_steps_on_the_labelled_message_without_a_flag(oracle):
    st = JR.yaw_state([A1, A2, C])
    case = _case(st, [JR.seen(st, 0, SHIFT), JR.seen(st, 2, SHIFT), AR.fresh(3)])
    g = JR.jhook(case, JR.joint_cfg())
    assert g["count_out"] == 3 and g["n_new"] == 1 and g["n_match"] == 2
    after, fl = IR.oracle_step(oracle, st, case["cmd"], g["meas_out"][:3], IR.config_for(case["noise"]), case["L_max"], False)
    assert not fl & IR.INST_INDEX_OOR
    assert np.asarray(after["ids"])[:4].tolist() == [200, 201, 202, 203] and int(after["M"]) == 4
