"""The host build of the fp64 functions the kernels and the oracle compile from one text (live_ekf_slam_amd/csrc/slam_math.h), at the
edge sets of tests/math_edges.py, against references that do not share that text: mpmath at 300 bits for sin / cos / atan2, glibc for
remainder and for the zero / axis / NaN conventions, the oracle's own 2x2 inverse and exact rational arithmetic for inv2x2_lu, and a
plain Python statement of assoc_abs.  The parity suites cannot see an error in that text, because both sides make it.
tests/test_math_edges_gpu.py then ties the device build to this host build bit for bit on the same sets."""
import ctypes as C
import math
from fractions import Fraction

import numpy as np
import pytest

import math_edges as E

_dp = C.POINTER(C.c_double)
MP_BITS = 300

# det_sincos: the header's claim, "error < 1 ulp" inside the domain.  Measured on sincos_in_domain(): 0.757 ulp (cos at x = 14.912774223267794).
SINCOS_ULP_BOUND = 1.0
# det_atan2: the maximum the host build reaches on atan2_pairs() is 1.163 ulp, at (y, x) = (-8.964202309202546, -3.353288908687162):
# third quadrant, where (z - pi_lo) - pi adds two roundings to det_atan's own error.  The bound is that maximum rounded up to the next
# quarter ulp; the margin absorbs changes of the set, not another algorithm.  (First / fourth quadrant alone: 0.861 ulp.)
ATAN2_ULP_BOUND = 1.25


def dp(a):
    return a.ctypes.data_as(_dp)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def assert_same_bits(got, ref, what):
    """Equal bit patterns (so equal signs of zero); where ref is NaN, got is NaN of any payload."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), what
    bad = np.flatnonzero((bits(got) != bits(ref)) & ~nan)
    assert bad.size == 0, f"{what}: {bad.size} differ, first at {bad[0]}: {got[bad[0]]!r} vs {ref[bad[0]]!r}"


def ulp_of(exact):
    """The fp64 unit in the last place at the magnitude of the mpmath number `exact` (the subnormal spacing below DBL_MIN)."""
    import mpmath
    e = int(mpmath.floor(mpmath.log(abs(exact), 2)))
    return mpmath.ldexp(1, max(e, -1022) - 52)


def ulp_err(got, exact):
    return abs(float(abs(got - exact) / ulp_of(exact)))   # float - mpf is exact at MP_BITS


def sincos_errs(L, x):
    """ulp errors (sin, cos) of det_sincos on the finite array x against mpmath."""
    import mpmath
    s, c = np.zeros(x.size), np.zeros(x.size)
    L.orc_det_sincos(dp(x), dp(s), dp(c), x.size)
    es, ec = np.zeros(x.size), np.zeros(x.size)
    with mpmath.workprec(MP_BITS + 64):   # sin next to k pi loses up to ~70 bits to cancellation at |x| < 2^21
        for i, xi in enumerate(x):
            m = mpmath.mpf(float(xi))
            rs, rc = mpmath.sin(m), mpmath.cos(m)
            es[i] = ulp_err(float(s[i]), rs) if rs != 0 else abs(s[i])
            ec[i] = ulp_err(float(c[i]), rc)
    return es, ec, s, c


def test_edge_sets_are_what_they_say():
    x = E.sincos_in_domain()
    assert 10000 < x.size < 12000 and np.all(np.isfinite(x)) and np.abs(x).max() > 1.64e6
    for k in (1, 3, 5):   # k * kPi is exact, so the rem2pi ties are hit exactly
        assert Fraction(k * E.K_PI) == k * Fraction(E.K_PI)
    b = E.sincos_beyond()
    assert b[0] == 1.65e6 and np.nanmax(np.abs(b[np.isfinite(b)])) <= 1e18 and np.isnan(b).sum() == 1 and np.isinf(b).sum() == 2
    seed, inst, t, p = E.philox_counters()
    assert seed.size == inst.size == t.size == p.size and seed.size >= 2000
    a, bb, c, d = E.pack_counters(seed, inst, t, p)
    for v in (a, bb, c, d):
        assert np.all(v < 2.0 ** 48) and np.all(v == np.floor(v))
    assert np.array_equal(a.astype(np.uint64) | ((c.astype(np.uint64) & np.uint64(0xFFFF)) << np.uint64(48)), seed)
    assert np.array_equal(bb.astype(np.uint64) | ((d.astype(np.uint64) & np.uint64(0xFFFF)) << np.uint64(48)), inst)
    assert np.array_equal((c.astype(np.uint64) >> np.uint64(16)).astype(np.uint32), t)
    assert np.array_equal((d.astype(np.uint64) >> np.uint64(16)).astype(np.uint32), p)


def test_det_sincos_within_one_ulp_of_exact(oracle):
    L = oracle.lib()
    x = E.sincos_in_domain()
    es, ec, s, c = sincos_errs(L, x)
    i, j = int(es.argmax()), int(ec.argmax())
    print(f"det_sincos on {x.size} points: max sin error {es[i]:.4f} ulp at {x[i]!r}, max cos error {ec[j]:.4f} ulp at {x[j]!r}")
    assert es[i] < SINCOS_ULP_BOUND and ec[j] < SINCOS_ULP_BOUND
    # zero arguments keep their sign, as with libm
    z = np.array([0.0, -0.0])
    sz, cz, ls, lc = (np.zeros(2) for _ in range(4))
    L.orc_det_sincos(dp(z), dp(sz), dp(cz), 2); L.orc_libm_sincos(dp(z), dp(ls), dp(lc), 2)
    assert_same_bits(sz, ls, "sin(+-0)"); assert_same_bits(cz, lc, "cos(+-0)")
    assert np.array_equal(bits(sz), bits(z))


def test_det_atan2_against_exact_and_libm_conventions(oracle):
    import mpmath
    L = oracle.lib()
    y, x = E.atan2_pairs()
    got, lm = np.zeros(y.size), np.zeros(y.size)
    L.orc_det_atan2(dp(y), dp(x), dp(got), y.size); L.orc_libm_atan2(dp(y), dp(x), dp(lm), y.size)
    special = np.isnan(y) | np.isnan(x) | (y == 0) | (x == 0)
    assert special.sum() >= 16 + 5
    # zeros, axes and NaN: the conventions of libm, bit for bit (mpmath has no signed zero)
    assert_same_bits(got[special], lm[special], "det_atan2 at zeros / axes / NaN")
    err = np.zeros(y.size)
    with mpmath.workprec(MP_BITS):
        for i in np.flatnonzero(~special):
            err[i] = ulp_err(float(got[i]), mpmath.atan2(mpmath.mpf(float(y[i])), mpmath.mpf(float(x[i]))))
    i = int(err.argmax())
    right = ~special & (x > 0)
    print(f"det_atan2 on {(~special).sum()} pairs: max error {err[i]:.4f} ulp at (y, x) = ({y[i]!r}, {x[i]!r}); x > 0 only: {err[right].max():.4f} ulp")
    assert err[i] < 2.0, "2 ulp or more is a finding, not a bound to adopt"
    assert err[i] < ATAN2_ULP_BOUND


def test_rem2pi_is_libm_remainder(oracle):
    L = oracle.lib()
    x = E.rem2pi_args()
    got, ref = np.zeros(x.size), np.zeros(x.size)
    L.orc_rem2pi(dp(x), dp(got), x.size); L.orc_libm_remainder2pi(dp(x), dp(ref), x.size)
    assert np.isnan(ref[np.isinf(x) | np.isnan(x)]).all()
    assert_same_bits(got, ref, "rem2pi vs remainder(x, 2 pi)")
    # the ties themselves, stated independently: x / 2 pi = 0.5 -> n = 0, 1.5 -> n = 2, 2.5 -> n = 2 (to even), so remainder(pi) = pi,
    # remainder(3 pi) = -pi, remainder(5 pi) = pi; a zero result carries the sign of x
    t = np.array([E.K_PI, -E.K_PI, 3 * E.K_PI, -3 * E.K_PI, 2 * E.K_PI, -2 * E.K_PI, 4 * E.K_PI, -4 * E.K_PI, 5 * E.K_PI])
    r = np.zeros(t.size)
    L.orc_rem2pi(dp(t), dp(r), t.size)
    assert_same_bits(r, np.array([E.K_PI, -E.K_PI, -E.K_PI, E.K_PI, 0.0, -0.0, 0.0, -0.0, E.K_PI]), "rem2pi at the ties")


def _inv2x2(L, name, S):
    Si, ok = np.zeros_like(S), np.zeros(S.shape[0], dtype=np.int32)
    getattr(L, name)(dp(S), dp(Si), ok.ctypes.data_as(C.POINTER(C.c_int)), S.shape[0])
    return Si, ok


def test_inv2x2_shared_is_the_oracles_own_sequence(oracle):
    L = oracle.lib()
    S = np.ascontiguousarray(E.inv2x2_cases())
    Si, ok = _inv2x2(L, "orc_inv2x2_shared", S)
    So, oko = _inv2x2(L, "orc_inv2x2_own", S)
    assert np.array_equal(ok, oko)
    assert_same_bits(Si.ravel(), So.ravel(), "slam::inv2x2_lu vs orc::inv2x2_lu")
    nb = len(E.INV2X2_BUILT)
    assert ok[:nb].tolist() == [f for _, f in E.INV2X2_BUILT]
    assert ok[nb:].all()
    assert Si[0].tolist() == [0.75, -0.25, -0.5, 0.5] and Si[6].tolist() == [-1.5, 0.5, 1.0, 0.0]   # worked by hand
    # the pivot tie |S[2]| == |S[0]| takes no swap: the elimination written out in fp64 with row 0 as the pivot row gives these bits,
    # and with the rows exchanged it gives other bits on at least one of the tie cases (so the comparison can tell)
    differs = 0
    for k in range(E.INV2X2_TIES):
        assert abs(S[k, 2]) == abs(S[k, 0])
        assert_same_bits(Si[k], _lu_inverse(S[k], swap=False), f"tie case {k}")
        differs += not np.array_equal(bits(_lu_inverse(S[k], swap=True)), bits(Si[k]))
    assert differs > 0


def _lu_inverse(S, swap):
    """The inverse of a 2x2 by LU with the given row order, solving against the columns of the (permuted) identity, every operation
    rounded to fp64 (Python floats)."""
    a00, a01, a10, a11 = (float(v) for v in ((S[2], S[3], S[0], S[1]) if swap else S))
    l = a10 / a00
    u11 = a11 - l * a01
    out = [0.0] * 4
    for j in range(2):
        r0, r1 = (1.0, 0.0) if (j == 0) != swap else (0.0, 1.0)
        x1 = (r1 - l * r0) / u11
        out[j] = (r0 - a01 * x1) / a00
        out[2 + j] = x1
    return np.array(out)


def test_inv2x2_left_residual_on_spd(oracle):
    """|| Si S - I ||_inf <= 16 u kappa_inf(S) on the random SPD cases, the product and kappa in exact rational arithmetic."""
    L = oracle.lib()
    S = np.ascontiguousarray(E.inv2x2_spd())
    Si, ok = _inv2x2(L, "orc_inv2x2_shared", S)
    assert ok.all()
    u = Fraction(1, 2 ** 53)
    worst = 0.0
    for m, mi in zip(S, Si):
        a, b, c, d = (Fraction(float(v)) for v in m)
        p, q, r, s = (Fraction(float(v)) for v in mi)
        det = a * d - b * c
        ninf = lambda w, x, y, z: max(abs(w) + abs(x), abs(y) + abs(z))
        kappa = ninf(a, b, c, d) * ninf(d, b, c, a) / abs(det)   # the exact inverse is [d, -b; -c, a] / det
        res = ninf(p * a + q * c - 1, p * b + q * d, r * a + s * c, r * b + s * d - 1)
        worst = max(worst, float(res / (u * kappa)))
        assert res <= 16 * u * kappa, (m, mi)
    print(f"inv2x2_lu: worst left residual {worst:.3f} u kappa_inf")


def _assoc_abs_py(d, as_int):
    """|d| as ekf.cpp:91-92 sees it: fabs and a conversion to float, or (abs resolving to ::abs(int)) the value truncated towards zero
    to an int first, saturated at +-(2^31 - 1), NaN -> 0."""
    if not as_int:
        return np.float32(abs(d))
    if math.isnan(d):
        return np.float32(0.0)
    return np.float32(abs(int(max(-2147483647.0, min(2147483647.0, d)))))


def test_assoc_abs_both_modes(oracle):
    L = oracle.lib()
    d, m = E.assoc_abs_args()
    got = np.zeros(d.size, dtype=np.float32)
    L.orc_assoc_abs(dp(d), m.ctypes.data_as(C.POINTER(C.c_int)), got.ctypes.data_as(C.POINTER(C.c_float)), d.size)
    with np.errstate(over="ignore"):
        ref = np.array([_assoc_abs_py(float(v), int(k)) for v, k in zip(d, m)], dtype=np.float32)
    assert np.isnan(ref).sum() == 1   # NaN with as_int = 0 only
    assert_same_bits(got.astype(np.float64), ref.astype(np.float64), "assoc_abs")
    pick = lambda v, k: float(got[np.flatnonzero((d == v) & (m == k))[0]])
    assert pick(0.999, 1) == 0.0 and pick(-1.5, 1) == 1.0 and pick(2147483646.5, 1) == 2147483648.0 and pick(-1e300, 1) == 2147483648.0
    assert pick(1e300, 0) == np.inf and pick(-np.inf, 1) == 2147483648.0


def test_double_to_float_and_noise_array_forms(oracle):
    """The two array exports the GPU test leans on: (float) against numpy's conversion at the ties, and orc_noise_pairs against the scalar
    orc_noise_pair (itself tied to the Random123 known answers by tests/test_oracle.py)."""
    L = oracle.lib()
    a = E.arith_args()[0]
    f = np.zeros(a.size, dtype=np.float32)
    L.orc_double_to_float(dp(a), f.ctypes.data_as(C.POINTER(C.c_float)), a.size)
    with np.errstate(over="ignore", under="ignore"):
        assert np.array_equal(f.view(np.uint32), a.astype(np.float32).view(np.uint32))
    one = lambda v: float(f[np.flatnonzero(a == v)[0]])
    assert one(1.0 + 2.0 ** -24) == 1.0 and one(1.0 + 3 * 2.0 ** -24) == 1.0 + 2.0 ** -22          # ties to even
    assert one(2.0 ** 128 - 2.0 ** 103) == np.inf and one(float(np.nextafter(2.0 ** 128 - 2.0 ** 103, 0.0))) == E.FLT_MAX
    assert one(2.0 ** -150) == 0.0 and one(float(np.nextafter(2.0 ** -150, 1.0))) == 2.0 ** -149 and one(1.5 * 2.0 ** -149) == 2.0 ** -148
    seed, inst, t, p = E.philox_counters()
    out = np.zeros(2 * seed.size)
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    L.orc_noise_pairs(seed.ctypes.data_as(u64), inst.ctypes.data_as(u64), t.ctypes.data_as(u32), p.ctypes.data_as(u32), dp(out), seed.size)
    out = out.reshape(-1, 2)
    assert np.all((out >= 0) & (out < 1))
    nz = np.zeros(2)
    for i in range(seed.size):
        L.orc_noise_pair(int(seed[i]), int(inst[i]), int(t[i]), int(p[i]), dp(nz))
        assert out[i, 0] == nz[0] and out[i, 1] == nz[1], i
    assert np.unique(out[:, 0]).size == seed.size   # every counter its own stream: no word of (seed, inst, t, p) is dropped


def test_sincos_domain_ends_where_the_header_says(oracle):
    """Nothing is claimed about accuracy beyond 2^20 pi/2 (fn = rint(x 2/pi) > 2^20), and the header's limit is within a factor four of
    where the accuracy does end.  Measured here:
      * the ladder 1.65e6 * 2^k reads 0.221, 0.289, 0.362 ulp at 1.65e6, 3.3e6, 6.6e6 and 1.07e9 ulp at 1.32e7 and every element after it
        below 1e9: the 1 ulp bound is missed by far more than a factor 1e3 within three doublings of the limit.  The smallest element
        itself is still accurate, so no assertion is made on it alone: pio2_1 = 0x3FF921FB54400000 has 31 significant bits and
        pio2_2 = 0x3DD0B4611A600000 has 32, so fn * pio2_1 stays exact up to fn < 2^22 (|x| < 6.59e6) and fn * pio2_2 up to
        fn < 2^53 / (pio2_2's significand) ~ 4.02e6 (|x| < 6.31e6);
      * past that, where fn * pio2_2 rounds (odd fn in 4.03e6 .. 2^22), the arguments next to fn * pi/2 are the first to go: the rounding
        of the product (~1e-20) is not small beside a reduced argument of 1e-10 or less."""
    L = oracle.lib()
    lad = E.sincos_ladder()
    assert lad[0] == 1.65e6 and lad[0] > E.SINCOS_DOMAIN and lad[-1] <= 1e18
    lad = lad[lad < 1e9]
    es, ec, s, c = sincos_errs(L, lad)
    el = np.maximum(es, ec)
    print("det_sincos beyond the domain, max(sin, cos) error in ulp:", ", ".join(f"{x:.3g}: {e:.3g}" for x, e in zip(lad, el)))
    assert el.max() > 1e3 * SINCOS_ULP_BOUND
    assert np.all(el[lad > 2.0 ** 23 * (np.pi / 2)] > 1e3 * SINCOS_ULP_BOUND)   # every element from 1.32e7 on
    k = np.arange(4030001, 2 ** 22, 2 * 409)   # 201 odd multiples of pi/2 where fn * pio2_2 rounds, each with its two neighbours
    hard = np.array([v for q in k for v in E.ulp_neighbours(float(int(q) * E.PI_Q / 2), 1)])
    assert hard.min() > E.SINCOS_DOMAIN and hard.max() < 2.0 ** 22 * (np.pi / 2)
    es, ec, s, c = sincos_errs(L, hard)
    eh = np.maximum(es, ec)
    print(f"next to k pi/2, odd k in 4.03e6 .. 2^22: max error {eh.max():.3g} ulp; over 1 ulp: {np.mean(eh > 1):.3f} of the points")
    assert eh.max() > 1e3 * SINCOS_ULP_BOUND and np.all(eh > SINCOS_ULP_BOUND)   # measured: 6.7e7 ulp, every point over 1 ulp
    # finite garbage, never a trap: every element up to 1e18 (where the quadrant's conversion to an integer is still defined)
    b = E.sincos_beyond()
    sb, cb = np.zeros(b.size), np.zeros(b.size)
    L.orc_det_sincos(dp(b), dp(sb), dp(cb), b.size)
    fin = np.isfinite(b)
    assert np.isfinite(sb[fin]).all() and np.isfinite(cb[fin]).all() and np.isnan(sb[~fin]).all() and np.isnan(cb[~fin]).all()
