"""Device build vs host build of the shared fp64 math (slam_math.h, slam_rng.h) and of the UKF kernels' own wrappers (tsincos, yaw_of in
ukf_kernel.h), bit for bit, on EVERY element of the edge sets of tests/math_edges.py: one slam_math_probe2 launch per function.  The
host side is the oracle's exports, which tests/test_math_edges_cpu.py ties to mpmath / glibc on the same sets.  Equal means equal bit
patterns, so equal signs of zero; where the host gives NaN the device gives NaN (payloads are not compared)."""
import ctypes as C

import numpy as np
import pytest

import math_edges as E

pytestmark = pytest.mark.gpu

_dp = C.POINTER(C.c_double)
SINCOS, ATAN2, REM2PI, ARITH, INV2X2, ASSOC_ABS, TSINCOS, YAW_OF, NOISE_PAIR = range(9)   # MathProbeOp, csrc/ukf_kernel.h


def dp(a):
    return a.ctypes.data_as(_dp)


@pytest.fixture(scope="module")
def probe():
    from live_ekf_slam_amd import _lib
    lib = _lib.lib()  # raises if the HIP extension is missing: there is no fallback path to test instead

    def run(op, nout, *inputs):
        ins = [np.ascontiguousarray(v, dtype=np.float64) for v in inputs]
        n = ins[0].size
        assert all(v.size == n for v in ins)
        out = np.full((n, nout), 12345.0)   # a value no op produces here: an item the kernel skipped shows
        ptr = [dp(v) for v in ins] + [None] * (4 - len(ins))
        _lib.check(lib.slam_math_probe2(op, *ptr, dp(out), nout, n, 0))
        return out
    return run


def assert_same_bits(got, ref, what):
    got, ref = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(ref, dtype=np.float64)
    assert got.shape == ref.shape
    got, ref = got.ravel(), ref.ravel()
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), f"{what}: NaN in other places than the host's"
    bad = np.flatnonzero((got.view(np.uint64) != ref.view(np.uint64)) & ~nan)
    assert bad.size == 0, (f"{what}: {bad.size} of {ref.size} differ, first at {bad[0]}: device {got[bad[0]]!r} "
                           f"({int(got.view(np.uint64)[bad[0]]):#018x}) vs host {ref[bad[0]]!r} ({int(ref.view(np.uint64)[bad[0]]):#018x})")


def host_sincos(L, x):
    s, c = np.zeros(x.size), np.zeros(x.size)
    L.orc_det_sincos(dp(x), dp(s), dp(c), x.size)
    return s, c


def host_to_float(L, x):
    f = np.zeros(x.size, dtype=np.float32)
    L.orc_double_to_float(dp(x), f.ctypes.data_as(C.POINTER(C.c_float)), x.size)
    return f.astype(np.float64)


def test_sincos(probe, oracle):
    """In the domain, and beyond it up to 1e18 and at +-inf / NaN: no accuracy there, but the same operations, so the same bits."""
    x = np.concatenate([E.sincos_in_domain(), E.sincos_beyond()])
    out = probe(SINCOS, 2, x)
    s, c = host_sincos(oracle.lib(), x)
    assert_same_bits(out[:, 0], s, "sin"); assert_same_bits(out[:, 1], c, "cos")


def test_atan2(probe, oracle):
    y, x = E.atan2_pairs()
    ref = np.zeros(y.size)
    oracle.lib().orc_det_atan2(dp(y), dp(x), dp(ref), y.size)
    assert_same_bits(probe(ATAN2, 1, y, x)[:, 0], ref, "det_atan2")


def test_rem2pi_and_library_remainder(probe, oracle):
    """rem2pi (shared text, library remainder above 4 pi) against the host's rem2pi; wrap2pi (the device library's remainder alone)
    against glibc's, on all of rem2pi_args(): 1e15, 1e300, +-inf and NaN too."""
    L = oracle.lib()
    x = E.rem2pi_args()
    r, lm = np.zeros(x.size), np.zeros(x.size)
    L.orc_rem2pi(dp(x), dp(r), x.size); L.orc_libm_remainder2pi(dp(x), dp(lm), x.size)
    out = probe(REM2PI, 2, x)
    assert_same_bits(out[:, 0], r, "rem2pi"); assert_same_bits(out[:, 1], lm, "wrap2pi vs glibc remainder")


def test_sqrt_division_float_conversion(probe, oracle):
    a, b = E.arith_args()
    out = probe(ARITH, 3, a, b)
    with np.errstate(all="ignore"):
        assert_same_bits(out[:, 0], np.sqrt(a), "sqrt"); assert_same_bits(out[:, 1], a / b, "division")
    assert_same_bits(out[:, 2], host_to_float(oracle.lib(), a), "(float)")


def test_inv2x2(probe, oracle):
    S = np.ascontiguousarray(E.inv2x2_cases())
    Si, ok = np.zeros_like(S), np.zeros(S.shape[0], dtype=np.int32)
    oracle.lib().orc_inv2x2_shared(dp(S), dp(Si), ok.ctypes.data_as(C.POINTER(C.c_int)), S.shape[0])
    out = probe(INV2X2, 5, S[:, 0], S[:, 1], S[:, 2], S[:, 3])
    assert_same_bits(out[:, :4], Si, "inv2x2_lu")
    assert np.array_equal(out[:, 4], ok.astype(np.float64))


def test_assoc_abs(probe, oracle):
    d, m = E.assoc_abs_args()
    ref = np.zeros(d.size, dtype=np.float32)
    oracle.lib().orc_assoc_abs(dp(d), m.ctypes.data_as(C.POINTER(C.c_int)), ref.ctypes.data_as(C.POINTER(C.c_float)), d.size)
    assert_same_bits(probe(ASSOC_ABS, 1, d, m.astype(np.float64))[:, 0], ref.astype(np.float64), "assoc_abs")


def test_tsincos(probe, oracle):
    """The UKF kernels' sin / cos of a float: det_sincos of the widened argument, rounded to float when float_trig is set."""
    L = oracle.lib()
    a, ft = E.tsincos_args()
    assert np.array_equal(a, a.astype(np.float32).astype(np.float64))
    s, c = host_sincos(L, a)
    s, c = np.where(ft != 0, host_to_float(L, s), s), np.where(ft != 0, host_to_float(L, c), c)
    out = probe(TSINCOS, 2, a, ft)
    assert_same_bits(out[:, 0], s, "tsincos sin"); assert_same_bits(out[:, 1], c, "tsincos cos")


def test_yaw_of(probe, oracle):
    """The UKF kernels' heading of (cos, sin): (float) remainder(det_atan2(s, c), 2 pi), built from the host's exports."""
    L = oracle.lib()
    c, s = E.yaw_pairs()
    at, rem = np.zeros(c.size), np.zeros(c.size)
    L.orc_det_atan2(dp(s), dp(c), dp(at), c.size); L.orc_libm_remainder2pi(dp(at), dp(rem), c.size)
    assert_same_bits(probe(YAW_OF, 1, c, s)[:, 0], host_to_float(L, rem), "yaw_of")


def test_noise_pair(probe, oracle):
    """Philox4x32-10 -> two 53-bit uniforms on ALL of philox_counters(): instance ids and seeds with the high word set, t and p at 2^32 - 1."""
    seed, inst, t, p = E.philox_counters()
    ref = np.zeros(2 * seed.size)
    u64, u32 = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    oracle.lib().orc_noise_pairs(seed.ctypes.data_as(u64), inst.ctypes.data_as(u64), t.ctypes.data_as(u32), p.ctypes.data_as(u32), dp(ref), seed.size)
    assert_same_bits(probe(NOISE_PAIR, 2, *E.pack_counters(seed, inst, t, p)), ref.reshape(-1, 2), "noise_pair")
