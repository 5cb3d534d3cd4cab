"""The edge sets of the fp64 functions the kernels share with the CPU oracle (live_ekf_slam_amd/csrc/slam_math.h, slam_rng.h): one
definition, imported by tests/test_math_edges_cpu.py (host build vs mpmath / libm) and tests/test_math_edges_gpu.py (device vs host, bit
for bit).  Every generator is deterministic and returns float64 arrays (or the integer types named) of a few thousand elements.
"""
from fractions import Fraction

import numpy as np

# filter.h:42 `#define pi 3.14159265358979323846`: slam::kPi, and kTwoPi = 2 * kPi exactly
K_PI = 3.14159265358979323846
K_TWO_PI = 2 * K_PI
# pi to 70 digits as an exact rational: float(Fraction) rounds correctly, so k * PI_Q / 2 gives THE double nearest k pi/2
PI_Q = Fraction(31415926535897932384626433832795028841971693993751058209749445923078164, 10 ** 70)
PIO4_THRESHOLD = 0.78539816339744827900        # the literal of det_sincos: at or below it no reduction is made
SINCOS_DOMAIN = 2.0 ** 20 * (np.pi / 2) - 1    # |x| of every element of sincos_in_domain() (fn = rint(x 2/pi) < 2^20 below it)
DBL_MIN = 2.2250738585072014e-308
FLT_MAX = float(np.finfo(np.float32).max)


def ulp_neighbours(x, k):
    """x and the doubles up to k ulp either side of it, ascending."""
    x = float(x)
    lo, hi = [x], [x]
    for _ in range(k):
        lo.append(float(np.nextafter(lo[-1], -np.inf)))
        hi.append(float(np.nextafter(hi[-1], np.inf)))
    return lo[:0:-1] + hi


def _both_signs(v):
    v = np.asarray(v, dtype=np.float64)
    return np.concatenate([v, -v])


SINCOS_K = list(range(1, 200)) + [1000, 4096, 65535, 65536, 100000, 636619, 1048575]


def sincos_hard():
    """The points of sincos_in_domain() that are built, not drawn: next to k pi/2 (the Cody-Waite reduction cancels), next to
    (2k+1) pi/4 (rint(x 2/pi) ties), the no-reduction threshold, zeros, subnormals and tiny arguments."""
    v = []
    for k in SINCOS_K:
        v += ulp_neighbours(float(k * PI_Q / 2), 2)
    for k in range(50):
        v += ulp_neighbours(float((2 * k + 1) * PI_Q / 4), 1)
    v += ulp_neighbours(PIO4_THRESHOLD, 1)
    v += [0.0, 5e-324, 1e-310, DBL_MIN, 1e-8]
    return _both_signs(v)   # (-0.0 included)


def sincos_float_valued():
    """4 000 arguments (double)(float)a in +-400: what the UKF kernels' tsincos passes."""
    rng = np.random.default_rng(20240)
    return rng.uniform(-400, 400, 4000).astype(np.float32).astype(np.float64)


def sincos_in_domain():
    rng = np.random.default_rng(20241)
    x = np.concatenate([sincos_hard(), sincos_float_valued(), rng.uniform(-1.6e6, 1.6e6, 4000)])
    assert np.all(np.abs(x) <= SINCOS_DOMAIN)
    return x


def sincos_ladder():
    """1.65e6 * 2^k while <= 1e18: the first element is the smallest argument the tests place outside the domain."""
    v, x = [], 1.65e6
    while x <= 1e18:
        v.append(x)
        x *= 2.0
    return np.array(v)


def sincos_beyond():
    """Finite elements have |x| <= 1e18 < 2^62 pi/2: the quadrant's conversion to an integer is still defined there."""
    rng = np.random.default_rng(20242)
    return np.concatenate([sincos_ladder(), rng.uniform(-1e18, 1e18, 50), [np.inf, -np.inf, np.nan]])


ATAN_RATIOS = [0.4375, 0.6875, 1.1875, 2.4375, 1.0, 2.0 ** 66, 1e17, 1e-17, 1e300, 1e-300]   # det_atan's breakpoints first


def atan2_pairs():
    """(y, x).  The built part first, then 4 000 uniform pairs in +-10."""
    ys, xs = [], []
    for r0 in ATAN_RATIOS:
        for r in ulp_neighbours(r0, 1):
            for x in (1.0, 3.0, 1e-200, 1e200):   # y / x exact, inexact, y near underflow, y near overflow
                y = r * x
                if not np.isfinite(y):             # 1e300 * 1e200: det_atan2 is for finite arguments
                    continue
                for sy in (1.0, -1.0):
                    for sx in (1.0, -1.0):
                        ys.append(sy * y); xs.append(sx * x)
    for y, x in [(1e-310, 1e300), (1e300, 1e-310), (5e-324, 5e-324), (1e308, 1e308), (1e308, -1e-308), (-1e-308, -1e308),
                 (-8.964202309202546, -3.353288908687162)]:   # (the last: the worst pair an earlier random search found, 1.163 ulp)
        ys.append(y); xs.append(x)
    for y in (0.0, -0.0, 1.0, -1.0):               # zeros and axes (and the four diagonals)
        for x in (0.0, -0.0, 1.0, -1.0):
            ys.append(y); xs.append(x)
    for y, x in [(np.nan, 1.0), (1.0, np.nan), (np.nan, np.nan), (np.nan, 0.0), (-0.0, np.nan)]:
        ys.append(y); xs.append(x)
    rng = np.random.default_rng(20243)
    u = rng.uniform(-10, 10, (4000, 2))
    return np.concatenate([ys, u[:, 0]]), np.concatenate([xs, u[:, 1]])


def rem2pi_args():
    v = []
    for k in range(6):                             # 0, pi, 2 pi, 3 pi, 4 pi, 5 pi: k * kPi is exact for every k here
        v += ulp_neighbours(k * K_PI, 1)
    v = list(_both_signs(v))
    v += [5e-324, 300.0, -300.0, 1e6, -1e6, 1e15, 1e300, np.inf, -np.inf, np.nan]
    return np.array(v)


def arith_args():
    """(a, b) for sqrt(a), a / b and (float)a: the cross product of two short lists."""
    f32_tie_inf = float(2.0 ** 128 - 2.0 ** 103)   # half way between FLT_MAX and 2^128: rounds to +inf (ties to even)
    a = [0.0, 5e-324, 1e-310, float(np.nextafter(DBL_MIN, 0.0)), DBL_MIN, 3 * DBL_MIN, 1e-300, 1.0, 2.0, 3.0, 1e300, 1e308, 1.7976931348623157e308,
         1.0 + 2.0 ** -24, 1.0 + 3 * 2.0 ** -24, 1.0 + 2.0 ** -24 + 2.0 ** -52, 1.0 + 2.0 ** -23,
         float(np.nextafter(f32_tie_inf, 0.0)), f32_tie_inf, float(np.nextafter(f32_tie_inf, np.inf)), FLT_MAX,
         2.0 ** -126, float(np.nextafter(2.0 ** -126, 0.0)), 1e-40, 1e-45, 2.0 ** -149, 1.5 * 2.0 ** -149, 2.5 * 2.0 ** -149, 2.0 ** -150,
         float(np.nextafter(2.0 ** -150, 1.0)), float(np.nextafter(2.0 ** -150, 0.0)), 7e-46]
    b = [0.0, 5e-324, 1e-310, DBL_MIN, 1e-300, 0.1, 0.5, 1.0, 2.0, 3.0, 7.0, 1e10, 1e300, 1.7976931348623157e308]
    A, B = np.meshgrid(_both_signs(a), _both_signs(b), indexing="ij")
    return A.ravel().copy(), B.ravel().copy()


INV2X2_BUILT = [   # (S row-major, the ok flag: 0 exactly when a pivot is zero, before or after the elimination)
    ([2.0, 1.0, 2.0, 3.0], 1), ([2.0, 1.0, -2.0, 3.0], 1), ([-2.0, 1.0, 2.0, 3.0], 1),   # |S[2]| == |S[0]|: the pivot tie, no swap
    ([3.0, 0.1, -3.0, 0.7], 1), ([0.3, 0.1, 0.3, 0.7], 1), ([0.7, 0.3, -0.7, 0.1], 1),    # the same with entries that round
    ([0.0, 1.0, 2.0, 3.0], 1), ([0.0, 1.0, 2.0, 0.0], 1),                                 # S[0] = 0, S[2] != 0: swap
    ([1.0, 2.0, 2.0, 4.0], 0), ([4.0, 2.0, 2.0, 1.0], 0),                                 # exactly singular: u11 = 0
    ([0.0, 0.0, 0.0, 0.0], 0), ([0.0, 1.0, 0.0, 1.0], 0),
    ([1.0, 1.0, 1.0, 1.0 + 2.0 ** -52], 1), ([1e8, 0.0, 0.0, 1e-8], 1),                   # condition number ~1e16
    ([np.nan, 1.0, 2.0, 3.0], 1), ([1.0, np.nan, 2.0, 3.0], 1), ([1.0, 2.0, np.nan, 3.0], 1), ([1.0, 2.0, 3.0, np.nan], 1),
]
INV2X2_TIES = 6   # the leading cases of INV2X2_BUILT with |S[2]| == |S[0]|


def inv2x2_spd():
    """1 000 random symmetric positive definite matrices of the innovation covariance's scale: diagonal 1e-4 .. 1e2, |correlation| < 0.95."""
    rng = np.random.default_rng(20244)
    a, d = (10.0 ** rng.uniform(-4, 2, 1000) for _ in range(2))
    b = rng.uniform(-0.95, 0.95, 1000) * np.sqrt(a * d)
    return np.stack([a, b, b, d], axis=1)


def inv2x2_cases():
    """[n][4] row-major; the built cases first, then inv2x2_spd()."""
    return np.concatenate([np.array([m for m, _ in INV2X2_BUILT]), inv2x2_spd()])


def assoc_abs_args():
    """(d, as_int): every value with both modes."""
    v = _both_signs([0.0, 0.5, 0.999, 1.0, 1.5, 2147483646.5, 2147483647.0, 2147483647.5, 2147483648.0, 1e300, np.inf])
    v = np.concatenate([v, [np.nan]])
    return np.concatenate([v, v]), np.concatenate([np.zeros(v.size, np.int32), np.ones(v.size, np.int32)])


def philox_counters():
    """(seed, inst: uint64; t, p: uint32).  The built corners, then a 2 000-element grid."""
    M64, M32 = 2 ** 64 - 1, 2 ** 32 - 1
    rows = [(0, 0, 0, 0), (0, 2 ** 32, 0, 0), (0, 2 ** 32 + 1, 7, 3), (12345, M64, 7, 3), (12345, 5, M32, 0), (12345, 5, 0, M32),
            (0xDEADBEEF00000001, 5, 7, 3), (2 ** 63, 2 ** 63, 2 ** 31, 2 ** 31), (M64, M64, M32, M32), (2 ** 48, 2 ** 48, 1, 1),
            (2 ** 48 - 1, 2 ** 48 - 1, 65535, 65536)]
    for seed in (0, 12345, 2 ** 32, 0x9E3779B97F4A7C15, M64):
        for inst in (0, 1, 2, 63, 5000, M32, 2 ** 32, 2 ** 40 + 17, 2 ** 63, M64 - 1):
            for t in (0, 1, 2, 999, 65536, 2 ** 31, M32 - 1, M32):
                for p in (0, 1, 2, 51, M32):
                    rows.append((seed, inst, t, p))
    r = np.array(list(dict.fromkeys(rows)), dtype=object)   # (a corner that is also a grid point once)
    return (np.array(r[:, 0], dtype=np.uint64), np.array(r[:, 1], dtype=np.uint64), np.array(r[:, 2], dtype=np.uint32),
            np.array(r[:, 3], dtype=np.uint32))


def pack_counters(seed, inst, t, p):
    """The four doubles slam_math_probe2's noise_pair op takes (include/slam_batch.h): integers below 2^48, exact in a double."""
    m48 = np.uint64(2 ** 48 - 1)
    s48 = np.uint64(48)
    a = (seed & m48).astype(np.float64)
    b = (inst & m48).astype(np.float64)
    c = ((seed >> s48) + np.uint64(65536) * t.astype(np.uint64)).astype(np.float64)
    d = ((inst >> s48) + np.uint64(65536) * p.astype(np.uint64)).astype(np.float64)
    return a, b, c, d


def yaw_pairs():
    """(c, s) for the UKF kernels' yaw_of: unit vectors at the rem2pi tie angles, then atan2_pairs() as (x, y)."""
    th = rem2pi_args()
    th = th[np.isfinite(th) & (np.abs(th) <= 1e6)]
    y, x = atan2_pairs()
    return np.concatenate([np.cos(th), x]), np.concatenate([np.sin(th), y])


def tsincos_args():
    """(a, float_trig): float-valued arguments (the built points of sincos_in_domain() rounded to float, and its float-valued
    draws), each with float_trig 0 and 1."""
    with np.errstate(under="ignore"):
        a = np.concatenate([sincos_hard().astype(np.float32).astype(np.float64), sincos_float_valued()])
    return np.concatenate([a, a]), np.concatenate([np.zeros(a.size), np.ones(a.size)])
