"""ctypes binding of oracle/libslam_oracle.so — the CPU checker.  TEST INFRASTRUCTURE ONLY.

May be imported only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg.
"""
import ctypes as C
import os
import subprocess
import numpy as np

from live_ekf_slam_amd.config import SlamConfig, default_config  # noqa: F401  (struct layout is shared)

HERE = os.path.dirname(os.path.abspath(__file__))
MATH_LIBM, MATH_DET = 0, 1
MODE_FAST, MODE_DENSE = 0, 1
STORAGE_F32 = 2   # OR into `mode`: x_t / P_t rounded to float whenever stored (SLAM_F32)
_lib = None

_dp = C.POINTER(C.c_double)
_fp = C.POINTER(C.c_float)
_ip = C.POINTER(C.c_int)


def build(force=False):
    so = os.path.join(HERE, "libslam_oracle.so")
    subprocess.check_call(["make", "-C", HERE, "-s"] + (["-B"] if force else []))   # no-op when up to date
    return so


def lib():
    global _lib
    if _lib is None:
        L = C.CDLL(build())
        L.orc_version.restype = C.c_char_p
        L.orc_ekf_create.restype = C.c_void_p
        L.orc_ekf_create.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int, C.c_int]
        L.orc_ekf_destroy.argtypes = [C.c_void_p]
        L.orc_ekf_init.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.orc_ekf_update.argtypes = [C.c_void_p, C.c_float, C.c_float, _fp, C.c_int]
        L.orc_ekf_get.argtypes = [C.c_void_p, _dp, _dp, _ip, _ip, _ip]
        L.orc_ekf_set.argtypes = [C.c_void_p, _dp, _dp, C.c_int, _ip, C.c_int]
        L.orc_sim_create.restype = C.c_void_p
        L.orc_sim_create.argtypes = [C.POINTER(SlamConfig), _dp, C.c_int, C.c_int]
        L.orc_sim_destroy.argtypes = [C.c_void_p]
        L.orc_sim_reset.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_double]
        L.orc_sim_step_draws.argtypes = [C.c_void_p, C.c_float, C.c_float, _dp, _dp, _fp, _dp, _ip]
        L.orc_sim_step_philox.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_uint64, C.c_uint64, C.c_uint32, _dp, _fp, _ip]
        L.orc_average_error.restype = C.c_double
        L.orc_average_error.argtypes = [_dp, _dp, _dp, _dp, C.c_int, C.c_int]
        L.orc_run_ekf_batch.restype = C.c_double
        L.orc_run_ekf_batch.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int, C.c_int, _dp, C.c_int, _fp, C.c_int,
                                        C.c_uint64, C.c_int64, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _ip, _dp,
                                        C.POINTER(C.c_int64), _dp]
        L.orc_ukf_create.restype = C.c_void_p
        L.orc_ukf_create.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int]
        L.orc_ukf_destroy.argtypes = [C.c_void_p]
        L.orc_ukf_init.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.orc_ukf_update.argtypes = [C.c_void_p, C.c_float, C.c_float, _fp, C.c_int]
        L.orc_ukf_get.argtypes = [C.c_void_p, _dp, _dp, _ip, _ip, _ip, _ip]
        L.orc_ukf_sqrt_probe.argtypes = [_dp, C.c_int, C.c_double, _dp, C.c_int]
        L.orc_ukf_jacobi_pair.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        L.orc_ukf_jacobi_pair.restype = None
        L.orc_ukf_set_loc_map.argtypes = [C.c_void_p, _dp, C.c_int]
        L.orc_run_ukf_batch.restype = C.c_double
        L.orc_run_ukf_batch.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int, _dp, C.c_int, _fp, C.c_int, C.c_uint64,
                                        C.c_int64, C.c_int, C.c_int, _dp, _dp, _ip, _ip, _dp, _ip, _dp, _dp]
        L.orc_pgs_create.restype = C.c_void_p
        L.orc_pgs_create.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int, C.c_int, C.c_int]
        L.orc_pgs_destroy.argtypes = [C.c_void_p]
        L.orc_pgs_init.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float]
        L.orc_pgs_set_secondary.argtypes = [C.c_void_p, _dp]
        L.orc_pgs_update.argtypes = [C.c_void_p, C.c_float, C.c_float, _fp, C.c_int]
        L.orc_pgs_solve.argtypes = [C.c_void_p, C.c_int, _ip, _dp]
        L.orc_pgs_adopt.argtypes = [C.c_void_p]
        L.orc_pgs_get.argtypes = [C.c_void_p, C.c_int, _dp, _dp, _ip, _ip, _ip]
        L.orc_pgs_connections.argtypes = [C.c_void_p, _ip, C.c_int]
        L.orc_pgs_cost.restype = C.c_double
        L.orc_pgs_cost.argtypes = [C.c_void_p, C.c_int]
        L.orc_pgs_residuals.argtypes = [C.c_void_p, _dp, _dp, _dp, C.c_int]
        L.orc_pgs_gradient.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp]
        L.orc_pgs_retract.argtypes = [C.c_void_p, _dp, _dp, _dp, _dp, _dp, _dp]
        L.orc_pgs_jacobian.argtypes = [C.c_void_p, _dp, _dp, _ip, _ip, _dp, C.c_int, _dp, C.c_int, _ip]
        L.orc_pgs_step.argtypes = [C.c_void_p, _dp, _dp, C.c_double, C.c_int, _dp, _dp]
        L.orc_run_pgs_batch.restype = C.c_double
        L.orc_run_pgs_batch.argtypes = [C.POINTER(SlamConfig), C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _fp, C.c_int,
                                        C.c_uint64, C.c_int64, C.c_int, C.c_int, _dp, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp,
                                        _fp, _ip]
        L.orc_run_pgs_batch_ex.restype = C.c_double
        L.orc_run_pgs_batch_ex.argtypes = L.orc_run_pgs_batch.argtypes + [C.c_int, _ip]
        L.orc_philox.argtypes = [C.c_uint32] * 6 + [C.POINTER(C.c_uint32)]
        L.orc_noise_pair.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32, _dp]
        for name in ("orc_det_sincos", "orc_libm_sincos"):
            getattr(L, name).argtypes = [_dp, _dp, _dp, C.c_int]
        for name in ("orc_det_atan2", "orc_libm_atan2"):
            getattr(L, name).argtypes = [_dp, _dp, _dp, C.c_int]
        L.orc_libm_remainder2pi.argtypes = [_dp, _dp, C.c_int]
        L.orc_rem2pi.argtypes = [_dp, _dp, C.c_int]
        for name in ("orc_inv2x2_shared", "orc_inv2x2_own"):
            getattr(L, name).argtypes = [_dp, _dp, _ip, C.c_int]
        L.orc_assoc_abs.argtypes = [_dp, _ip, _fp, C.c_int]
        L.orc_noise_pairs.argtypes = [C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32), _dp, C.c_int]
        L.orc_double_to_float.argtypes = [_dp, _fp, C.c_int]
        for name in ("orc_det_sincos", "orc_libm_sincos", "orc_det_atan2", "orc_libm_atan2", "orc_libm_remainder2pi", "orc_rem2pi", "orc_inv2x2_shared",
                     "orc_inv2x2_own", "orc_assoc_abs", "orc_noise_pairs", "orc_double_to_float"):
            getattr(L, name).restype = None
        _lib = L
    return _lib


def _d(a):
    return a.ctypes.data_as(_dp)


def _f(a):
    return a.ctypes.data_as(_fp)


def _i(a):
    return a.ctypes.data_as(_ip)


class OracleEKF:
    """One reference-equivalent EKF-SLAM filter instance (ekf.cpp)."""

    def __init__(self, cfg=None, L_max=50, math=MATH_DET, mode=MODE_FAST):
        self.cfg = cfg or default_config()
        self.L_max = L_max
        self.h = lib().orc_ekf_create(C.byref(self.cfg), L_max, math, mode)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_ekf_destroy(self.h)
            self.h = None

    def init(self, x0=0.0, y0=0.0, yaw0=0.0):
        lib().orc_ekf_init(self.h, x0, y0, yaw0)

    def update(self, fwd, ang, meas):
        """meas: array-like [k][3] float32 (id, r, b)."""
        m = np.ascontiguousarray(np.asarray(meas, dtype=np.float32).reshape(-1, 3))
        return lib().orc_ekf_update(self.h, float(np.float32(fwd)), float(np.float32(ang)), _f(m), m.shape[0])

    def state(self):
        nmax = 3 + 2 * self.L_max
        x = np.zeros(nmax); P = np.zeros(nmax * nmax); ids = np.zeros(self.L_max, dtype=np.int32)
        M = C.c_int(0); ts = C.c_int(0)
        lib().orc_ekf_get(self.h, _d(x), _d(P), C.byref(M), _i(ids), C.byref(ts))
        n = 3 + 2 * M.value
        return dict(x=x[:n].copy(), P=P[:n * n].reshape(n, n).copy(), M=M.value, ids=ids[:M.value].copy(), timestep=ts.value)

    def set_state(self, x, P, ids, timestep=0):
        x = np.ascontiguousarray(x, dtype=np.float64); P = np.ascontiguousarray(P, dtype=np.float64)
        ids = np.ascontiguousarray(ids, dtype=np.int32)
        lib().orc_ekf_set(self.h, _d(x), _d(P), len(ids), _i(ids), timestep)


class OracleSim:
    """The reference's measurement generator get_cmd (sim_node.py:209-250)."""

    def __init__(self, map_xy, cfg=None, math=MATH_DET):
        self.cfg = cfg or default_config()
        self.map = np.ascontiguousarray(map_xy, dtype=np.float64)
        self.L = self.map.shape[0]
        self.h = lib().orc_sim_create(C.byref(self.cfg), _d(self.map), self.L, math)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_sim_destroy(self.h)
            self.h = None

    def step_draws(self, fwd, ang, draws):
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        truth = np.zeros(3); meas = np.zeros((self.L, 3), dtype=np.float32); meas64 = np.zeros((self.L, 3))
        k = C.c_int(0)
        used = lib().orc_sim_step_draws(self.h, float(np.float32(fwd)), float(np.float32(ang)), _d(draws), _d(truth), _f(meas), _d(meas64), C.byref(k))
        return truth, meas[:k.value], meas64[:k.value], used

    def step_philox(self, fwd, ang, seed, inst, t):
        truth = np.zeros(3); meas = np.zeros((self.L, 3), dtype=np.float32); k = C.c_int(0)
        lib().orc_sim_step_philox(self.h, float(np.float32(fwd)), float(np.float32(ang)), seed, inst, t, _d(truth), _f(meas), C.byref(k))
        return truth, meas[:k.value]


def average_error(est_x, est_y, true_x, true_y, math=MATH_LIBM):
    a = [np.ascontiguousarray(v, dtype=np.float64) for v in (est_x, est_y, true_x, true_y)]
    return lib().orc_average_error(_d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), len(a[0]), math)


def run_ekf_batch(map_xy, cmds, B, L_max, seed=2025, inst0=0, cfg=None, math=MATH_DET, mode=MODE_FAST, nthreads=1, want_P=True, vision=None):
    """Lockstep sim + EKF for instances inst0..inst0+B-1 over all commands. Returns dict of numpy outputs."""
    cfg = cfg or default_config()
    map_xy = np.ascontiguousarray(map_xy, dtype=np.float64); cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    L, T, nmax = map_xy.shape[0], cmds.shape[0], 3 + 2 * L_max
    x = np.zeros((B, nmax)); P = np.zeros((B, nmax * nmax)) if want_P else None
    M = np.zeros(B, dtype=np.int32); ids = np.zeros((B, L_max), dtype=np.int32)
    err = np.zeros(B); flags = np.zeros(B, dtype=np.int32); truth = np.zeros((B, 3)); ktot = C.c_int64(0)
    if vision is not None:
        vision = np.ascontiguousarray(vision, dtype=np.float64).reshape(T, 3)
    secs = lib().orc_run_ekf_batch(C.byref(cfg), L_max, math, mode, _d(map_xy), L, _f(cmds), T, seed, inst0, B, nthreads,
                                   _d(x), _d(P) if want_P else None, _i(M), _i(ids), _d(err), _i(flags), _d(truth), C.byref(ktot),
                                   _d(vision) if vision is not None else None)
    return dict(x=x, P=P, M=M, ids=ids, avg_err=err, flags=flags, truth=truth, seconds=secs, k_total=ktot.value)


class OracleUKF:
    """One reference-equivalent UKF-SLAM filter instance (ukf.cpp)."""

    def __init__(self, cfg=None, L_max=20, math=MATH_DET):
        self.cfg = cfg or default_config()
        self.L_max = L_max
        self.h = lib().orc_ukf_create(C.byref(self.cfg), L_max, math)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_ukf_destroy(self.h)
            self.h = None

    def set_loc_map(self, map_xy):
        """Switch to UKF_LOC (localisation against the known map)."""
        m = np.ascontiguousarray(map_xy, dtype=np.float64)
        lib().orc_ukf_set_loc_map(self.h, _d(m), m.shape[0])

    def init(self, x0=0.0, y0=0.0, yaw0=0.0):
        lib().orc_ukf_init(self.h, x0, y0, yaw0)

    def update(self, fwd, ang, meas):
        m = np.ascontiguousarray(np.asarray(meas, dtype=np.float32).reshape(-1, 3))
        return lib().orc_ukf_update(self.h, float(np.float32(fwd)), float(np.float32(ang)), _f(m), m.shape[0])

    def state(self):
        nmax = 4 + 2 * self.L_max
        x = np.zeros(nmax); P = np.zeros(nmax * nmax); ids = np.zeros(self.L_max, dtype=np.int32)
        M = C.c_int(0); ts = C.c_int(0); sw = C.c_int(0)
        lib().orc_ukf_get(self.h, _d(x), _d(P), C.byref(M), _i(ids), C.byref(ts), C.byref(sw))
        n = 4 + 2 * M.value
        return dict(x=x[:n].copy(), P=P[:n * n].reshape(n, n).copy(), M=M.value, ids=ids[:M.value].copy(),
                    timestep=ts.value, sweeps=sw.value)


def ukf_jacobi_pair(k, t, n):
    """Pair k of round t of a Jacobi sweep at state size n (the schedule the oracle and the kernels share)."""
    p = C.c_int(0); q = C.c_int(0)
    lib().orc_ukf_jacobi_pair(k, t, n, C.byref(p), C.byref(q))
    return p.value, q.value


def ukf_sqrt_probe(P, scale, pad=None):
    """pad: None = the rule of a handle just large enough for n (sizes n = 2 mod 4 are padded to n + 2 up to n = 104, the LDS classes);
    False = the unpadded circle schedule the HBM-streamed class (L_max > 50) runs at every n it holds; True = padded."""
    P = np.ascontiguousarray(P, dtype=np.float64); n = P.shape[0]
    out = np.zeros((n, n))
    sweeps = lib().orc_ukf_sqrt_probe(_d(P), n, float(scale), _d(out), -1 if pad is None else int(bool(pad)))
    return out, sweeps


def run_ukf_batch(map_xy, cmds, B, L_max, seed=2025, inst0=0, cfg=None, math=MATH_DET, nthreads=1, want_P=True, vision=None, loc=False,
                  ref_order=False):
    """ref_order: reference-order arithmetic (no fused multiply-adds, textbook Jacobi parameters, cold start every step) instead
    of the device-order evaluation the GPU parity tests compare with bit for bit."""
    cfg = (cfg or default_config()).copy()
    cfg.reserved[0] = 1 if loc else 0
    cfg.reserved[1] = 1 if ref_order else 0
    map_xy = np.ascontiguousarray(map_xy, dtype=np.float64); cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    L, T, nmax = map_xy.shape[0], cmds.shape[0], 4 + 2 * L_max
    x = np.zeros((B, nmax)); P = np.zeros((B, nmax * nmax)) if want_P else None
    M = np.zeros(B, dtype=np.int32); ids = np.zeros((B, L_max), dtype=np.int32)
    err = np.zeros(B); flags = np.zeros(B, dtype=np.int32); truth = np.zeros((B, 3))
    if vision is not None:
        vision = np.ascontiguousarray(vision, dtype=np.float64).reshape(T, 3)
    secs = lib().orc_run_ukf_batch(C.byref(cfg), L_max, math, _d(map_xy), L, _f(cmds), T, seed, inst0, B, nthreads,
                                   _d(x), _d(P) if want_P else None, _i(M), _i(ids), _d(err), _i(flags), _d(truth),
                                   _d(vision) if vision is not None else None)
    return dict(x=x, P=P, M=M, ids=ids, avg_err=err, flags=flags, truth=truth, seconds=secs)


LIN_SCHUR, LIN_DENSE, LIN_SEG = 0, 1, 2   # LIN_SEG | (SL << 8): poses eliminated segment by segment (SL = 0: 32), what the GPU path does


class OraclePoseGraph:
    """One reference-equivalent PoseGraph instance (pose_graph.cpp, GTSAM implementation)."""

    def __init__(self, cfg=None, N_max=1000, L_max=20, KP=8, math=MATH_DET):
        self.cfg = cfg or default_config()
        self.N_max, self.L_max, self.KP = N_max, L_max, KP
        self.h = lib().orc_pgs_create(C.byref(self.cfg), N_max, L_max, KP, math)

    def __del__(self):
        if getattr(self, "h", None):
            lib().orc_pgs_destroy(self.h)
            self.h = None

    def init(self, x0=0.0, y0=0.0, yaw0=0.0):
        lib().orc_pgs_init(self.h, x0, y0, yaw0)

    def updateNaiveVehPoseEstimate(self, state_vector):
        sv = np.ascontiguousarray(state_vector, dtype=np.float64)
        lib().orc_pgs_set_secondary(self.h, _d(sv))

    def update(self, fwd, ang, meas):
        m = np.ascontiguousarray(np.asarray(meas, dtype=np.float32).reshape(-1, 3))
        return lib().orc_pgs_update(self.h, float(np.float32(fwd)), float(np.float32(ang)), _f(m), m.shape[0])

    def solve(self, lin_mode=LIN_SCHUR):
        io = np.zeros(3, dtype=np.int32); do = np.zeros(3)
        lib().orc_pgs_solve(self.h, lin_mode, _i(io), _d(do))
        return dict(iterations=int(io[0]), trials=int(io[1]), flags=int(io[2]), err_init=do[0], err_final=do[1], lam=do[2])

    def adopt(self):
        lib().orc_pgs_adopt(self.h)

    def values(self, which=1):
        poses = np.zeros((self.N_max, 3)); lms = np.zeros((self.L_max, 2)); ids = np.zeros(self.L_max, dtype=np.int32)
        ts = C.c_int(0); M = C.c_int(0)
        lib().orc_pgs_get(self.h, which, _d(poses), _d(lms), C.byref(ts), C.byref(M), _i(ids))
        return dict(poses=poses[:ts.value + 1].copy(), landmarks=lms[:M.value].copy(), timestep=ts.value, M=M.value, ids=ids[:M.value].copy())

    def connections(self):
        cap = self.N_max * self.KP
        c = np.zeros((cap, 2), dtype=np.int32)
        n = lib().orc_pgs_connections(self.h, _i(c), cap)
        return c[:n].copy()

    def cost(self, which=1):
        return lib().orc_pgs_cost(self.h, which)

    def residuals(self, poses, lms):
        poses = np.ascontiguousarray(poses, dtype=np.float64); lms = np.ascontiguousarray(lms, dtype=np.float64).reshape(-1)
        lms = lms if lms.size else np.zeros(2)
        cap = 3 + 3 * self.N_max + 2 * self.N_max * self.KP
        out = np.zeros(cap)
        n = lib().orc_pgs_residuals(self.h, _d(poses), _d(lms), _d(out), cap)
        return out[:n].copy()

    def gradient(self, poses, lms):
        poses = np.ascontiguousarray(poses, dtype=np.float64); lms = np.ascontiguousarray(lms, dtype=np.float64).reshape(-1, 2)
        gp = np.zeros_like(poses); gl = np.zeros((max(len(lms), 1), 2))
        lib().orc_pgs_gradient(self.h, _d(poses), _d(lms if lms.size else np.zeros(2)), _d(gp), _d(gl))
        return gp, gl[:len(lms)]

    def retract(self, poses, lms, dp, dl):
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (poses, lms, dp, dl)]
        a = [v if v.size else np.zeros(2) for v in a]
        pn = np.zeros_like(a[0]); ln = np.zeros_like(a[1])
        lib().orc_pgs_retract(self.h, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(pn), _d(ln))
        return pn, ln

    def jacobian(self, poses, lms):
        """Whitened sparse Jacobian of the factors at (poses [N][3], lms [M][2]) and the residual: (rows, cols, vals, e).  Rows in the
        order of residuals(), columns 3 i + a for pose i and 3 N + 2 j + b for landmark j; 0.5 |e|^2 = cost, J^T e = gradient(), and
        J^T J is the matrix linearize() forms (GTSAM's Between / Prior Jacobians).  Entries are listed per factor block, zeros included."""
        poses = np.ascontiguousarray(poses, dtype=np.float64); lms = np.ascontiguousarray(lms, dtype=np.float64).reshape(-1)
        lms = lms if lms.size else np.zeros(2)
        N = poses.shape[0]
        cap_rows = 3 * N + 2 * N * self.KP
        cap_nnz = 3 + 12 * N + 10 * N * self.KP
        rows = np.zeros(cap_nnz, dtype=np.int32); cols = np.zeros(cap_nnz, dtype=np.int32); vals = np.zeros(cap_nnz)
        e = np.zeros(cap_rows); nnz = C.c_int(0)
        m = lib().orc_pgs_jacobian(self.h, _d(poses), _d(lms), _i(rows), _i(cols), _d(vals), cap_nnz, _d(e), cap_rows, C.byref(nnz))
        assert m <= cap_rows and nnz.value <= cap_nnz
        k = nnz.value
        return rows[:k].copy(), cols[:k].copy(), vals[:k].copy(), e[:m].copy()

    def step(self, poses, lms, lam, lin_mode=LIN_SCHUR):
        """The damped step (J^T J + lam I) delta = -J^T e at (poses, lms) with the elimination of lin_mode: (ok, dp [N][3], dl [M][2])."""
        poses = np.ascontiguousarray(poses, dtype=np.float64); lms = np.ascontiguousarray(lms, dtype=np.float64).reshape(-1, 2)
        M = lms.shape[0]
        dp = np.zeros_like(poses); dl = np.zeros((max(M, 1), 2))
        ok = lib().orc_pgs_step(self.h, _d(poses), _d(lms if M else np.zeros(2)), float(lam), int(lin_mode), _d(dp), _d(dl))
        return bool(ok), dp, dl[:M].copy()


def run_pgs_batch(map_xy, cmds, B, L_max, KP=8, seed=2025, inst0=0, cfg=None, math=MATH_DET, lin_mode=LIN_SCHUR, nthreads=1,
                  want_streams=False, every_iteration=False):
    """Simulator + NaiveFilter secondary + graph building + one LM solve per instance (T commands -> T+1 poses).
    every_iteration: solve_graph_every_iteration (params.yaml:64) - solve + `initial_estimate = result` after every update; `iterations` /
    `trials` are then the sums over the T ticks, `tick_counts` [B][T][2] those of every tick, `seconds` covers all T solves."""
    cfg = cfg or default_config()
    map_xy = np.ascontiguousarray(map_xy, dtype=np.float64); cmds = np.ascontiguousarray(cmds, dtype=np.float32)
    L, T = map_xy.shape[0], cmds.shape[0]
    N = T + 1
    pose_init = np.zeros((B, N, 3)); pose_res = np.zeros((B, N, 3)); lm_res = np.zeros((B, L_max, 2))
    M = np.zeros(B, dtype=np.int32); ids = np.zeros((B, L_max), dtype=np.int32)
    istats = np.zeros((B, 3), dtype=np.int32); dstats = np.zeros((B, 3)); avg_err = np.zeros((B, 2)); truth = np.zeros((B, T, 2))
    meas = np.zeros((B, T, KP, 3), dtype=np.float32) if want_streams else None
    cnt = np.zeros((B, T), dtype=np.int32) if want_streams else None
    tick = np.zeros((B, T, 2), dtype=np.int32) if every_iteration else None
    secs = lib().orc_run_pgs_batch_ex(C.byref(cfg), L_max, KP, math, lin_mode, _d(map_xy), L, _f(cmds), T, seed, inst0, B, nthreads,
                                      _d(pose_init), _d(pose_res), _d(lm_res), _i(M), _i(ids), _i(istats), _d(dstats), _d(avg_err),
                                      _d(truth), _f(meas) if want_streams else None, _i(cnt) if want_streams else None,
                                      1 if every_iteration else 0, _i(tick) if every_iteration else None)
    return dict(tick_counts=tick, pose_init=pose_init, pose_res=pose_res, lm_res=lm_res, M=M, ids=ids, iterations=istats[:, 0], trials=istats[:, 1],
                flags=istats[:, 2], err_init=dstats[:, 0], err_final=dstats[:, 1], lam=dstats[:, 2], avg_err_init=avg_err[:, 0],
                avg_err_result=avg_err[:, 1], truth_xy=truth, meas=meas, cnt=cnt, seconds=secs)
