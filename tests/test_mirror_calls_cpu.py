"""What reaches the library from the Python mirror, call by call, without a GPU and without libslam_hip.so.

`_lib.lib` is replaced by a recorder that checks every call against `_lib.SIGNATURES` (argument count, `from_param` of every argument),
records one row per argument and then writes the argument's POSITION into element 0 of everything a typed pointer points at.  Because of
that write, what a method returns shows for every array which argument slot it was passed in: two int32 outputs swapped in a call change
the outcome although their types agree.  The expected trace, tests/mirror_calls_expected.json, is data this project's own code produced;
`python tests/test_mirror_calls_cpu.py --record` rewrites it, pytest only compares.

Rows: None = NULL; ints and floats by value; a c_void_p by its integer, or {"host": type, "first": element 0} where it is the cast of a
host array; byref(struct) / an array of rows as the hex of its bytes, SenseLog / FixLog as one 0 / 1 per pointer field; a typed pointer as
{"ptr": type, "first": element 0} (first = None: an empty array, which is neither read nor written).
"""
import ctypes as C
import json
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
if os.path.dirname(HERE) not in sys.path:
    sys.path.insert(0, os.path.dirname(HERE))
EXPECTED = os.path.join(HERE, "mirror_calls_expected.json")

_ELEM = {C.c_double: "f64", C.c_float: "f32", C.c_int32: "i32", C.c_uint64: "u64", C.c_void_p: "ptr"}
# what the recorder returns where 0 would make the mirror allocate nothing: the state dimension, large enough for the M that
# slam_get_state's slot 4 becomes (UKF: 4 + 2 * 4)
RETURNS = {"slam_state_dim_max": 12}
# symbols the package names that are not driven, each with its reason (at most five)
LEFT_OUT = {"slam_debug_read_prof_raw": "not in SIGNATURES: step_stamps binds it on the loaded library itself",
            "slam_last_error": "read by _lib.check only after a non-zero return, which the recorder never gives"}


def _behind(arg):
    """byref(x) -> x; a pointer or an array is its own target."""
    return getattr(arg, "_obj", arg)


def _slot(o):
    """The object whose element 0 a typed-pointer argument points at, or None where that is an empty numpy array."""
    arr = getattr(o, "_arr", None)
    return None if arr is not None and arr.size == 0 else o


def _get0(o):
    v = o.value if isinstance(o, C._SimpleCData) else o[0]
    return v.item() if hasattr(v, "item") else v


def _set0(o, v):
    if isinstance(o, C._SimpleCData):
        o.value = v
    else:
        o[0] = v


def _host_source(a):
    """The numpy-backed pointer a c_void_p was cast from (C.cast keeps it alive in _objects), or None."""
    for o in (getattr(a, "_objects", None) or {}).values():
        if hasattr(o, "_arr"):
            return o
    return None


def _pointer_fields(struct):
    return [n for n, t in struct._fields_ if isinstance(t, type) and issubclass(t, C._Pointer)]


def _describe(t, a):
    if a is None:
        return None
    t.from_param(a)                                     # what ctypes would refuse fails here too
    if t is C.c_char_p:
        return "buffer" if isinstance(a, C.Array) else os.path.basename(a.decode())
    if t is C.c_void_p:
        src = _host_source(a)
        if src is not None:
            s = _slot(src)
            return {"host": _ELEM[type(src)._type_], "first": None if s is None else _get0(s)}
        return a.value if isinstance(a, C.c_void_p) else int(a)
    if issubclass(t, C._Pointer):
        e, o = t._type_, _behind(a)
        if issubclass(e, C.Structure):
            pf = _pointer_fields(e)
            return {"fields": [int(bool(getattr(o, n))) for n in pf]} if pf else bytes(o).hex()
        s = _slot(o)
        return {"ptr": _ELEM[e], "first": None if s is None else _get0(s)}
    return float(a) if t in (C.c_float, C.c_double) else int(a)


def _write(t, a, pos):
    if a is None:
        return
    if t is C.c_void_p:
        src = _host_source(a)
        if src is not None and _slot(src) is not None:
            _set0(src, pos)
    elif isinstance(t, type) and issubclass(t, C._Pointer):
        e, o = t._type_, _behind(a)
        if issubclass(e, C.Structure):
            for n in _pointer_fields(e):
                if getattr(o, n):
                    getattr(o, n)[0] = pos
        elif _slot(o) is not None:
            _set0(_slot(o), pos)


class Recorder:
    """Stands in for the loaded library: every attribute is a function that records its arguments and returns 0."""

    def __init__(self, signatures):
        self._signatures = signatures
        self.calls = []

    def __getattr__(self, name):
        assert name in self._signatures, f"{name} is not in _lib.SIGNATURES"
        argtypes = self._signatures[name][1]

        def fn(*args):
            assert len(args) == len(argtypes), f"{name}: {len(args)} arguments, {len(argtypes)} declared"
            self.calls.append([name, [_describe(t, a) for t, a in zip(argtypes, args)]])
            for pos, (t, a) in enumerate(zip(argtypes, args)):
                _write(t, a, pos)
            return RETURNS.get(name, 0)
        return fn


class NoLib:
    def __getattr__(self, name):
        raise AssertionError(f"the library was reached ({name}) although the arguments were malformed")


class NoCall:
    """For the settings a method converts inside the call expression itself: the symbol may be looked up, the call must not happen."""

    def __getattr__(self, name):
        def fn(*args):
            raise AssertionError(f"the library was called ({name}) although the arguments were malformed")
        return fn


def _summary(x):
    if x is None or isinstance(x, (bool, int, float, str)):
        return x
    if isinstance(x, np.generic):
        return x.item()
    if isinstance(x, np.ndarray):
        return {"shape": list(x.shape), "dtype": str(x.dtype), "first": x.flat[0].item() if x.size else None}
    if isinstance(x, dict):
        return {k: _summary(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return [_summary(v) for v in x]
    return {"class": type(x).__name__, **{k: _summary(v) for k, v in vars(x).items()}}


# batch, L_max, k_stride, ticks: the smallest that keep every buffer non-empty; L_max is 4, not 2, because slam_get_state's M sits in
# argument slot 4 and publishState pairs that many ids with that many landmarks
B, L, KS, T = 2, 4, 2, 2


class Drive:
    """Runs the mirror's public surface under the recorder and collects one entry per call."""

    def __init__(self, rec):
        self.rec, self.n, self.entries, self.made = rec, 0, [], []

    def A(self, *shape, dt=np.float64):
        """A fresh array of zeros whose element 0 is a number no other array of the run holds."""
        self.n += 1
        a = np.zeros(shape, dtype=dt)
        if a.size:
            a.flat[0] = self.n
        return a

    def F(self, *shape):
        return self.A(*shape, dt=np.float32)

    def I(self, *shape):
        return self.A(*shape, dt=np.int32)

    def D(self):
        """A fresh (fake) device pointer."""
        self.n += 1
        return 0x10000 + 0x100 * self.n

    def log(self, each=False, T=T):
        return (self.F(T, B, 2) if each else self.F(T, 2)), self.F(T, B, KS, 3), self.I(T, B)

    def call(self, label, obj, fn, *a, **k):
        start = len(self.rec.calls)
        ret = fn(*a, **k)
        self.entries.append(dict(call=label, rows=self.rec.calls[start:], timestep=getattr(obj, "timestep", None), ret=_summary(ret)))

    def m(self, obj, name, variant, *a, **k):
        self.call(f"{type(obj).__name__}.{name}[{variant}]", obj, getattr(obj, name), *a, **k)

    def hook(self, fn, variant, *a, **k):
        self.call(f"{fn.__name__}[{variant}]", None, fn, *a, **k)


def _params_yaml(tmp):
    path = os.path.join(tmp, "params.yaml")
    with open(path, "w") as fh:
        fh.write("num_iterations: 4\npose_graph:\n  implementation: \"gtsam\"\n  solve_graph_every_iteration: false\n")
    return path


def drive_filters(d, S, tmp):
    from live_ekf_slam_amd import config as K
    from live_ekf_slam_amd import filters as Fm
    e = S.BatchedEKF(B, L); d.made.append(e)
    d.m(e, "readParams", "none")
    d.m(e, "readParams", "struct, recreate", S.default_config())
    d.m(e, "readParams", "path", _params_yaml(tmp))
    d.m(e, "readParams", "dict", dict(process_noise=dict(cov=dict(V_00=0.5)), init_pose=dict(x=1.0)))
    d.m(e, "init", "scalars", 0.5, 0.25, 0.125)
    d.m(e, "init", "each", d.F(B, 3))
    d.m(e, "init", "each, truth0", d.F(B, 3), truth0=d.A(B, 3))
    d.m(e, "init", "scalars, truth0", 0.5, 0.25, 0.125, truth0=d.A(B, 3))
    d.m(e, "set_stream", "", d.D())
    d.m(e, "set_seed", "", 11)
    d.m(e, "set_instance_offset", "", 3)
    d.m(e, "set_vision", "", 3.0, -1.5, 1.5)
    d.m(e, "set_map", "shared", d.A(3, 2))
    d.m(e, "set_map", "each", d.A(B, 3, 2))
    d.m(e, "set_map", "each, counts", d.A(B, 3, 2), counts=[3, 2])
    d.m(e, "set_map", "list", [d.A(3, 2), d.A(2, 2)])
    d.m(e, "set_noise", "none", None)
    d.m(e, "set_noise", "rows", K.noise_rows(e.cfg, B, V_00=[0.5, 0.25]))
    d.m(e, "set_noise", "sequence", [K.noise_from_config(e.cfg)] * B)
    d.m(e, "update", "one command, flat message", S.Command(0.5, 0.25), [1.0, 2.0, 0.5])
    d.m(e, "update", "one command, empty message", (0.5, 0.25), [])
    d.m(e, "update", "each", d.F(B, 2), d.F(B, KS, 3), d.I(B))
    d.m(e, "update_dev", "", (0.5, 0.25), d.D(), d.D(), KS)
    d.m(e, "update_dev_each", "", d.D(), d.D(), d.D(), KS)
    d.m(e, "update_sim", "one", d.F(2))
    d.m(e, "update_sim", "each", d.F(B, 2))
    d.m(e, "run_sim", "shared", d.F(T, 2))
    d.m(e, "run_sim", "each", d.F(T, B, 2))
    d.m(e, "get_state", "", 1)
    d.m(e, "getStateVector", "", 0)
    d.m(e, "publishState", "", 1)
    d.m(e, "track_instance", "", 1)
    d.m(e, "save_state", "", os.path.join(tmp, "state.bin"))
    d.m(e, "load_state", "", os.path.join(tmp, "state.bin"))
    for name in ("poses", "landmark_counts", "truth", "status", "error_stats", "algorithmic_bytes", "reset_counters_async", "consistency",
                 "last_consistency_work", "last_monitor_work", "nav_state", "nav_estimates", "last_nav_work", "sync", "last_innovation_work",
                 "last_gate_work", "last_associate_work", "last_joint_work", "last_map_work", "last_merge_work", "last_fix_work", "map_track",
                 "map_track_reset"):
        d.m(e, name, "")
    d.m(e, "last_meas", "", KS)
    d.m(e, "set_run_chunk", "", 5)
    d.m(e, "set_debug_flags", "", 32)
    d.m(e, "set_lazy_steps", "", 4)
    d.m(e, "set_nav_timing", "", True)
    for name in ("k_histogram", "sweep_stats", "traffic_counters"):
        d.m(e, name, "", reset=True)
    d.m(e, "kernel_info", "", multi_step=False)
    # monitor
    mc = K.default_monitor_config(); mc.full_every = 3
    d.m(e, "monitor_now", "cfg none")
    d.m(e, "monitor_now", "cfg dict", cfg=dict(nees_lo=0.5, full_every=2))
    d.m(e, "monitor_now", "cfg struct", cfg=mc)
    d.m(e, "monitor_run", "shared", d.F(T, 2))
    d.m(e, "monitor_run", "each, series, source", d.F(T, B, 2), source=K.MONITOR_EACH, series=True, cfg=dict(nees_hi=7.0))
    d.m(e, "monitor_run", "nav, series", T=T, series=True, cfg=mc)
    d.m(e, "monitor_run", "nav, source", T=T, source=K.MONITOR_NAV)
    d.m(e, "monitor_run", "T = 0, series", d.F(0, 2), series=True)
    d.m(e, "monitor_run", "nav, T = 0", T=0, series=True)
    # controller
    nc = K.default_nav_config(); nc.method = K.NAV_DIRECT
    d.m(e, "set_path", "nav none", d.A(3, 2))
    d.m(e, "set_path", "nav dict", d.A(3, 2), nav=dict(dt=0.5, control=K.NAV_TIGHT))
    d.m(e, "set_path", "nav struct", d.A(3, 2), nav=nc)
    d.m(e, "set_paths", "list", [d.A(3, 2), d.A(2, 2)])
    d.m(e, "set_paths", "array, counts", d.A(B, 3, 2), counts=[3, 1], nav=dict(dt=0.25))
    d.m(e, "run_nav", "", T)
    d.m(e, "run_nav", "return_cmds", T, return_cmds=True)
    d.m(e, "run_nav", "T = 0, return_cmds", 0, return_cmds=True)
    # innovation
    ic = K.default_innovation_config(); ic.nis_lo = 0.125
    d.m(e, "innovation", "one, cfg none", (0.5, 0.25), d.F(B, KS, 3), d.I(B))
    d.m(e, "innovation", "each, no det, cfg dict", d.F(B, 2), d.F(B, KS, 3), d.I(B), det=False, cfg=dict(nis_hi=6.0))
    d.m(e, "innovation", "cfg struct", (0.5, 0.25), d.F(B, KS, 3), d.I(B), cfg=ic)
    d.m(e, "innovation_run", "shared", d.F(T, 2))
    d.m(e, "innovation_run", "each, series", d.F(T, B, 2), series=True, cfg=ic)
    d.m(e, "innovation_run", "nav, series", T=T, series=True)
    d.m(e, "innovation_run", "log, series", d.F(T, 2), None, d.F(T, B, KS, 3), d.I(T, B), series=True, cfg=dict(nis_lo=0.25))
    d.m(e, "innovation_run", "log, T given", d.F(T, 2), T, d.F(T, B, KS, 3), d.I(T, B))
    d.m(e, "innovation_run", "T = 0, series", d.F(0, 2), series=True)
    d.m(e, "innovation_run", "log, T = 0, series", d.F(0, 2), None, d.F(0, B, KS, 3), d.I(0, B), series=True)
    # gate
    gc = K.default_gate_config(); gc.gate = 5.0
    d.m(e, "gate", "one, cfg none", (0.5, 0.25), d.F(B, KS, 3), d.I(B))
    d.m(e, "gate", "each, no det, cfg dict", d.F(B, 2), d.F(B, KS, 3), d.I(B), det=False, cfg=dict(gate=4.0, nis_hi=6.0))
    d.m(e, "gate", "cfg struct", (0.5, 0.25), d.F(B, KS, 3), d.I(B), cfg=gc)
    d.m(e, "gate_dev", "host command", d.F(2), d.D(), d.D(), KS, d.D(), d.D())
    d.m(e, "gate_dev", "device commands, no det", d.D(), d.D(), d.D(), KS, d.D(), d.D(), det=False, cfg=gc)
    d.m(e, "step_gated", "one", d.F(2), d.F(B, KS, 3), d.I(B))
    d.m(e, "step_gated", "each, no stats", d.F(B, 2), d.F(B, KS, 3), d.I(B), stats=False, cfg=gc)
    d.m(e, "step_gated_dev", "host command", d.F(2), d.D(), d.D(), KS)
    d.m(e, "step_gated_dev", "device commands, no stats", d.D(), d.D(), d.D(), KS, stats=False, cfg=dict(gate=3.0))
    d.m(e, "gate_run", "shared", *d.log())
    d.m(e, "gate_run", "each, series", *d.log(each=True), series=True, cfg=gc)
    d.m(e, "gate_run", "T = 0, series", *d.log(T=0), series=True, cfg=dict(gate=3.0))
    # association
    ac = K.default_assoc_config(); ac.gate_new = 20.0
    d.m(e, "associate", "one, cfg none", (0.5, 0.25), d.F(B, KS, 3), d.I(B))
    d.m(e, "associate", "each, no det, cfg dict", d.F(B, 2), d.F(B, KS, 3), d.I(B), det=False, cfg=dict(gate_match=4.0))
    d.m(e, "associate", "cfg struct", (0.5, 0.25), d.F(B, KS, 3), d.I(B), cfg=ac)
    d.m(e, "associate_dev", "host command", d.F(2), d.D(), d.D(), KS, d.D(), d.D())
    d.m(e, "associate_dev", "device commands, no det", d.D(), d.D(), d.D(), KS, d.D(), d.D(), det=False, cfg=ac)
    d.m(e, "step_associated", "one", d.F(2), d.F(B, KS, 3), d.I(B))
    d.m(e, "step_associated", "each, no stats", d.F(B, 2), d.F(B, KS, 3), d.I(B), stats=False, cfg=ac)
    d.m(e, "step_associated_dev", "host command", d.F(2), d.D(), d.D(), KS)
    d.m(e, "step_associated_dev", "device commands, no stats", d.D(), d.D(), d.D(), KS, stats=False, cfg=dict(gate_new=9.0))
    d.m(e, "associate_run", "shared", *d.log())
    d.m(e, "associate_run", "each, series", *d.log(each=True), series=True, cfg=ac)
    d.m(e, "associate_run", "T = 0, series", *d.log(T=0), series=True)
    # joint association
    jc = K.default_joint_config(); jc.max_nodes = 9
    jd = dict(max_nodes=7, gate_joint=[float(i + 1) for i in range(16)])
    d.m(e, "associate_joint", "one, cfg none", (0.5, 0.25), d.F(B, KS, 3), d.I(B))
    d.m(e, "associate_joint", "each, no det, cfg dict", d.F(B, 2), d.F(B, KS, 3), d.I(B), det=False, cfg=jd)
    d.m(e, "associate_joint", "cfg struct", (0.5, 0.25), d.F(B, KS, 3), d.I(B), cfg=jc)
    d.m(e, "associate_joint", "device message, host command", d.F(2), d.D(), (d.D(), KS), dev_out=(d.D(), d.D()))
    d.m(e, "associate_joint", "device message, device commands, no det", d.D(), d.D(), (d.D(), KS), det=False, cfg=jc, dev_out=(d.D(), d.D()))
    d.m(e, "step_associated_joint", "one", d.F(2), d.F(B, KS, 3), d.I(B))
    d.m(e, "step_associated_joint", "each, no stats", d.F(B, 2), d.F(B, KS, 3), d.I(B), stats=False, cfg=jd)
    d.m(e, "step_associated_joint", "device message, host command", d.F(2), d.D(), (d.D(), KS))
    d.m(e, "step_associated_joint", "device message, device commands, no stats", d.D(), d.D(), (d.D(), KS), stats=False, cfg=jc)
    d.m(e, "associate_joint_run", "shared", *d.log())
    d.m(e, "associate_joint_run", "each, series", *d.log(each=True), series=True, cfg=jd)
    d.m(e, "associate_joint_run", "T = 0, series", *d.log(T=0), series=True)
    # map management
    pc = K.default_map_config(); pc.prune_every = 3
    d.m(e, "remove_landmarks", "host", d.I(B, L))
    d.m(e, "remove_landmarks", "host, no stats", d.I(B, L), stats=False)
    d.m(e, "remove_landmarks", "device", d.D())
    d.m(e, "remove_landmarks", "device, no stats", d.D(), stats=False)
    d.m(e, "map_tally", "host", d.F(B, KS, 3), d.I(B))
    d.m(e, "map_tally", "host, flags", d.F(B, KS, 3), d.I(B), assoc_flags=d.I(B), cfg=dict(min_ratio=0.5))
    d.m(e, "map_tally", "device", d.D(), (d.D(), KS))
    d.m(e, "map_tally", "device, flags", d.D(), (d.D(), KS), assoc_flags=d.D(), cfg=pc)
    d.m(e, "map_prune", "cfg none")
    d.m(e, "map_prune", "no stats, cfg dict", stats=False, cfg=dict(min_expected=4, range_shrink=0.5))
    d.m(e, "map_prune", "cfg struct", cfg=pc)
    d.m(e, "step_managed", "one", d.F(2), d.F(B, KS, 3), d.I(B))
    d.m(e, "step_managed", "each, no stats", d.F(B, 2), d.F(B, KS, 3), d.I(B), stats=False, cfg=ac, map_cfg=pc)
    d.m(e, "step_managed", "device message, host command", d.F(2), d.D(), (d.D(), KS), map_cfg=dict(prune_every=2))
    d.m(e, "step_managed", "device message, device commands, no stats", d.D(), d.D(), (d.D(), KS), stats=False, cfg=dict(gate_new=9.0))
    d.m(e, "manage_run", "shared", *d.log())
    d.m(e, "manage_run", "each, series", *d.log(each=True), series=True, cfg=ac, map_cfg=pc)
    d.m(e, "manage_run", "T = 0, series", *d.log(T=0), series=True, map_cfg=dict(prune_every=1))
    # merging
    gm = K.default_merge_config(); gm.merge_every = 3
    d.m(e, "map_duplicates", "cfg none")
    d.m(e, "map_duplicates", "no d2, cfg dict", d2=False, cfg=dict(sigma=0.5))
    d.m(e, "map_duplicates", "device", dev=(d.D(), d.D()), cfg=gm)
    d.m(e, "map_duplicates", "device, no d2", dev=(d.D(), None))
    d.m(e, "merge_landmarks", "host", d.I(B, L))
    d.m(e, "merge_landmarks", "host, no stats", d.I(B, L), stats=False, cfg=gm)
    d.m(e, "merge_landmarks", "device", d.D(), cfg=dict(gate_merge=3.0))
    d.m(e, "merge_landmarks", "device, no stats", d.D(), stats=False)
    d.m(e, "map_merge", "cfg none")
    d.m(e, "map_merge", "no stats, cfg dict", stats=False, cfg=dict(merge_every=2))
    d.m(e, "map_merge", "cfg struct", cfg=gm)
    d.m(e, "manage_merge_run", "shared", *d.log())
    d.m(e, "manage_merge_run", "each, series", *d.log(each=True), series=True, cfg=ac, map_cfg=pc, merge_cfg=gm)
    d.m(e, "manage_merge_run", "T = 0, series", *d.log(T=0), series=True, merge_cfg=dict(sigma=0.25))
    # fixes
    fc = K.default_fix_config(); fc.fix_every = 3
    d.m(e, "fix", "host, cfg none", d.A(B, 5), d.I(B))
    d.m(e, "fix", "host, no stats, cfg dict", d.A(B, 5), d.I(B), stats=False, cfg=dict(gate_pos=4.0))
    d.m(e, "fix", "device, cfg struct", d.D(), d.D(), cfg=fc)
    fs = K.default_fix_sensor_config(sigma_pos=0.5, kinds=3)
    d.m(e, "set_fix_sensor", "none", None)
    d.m(e, "set_fix_sensor", "dict", dict(pos_halfwidth=0.25, kinds=1))
    d.m(e, "set_fix_sensor", "one row", fs)
    d.m(e, "set_fix_sensor", "sequence", [fs, K.default_fix_sensor_config(p_jump=0.5)])
    d.m(e, "set_fix_sensor", "ctypes array", (K.FixSensorConfig * B)(fs, fs))
    d.m(e, "fix_sense", "host")
    d.m(e, "fix_sense", "device", dev=(d.D(), d.D(), d.D()))
    d.m(e, "fix_sense", "device, no jumped", dev=(d.D(), d.D(), None))
    d.m(e, "fix_run", "shared", d.F(T, 2))
    d.m(e, "fix_run", "each, series, source", d.F(T, B, 2), source=K.MONITOR_EACH, series=True, cfg=fc)
    d.m(e, "fix_run", "nav, series", T=T, series=True, cfg=dict(fix_every=1))
    d.m(e, "fix_run", "nav, source", T=T, source=K.MONITOR_NAV)
    d.m(e, "fix_run", "T = 0, series", d.F(0, 2), series=True)
    # sensor model
    sc = K.default_sensor_config(p_miss=0.5, n_clutter=2)
    d.m(e, "set_sensor", "none", None)
    d.m(e, "set_sensor", "dict", dict(p_spike=0.25, shuffle=1))
    d.m(e, "set_sensor", "one row", sc)
    d.m(e, "set_sensor", "sequence", [sc, K.default_sensor_config(erase_ids=1)])
    d.m(e, "set_sensor", "ctypes array", (K.SensorConfig * B)(sc, sc))
    d.m(e, "sense", "one", d.F(2), KS)
    d.m(e, "sense", "each, no labels", d.F(B, 2), KS, labels=False)
    d.m(e, "sense", "no stats", d.F(2), KS, stats=False)
    d.m(e, "sense_dev", "host command", d.F(2), d.D(), d.D(), KS)
    d.m(e, "sense_dev", "device commands, labels", d.D(), d.D(), d.D(), KS, d_origin_ptr=d.D(), d_fault_ptr=d.D())
    d.m(e, "sense_commit", "")
    d.m(e, "sense_commit", "no stats", stats=False)
    cfgs = dict(gate_run_sim=dict(cfg=gc), associate_run_sim=dict(cfg=ac), associate_joint_run_sim=dict(cfg=jd),
                manage_run_sim=dict(cfg=ac, map_cfg=pc), manage_merge_run_sim=dict(cfg=dict(gate_match=4.0), map_cfg=pc, merge_cfg=gm))
    for name, kw in cfgs.items():
        d.m(e, name, "shared", d.F(T, 2))
        d.m(e, name, "each, series, log, source", d.F(T, B, 2), source=K.INNOVATION_EACH, series=True, log=True, k_stride=KS, **kw)
        d.m(e, name, "nav, series, log origin", T=T, series=True, log=("origin",), k_stride=KS)
        d.m(e, name, "nav, source", T=T, source=K.INNOVATION_NAV, k_stride=KS)
        d.m(e, name, "T = 0, series, log", d.F(0, 2), series=True, log=True, k_stride=KS)
    d.m(e, "close", "")
    # the UKF's own methods
    u = S.BatchedUKF(B, L); d.made.append(u)
    d.m(u, "readParams", "none")
    d.m(u, "init", "scalars", 0.5, 0.25, 0.125)
    d.m(u, "predictionStage", "one", d.F(2))
    d.m(u, "predictionStage", "each", d.F(B, 2))
    d.m(u, "updateStage", "empty")
    d.m(u, "updateStage", "message", d.D(), d.D(), KS)
    d.m(u, "set_sqrt_mode", "", "cholesky")
    d.m(u, "sqrt_stats", "", reset=True)
    d.m(u, "sigma_points", "", 1)
    d.m(u, "get_state", "", 1)
    d.m(u, "getStateVector", "", 1)
    d.m(u, "publishState", "", 1)
    d.m(u, "close", "")
    loc = S.BatchedUKFLoc(B); d.made.append(loc)
    d.m(loc, "readParams", "none")
    d.m(loc, "get_state", "", 0)
    d.m(loc, "close", "")
    # the host hooks
    M = 1
    noise = K.noise_from_config(S.default_config())

    def state(M):
        return d.A(3 + 2 * M), d.A(3 + 2 * M, 3 + 2 * M), d.I(M)
    d.hook(Fm.innovation_instance_host, "", *state(M), L, 0, d.F(2), d.F(1, 3), noise)
    d.hook(Fm.innovation_instance_host, "M = 0, no message, cfg", *state(0), L, 1, d.F(2), d.F(0, 3), noise, lm_from_pred=True, f32_storage=True, cfg=ic)
    d.hook(Fm.gate_instance_host, "", *state(M), L, 0, d.F(2), d.F(1, 3), noise)
    d.hook(Fm.gate_instance_host, "M = 0, count, k_stride, cfg", *state(0), L, 1, d.F(2), d.F(1, 3), noise, True, True, gc, count=5, k_stride=3)
    d.hook(Fm.associate_instance_host, "", *state(M), L, 0, d.F(2), d.F(1, 3), noise)
    d.hook(Fm.associate_instance_host, "M = 0, count, k_stride, cfg", *state(0), L, 1, d.F(2), d.F(1, 3), noise, True, True, ac, count=5, k_stride=3)
    d.hook(Fm.associate_joint_instance_host, "", *state(M), L, 0, d.F(2), d.F(1, 3), noise)
    d.hook(Fm.associate_joint_instance_host, "M = 0, count, k_stride, cfg dict", *state(0), L, 1, d.F(2), d.F(1, 3), noise, True, True, jd, count=5,
           k_stride=3)
    d.hook(Fm.associate_joint_instance_host, "cfg struct", *state(M), L, 0, d.F(2), d.F(2, 3), noise, cfg=jc)
    # the map and merge hooks read their landmark count back from an output slot (20 and 15): a state that large keeps the slices whole
    Mh = 20
    d.hook(Fm.map_instance_host, "no message", *state(Mh), Mh)
    d.hook(Fm.map_instance_host, "message, counters, remove, prune", *state(Mh), Mh, status=1, meas=d.F(1, 3), count=1, k_stride=KS, assoc_flag=2,
           vision=(2.0, -1.0, 1.0), f32_storage=True, cfg=pc, seen=d.I(Mh), expected=d.I(Mh), remove=d.I(Mh), prune=True)
    d.hook(Fm.merge_instance_host, "", *state(Mh), Mh)
    d.hook(Fm.merge_instance_host, "counters, partner, decision only", *state(Mh), Mh, status=1, f32_storage=True, cfg=gm, seen=d.I(Mh),
           expected=d.I(Mh), partner=d.I(Mh), fuse=False)
    d.hook(Fm.fix_instance_host, "", *state(M)[:2], L, d.A(5), 3)
    d.hook(Fm.fix_instance_host, "cfg", *state(M)[:2], L, d.A(5), 1, status=1, f32_storage=True, cfg=fc)
    d.hook(Fm.fix_sense_instance_host, "no row", 11, 1, 2, d.A(3))
    d.hook(Fm.fix_sense_instance_host, "row", 11, 1, 2, d.A(3), row=fs)
    d.hook(Fm.sense_instance_host, "no row", 11, 1, 2, d.A(3), d.F(2), d.A(3, 2), S.default_config())
    d.hook(Fm.sense_instance_host, "row, sim_noise", 11, 1, 2, d.A(3), d.F(2), d.A(3, 2), S.default_config(), vision=(2.0, -1.0, 1.0),
           sim_noise=(0.5, 0.25, 0.125, 0.0625), row=sc, k_stride=KS, status=1)
    from live_ekf_slam_amd.scenario import make_scenario_native
    d.hook(make_scenario_native, "", 5, 3, T)


def drive_pose_graph(d, S, tmp):
    from live_ekf_slam_amd import config as K
    from live_ekf_slam_amd import pose_graph as Pm
    g = S.BatchedPoseGraph(B, num_iterations=4, L_max=L, k_per_pose=2); d.made.append(g)
    d.m(g, "readParams", "none")
    d.m(g, "readParams", "struct, recreate", S.default_config())
    d.m(g, "readParams", "path", _params_yaml(tmp))
    d.m(g, "readParams", "dict", dict(num_iterations=4, pose_graph=dict(solve_graph_every_iteration=False)))
    d.m(g, "init", "scalars", 0.5, 0.25, 0.125)
    d.m(g, "init", "each", d.F(B, 3))
    d.m(g, "init", "each, truth0", d.F(B, 3), truth0=d.A(B, 3))
    d.m(g, "set_stream", "", d.D())
    d.m(g, "set_seed", "", 11)
    d.m(g, "set_instance_offset", "", 3)
    d.m(g, "set_map", "shared", d.A(3, 2))
    d.m(g, "set_map", "each", d.A(B, 3, 2))
    d.m(g, "set_map", "each, counts", d.A(B, 3, 2), counts=[3, 2])
    d.m(g, "update", "one command, flat message, no secondary", S.Command(0.5, 0.25), [1.0, 2.0, 0.5])
    g.updateNaiveVehPoseEstimate(d.A(3))
    d.m(g, "update", "each, secondary", d.F(B, 2), d.F(B, KS, 3), d.I(B))
    g.updateNaiveVehPoseEstimate(d.A(B, 5))
    d.m(g, "update", "empty message", (0.5, 0.25), [])
    d.m(g, "update", "the last tick solves", (0.5, 0.25), [])
    d.m(g, "update", "solved: nothing", (0.5, 0.25), [])
    d.m(g, "readParams", "every iteration", solve_graph_every_iteration=True)
    d.m(g, "init", "scalars again", 0.0, 0.0, 0.0)
    d.m(g, "update", "every iteration", (0.5, 0.25), d.F(B, KS, 3), d.I(B))
    d.m(g, "run_sim", "shared", d.F(T, 2))
    d.m(g, "init", "scalars, third", 0.0, 0.0, 0.0)
    d.m(g, "run_sim", "each", d.F(T, B, 2))
    d.m(g, "run_sim_every_iteration", "shared, flat", d.F(2))
    d.m(g, "init", "scalars, fourth", 0.0, 0.0, 0.0)
    d.m(g, "run_sim_every_iteration", "each", d.F(T, B, 2))
    d.m(g, "run_sim_fix", "shared", d.F(1, 2), 2)
    d.m(g, "init", "scalars, fifth", 0.0, 0.0, 0.0)
    d.m(g, "run_sim_fix", "each", d.F(T, B, 2), 1)
    for name in ("last_iter_phases", "solvePoseGraph", "last_solve_timeline", "adopt_result", "stats", "last_marginals_work", "last_solve_work",
                 "last_solve_kernel_ms", "last_solve_paths", "sync"):
        d.m(g, name, "")
    d.m(g, "set_groups", "", 2)
    d.m(g, "set_slots", "", 3)
    d.m(g, "set_profiling", "", True)
    d.m(g, "get_graph", "default", 1)
    d.m(g, "get_graph", "initial", 0, which=0)
    d.m(g, "connections", "", 1)
    d.m(g, "publishState", "", 1)
    d.m(g, "marginals", "default")
    d.m(g, "marginals", "initial", which=0)
    d.m(g, "get_marginals", "", 1)
    d.m(g, "marginalCovariance", "pose", 1, pose=1)
    d.m(g, "marginalCovariance", "landmark", 0, landmark=0)
    d.m(g, "set_robust", "name", "huber", 1.345)
    d.m(g, "set_robust", "number", Pm.LOSS_GEMAN_MCCLURE, 2.0)
    d.call("BatchedPoseGraph.robust[]", g, lambda: g.robust)
    d.m(g, "factor_weights", "default")
    d.m(g, "factor_weights", "initial", which=0)
    d.m(g, "fix", "host", d.A(B, 5), d.I(B))
    d.m(g, "fix", "device", d.D(), d.D(), dev=True)
    d.m(g, "set_fix_robust", "name", "geman_mcclure", 2.5)
    d.call("BatchedPoseGraph.fix_robust[]", g, lambda: g.fix_robust)
    d.m(g, "fixes", "", 1)
    d.m(g, "fix_weights", "default")
    d.m(g, "fix_weights", "initial", which=0)
    fs = K.default_fix_sensor_config(sigma_pos=0.5, kinds=3)
    d.m(g, "set_fix_sensor", "none", None)
    d.m(g, "set_fix_sensor", "dict", dict(pos_halfwidth=0.25, kinds=1))
    d.m(g, "set_fix_sensor", "one row", fs)
    d.m(g, "set_fix_sensor", "sequence", [fs, K.default_fix_sensor_config(p_jump=0.5)])
    d.m(g, "set_fix_sensor", "ctypes array", (K.FixSensorConfig * B)(fs, fs))
    d.m(g, "fix_sense", "host")
    d.m(g, "fix_sense", "device", dev=(d.D(), d.D(), d.D()))
    d.m(g, "fix_sense", "device, no jumped", dev=(d.D(), d.D(), None))
    d.m(g, "error_stats", "result")
    d.m(g, "error_stats", "initial", which=0)
    d.m(g, "close", "")
    d.hook(Pm.fix_factor_host, "", d.A(3), d.A(5), 3)
    d.hook(Pm.fix_factor_host, "loss", d.A(3), d.A(5), 1, loss_kind=Pm.LOSS_HUBER, loss_k=1.5)
    d.hook(Pm.robust_loss_host, "", Pm.LOSS_HUBER, 1.5, 2.5)


def refusals(S):
    """(label, callable) for every ValueError / SlamError the mirror raises before the library: one malformed call each."""
    from live_ekf_slam_amd import config as K
    from live_ekf_slam_amd import filters as Fm
    from live_ekf_slam_amd import pose_graph as Pm
    made = []

    def mk(cls, *a, **k):
        f = cls(*a, **k)
        f.h = C.c_void_p(1)
        f.isInit = True
        made.append(f)
        return f
    e, u, g = mk(S.BatchedEKF, B, L), mk(S.BatchedUKF, B, L), mk(S.BatchedPoseGraph, B, num_iterations=4, L_max=L, k_per_pose=2)
    e0, g0 = S.BatchedEKF(B, L), S.BatchedPoseGraph(B, num_iterations=4, L_max=L, k_per_pose=2)
    cold, gcold = mk(S.BatchedEKF, B, L), mk(S.BatchedPoseGraph, B, 4, L, 2)
    cold.isInit = gcold.isInit = False
    F, I, Z = (lambda *s: np.zeros(s, np.float32)), (lambda *s: np.zeros(s, np.int32)), (lambda *s: np.zeros(s))
    msg = (F(B, KS, 3), I(B))
    badlog = (F(T, 2), F(T, B + 1, KS, 3), I(T, B + 1))
    x5, P5, id1, noise = Z(5), Z(5, 5), I(1), K.noise_from_config(S.default_config())
    cases = [
        ("filter: no handle", lambda: e0.poses()),
        ("filter: no handle, run", lambda: e0.gate_run_sim(T=T)),
        ("filter: update before init", lambda: cold.update((0, 0), [])),
        ("filter: readParams type", lambda: e.readParams(3)),
        ("filter: init rows", lambda: e.init(Z(3, 3))),
        ("filter: init truth0", lambda: e.init(Z(B, 3), truth0=Z(B, 2))),
        ("filter: set_map list with counts", lambda: e.set_map([Z(3, 2)] * B, counts=[3, 3])),
        ("filter: set_map list length", lambda: e.set_map([Z(3, 2)] * 3)),
        ("filter: set_map width", lambda: e.set_map(Z(3, 3))),
        ("filter: set_map batch", lambda: e.set_map(Z(3, 3, 2))),
        ("filter: set_map counts", lambda: e.set_map(Z(B, 3, 2), counts=[3, 4])),
        ("filter: set_noise length", lambda: e.set_noise([K.Noise()] * 3)),
        ("filter: set_noise dict", lambda: e.set_noise(dict(v_d=1.0))),
        ("filter: set_noise one row", lambda: e.set_noise(K.Noise())),
        ("filter: command shape", lambda: e.update(F(3, 2), *msg)),
        ("filter: update meas_count", lambda: e.update(F(B, 2), F(B, KS, 3), I(3))),
        ("filter: update_dev each", lambda: e.update_dev(F(B, 2), 0, 0, 1)),
        ("filter: run_sim each", lambda: e.run_sim(F(T, 3, 2))),
        ("filter: run_sim shared", lambda: e.run_sim(F(T, 3))),
        ("filter: run commands or T", lambda: e.monitor_run()),
        ("filter: run commands shape", lambda: e.fix_run(F(T, 3))),
        ("filter: run T mismatch", lambda: e.innovation_run(F(T, 2), T=3)),
        ("filter: monitor_run source", lambda: e.monitor_run(F(T, 2), source=K.MONITOR_EACH)),
        ("filter: fix_run source", lambda: e.fix_run(F(T, B, 2), source=K.MONITOR_SHARED)),
        ("filter: sim run source", lambda: e.manage_run_sim(F(T, 2), source=K.INNOVATION_NAV)),
        ("filter: sim run commands or T", lambda: e.associate_joint_run_sim()),
        ("filter: sim run log name", lambda: e.gate_run_sim(T=T, log=("bogus",))),
        ("filter: set_path shape", lambda: e.set_path(Z(3, 3))),
        ("filter: set_paths list", lambda: e.set_paths([Z(3, 2)] * 3)),
        ("filter: set_paths array", lambda: e.set_paths(Z(3, 3, 2))),
        ("filter: set_paths counts", lambda: e.set_paths(Z(B, 3, 2), counts=[1, 2, 3])),
        ("config: monitor", lambda: e.monitor_now(cfg=dict(bogus=1))),
        ("config: controller", lambda: e.set_path(Z(3, 2), nav=dict(bogus=1))),
        ("config: innovation", lambda: e.innovation((0, 0), *msg, cfg=dict(bogus=1))),
        ("config: gate", lambda: e.gate((0, 0), *msg, cfg=dict(bogus=1))),
        ("config: association", lambda: e.associate((0, 0), *msg, cfg=dict(bogus=1))),
        ("config: joint association", lambda: e.associate_joint((0, 0), *msg, cfg=dict(gate=3.0))),
        ("config: map", lambda: e.map_prune(cfg=dict(bogus=1))),
        ("config: merge", lambda: e.map_merge(cfg=dict(bogus=1))),
        ("config: fix", lambda: e.fix(Z(B, 5), I(B), cfg=dict(bogus=1))),
        ("config: sensor", lambda: e.set_sensor(dict(bogus=1))),
        ("config: fix sensor", lambda: e.set_fix_sensor(dict(bogus=1))),
        ("config: default_sensor_config", lambda: K.default_sensor_config(bogus=1)),
        ("config: default_fix_sensor_config", lambda: K.default_fix_sensor_config(bogus=1)),
        ("ekf: innovation message", lambda: e.innovation((0, 0), F(B, KS, 2), I(B))),
        ("ekf: innovation_run log", lambda: e.innovation_run(F(T, 2), None, F(T, B, KS, 3), I(T, 3))),
        ("ekf: gate message", lambda: e.gate((0, 0), F(B, 0, 3), I(B))),
        ("ekf: gate_dev each", lambda: e.gate_dev(F(B, 2), 1, 2, KS, 3, 4)),
        ("ekf: step_gated_dev each", lambda: e.step_gated_dev(F(B, 2), 1, 2, KS)),
        ("ekf: associate_dev each", lambda: e.associate_dev(F(B, 2), 1, 2, KS, 3, 4)),
        ("ekf: step_associated_dev each", lambda: e.step_associated_dev(F(B, 2), 1, 2, KS)),
        ("ekf: associate_joint device each", lambda: e.associate_joint(F(B, 2), 1, (2, KS), dev_out=(3, 4))),
        ("ekf: step_associated_joint device each", lambda: e.step_associated_joint(F(B, 2), 1, (2, KS))),
        ("ekf: step_managed device each", lambda: e.step_managed(F(B, 2), 1, (2, KS))),
        ("ekf: sense_dev each", lambda: e.sense_dev(F(B, 2), 1, 2, KS)),
        ("ekf: gate_run log", lambda: e.gate_run(*badlog)),
        ("ekf: associate_run log", lambda: e.associate_run(F(T, 3, 2), F(T, B, KS, 3), I(T, B))),
        ("ekf: associate_joint_run log", lambda: e.associate_joint_run(F(T, 2), F(T, B, 0, 3), I(T, B))),
        ("ekf: manage_run log", lambda: e.manage_run(F(T, 2), F(T, B, KS, 3), I(T + 1, B))),
        ("ekf: manage_merge_run log", lambda: e.manage_merge_run(F(T, 2), F(T + 1, B, KS, 3), I(T + 1, B))),
        ("ekf: remove_landmarks shape", lambda: e.remove_landmarks(I(B, L + 1))),
        ("ekf: map_tally flags", lambda: e.map_tally(*msg, assoc_flags=I(3))),
        ("ekf: merge_landmarks shape", lambda: e.merge_landmarks(I(B + 1, L))),
        ("ekf: fix one pointer", lambda: e.fix(1, I(B))),
        ("ekf: fix shapes", lambda: e.fix(Z(B, 4), I(B))),
        ("ekf: set_fix_sensor length", lambda: e.set_fix_sensor([K.FixSensorConfig()] * 3)),
        ("ekf: set_sensor length", lambda: e.set_sensor([K.SensorConfig()] * 3)),
        ("ukf: command shape", lambda: u.predictionStage(F(3, 2))),
        ("ukf: set_sqrt_mode", lambda: u.set_sqrt_mode("bogus")),
        ("hook: innovation state", lambda: Fm.innovation_instance_host(x5, P5, I(2), L, 0, F(2), F(1, 3), noise)),
        ("hook: gate state", lambda: Fm.gate_instance_host(x5, Z(5, 4), id1, L, 0, F(2), F(1, 3), noise)),
        ("hook: gate k_stride", lambda: Fm.gate_instance_host(x5, P5, id1, L, 0, F(2), F(2, 3), noise, k_stride=1)),
        ("hook: associate state", lambda: Fm.associate_instance_host(Z(4), P5, id1, L, 0, F(2), F(1, 3), noise)),
        ("hook: associate k_stride", lambda: Fm.associate_instance_host(x5, P5, id1, L, 0, F(2), F(2, 3), noise, k_stride=1)),
        ("hook: associate_joint state", lambda: Fm.associate_joint_instance_host(x5, P5, I(2), L, 0, F(2), F(1, 3), noise)),
        ("hook: associate_joint k_stride", lambda: Fm.associate_joint_instance_host(x5, P5, id1, L, 0, F(2), F(2, 3), noise, k_stride=1)),
        ("config: joint association, hook", lambda: Fm.associate_joint_instance_host(x5, P5, id1, L, 0, F(2), F(1, 3), noise, cfg=dict(gate=3.0))),
        ("hook: map state", lambda: Fm.map_instance_host(x5, P5, I(2), L)),
        ("hook: map k_stride", lambda: Fm.map_instance_host(x5, P5, id1, L, meas=F(2, 3), k_stride=1)),
        ("hook: map remove", lambda: Fm.map_instance_host(x5, P5, id1, L, remove=I(2))),
        ("hook: merge state", lambda: Fm.merge_instance_host(x5, P5, I(2), L)),
        ("hook: merge counters", lambda: Fm.merge_instance_host(x5, P5, id1, L, seen=I(L))),
        ("hook: merge partner", lambda: Fm.merge_instance_host(x5, P5, id1, L, partner=I(L + 1))),
        ("hook: fix state", lambda: Fm.fix_instance_host(Z(4), Z(4, 4), L, Z(5), 3)),
        ("hook: fix row", lambda: Fm.fix_instance_host(x5, P5, L, Z(4), 3)),
        ("graph: no handle", lambda: g0.stats()),
        ("graph: update before init", lambda: gcold.update((0, 0), [])),
        ("graph: readParams type", lambda: g.readParams(3)),
        ("graph: readParams implementation", lambda: g.readParams(dict(pose_graph=dict(implementation="sesync")))),
        ("graph: init rows", lambda: g.init(Z(3, 3))),
        ("graph: init truth0", lambda: g.init(Z(B, 3), truth0=Z(B, 2))),
        ("graph: command shape", lambda: g.update(F(3, 2), [])),
        ("graph: update meas_count", lambda: g.update((0, 0), F(B, KS, 3), I(3))),
        ("graph: commands each", lambda: g.run_sim(F(T, 3, 2))),
        ("graph: commands shared", lambda: g.run_sim_fix(F(T, 3), 1)),
        ("graph: commands empty", lambda: g.run_sim_every_iteration(F(0, 2))),
        ("graph: set_map width", lambda: g.set_map(Z(3, 3))),
        ("graph: set_map batch", lambda: g.set_map(Z(3, 3, 2))),
        ("graph: set_map counts", lambda: g.set_map(Z(B, 3, 2), counts=[0, 3])),
        ("graph: marginalCovariance", lambda: g.marginalCovariance(0)),
        ("graph: fix rows", lambda: g.fix(Z(B, 4), I(B))),
        ("graph: fix kinds", lambda: g.fix(Z(B, 5), I(3))),
        ("graph: set_fix_sensor length", lambda: g.set_fix_sensor([K.FixSensorConfig()] * 3)),
        ("graph: set_fix_sensor dict", lambda: g.set_fix_sensor(dict(bogus=1))),
        ("hook: fix_factor shapes", lambda: Pm.fix_factor_host(Z(2), Z(5), 3)),
    ]
    return cases, made


def named_symbols(S):
    """The slam_* / pgs_* names that appear in the package's Python files as attribute accesses or - where a helper looks the symbol up
    by name - as whole string literals; _lib.py's literals are SIGNATURES itself and do not count."""
    here = os.path.dirname(os.path.abspath(S.__file__))
    names = set()
    for f in sorted(os.listdir(here)):
        if f.endswith(".py"):
            text = open(os.path.join(here, f)).read()
            names.update(re.findall(r"\.((?:slam|pgs)_\w+)", text))
            if f != "_lib.py":
                names.update(re.findall(r"\"((?:slam|pgs)_\w+)\"", text))
    return names


def trace(tmp):
    """Everything the test compares: {"calls": [...], "refusals": [...]}, and the set of symbols that were recorded."""
    import live_ekf_slam_amd as S
    from live_ekf_slam_amd import _lib
    saved, cwd = _lib.lib, os.getcwd()
    rec = Recorder(_lib.SIGNATURES)
    d = Drive(rec)
    made = d.made
    try:
        os.chdir(tmp)
        _lib.lib = lambda: rec
        drive_filters(d, S, tmp)
        drive_pose_graph(d, S, tmp)
        cases, more = refusals(S)
        made = made + more
        refused = []
        for label, fn in cases:
            _lib.lib = (lambda: NoCall()) if label.startswith("config:") else (lambda: NoLib())
            try:
                fn()
            except (ValueError, TypeError, _lib.SlamError) as err:
                refused.append(dict(call=label, raises=type(err).__name__, text=str(err)))
            else:
                raise AssertionError(f"{label}: the malformed call was not refused")
    finally:
        for f in made:
            f.h = None              # nothing the recorder handed out reaches the real library's destroy
        _lib.lib = saved
        os.chdir(cwd)
    labels = [e["call"] for e in d.entries] + [r["call"] for r in refused]
    assert len(set(labels)) == len(labels), "two entries share a label"
    return dict(calls=d.entries, refusals=refused), {name for name, _ in rec.calls}, named_symbols(S)


def _lines(doc):
    return {e["call"]: json.dumps(e, sort_keys=True) for e in doc["calls"] + doc["refusals"]}


def _write_expected(doc):
    with open(EXPECTED, "w") as fh:
        fh.write("{\n")
        for i, key in enumerate(("calls", "refusals")):
            fh.write(f' "{key}": [\n' + ",\n".join("  " + json.dumps(e, sort_keys=True) for e in doc[key]) + "\n ]" + (",\n" if i == 0 else "\n"))
        fh.write("}\n")


def test_every_named_symbol_is_driven(tmp_path):
    _, recorded, named = trace(str(tmp_path))
    assert len(LEFT_OUT) <= 5
    assert named - recorded == set(LEFT_OUT), sorted(named - recorded ^ set(LEFT_OUT))
    assert len(named) > 170, "the scan of the package's files found too few symbols to mean anything"


def test_mirror_calls_match_the_recorded_trace(tmp_path):
    got, _, _ = trace(str(tmp_path))
    got, want = _lines(got), _lines(json.load(open(EXPECTED)))
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    for label in want:
        assert got[label] == want[label], f"{label}\n got  {got[label]}\n want {want[label]}"


if __name__ == "__main__":
    import tempfile
    if sys.argv[1:] != ["--record"]:
        sys.exit("usage: python tests/test_mirror_calls_cpu.py --record")
    with tempfile.TemporaryDirectory() as tmp:
        doc, recorded, named = trace(tmp)
    assert named - recorded == set(LEFT_OUT), sorted(named - recorded ^ set(LEFT_OUT))
    _write_expected(doc)
    print(f"{EXPECTED}: {len(doc['calls'])} calls, {len(doc['refusals'])} refusals, {len(recorded)} symbols")
