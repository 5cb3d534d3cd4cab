"""The marginal-covariance entry points of the C ABI (include/slam_pgs.h) and their mirrors, without a GPU: the library exports them,
they are declared and mirrored, and they fail loudly - with an error text - on a NULL handle or a machine without a HIP device."""
import ctypes as C
import os
import re

import numpy as np

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import default_config

SYMBOLS = ("pgs_marginals", "pgs_get_marginals", "pgs_marginals_dev", "pgs_last_marginals_work")


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_pgs.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(pgs_handle\* h" % name, header), name
    assert "marginalCovariance" in header and "Marginals" not in header.split("Not covered:")[1].split("*/")[0]
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    for name in ("void marginals(int which = 1)", "marginalCovariance(int instance, int pose)", "landmarkCovariance(int instance, int j)"):
        assert name in hpp, name
    from live_ekf_slam_amd.pose_graph import BatchedPoseGraph
    for name in ("marginals", "get_marginals", "marginalCovariance", "last_marginals_work"):
        assert callable(getattr(BatchedPoseGraph, name))


def test_a_null_handle_is_an_error_with_a_text():
    L = _lib.lib()
    d = np.zeros(9)
    st = C.c_int32(0)
    p = C.c_void_p()
    for rc in (L.pgs_marginals(None, 1), L.pgs_get_marginals(None, 0, _lib._dp(), _lib._dp(), C.byref(st)),
               L.pgs_marginals_dev(None, C.byref(p), C.byref(p), C.byref(p)),
               L.pgs_last_marginals_work(None, d.ctypes.data_as(_lib._dp), d.ctypes.data_as(_lib._dp))):
        assert rc != 0 and "NULL handle" in _err()


def test_without_a_device_the_call_fails_loudly_and_with_one_it_checks_its_arguments():
    import pytest
    from live_ekf_slam_amd.pose_graph import BatchedPoseGraph
    pg = BatchedPoseGraph(2, num_iterations=8, L_max=4, k_per_pose=4)
    try:
        pg.readParams(default_config())
    except _lib.SlamError as e:   # no HIP device: no handle, and the mirror refuses to compute without one
        assert "no HIP device" in str(e) or "hip" in str(e).lower(), str(e)
        with pytest.raises(_lib.SlamError, match="readParams"):
            pg.marginals(0)
        with pytest.raises(_lib.SlamError, match="readParams"):
            pg.get_marginals(0)
        return
    pg.init(0.0, 0.0, 0.0)
    with pytest.raises(_lib.SlamError, match="which = 2"):
        pg.marginals(2)
    with pytest.raises(_lib.SlamError, match="which = -1"):
        pg.marginals(-1)
    with pytest.raises(_lib.SlamError, match="no result yet"):
        pg.marginals(1)
    with pytest.raises(_lib.SlamError, match="no marginals"):
        pg.get_marginals(0)
    pg.marginals(0)
    with pytest.raises(_lib.SlamError, match="instance 2 out of range"):
        pg.get_marginals(2)
    with pytest.raises(_lib.SlamError, match="instance -1 out of range"):
        pg.get_marginals(-1)
    m = pg.get_marginals(1)   # a graph of the prior alone: its covariance
    assert m["status"] == 0 and m["lm_cov"].shape == (0, 2, 2)
    assert np.allclose(m["pose_cov"][0], np.diag([1.3 ** 2, 1.3 ** 2, 1.2 ** 2]), rtol=1e-14, atol=0)
    pg.close()
