"""The consistency entry points of the C ABI (include/slam_batch.h) and their mirrors, without a GPU: the library exports them, they
are declared and mirrored, and they fail loudly - with an error text - on a NULL handle or a machine without a HIP device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import default_config

SYMBOLS = ("slam_consistency", "slam_last_consistency_work")


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(slam_handle\* h" % name, header), name
    for flag, value in (("FULL_NOT_PD", 1), ("POSE_NOT_PD", 2), ("NO_TRUTH", 4), ("INSTANCE_FAILED", 8)):
        assert re.search(r"SLAM_CONSISTENCY_%s = %d\b" % (flag, value), header), flag
    doc = header.split("---- consistency")[1].split("enum slam_consistency_flags")[0]
    assert "Not covered:" in doc and "UKF" in doc.split("Not covered:")[1] and "host-fed" in doc
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    assert "Consistency consistency()" in hpp and "slam_consistency(h_" in hpp
    drv = open(os.path.join(ROOT, "live_ekf_slam_amd", "csrc", "host", "filter_driver.cpp")).read()
    assert 'mode == "consistency"' in drv
    from live_ekf_slam_amd import filters
    for name in ("consistency", "last_consistency_work"):
        assert callable(getattr(filters.BatchedEKF, name))
    assert callable(filters.consistency_summary)
    assert (filters.BatchedFilter.FULL_NOT_PD, filters.BatchedFilter.POSE_NOT_PD, filters.BatchedFilter.NO_TRUTH,
            filters.BatchedFilter.INSTANCE_FAILED) == (1, 2, 4, 8)


def test_a_null_handle_is_an_error_with_a_text():
    L = _lib.lib()
    d = np.zeros(4)
    i = np.zeros(4, dtype=np.int32)
    dp, ip = d.ctypes.data_as(_lib._dp), i.ctypes.data_as(_lib._ip)
    for rc in (L.slam_consistency(None, dp, dp, dp, ip, ip), L.slam_consistency(None, None, None, None, None, None),
               L.slam_last_consistency_work(None, dp, dp)):
        assert rc == -1 and "NULL handle" in _err()


def test_without_a_device_the_mirror_fails_loudly_and_with_one_it_checks_the_call_order():
    from live_ekf_slam_amd.filters import BatchedEKF, BatchedUKF
    f = BatchedEKF(3, 4)
    with pytest.raises(_lib.SlamError, match="readParams"):
        f.consistency()
    with pytest.raises(_lib.SlamError, match="readParams"):
        f.last_consistency_work()
    try:
        f.readParams(default_config())
    except _lib.SlamError as e:   # no HIP device: no handle, and the mirror refuses to compute without one
        assert "hip" in str(e).lower(), str(e)
        with pytest.raises(_lib.SlamError, match="readParams"):
            f.consistency()
        return
    with pytest.raises(_lib.SlamError, match="slam_init has not been called"):
        f.consistency()
    f.init(0.0, 0.0, 0.0)
    with pytest.raises(_lib.SlamError, match="slam_set_map"):
        f.consistency()
    with pytest.raises(_lib.SlamError, match="has not run"):
        f.last_consistency_work()
    f.set_map(np.array([[1.0, 2.0], [3.0, 4.0]]))
    c = f.consistency()   # the start state: P = diag(1e-4, 1e-4, 2.5e-5) (ekf.cpp:11-14), no landmarks
    assert c["dof"].tolist() == [3, 3, 3] and c["flags"].tolist() == [0, 0, 0] and np.all(c["map_rms"] == 0)
    assert np.all(np.isfinite(c["nees_pose"])) and np.array_equal(c["nees_full"], c["nees_pose"])
    f.close()
    u = BatchedUKF(2, 4).readParams(default_config())
    u.init(0.0, 0.0, 0.0)
    with pytest.raises(_lib.SlamError, match="rank-deficient"):
        u.consistency()
    u.close()
