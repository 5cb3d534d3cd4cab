"""The map score (slam_map_score; include/slam_batch.h) without a GPU: the entry points exist, are declared and listed in
_lib.SIGNATURES with matching argument counts, the C++ mirror names them, the build lists the new files, the struct layout is the
compiler's, the defaults are the documented ones, and every SLAM_ERR_ARG path returns its code with a text before the handle is looked at."""
import ctypes as C
import math
import os
import re
import subprocess

import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib

import score_reference as R

ERR_ARG = -1
SYMBOLS = ("slam_score_config_default", "slam_map_score", "slam_last_score_work", "slam_map_score_instance_host")
BAD_CONFIGS = [("match_radius", float("nan")), ("match_radius", 0.0), ("match_radius", -1.0), ("match_radius", float("-inf")),
               ("lm_lo", float("nan")), ("lm_lo", float("-inf")), ("lm_hi", float("nan")), ("lm_hi", float("inf")), ("lm_lo", 8.0)]


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        m = re.search(r"\bint %s\(([^)]*)\)" % name, code)
        assert m and len(m.group(1).split(",")) == len(_lib.SIGNATURES[name][1]), name
    assert header.index("---- map score") < header.index("int slam_score_config_default(") < header.index("int slam_map_score_instance_host(")
    doc = " ".join(w for w in header.split("---- map score")[1].split("typedef struct slam_score_config")[0].split() if w != "*")
    for word in ("ties to the lowest r", "never wins", "ties to the lowest j", "MATCHED", "DUPLICATE", "SPURIOUS", "one addition per slot",
                 "principal submatrix", "marginalised out", "CHANGES NOTHING", "byte-identical", "before the handle is looked at",
                 "SLAM_ERR_UNSUPPORTED", "SLAM_ERR_STATE", "Not covered:", "Hungarian", "Mahalanobis", "slam_multi_", "the pose graph", "*_run form",
                 "checkpoint state"):
        assert word in doc, word
    # slam_consistency still says that it does not guess an association
    assert "guessing a landmark association for unknown ids" in header
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    assert "slam_map_score(" in hpp and "mapScore(const slam_score_config* cfg = nullptr)" in hpp
    assert hpp.index("Consistency consistency()") < hpp.index("MapScore mapScore(")
    from live_ekf_slam_amd import build
    assert "score_kernel.hip" in build.SOURCES and "capi_score.cpp" in build.SOURCES and "score_kernel.h" in build.HEADERS


def test_default_config_and_struct_layout(tmp_path):
    L = _lib.lib()
    c = _lib.ScoreConfig()
    assert L.slam_score_config_default(C.byref(c)) == 0
    assert (c.match_radius, c.lm_lo, c.lm_hi, c.full) == (math.inf, -2.0 * math.log(0.975), -2.0 * math.log(0.025), 0)
    from live_ekf_slam_amd.config import InnovationConfig
    ic = InnovationConfig()
    assert L.slam_innovation_config_default(C.byref(ic)) == 0 and (ic.nis_lo, ic.nis_hi) == (c.lm_lo, c.lm_hi) == (R.LM_LO, R.LM_HI)
    assert L.slam_score_config_default(None) == ERR_ARG and "NULL" in _err()
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\n'
                   'int main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(slam_score_config), offsetof(slam_score_config, match_radius),'
                   ' offsetof(slam_score_config, lm_lo), offsetof(slam_score_config, lm_hi), offsetof(slam_score_config, full));'
                   'return (SLAM_SCORE_MATCHED == 1 && SLAM_SCORE_DUPLICATE == 2 && SLAM_SCORE_SPURIOUS == 3 && SLAM_SCORE_MATCHED_NOT_PD == 1 &&'
                   ' SLAM_SCORE_LM_NOT_PD == 4 && SLAM_SCORE_INSTANCE_FAILED == 8) ? 0 : 1;}\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    S = _lib.ScoreConfig
    assert got == [C.sizeof(S), S.match_radius.offset, S.lm_lo.offset, S.lm_hi.offset, S.full.offset]


@pytest.mark.parametrize("field,value", BAD_CONFIGS)
def test_config_checks_come_before_the_handle(field, value):
    L = _lib.lib()
    cfg = R.config(1.5)
    setattr(cfg, field, value)
    rc = L.slam_map_score(None, C.byref(cfg), *([None] * 13))
    word = "match_radius" if field == "match_radius" else "band"
    assert rc == ERR_ARG and "score config" in _err() and word in _err() and "NULL handle" not in _err()
    m = R.grid_map(4)
    s = R.make(__import__("numpy").random.default_rng(1), 2, m, {})
    rc, _ = R.host_hook(s["x"], s["P"], 2, 4, 0, s["truth"], m, cfg)
    assert rc == ERR_ARG and "score config" in _err()


def test_the_limits_of_the_config_are_allowed_and_the_handle_is_checked_next():
    L = _lib.lib()
    for cfg in (None, R.config(math.inf), R.config(1e-300), R.config(1e300, 0.0, 0.0, 1), R.config(2.0, -5.0, 1e300, 7)):
        rc = L.slam_map_score(None, None if cfg is None else C.byref(cfg), *([None] * 13))
        assert rc == ERR_ARG and "NULL handle" in _err()
    assert L.slam_last_score_work(None, None, None) == ERR_ARG and "NULL handle" in _err()
