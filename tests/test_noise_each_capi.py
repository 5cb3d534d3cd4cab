"""Per-instance noise parameters (slam_set_noise_each, include/slam_batch.h) without a GPU: the entry points exist and are mirrored,
slam_noise_from_config field by field, the struct layouts, noise_rows, the argument checks that need no device, what the header says
is not covered, and the host-side packing of the rows (validation and the replicate_vw_quirk mapping) under AddressSanitizer +
UndefinedBehaviorSanitizer in a stand-alone program."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from live_ekf_slam_amd import _lib
from live_ekf_slam_amd.config import NOISE_FIELDS, Noise, default_config, noise_from_config, noise_rows

ERR_ARG = -1
SYMBOLS = ("slam_noise_from_config", "slam_set_noise_each")


def _err():
    return _lib.lib().slam_last_error().decode()


def test_the_library_exports_and_the_headers_declare_the_entry_points():
    L = C.CDLL(_lib.LIB_PATH)
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    for name in SYMBOLS:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
        assert re.search(r"\bint %s\(" % name, header), name
    assert _lib.SIGNATURES["slam_set_noise_each"][1] == [C.c_void_p, C.POINTER(Noise)]
    hpp = open(os.path.join(ROOT, "include", "slam_filter.hpp")).read()
    assert "void setNoiseEach(const std::vector<slam_noise>& rows)" in hpp and "slam_set_noise_each(h_" in hpp
    ros = open(os.path.join(ROOT, "include", "slam_filter_ros.hpp")).read()
    assert "slam_set_noise_each" not in ros and "setNoiseEach" not in ros          # the ROS adapter stays single-robot
    from live_ekf_slam_amd import build, filters
    assert "noise_row.h" in build.HEADERS and "host/noise_pack.h" in build.HEADERS
    assert callable(filters.BatchedFilter.set_noise)


def test_what_the_header_says_is_covered():
    header = open(os.path.join(ROOT, "include", "slam_batch.h")).read()
    doc = " ".join(header.split("---- per-instance noise parameters")[1].split("typedef struct slam_noise")[0].split())
    not_covered = doc.split("Not covered:")[1]
    for what in ("slam_multi_", "pose graph", "vision limits", "d_max / th_max", "quirk switches", "on the host"):
        assert what in not_covered, what
    for what in ("slam_nav_run", "slam_monitor_run", "slam_predict", "UKF_LOC", "Cholesky", "SLAM_ERR_STATE", "not state"):
        assert what in doc, what
    each = " ".join(header.split("---- heterogeneous batches")[1].split("int slam_init_each")[0].split())
    assert "per-instance noise configs" not in each.split("Not covered:")[1] and "slam_set_noise_each" in each
    pgs = " ".join(open(os.path.join(ROOT, "include", "slam_pgs.h")).read().split())
    assert "per-instance noise configs" in pgs                                     # the pose graph keeps its sentence
    integ = " ".join(open(os.path.join(ROOT, "INTEGRATION.md")).read().split())
    assert "a per-instance known map for UKF_LOC, per-instance noise configs" not in integ and "slam_set_noise_each" in integ
    design = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "4.9" in design and "noise_each" in design


def test_struct_layout(tmp_path):
    """slam_noise: 4 floats, 8 doubles, no padding: 80 bytes - the ctypes mirror against what a C compiler makes of the header."""
    assert C.sizeof(Noise) == 80
    assert [getattr(Noise, n).offset for n in NOISE_FIELDS] == [0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "slam_batch.h"\n'
                   'int main(void) { printf("%zu", sizeof(slam_noise));\n'
                   + "".join('printf(" %%zu", offsetof(slam_noise, %s));\n' % n for n in NOISE_FIELDS) + 'return 0; }\n')
    exe = tmp_path / "layout"
    cc = subprocess.run(["gcc", "-std=c99", "-Wall", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], capture_output=True, text=True, timeout=120)
    assert cc.returncode == 0, cc.stderr[-2000:]                                   # (the header is valid C)
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert out.stdout.split() == [str(v) for v in [80, 0, 4, 8, 12, 16, 24, 32, 40, 48, 56, 64, 72]], out.stdout


@pytest.mark.parametrize("quirk", [0, 1])
def test_noise_from_config_field_by_field(quirk):
    L = _lib.lib()
    c = default_config()
    c.v_d, c.v_th, c.w_r, c.w_b = 0.25, -0.5, 0.125, 0.0625
    c.V_00, c.V_11, c.W_00, c.W_11 = 0.011, 0.0012, 0.013, 0.014
    c.replicate_vw_quirk = quirk
    n = Noise()
    assert L.slam_noise_from_config(C.byref(c), C.byref(n)) == 0
    # the YAML keys as they are, whatever the quirk (the handle applies it when the rows are set); simulator = the same keys
    assert (n.v_d, n.v_th, n.w_r, n.w_b) == (0.25, -0.5, 0.125, 0.0625)
    assert (n.V_00, n.V_11, n.W_00, n.W_11) == (0.011, 0.0012, 0.013, 0.014)
    assert (n.sim_V_00, n.sim_V_11, n.sim_W_00, n.sim_W_11) == (0.011, 0.0012, 0.013, 0.014)
    assert bytes(n) == bytes(noise_from_config(c))
    assert L.slam_noise_from_config(None, C.byref(n)) == ERR_ARG and "NULL" in _err()
    assert L.slam_noise_from_config(C.byref(c), None) == ERR_ARG and "NULL" in _err()


def test_noise_rows_overrides():
    c = default_config()
    rows = noise_rows(c, 5)
    assert len(rows) == 5 and all(bytes(r) == bytes(noise_from_config(c)) for r in rows)
    grid = np.logspace(-4, 0, 5)
    rows = noise_rows(c, 5, V_00=grid, sim_W_11=0.5, v_d=[0.1, 0.2, 0.3, 0.4, 0.5])
    for b in range(5):
        assert rows[b].V_00 == grid[b] and rows[b].sim_W_11 == 0.5 and rows[b].v_d == np.float32(0.1 * (b + 1))
        assert rows[b].V_11 == c.V_11 and rows[b].W_00 == c.W_00 and rows[b].sim_V_00 == c.V_00      # the simulator rows are unchanged
    with pytest.raises(ValueError, match="unknown noise field"):
        noise_rows(c, 5, V00=1.0)
    with pytest.raises(ValueError, match="expected a scalar or 5 values"):
        noise_rows(c, 5, V_00=[1.0, 2.0])


def test_argument_checks_that_need_no_device():
    L = _lib.lib()
    rows = noise_rows(default_config(), 4)
    assert L.slam_set_noise_each(None, rows) == ERR_ARG and "NULL handle" in _err()
    assert L.slam_set_noise_each(None, None) == ERR_ARG and "NULL handle" in _err()
    from live_ekf_slam_amd.filters import BatchedEKF
    f = BatchedEKF(3, 4)
    with pytest.raises(_lib.SlamError, match="readParams"):
        f.set_noise(rows)


DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "noise_pack.h"

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures += 1; } } while (0)

static slam_noise row(int k) {
    slam_noise r;
    r.v_d = 0.5f + k; r.v_th = 1.5f + k; r.w_r = 2.5f + k; r.w_b = 3.5f + k;
    r.V_00 = 10.0 + k; r.V_11 = 11.0 + k; r.W_00 = 12.0 + k; r.W_11 = 13.0 + k;
    r.sim_V_00 = 20.0 + k; r.sim_V_11 = 21.0 + k; r.sim_W_00 = 22.0 + k; r.sim_W_11 = 23.0 + k;
    return r;
}

int main() {
    CHECK(sizeof(slam_noise) == 80 && sizeof(slam::NoiseRow) == 80);
    const size_t B = 37;
    std::vector<slam_noise> rows(B);
    for (size_t b = 0; b < B; ++b) rows[b] = row((int)b);
    for (int quirk = 0; quirk < 2; ++quirk) {
        std::vector<slam::NoiseRow> out(B);               // exactly B rows: a write past the end is the sanitizer's to find
        size_t bad = 99; const char* field = nullptr;
        CHECK(slam_host::noise_pack(rows.data(), B, quirk, out.data(), &bad, &field) == 0 && bad == 99 && field == nullptr);
        for (size_t b = 0; b < B; ++b) {
            const double k = (double)b;
            const slam::NoiseRow& o = out[b];
            CHECK(o.v_d == 0.5f + (float)k && o.v_th == 1.5f + (float)k && o.w_r == 2.5f + (float)k && o.w_b == 3.5f + (float)k);
            if (quirk) CHECK(o.V00 == 12.0 + k && o.V11 == 13.0 + k && o.W00 == 1.0 && o.W11 == 1.0);   // filter.h:116-117
            else CHECK(o.V00 == 10.0 + k && o.V11 == 11.0 + k && o.W00 == 12.0 + k && o.W11 == 13.0 + k);
            CHECK(o.sV00 == 20.0 + k && o.sV11 == 21.0 + k && o.sW00 == 22.0 + k && o.sW11 == 23.0 + k);   // never touched by the quirk
        }
    }
    // every field, every kind of non-finite value, first and last row: refused with the instance and the field's name
    const char* names[12] = {"v_d", "v_th", "w_r", "w_b", "V_00", "V_11", "W_00", "W_11", "sim_V_00", "sim_V_11", "sim_W_00", "sim_W_11"};
    const double bads[3] = {NAN, INFINITY, -INFINITY};
    for (int fi = 0; fi < 12; ++fi)
        for (int bi = 0; bi < 3; ++bi)
            for (size_t at : {(size_t)0, B - 1}) {
                std::vector<slam_noise> r2 = rows;
                slam_noise& r = r2[at];
                float* fl[4] = {&r.v_d, &r.v_th, &r.w_r, &r.w_b};
                double* db[8] = {&r.V_00, &r.V_11, &r.W_00, &r.W_11, &r.sim_V_00, &r.sim_V_11, &r.sim_W_00, &r.sim_W_11};
                if (fi < 4) *fl[fi] = (float)bads[bi]; else *db[fi - 4] = bads[bi];
                std::vector<slam::NoiseRow> out(B);
                size_t bad = 99; const char* field = nullptr;
                CHECK(slam_host::noise_pack(r2.data(), B, 1, out.data(), &bad, &field) == 1);
                CHECK(bad == at && field != nullptr && strcmp(field, names[fi]) == 0);
            }
    {   // two bad rows: the first one is named; no rows at all: nothing is read or written
        std::vector<slam_noise> r2 = rows;
        r2[5].W_00 = NAN; r2[3].sim_V_11 = INFINITY;
        std::vector<slam::NoiseRow> out(B);
        size_t bad = 99; const char* field = nullptr;
        CHECK(slam_host::noise_pack(r2.data(), B, 0, out.data(), &bad, &field) == 1 && bad == 3 && strcmp(field, "sim_V_11") == 0);
        bad = 99; field = nullptr;
        CHECK(slam_host::noise_pack(nullptr, 0, 0, nullptr, &bad, &field) == 0 && bad == 99);
    }
    {   // values the reference does not check either pass: negative, zero, huge, denormal
        slam_noise r = row(0);
        r.V_00 = -1.0; r.W_11 = 0.0; r.sim_W_00 = 1e300; r.v_d = 1e-45f;
        CHECK(slam_host::noise_bad_field(r) == nullptr);
    }
    {   // slam_noise_from_config's body
        slam_config c;
        memset(&c, 0, sizeof(c));
        c.v_d = 1.f; c.v_th = 2.f; c.w_r = 3.f; c.w_b = 4.f; c.V_00 = 5.0; c.V_11 = 6.0; c.W_00 = 7.0; c.W_11 = 8.0; c.replicate_vw_quirk = 1;
        slam_noise n;
        slam_host::noise_from_config(c, &n);
        CHECK(n.v_d == 1.f && n.v_th == 2.f && n.w_r == 3.f && n.w_b == 4.f && n.V_00 == 5.0 && n.V_11 == 6.0 && n.W_00 == 7.0 && n.W_11 == 8.0);
        CHECK(n.sim_V_00 == 5.0 && n.sim_V_11 == 6.0 && n.sim_W_00 == 7.0 && n.sim_W_11 == 8.0);
    }
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
"""


def test_row_packing_under_asan_ubsan(tmp_path):
    src = tmp_path / "noise_pack_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "noise_pack_driver"
    inc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-fno-omit-frame-pointer", "-I", inc, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    text = out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-3000:]
    assert out.returncode == 0, text[-3000:]
    assert "0 failed" in out.stdout, text[-3000:]
