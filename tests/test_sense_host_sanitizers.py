"""The sensor model's per-instance function (live_ekf_slam_amd/csrc/sense_kernel.h: the source the kernel compiles) in a stand-alone host
program built with AddressSanitizer + UndefinedBehaviorSanitizer: maps of 3, 64 and 80 landmarks in view (80: TOO_LONG), every fault on,
both orders, erased ids, rows of 1, 5, 16 and 80 detections and a frozen instance, on heap arrays of EXACTLY the sizes the interface states
(the message row of k_stride triplets, origin and fault of k_stride entries), so any read or write outside them is reported.  The program
also checks the bookkeeping: the record's counts add up, the written slots are a message, the tail is zero."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "sense_kernel.h"
using namespace slam;

static int failures = 0, cases = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, cases, #c); failures += 1; } } while (0)

int main() {
    std::vector<SenseWork> ws(1);
    std::vector<double> map(160);
    for (int i = 0; i < 80; ++i) { const double a = -1.2 + 2.4 * i / 79.0; map[2 * i] = 2.0 * cos(a); map[2 * i + 1] = 2.0 * sin(a); }
    const int strides[4] = {1, 5, 16, 80}, sizes[3] = {3, 64, 80};
    for (int ks : strides) for (int sh = 0; sh < 2; ++sh) for (int L : sizes) for (unsigned g = 0; g < 20; ++g) {
        cases += 1;
        const slam_sensor r = {0.3, 0.4, -0.5, 1.5, 0.6, 0.5, 8, sh, (int32_t)(g & 1)};
        CHECK(sense_bad_field(r, 3.0) == nullptr);
        const SenseSim sc = {2025, g, 0.1, 0.0546, 3.0, -1.57, 1.57, 0.01, 0.001, 0.01, 0.01};
        double tx = 0.0, ty = 0.0, tth = 0.0;
        std::vector<double> m(map.begin(), map.begin() + 2 * L);          // exactly L landmarks
        const int c_vis = sense_clean_seq(sc, 0.05f, 0.01f, g, m.data(), L, tx, ty, tth, ws[0].meas);
        CHECK(c_vis == L);
        std::vector<float> row(3 * (size_t)ks, 7.0f); std::vector<int32_t> org(ks, 9), flt(ks, 9);
        const SenseResult v = g == 7 ? sense_frozen(InnovSeq(), ks, row.data(), org.data(), flt.data())
                                     : sense_instance(InnovSeq(), ws[0], r, 2025, g, g, c_vis, L, 3.0, -1.57, 1.57, ks, row.data(), org.data(), flt.data());
        double rec[kSenseRecLen];
        sense_record(v, ks, rec);
        if (g == 7) { CHECK(v.flags == kSenseFrozen && v.count == 0 && rec[kSenFrozen] == 1.0); }
        else {
            CHECK(v.flags == (L > kSenseMaxDet ? kSenseTooLong : 0) && v.c == (L < kSenseMaxDet ? L : kSenseMaxDet));
            CHECK(v.count == v.c - v.n_miss + v.n_clutter && v.n_spike <= v.c - v.n_miss && v.n_clutter <= 8);
            CHECK(rec[kSenOut] == (double)v.count && rec[kSenOverflow] == (double)(v.count > ks ? v.count - ks : 0));
        }
        int spiked = 0;
        for (int e = 0; e < ks; ++e) {
            if (e < v.count) {
                CHECK(org[e] >= -1 && org[e] < L && (flt[e] == 0 || flt[e] == 1) && !(org[e] < 0 && flt[e]));
                CHECK((g & 1) ? row[3 * e] != row[3 * e] : (org[e] < 0 ? row[3 * e] >= (float)L : row[3 * e] == (float)org[e]));
                spiked += flt[e];
            } else {
                CHECK(row[3 * e] == 0.0f && row[3 * e + 1] == 0.0f && row[3 * e + 2] == 0.0f && org[e] == -1 && flt[e] == 0);
            }
        }
        CHECK(spiked <= v.n_spike && (v.count > ks || spiked == v.n_spike));
    }
    printf(failures ? "%d check(s) failed\n" : "sense host driver ok: %d cases\n", failures ? failures : cases);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_function_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "sense_host.cpp"
    exe = tmp_path / "sense_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "sense host driver ok: 480 cases" in out.stdout, out.stdout + out.stderr
