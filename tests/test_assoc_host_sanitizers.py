"""The association's per-instance function (live_ekf_slam_amd/csrc/assoc_kernel.h: the source the kernel compiles) in a stand-alone host
program built with AddressSanitizer + UndefinedBehaviorSanitizer: crafted messages - k = 0, 1, 64 and 65 detections, an empty map, a map of
66 landmarks, a full map, ids at the top of the range a float carries (and INT_MAX), a landmark twice, an exact tie, a NaN range, a
frozen status, in place - on heap arrays of EXACTLY the sizes the interface states (x, P, ids, the message row of k_stride triplets, the
cost matrix of k x M, 64 verdicts and slots, 64 x 4 det values), so any read or write outside them is reported.  The program also checks
the bookkeeping: count_out = matched + new, the counts add up to k, the labelled rows carry the detection's r and b, the tail is zero."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <limits.h>
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "assoc_kernel.h"
using namespace slam;

static int failures = 0;
static int g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static double uni() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (double)(g_s >> 11) / 9007199254740992.0; }

struct State { std::vector<double> x, P; std::vector<int32_t> ids; int M; };
static State make_state(int M, int32_t id0) {
    State s; s.M = M; const int n = 3 + 2 * M;
    s.x.assign(n, 0.0); s.P.assign((size_t)n * n, 0.0); s.ids.resize(M);
    s.x[0] = 0.3; s.x[1] = -0.2; s.x[2] = 0.4;
    for (int j = 0; j < M; ++j) {
        const double r = 1.5 + 1.0 * (j / 5), b = -1.0 + 0.5 * (j % 5);
        s.x[3 + 2 * j] = s.x[0] + r * cos(s.x[2] + b); s.x[4 + 2 * j] = s.x[1] + r * sin(s.x[2] + b);
        s.ids[j] = id0 + j;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = (i == j ? 4e-4 : 2e-5 * (uni() - 0.5));
            s.P[(size_t)i * n + j] = v; s.P[(size_t)j * n + i] = v;
        }
    return s;
}
static void clean(const State& s, int slot, std::vector<float>& m) {
    const double dx = s.x[3 + 2 * slot] - s.x[0], dy = s.x[4 + 2 * slot] - s.x[1];
    m.push_back(NAN); m.push_back((float)(sqrt(dx * dx + dy * dy) + 0.02 * (uni() - 0.5)));
    m.push_back((float)(remainder(atan2(dy, dx) - s.x[2], 6.283185307179586) + 0.02 * (uni() - 0.5)));
}
static void fresh(int cell, std::vector<float>& m) {
    m.push_back(-1.0f); m.push_back((float)(2.0 + 1.0 * (cell / 5))); m.push_back((float)(-0.75 + 0.5 * (cell % 5)));
}

static void run(const State& s, int L_max, int32_t status, const std::vector<float>& msg, int32_t want_flags, bool f32, int want_match, int want_new) {
    g_case += 1;
    const int k = (int)msg.size() / 3, n = 3 + 2 * s.M;
    const InnovNoise nz = {0.f, 0.f, 0.f, 0.f, 1e-4, 1e-4, 2.5e-3, 2.5e-3};
    const double* x = s.x.data(); const double* P = s.P.data();
    auto lx = [&](int i) { return f32 ? (double)(float)x[i] : x[i]; };
    auto lp = [&](int r, int c) { const double e = P[(size_t)r * n + c]; return f32 ? (double)(float)e : e; };
    for (int pass = 0; pass < 2; ++pass) {            // separate output; in place
        // heap blocks of exactly the stated sizes
        std::vector<float> row(msg), out(msg.size());
        std::vector<double> cost((size_t)(k <= kInnovMaxDet ? k : 0) * s.M), det((size_t)kInnovMaxDet * kAssocDetLen);
        std::vector<int32_t> verdict(kInnovMaxDet), slot(kInnovMaxDet);
        std::vector<AssocWork> ws(1);
        float* const o = pass == 1 ? row.data() : out.data();
        int32_t count_out = -1;
        const AssocResult v = associate_instance_host(ws[0], lx, lp, s.M ? s.ids.data() : nullptr, s.M, L_max, status, 0.01f, 0.004f,
                                                      k ? row.data() : nullptr, k, k > 0 ? k : 1, nz, 9.210340371976182, 27.631021115928547,
                                                      cost.empty() ? nullptr : cost.data(), verdict.data(), slot.data(), det.data(), k ? o : nullptr,
                                                      &count_out);
        CHECK(v.flags == want_flags);
        double rec[kInnovRecLen];
        assoc_record(v, rec);
        if (v.flags) {
            CHECK(count_out == 0 && v.n_match == 0 && v.n_new == 0 && v.n_drop == 0 && rec[kAscEval] == 0.0);
            for (int l = 0; l < kInnovMaxDet; ++l) CHECK(verdict[l] == kAssocNone && slot[l] == -1);
            for (int i = 0; i < 3 * k; ++i) CHECK(o[i] == 0.0f);
            continue;
        }
        CHECK(count_out == v.n_match + v.n_new && v.n_match + v.n_new + v.n_drop == k && rec[kAscDetIn] == (double)k);
        if (want_match >= 0) CHECK(v.n_match == want_match && v.n_new == want_new);
        int kept = 0;
        for (int l = 0; l < kInnovMaxDet; ++l) {
            CHECK(l < k ? verdict[l] != kAssocNone : (verdict[l] == kAssocNone && slot[l] == -1));
            CHECK(slot[l] >= -1 && slot[l] < s.M);
            if (l < k && (verdict[l] == kAssocMatched || verdict[l] == kAssocNew)) {
                CHECK(memcmp(o + 3 * kept + 1, msg.data() + 3 * l + 1, 2 * sizeof(float)) == 0);
                if (verdict[l] == kAssocMatched) CHECK(o[3 * kept] == (float)s.ids[slot[l]]);
                else CHECK(o[3 * kept] >= 0.0f && o[3 * kept] < 16777216.0f);
                kept += 1;
            }
        }
        CHECK(kept == count_out);
        for (int i = 3 * kept; i < 3 * k; ++i) CHECK(o[i] == 0.0f);
    }
}

int main() {
    for (int f32 = 0; f32 < 2; ++f32)
        for (int L_max = 20; L_max <= 70; L_max += 50) {
            const State st = make_state(18, 100), none = make_state(0, 0), full = make_state(L_max, 100), wrap = make_state(66, 100),
                        top = make_state(5, (1 << 24) - 6), huge = make_state(3, INT_MAX - 2);
            std::vector<float> m;
            run(st, L_max, 0, m, 0, f32, 0, 0);                                                                    // k = 0
            clean(st, 2, m); run(st, L_max, 0, m, 0, f32, 1, 0);                                                   // k = 1
            m.clear(); fresh(1, m); fresh(7, m); run(none, L_max, 0, m, 0, f32, 0, 2);                             // M = 0
            m.clear(); for (int j = 17; j >= 0; --j) clean(st, j, m); run(st, L_max, 0, m, 0, f32, 18, 0);         // every landmark
            m.clear(); clean(st, 0, m); fresh(2, m); clean(st, 3, m); fresh(11, m); run(st, L_max, 0, m, 0, f32, 2, 2);
            m.clear(); clean(st, 2, m); clean(st, 4, m); clean(st, 2, m); run(st, L_max, 0, m, 0, f32, 2, 0);      // a landmark twice
            m.clear(); clean(st, 3, m); m.insert(m.end(), m.begin(), m.begin() + 3); run(st, L_max, 0, m, 0, f32, 1, 0);   // an exact tie
            m.clear(); clean(st, 0, m); m.push_back(0.f); m.push_back(NAN); m.push_back(0.1f); run(st, L_max, 0, m, 0, f32, 1, 0);
            m.clear(); clean(full, 1, m); fresh(3, m); run(full, L_max, 0, m, 0, f32, 1, 0);                        // a full map
            m.clear(); fresh(0, m); clean(top, 0, m); fresh(3, m); fresh(6, m); run(top, 70, 0, m, 0, f32, 1, 1);  // ids near 2^24
            m.clear(); fresh(0, m); clean(huge, 1, m); run(huge, 70, 0, m, 0, f32, 1, 0);                          // ids at INT_MAX
            if (L_max == 70) {
                m.clear(); for (int l = 0; l < kInnovMaxDet; ++l) clean(wrap, 65 - l, m); run(wrap, L_max, 0, m, 0, f32, 64, 0);   // two groups of landmarks
                clean(wrap, 0, m); run(wrap, L_max, 0, m, kInnovTooLong, f32, -1, -1);                              // 65 detections
            }
            m.clear(); clean(st, 2, m); fresh(1, m); run(st, L_max, kInnovStatusFrozen, m, kInnovFrozen, f32, -1, -1);
        }
    printf(failures ? "%d check(s) failed\n" : "assoc host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_function_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "assoc_host.cpp"
    exe = tmp_path / "assoc_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "assoc host driver ok: 52 cases" in out.stdout, out.stdout + out.stderr
