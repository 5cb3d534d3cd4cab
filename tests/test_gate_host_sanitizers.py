"""The gate's per-instance function (live_ekf_slam_amd/csrc/gate_kernel.h with innovation_kernel.h: the source the kernel compiles) in a
stand-alone host program built with AddressSanitizer + UndefinedBehaviorSanitizer: crafted messages - k = 0, 1, 64 and 65 detections,
spikes first, last and everywhere, a landmark twice, insertions up to and beyond the capacity, more than 16 distinct landmarks, a message
that would freeze, a frozen status - on heap arrays of EXACTLY the sizes the interface states (x, P, ids, the message row of k_stride = k
triplets, 64 verdicts, 64 x 6 det values), so any read or write outside them is reported.  The program also checks the bookkeeping
(count_out + n_rej = k, verdicts against the message) and that an infinite gate gives innovation_instance()'s result in bits."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "gate_kernel.h"
using namespace slam;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static int g_case = 0;
static unsigned long long g_s = 88172645463325252ull;
static double uni() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (double)(g_s >> 11) / 9007199254740992.0; }

struct State { std::vector<double> x, P; std::vector<int32_t> ids; int M; };
static State make_state(int M) {
    State s; s.M = M; const int n = 3 + 2 * M;
    s.x.assign(n, 0.0); s.P.assign((size_t)n * n, 0.0); s.ids.resize(M);
    s.x[0] = 0.3; s.x[1] = -0.2; s.x[2] = 0.4;
    for (int j = 0; j < M; ++j) {
        const double r = 1.0 + 2.0 * uni(), b = -1.2 + 2.4 * uni();
        s.x[3 + 2 * j] = s.x[0] + r * cos(s.x[2] + b); s.x[4 + 2 * j] = s.x[1] + r * sin(s.x[2] + b);
    }
    for (int j = 0; j < M; ++j) s.ids[j] = 100 + j;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = (i == j ? 1e-3 : 1e-4 * (uni() - 0.5));
            s.P[(size_t)i * n + j] = v; s.P[(size_t)j * n + i] = v;
        }
    return s;
}
static void detection(const State& s, int slot, int new_id, bool spike, std::vector<float>& m) {
    double r = 1.0 + 2.0 * uni(), b = -1.2 + 2.4 * uni(); int id = new_id;
    if (slot >= 0) {
        const double dx = s.x[3 + 2 * slot] - s.x[0], dy = s.x[4 + 2 * slot] - s.x[1];
        r = sqrt(dx * dx + dy * dy) + 0.02 * (uni() - 0.5); b = remainder(atan2(dy, dx) - s.x[2], 6.283185307179586) + 0.02 * (uni() - 0.5);
        id = s.ids[slot];
    }
    m.push_back((float)id); m.push_back((float)(r + (spike ? 10.0 : 0.0))); m.push_back((float)b);
}

static void run(const State& s, int L_max, int32_t status, const std::vector<float>& msg, int32_t want_flags, bool f32) {
    g_case += 1;
    const int k = (int)msg.size() / 3, n = 3 + 2 * s.M;
    const InnovNoise nz = {0.f, 0.f, 0.f, 0.f, 1e-4, 1e-4, 2.5e-3, 2.5e-3};
    // heap blocks of exactly the stated sizes
    std::vector<float> row(msg), out(msg.size());
    std::vector<double> det((size_t)kInnovMaxDet * kInnovDetLen), det0(det.size());
    std::vector<int32_t> verdict(kInnovMaxDet);
    std::vector<InnovWork> ws(1);
    const double* x = s.x.data(); const double* P = s.P.data();
    auto lx = [&](int i) { return f32 ? (double)(float)x[i] : x[i]; };
    auto lp = [&](int r, int c) { const double e = P[(size_t)r * n + c]; return f32 ? (double)(float)e : e; };
    int32_t count_out = -1, n_rej = -1;
    for (int pass = 0; pass < 3; ++pass) {        // the default gate; in place; an infinite gate
        const double gate = pass == 2 ? INFINITY : 13.815510557964274;
        std::vector<float> inplace(msg);
        float* const in = pass == 1 ? inplace.data() : row.data();
        float* const o = pass == 1 ? inplace.data() : out.data();
        const InnovResult v = gate_instance_host(ws[0], lx, lp, s.M ? s.ids.data() : nullptr, s.M, L_max, status, 0.01f, 0.004f, k ? in : nullptr, k,
                                                 k > 0 ? k : 1, nz, false, 0.05, 7.4, gate, det.data(), k ? o : nullptr, &count_out, &n_rej, verdict.data());
        CHECK(v.flags == want_flags);
        double rec[kInnovRecLen];
        gate_record(v, n_rej, rec);
        CHECK(rec[kGateRej] == (double)n_rej);
        if (gate_passes_through(v.flags)) {
            CHECK(n_rej == 0 && count_out == k && (k == 0 || memcmp(o, msg.data(), sizeof(float) * msg.size()) == 0));
            for (int l = 0; l < kInnovMaxDet; ++l) CHECK(verdict[l] == kGateNone);
            continue;
        }
        int rej = 0, kept = 0;
        for (int l = 0; l < kInnovMaxDet; ++l) {
            bool found = false;
            for (int j = 0; l < k && j < s.M; ++j) found = found || s.ids[j] == (int)msg[3 * l];
            CHECK(found ? verdict[l] != kGateNone : verdict[l] == kGateNone);
            if (l < k && verdict[l] == kGateRejected) { rej += 1; continue; }
            if (l < k) { CHECK(memcmp(o + 3 * kept, msg.data() + 3 * l, 3 * sizeof(float)) == 0); kept += 1; }
        }
        CHECK(rej == n_rej && kept == count_out && kept + rej == k);
        for (int i = 3 * kept; i < 3 * k; ++i) CHECK(o[i] == 0.0f);
        if (pass == 2) {                          // an infinite gate: the plain evaluation, bit for bit
            CHECK(n_rej == 0);
            for (int i = 0; i < 3 * (k < kInnovMaxDet ? k : kInnovMaxDet); ++i) ws[0].meas[i] = msg[i];
            const InnovResult u = innovation_instance(InnovSeq(), ws[0], lx, lp, s.M ? s.ids.data() : nullptr, s.M, L_max, status, 0.01f, 0.004f, k, nz,
                                                      false, 0.05, 7.4, det0.data());
            CHECK(memcmp(det.data(), det0.data(), sizeof(double) * det.size()) == 0 && memcmp(u.post, v.post, sizeof(u.post)) == 0);
            CHECK(memcmp(&u.nis_sum, &v.nis_sum, sizeof(double)) == 0 && u.n_upd == v.n_upd && u.n_new == v.n_new && u.n_fin == v.n_fin);
        } else if (want_flags == 0) {
            int spikes = 0;
            for (int l = 0; l < k; ++l) spikes += verdict[l] != kGateNone && msg[3 * l + 1] > 5.0f;   // (clean ranges are below 3.02 m, a spike adds 10 m)
            CHECK(n_rej == spikes);
        }
    }
}

int main() {
    for (int f32 = 0; f32 < 2; ++f32)
        for (int L_max = 20; L_max <= 50; L_max += 30) {
            const State st = make_state(5), big = make_state(kInnovMaxLm + 1), nearly = make_state(L_max - 1), none = make_state(0);
            std::vector<float> m;
            run(st, L_max, 0, m, 0, f32);                                                              // k = 0
            detection(st, 2, 0, false, m); run(st, L_max, 0, m, 0, f32);                               // k = 1
            m.clear(); detection(st, 2, 0, true, m); run(st, L_max, 0, m, 0, f32);
            m.clear(); detection(st, 0, 0, true, m); detection(st, 1, 0, false, m); detection(st, 2, 0, false, m); run(st, L_max, 0, m, 0, f32);
            m.clear(); detection(st, 0, 0, false, m); detection(st, 1, 0, false, m); detection(st, 2, 0, true, m); run(st, L_max, 0, m, 0, f32);
            m.clear(); for (int j = 0; j < 3; ++j) detection(st, j, 0, true, m); run(st, L_max, 0, m, 0, f32);
            m.clear(); detection(st, 1, 0, true, m); detection(st, 1, 0, false, m); run(st, L_max, 0, m, 0, f32);
            m.clear(); detection(nearly, 0, 0, true, m); detection(nearly, -1, 7, false, m); detection(nearly, 1, 0, false, m);
            detection(nearly, -1, 8, false, m); detection(nearly, 2, 0, true, m); detection(nearly, -1, 8, false, m); run(nearly, L_max, 0, m, 0, f32);
            m.clear(); for (int l = 0; l < kInnovMaxDet; ++l) detection(big, l % 8, 0, l % 5 == 2, m); run(big, L_max, 0, m, 0, f32);
            detection(big, 0, 0, true, m); run(big, L_max, 0, m, kInnovTooLong, f32);                   // 65 detections
            m.clear(); for (int j = 0; j < kInnovMaxLm; ++j) detection(big, j, 0, j == 3, m); run(big, L_max, 0, m, 0, f32);
            detection(big, kInnovMaxLm, 0, false, m); run(big, L_max, 0, m, kInnovTooLong, f32);        // 17 distinct landmarks
            m.clear(); detection(st, 0, 0, true, m); detection(st, -1, 7, false, m); detection(st, -1, 7, false, m); run(st, L_max, 0, m, kInnovWouldFreeze, f32);
            m.clear(); detection(st, 2, 0, true, m); run(st, L_max, kInnovStatusFrozen, m, kInnovFrozen, f32);
            m.clear(); detection(none, -1, 3, false, m); detection(none, -1, 4, false, m); run(none, L_max, 0, m, 0, f32);
        }
    printf(failures ? "%d check(s) failed\n" : "gate host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_function_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "gate_host.cpp"
    exe = tmp_path / "gate_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "gate host driver ok: 60 cases" in out.stdout, out.stdout + out.stderr
