"""The joint association's per-instance function (live_ekf_slam_amd/csrc/joint_kernel.h: the source the kernel compiles) in a stand-alone
host program built with AddressSanitizer + UndefinedBehaviorSanitizer, on heap arrays of EXACTLY the sizes the interface states (x, P,
ids, the message row of k_stride triplets, the cost matrix of k x M, 64 verdicts, slots and candidate counts, 64 x 4 det values), so any
read or write outside them is reported: M = 0, k = 0, 64 and 65 detections, a frozen status, in place, fp32 storage, a budget that ends
inside and right after the first dive, more than 16 associable detections, a singular joint S, and wide gates on a map of 66 landmarks
(several candidates per detection, the candidate table, deep branches).  The program also checks the bookkeeping: count_out = matched +
new, the counts add up to k, at most 16 matches, no landmark twice, the labelled rows carry the detection's r and b, the tail is zero."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "joint_kernel.h"
using namespace slam;

static int failures = 0;
static int g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static double uni() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (double)(g_s >> 11) / 9007199254740992.0; }
static const double GJ[16] = {9.210340371976182, 13.276704135987625, 16.81189382977093, 20.090235029663233, 23.20925115895436, 26.21696730553585,
                              29.141237740672796, 31.99992690881518, 34.80530573470507, 37.56623478662505, 40.289360437593864, 42.97982013935164,
                              45.64168266628315, 48.2782357703155, 50.89218131151709, 53.485771836235365};

struct State { std::vector<double> x, P; std::vector<int32_t> ids; int M; };
static State make_state(int M, double diag, double yaw_var) {
    State s; s.M = M; const int n = 3 + 2 * M;
    s.x.assign(n, 0.0); s.P.assign((size_t)n * n, 0.0); s.ids.resize(M);
    s.x[0] = 0.3; s.x[1] = -0.2; s.x[2] = 0.4;
    for (int j = 0; j < M; ++j) {
        const double r = 1.5 + 1.0 * (j / 5), b = -1.0 + 0.5 * (j % 5);
        s.x[3 + 2 * j] = s.x[0] + r * cos(s.x[2] + b); s.x[4 + 2 * j] = s.x[1] + r * sin(s.x[2] + b);
        s.ids[j] = 100 + j;
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = (i == j ? diag : 0.05 * diag * (uni() - 0.5));
            s.P[(size_t)i * n + j] = v; s.P[(size_t)j * n + i] = v;
        }
    if (yaw_var >= 0.0) s.P[(size_t)2 * n + 2] = yaw_var;
    return s;
}
static void clean(const State& s, int slot, std::vector<float>& m, double shift = 0.0) {
    const double dx = s.x[3 + 2 * slot] - s.x[0], dy = s.x[4 + 2 * slot] - s.x[1];
    m.push_back(NAN); m.push_back((float)(sqrt(dx * dx + dy * dy) + 0.02 * (uni() - 0.5)));
    m.push_back((float)(remainder(atan2(dy, dx) - s.x[2], 6.283185307179586) + 0.02 * (uni() - 0.5) + shift));
}
static void fresh(int cell, std::vector<float>& m) {
    m.push_back(-1.0f); m.push_back((float)(2.0 + 1.0 * (cell / 5))); m.push_back((float)(-0.75 + 0.5 * (cell % 5)));
}

struct Want { int32_t flags_all, flags_any; int match, fresh, max_nodes; double gate_match, gate_new; InnovNoise nz; };

static JointResult run(const State& s, int L_max, int32_t status, const std::vector<float>& msg, bool f32, const Want& wt) {
    g_case += 1;
    JointResult last;
    memset(&last, 0, sizeof(last));
    const int k = (int)msg.size() / 3, n = 3 + 2 * s.M;
    const double* x = s.x.data(); const double* P = s.P.data();
    auto lx = [&](int i) { return f32 ? (double)(float)x[i] : x[i]; };
    auto lp = [&](int r, int c) { const double e = P[(size_t)r * n + c]; return f32 ? (double)(float)e : e; };
    for (int pass = 0; pass < 2; ++pass) {            // separate output; in place
        std::vector<float> row(msg), out(msg.size());
        std::vector<double> cost((size_t)(k <= kInnovMaxDet ? k : 0) * s.M), det((size_t)kInnovMaxDet * kAssocDetLen), gj(GJ, GJ + 16);
        std::vector<int32_t> verdict(kInnovMaxDet), slot(kInnovMaxDet), ncand(kInnovMaxDet);
        std::vector<JointWork> ws(1);
        float* const o = pass == 1 ? row.data() : out.data();
        int32_t count_out = -1;
        const JointResult v = joint_instance_host(ws[0], lx, lp, s.M ? s.ids.data() : nullptr, s.M, L_max, status, 0.01f, 0.004f,
                                                  k ? row.data() : nullptr, k, k > 0 ? k : 1, wt.nz, wt.gate_match, wt.gate_new, gj.data(), wt.max_nodes,
                                                  cost.empty() ? nullptr : cost.data(), verdict.data(), slot.data(), det.data(), ncand.data(),
                                                  k ? o : nullptr, &count_out);
        last = v;
        CHECK((v.flags & wt.flags_all) == wt.flags_all && (v.flags & ~(wt.flags_all | wt.flags_any)) == 0);
        double rec[kInnovRecLen];
        joint_record(v, rec);
        if (v.flags & (kInnovFrozen | kInnovTooLong)) {
            CHECK(count_out == 0 && v.n_match == 0 && v.n_new == 0 && v.n_drop == 0 && rec[kJntEval] == 0.0 && v.nodes == 0);
            for (int l = 0; l < kInnovMaxDet; ++l) CHECK(verdict[l] == kAssocNone && slot[l] == -1 && ncand[l] == 0);
            for (int i = 0; i < 3 * k; ++i) CHECK(o[i] == 0.0f);
            continue;
        }
        CHECK(count_out == v.n_match + v.n_new && v.n_match + v.n_new + v.n_drop == k && rec[kJntDetIn] == (double)k);
        CHECK(v.n_match <= kJointMaxPair && v.nodes <= wt.max_nodes && v.nodes >= v.n_match && v.d2_joint >= 0.0 && rec[kJntNodes] == (double)v.nodes);
        if (wt.match >= 0) CHECK(v.n_match == wt.match && v.n_new == wt.fresh);
        int kept = 0;
        std::vector<int> used(s.M + 1, 0);
        for (int l = 0; l < kInnovMaxDet; ++l) {
            CHECK(l < k ? verdict[l] != kAssocNone : (verdict[l] == kAssocNone && slot[l] == -1 && ncand[l] == 0));
            CHECK(slot[l] >= -1 && slot[l] < s.M && ncand[l] >= 0 && ncand[l] <= kJointMaxCand);
            if (l < k && verdict[l] == kAssocJointUnpaired) CHECK(ncand[l] > 0);
            if (l < k && (verdict[l] == kAssocMatched || verdict[l] == kAssocNew)) {
                CHECK(memcmp(o + 3 * kept + 1, msg.data() + 3 * l + 1, 2 * sizeof(float)) == 0);
                if (verdict[l] == kAssocMatched) { CHECK(o[3 * kept] == (float)s.ids[slot[l]] && ncand[l] > 0); CHECK(used[slot[l]]++ == 0); }
                else CHECK(o[3 * kept] >= 0.0f && o[3 * kept] < 16777216.0f);
                kept += 1;
            }
        }
        CHECK(kept == count_out);
        for (int i = 3 * kept; i < 3 * k; ++i) CHECK(o[i] == 0.0f);
    }
    return last;
}

int main() {
    const InnovNoise nz = {0.f, 0.f, 0.f, 0.f, 1e-4, 1e-4, 2.5e-3, 2.5e-3};
    const InnovNoise w0 = {0.f, 0.f, 0.f, 0.f, 0.0, 0.0, 1e-4, 0.0};
    const Want def = {0, 0, -1, -1, 2048, 9.210340371976182, 27.631021115928547, nz};
    for (int f32 = 0; f32 < 2; ++f32) {
        const State st = make_state(18, 4e-4, -1.0), none = make_state(0, 4e-4, -1.0), wrap = make_state(66, 4e-4, -1.0);
        std::vector<float> m;
        Want w = def;
        w.match = 0; w.fresh = 0; run(st, 20, 0, m, f32, w);                                                // k = 0
        m.clear(); fresh(1, m); fresh(7, m); w.fresh = 2; run(none, 20, 0, m, f32, w);                     // M = 0
        m.clear(); clean(st, 2, m); fresh(1, m); clean(st, 5, m); w.match = 2; w.fresh = 1; run(st, 20, 0, m, f32, w);
        m.clear(); for (int j = 17; j >= 0; --j) clean(st, j, m);                                           // 18 associable detections
        w = def; w.flags_any = kJointBudget; w.match = 16; w.fresh = 0; run(st, 20, 0, m, f32, w);
        w.max_nodes = 16; w.flags_all = kJointBudget; run(st, 20, 0, m, f32, w);                            // right after the first dive
        w.max_nodes = 5; w.match = 5; run(st, 20, 0, m, f32, w);                                            // inside the first dive
        m.clear(); for (int l = 0; l < kInnovMaxDet; ++l) clean(wrap, 65 - l, m);                           // 64 detections, two groups of landmarks
        w = def; w.flags_any = kJointBudget; w.match = 16; w.fresh = 0; run(wrap, 70, 0, m, f32, w);
        w.gate_match = 400.0; w.gate_new = 1e4; w.match = -1; w.max_nodes = 300;                            // wide gates: several candidates each,
        w.flags_any = kJointBudget | kJointLmTable;                                                        // more than 64 candidate landmarks
        const JointResult wide = run(wrap, 70, 0, m, f32, w);
        CHECK(wide.nodes > wide.n_match && (wide.flags & kJointLmTable));                                   // 66 candidate landmarks: the table is full
        clean(wrap, 0, m); w = def; w.flags_all = kInnovTooLong; run(wrap, 70, 0, m, f32, w);               // 65 detections
        m.clear(); clean(st, 2, m); fresh(1, m); w = def; w.flags_all = kInnovFrozen; run(st, 20, kInnovStatusFrozen, m, f32, w);
        // a singular joint S: the yaw variance alone, W_11 = 0
        State yaw = make_state(6, 0.0, 0.0625);
        for (size_t i = 0; i < yaw.P.size(); ++i) yaw.P[i] = 0.0;
        yaw.P[(size_t)2 * (3 + 2 * 6) + 2] = 0.0625;
        m.clear();
        for (int j = 0; j < 3; ++j) {
            const double dx = yaw.x[3 + 2 * j] - yaw.x[0], dy = yaw.x[4 + 2 * j] - yaw.x[1];
            m.push_back(0.f); m.push_back((float)sqrt(dx * dx + dy * dy)); m.push_back((float)(remainder(atan2(dy, dx) - yaw.x[2], 6.283185307179586) + 0.01));
        }
        w = def; w.nz = w0; w.flags_all = kJointSingular; w.match = 1; w.fresh = 0;
        run(yaw, 8, 0, m, f32, w);
    }
    printf(failures ? "%d check(s) failed\n" : "joint host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_function_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "joint_host.cpp"
    exe = tmp_path / "joint_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "joint host driver ok: 22 cases" in out.stdout, out.stdout + out.stderr
