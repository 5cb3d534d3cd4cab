"""The map score's per-instance function (live_ekf_slam_amd/csrc/score_kernel.h: the source the kernel compiles) in a stand-alone host
program built with AddressSanitizer + UndefinedBehaviorSanitizer: M = 0, 1 and L_max slots against maps of 1, L_max - 1 and L_max + 7 rows,
in both storage types and with a finite and an infinite radius, and the edge cases of the definition (ties between rows and between
slots, three claimants, d2 at the bound and one ulp above it, NaN and inf coordinates, a 2 x 2 block that is not PD, a failed status) -
on heap arrays of EXACTLY the sizes the interface states (x [3 + 2 M], P [n][n], truth [3], map [L][2], the workspace and the list [M], the
per-slot outputs [L_max]), so any read or write outside them is reported.  The program also checks the bookkeeping: the roles add up to M,
no true row is MATCHED twice, every DUPLICATE has a MATCHED slot of its row that is not farther, the list is the MATCHED slots in order."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "score_kernel.h"
using namespace slam;

static int failures = 0, g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static double uni() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return (double)(g_s >> 11) / 9007199254740992.0; }

struct State { std::vector<double> x, P, map; int M, L; int32_t status; };
static State make_state(int M, int L) {
    State s; s.M = M; s.L = L; s.status = 0; const int n = 3 + 2 * M;
    s.x.assign(n, 0.0); s.P.assign((size_t)n * n, 0.0); s.map.resize((size_t)2 * L);
    for (int r = 0; r < L; ++r) { s.map[2 * r] = 4.0 * (r % 8); s.map[2 * r + 1] = 4.0 * (r / 8); }
    s.x[0] = 0.3; s.x[1] = -0.2; s.x[2] = 0.4;
    for (int j = 0; j < M; ++j) {
        const int r = (int)(uni() * L) % L;
        s.x[3 + 2 * j] = s.map[2 * r] + 0.6 * (uni() - 0.5); s.x[4 + 2 * j] = s.map[2 * r + 1] + 0.6 * (uni() - 0.5);
    }
    for (int i = 0; i < n; ++i)
        for (int j = 0; j <= i; ++j) {
            const double v = (i == j ? 1e-2 : 1e-3 * (uni() - 0.5));
            s.P[(size_t)i * n + j] = v; s.P[(size_t)j * n + i] = v + (i == j ? 0.0 : 1e-13);
        }
    return s;
}
static void place(State& s, int j, int r, double ox, double oy) { s.x[3 + 2 * j] = s.map[2 * r] + ox; s.x[4 + 2 * j] = s.map[2 * r + 1] + oy; }

struct Out { ScoreResult v; std::vector<int32_t> row, role, sel, sel_row; std::vector<double> err, nees; };
static Out run(const State& s, int L_max, double radius, bool f32) {
    g_case += 1;
    const int n = 3 + 2 * s.M;
    const double truth_[3] = {0.29, -0.21, 0.41 + 4.0 * 3.14159265358979323846};
    std::vector<double> truth(truth_, truth_ + 3);
    // heap blocks of exactly the stated sizes
    Out o;
    o.row.assign(L_max, -7); o.role.assign(L_max, -7); o.err.assign(L_max, -7.0); o.nees.assign(L_max, -7.0);
    o.sel.assign(s.M, -7); o.sel_row.assign(s.M, -7);
    std::vector<int32_t> ws_row(s.M), ws_role(s.M);
    std::vector<double> ws_d2(s.M), ws_nees(s.M);
    const double* x = s.x.data(); const double* P = s.P.data();
    auto lx = [&](int i) { return f32 ? (double)(float)x[i] : x[i]; };
    auto lp = [&](int r, int c) { const double e = P[(size_t)r * n + c]; return f32 ? (double)(float)e : e; };
    o.v = score_instance(ScoreSeq(), lx, lp, s.M, L_max, s.status, truth.data(), s.map.data(), s.L, radius * radius, 0.05, 7.4, ws_row.data(),
                         ws_role.data(), ws_d2.data(), ws_nees.data(), o.row.data(), o.role.data(), o.err.data(), o.nees.data(), o.sel.data(),
                         o.sel_row.data());
    const ScoreResult& v = o.v;
    if (v.flags & kScoreFailed) {
        CHECK(v.flags == kScoreFailed && v.n_matched == 0 && v.n_duplicate == 0 && v.n_spurious == 0 && isnan(v.map_rms) && isnan(v.max_err));
        for (int j = 0; j < L_max; ++j) CHECK(o.row[j] == -1 && o.role[j] == kScoreNone && isnan(o.err[j]) && isnan(o.nees[j]));
        return o;
    }
    CHECK(v.n_matched + v.n_duplicate + v.n_spurious == s.M);
    int nm = 0;
    for (int j = 0; j < L_max; ++j) {
        if (j >= s.M) { CHECK(o.role[j] == kScoreNone && o.row[j] == -1 && isnan(o.err[j]) && isnan(o.nees[j])); continue; }
        CHECK(o.role[j] >= kScoreMatched && o.role[j] <= kScoreSpurious);
        CHECK((o.role[j] == kScoreSpurious) == (o.row[j] == -1) && o.row[j] < s.L);
        if (o.role[j] == kScoreSpurious) { CHECK(isnan(o.err[j]) && isnan(o.nees[j])); continue; }
        CHECK(o.err[j] >= 0.0 && o.err[j] <= radius);
        if (o.role[j] == kScoreMatched) {
            CHECK(nm < s.M && o.sel[nm] == j && o.sel_row[nm] == o.row[j]);
            nm += 1;
            for (int k = 0; k < s.M; ++k) CHECK(k == j || o.row[k] != o.row[j] || o.role[k] == kScoreDuplicate);
            CHECK(o.err[j] <= v.max_err);
        } else {
            bool owner = false;
            for (int k = 0; k < s.M; ++k)
                owner = owner || (o.role[k] == kScoreMatched && o.row[k] == o.row[j] && (o.err[k] < o.err[j] || (o.err[k] == o.err[j] && k < j)));
            CHECK(owner);
        }
    }
    CHECK(nm == v.n_matched && (nm > 0 || (v.map_rms == 0.0 && v.max_err == 0.0)) && v.map_rms <= v.max_err && v.lm_n <= nm);
    return o;
}

int main() {
    const double two = ldexp(1.0, -25);
    for (int f32 = 0; f32 < 2; ++f32)
        for (int L_max = 9; L_max <= 70; L_max += 61) {          // below and above one pass of 64 slots
            const int Ms[3] = {0, 1, L_max}, Ls[3] = {1, L_max - 1, L_max + 7};
            for (int a = 0; a < 3; ++a)
                for (int b = 0; b < 3; ++b) {
                    const State s = make_state(Ms[a], Ls[b]);
                    run(s, L_max, 2.5, f32); run(s, L_max, INFINITY, f32);
                }
            State s = make_state(9, L_max + 7);
            place(s, 1, 2, 2.0, 0.0); place(s, 3, 8, 0.0, -2.0);             // ties between two true rows
            place(s, 0, 5, 0.25, 0.0); place(s, 4, 5, -0.25, 0.0);           // a tie between two slots
            place(s, 2, 6, 0.75, 0.0); place(s, 5, 6, 0.0, 0.25); place(s, 8, 6, 0.5, 0.0);   // three claimants
            place(s, 6, 10, 0.1, 0.1); place(s, 7, 11, 0.1, 0.1);
            Out o = run(s, L_max, 2.5, f32);
            CHECK(o.row[1] == 2 && o.row[3] == 0 && o.err[1] == 2.0);
            CHECK(o.role[0] == kScoreMatched && o.role[4] == kScoreDuplicate && o.err[0] == 0.25 && o.err[4] == 0.25);
            CHECK(o.role[2] == kScoreDuplicate && o.role[5] == kScoreMatched && o.role[8] == kScoreDuplicate);
            s = make_state(4, L_max + 7);
            place(s, 0, 8, -2.5, 0.0); place(s, 2, 0, -2.5, two);            // d2 at the bound, and the next double above it
            place(s, 1, 3, 0.1, 0.1); place(s, 3, 4, 0.1, 0.1);
            o = run(s, L_max, 2.5, f32);
            CHECK(o.role[0] == kScoreMatched && o.row[0] == 8 && o.err[0] == 2.5 && o.role[2] == kScoreSpurious);
            o = run(s, L_max, INFINITY, f32);
            CHECK(o.row[2] == 0 && o.role[2] != kScoreSpurious && o.err[2] >= 2.5);   // (the square root rounds back to 2.5)
            s = make_state(6, L_max - 1);
            s.x[3] = NAN; s.x[8] = INFINITY; s.x[13] = -INFINITY; s.x[14] = NAN;   // slots 0, 2 and 5
            o = run(s, L_max, INFINITY, f32);
            CHECK(o.v.flags == 0 && o.v.n_spurious == 3 && o.role[0] == kScoreSpurious && o.role[2] == kScoreSpurious && o.role[5] == kScoreSpurious);
            s = make_state(5, L_max);
            s.P[(size_t)5 * 13 + 5] = -1e-3; s.P[(size_t)10 * 13 + 10] = 0.0; s.P[(size_t)11 * 13 + 11] = INFINITY;   // slots 1, 3 and 4
            o = run(s, L_max, INFINITY, f32);
            CHECK(o.v.flags == kScoreLmNotPd && isnan(o.nees[1]) && isnan(o.nees[3]) && isnan(o.nees[4]) && o.nees[0] >= 0.0 && o.nees[2] >= 0.0);
            s = make_state(3, L_max); s.status = 1; run(s, L_max, 2.5, f32);
            s.status = 32; run(s, L_max, 2.5, f32);
            s.status = 2 | 4 | 8; o = run(s, L_max, 2.5, f32); CHECK(o.v.flags == 0);
            s.status = 0; s.x[2] = NAN; o = run(s, L_max, 2.5, f32); CHECK(o.v.flags == kScoreFailed);
        }
    printf(failures ? "%d check(s) failed\n" : "score host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_function_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "score_host.cpp"
    exe = tmp_path / "score_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "score host driver ok: 108 cases" in out.stdout, out.stdout + out.stderr
