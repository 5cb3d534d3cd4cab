"""The per-instance functions of the position / heading fix (live_ekf_slam_amd/csrc/fix_kernel.h: the source the kernels compile) in a
stand-alone host program built with AddressSanitizer + UndefinedBehaviorSanitizer: M = 0, 1, 2, 7, L_max - 1 and L_max for L_max 20, 50
and 66, both storage types, every combination of kinds, accepted / rejected / singular / invalid parts - on heap arrays of EXACTLY the
sizes the interface states (the slab of n rows at the padded leading dimension map_ld, x of n, the workspace of fix_ws_len(n) = 6 n + 3),
so any read or write outside them is reported.  The program checks the result too: the two sequential passes (the host hook's form)
against an out-of-place dense evaluation of the same updates, and the ONE-PASS form the device kernel compiles against the sequential
one IN BITS.  No Python process is involved in the run."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "fix_kernel.h"
using namespace slam;

static int failures = 0;
static int g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static unsigned long long rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// an SPD state of M landmarks, not exactly symmetric after the rounding of an asymmetric perturbation
template <class ST>
static void make_state(int M, std::vector<ST>& P, std::vector<ST>& x) {
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(ST));
    std::vector<double> A((size_t)n * n);
    for (auto& v : A) v = (uni() - 0.5) * 0.02;
    P.assign((size_t)n * ld, (ST)0); x.resize((size_t)n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            double acc = r == c ? 1.6e-5 : 0.0;
            for (int k = 0; k < n; ++k) acc += A[(size_t)r * n + k] * A[(size_t)c * n + k];
            P[(size_t)r * ld + c] = (ST)(acc * (1.0 + 1e-9 * (r - c)));
        }
    for (int i = 0; i < n; ++i) x[i] = (ST)(i < 3 ? 0.4 * i - 0.3 : 0.5 * (i / 2) + 0.37 * (i & 1));
}

template <class ST>
static bool same_bits(const std::vector<ST>& a, const std::vector<ST>& b) { return a.size() == b.size() && (a.empty() || memcmp(a.data(), b.data(), sizeof(ST) * a.size()) == 0); }

// how: 0 a fix near the estimate (accepted), 1 a far position (rejected), 2 a far heading (rejected), 3 sigma NaN (invalid), 4 negative
// sigma (invalid), 5 a zero position block with sigma 0 (singular)
template <class ST>
static void fix_case(int M, int kinds, int how) {
    g_case += 1;
    std::vector<ST> P, x;
    make_state<ST>(M, P, x);
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(ST));
    double row[5] = {(double)x[0] + 0.03, (double)x[1] - 0.02, (double)x[2] + 0.01, 0.05, 0.02};
    if (how == 1) row[0] += 50.0;
    if (how == 2) row[2] += 2.0;
    if (how == 3) { row[3] = NAN; row[4] = INFINITY; }
    if (how == 4) { row[3] = -0.1; row[4] = -1e-300; }
    if (how == 5) {
        row[3] = 0.0;
        for (int a = 0; a < 2; ++a) for (int c = 0; c < n; ++c) { P[(size_t)a * ld + c] = (ST)0; P[(size_t)c * ld + a] = (ST)0; }
    }
    const double gates[2] = {13.815510557964274, 10.827566170662733};
    const std::vector<ST> P0(P), x0(x);
    std::vector<double> ws((size_t)fix_ws_len(n));             // exactly 6 n + 3
    std::vector<ST> P1(P0), x1(x0);
    const FixResult o = fix_instance<false>(MapSeq(), P.data(), x.data(), M, row, kinds, gates, ws.data());
    std::vector<double> ws1((size_t)fix_ws_len(n));
    const FixResult o1 = fix_instance<true>(MapSeq(), P1.data(), x1.data(), M, row, kinds, gates, ws1.data());
    // the one-pass form equals the two passes in bits
    CHECK(o.verdict == o1.verdict && o.written == o1.written && memcmp(o.nis, o1.nis, sizeof(o.nis)) == 0);
    CHECK(same_bits(P, P1) && same_bits(x, x1));
    const int vp = o.verdict & 15, vy = o.verdict >> 4;
    int wp = (kinds & 1) ? kFixApplied : kFixAbsent, wy = (kinds & 2) ? kFixApplied : kFixAbsent;
    if (how == 1 && wp) wp = kFixRejected;
    if (how == 2 && wy) wy = kFixRejected;
    if ((how == 3 || how == 4) && wp) wp = kFixInvalid;
    if ((how == 3 || how == 4) && wy) wy = kFixInvalid;
    if (how == 5 && wp) wp = kFixSingular;
    CHECK(vp == wp && vy == wy);
    CHECK((o.nis[0] == o.nis[0]) == (vp == kFixApplied || vp == kFixRejected));
    CHECK((o.nis[1] == o.nis[1]) == (vy == kFixApplied || vy == kFixRejected));
    CHECK(o.written == ((vp == kFixApplied || vy == kFixApplied) ? 1 : 0));
    if (!o.written) { CHECK(same_bits(P, P0) && same_bits(x, x0)); return; }
    // the same updates out of place, dense, with the closed-form inverse
    std::vector<ST> Q(P0), y(x0);
    if (vp == kFixApplied) {
        const std::vector<ST> Qi(Q), yi(y);
        const double s2 = row[3] * row[3];
        const double S[4] = {(double)Qi[0] + s2, (double)Qi[1], (double)Qi[ld], (double)Qi[ld + 1] + s2};
        const double det = S[0] * S[3] - S[1] * S[2];
        const double Si[4] = {S[3] / det, -S[1] / det, -S[2] / det, S[0] / det};
        const double nu0 = row[0] - (double)yi[0], nu1 = row[1] - (double)yi[1];
        for (int r = 0; r < n; ++r) {
            const double c0 = (double)Qi[(size_t)r * ld], c1 = (double)Qi[(size_t)r * ld + 1];
            const double k0 = c0 * Si[0] + c1 * Si[2], k1 = c0 * Si[1] + c1 * Si[3];
            for (int c = 0; c < n; ++c) Q[(size_t)r * ld + c] = (ST)((double)Qi[(size_t)r * ld + c] - (k0 * (double)Qi[c] + k1 * (double)Qi[ld + c]));
            double v = (double)yi[r] + (k0 * nu0 + k1 * nu1);
            if (r == 2) v = remainder(v, 2 * 3.14159265358979323846);
            y[r] = (ST)v;
        }
    }
    if (vy == kFixApplied) {
        const std::vector<ST> Qi(Q), yi(y);
        const double S = (double)Qi[(size_t)2 * ld + 2] + row[4] * row[4];
        const double nu = remainder(row[2] - (double)yi[2], 2 * 3.14159265358979323846);
        for (int r = 0; r < n; ++r) {
            const double k = (double)Qi[(size_t)r * ld + 2] / S;
            for (int c = 0; c < n; ++c) Q[(size_t)r * ld + c] = (ST)((double)Qi[(size_t)r * ld + c] - k * (double)Qi[(size_t)2 * ld + c]);
            double v = (double)yi[r] + k * nu;
            if (r == 2) v = remainder(v, 2 * 3.14159265358979323846);
            y[r] = (ST)v;
        }
    }
    const double tol = sizeof(ST) == 4 ? 2e-5 : 1e-9;         // (the closed-form inverse against the LU one, on entries below 1e-2 and x of a few tens)
    for (int r = 0; r < n; ++r) {
        for (int c = 0; c < ld; ++c) {
            if (c >= n) CHECK(P[(size_t)r * ld + c] == (ST)0);   // pad columns stay zero
            else CHECK(fabs((double)P[(size_t)r * ld + c] - (double)Q[(size_t)r * ld + c]) <= tol);
        }
        CHECK(fabs((double)x[r] - (double)y[r]) <= tol * 30.0);
    }
    // a fix pulls the estimate onto the measurement and shrinks the measured variances
    if (vp == kFixApplied) CHECK((double)P[0] < (double)P0[0] && (double)P[ld + 1] < (double)P0[ld + 1]);
    if (vy == kFixApplied) CHECK((double)P[(size_t)2 * ld + 2] < (double)P0[(size_t)2 * ld + 2]);
}

int main() {
    const int Ls[3] = {20, 50, 66};
    for (int li = 0; li < 3; ++li) {
        const int L_max = Ls[li];
        const int Ms[6] = {0, 1, 2, 7, L_max - 1, L_max};
        for (int mi = 0; mi < 6; ++mi)
            for (int kinds = 0; kinds < 4; ++kinds)
                for (int how = 0; how < 6; ++how) { fix_case<double>(Ms[mi], kinds, how); fix_case<float>(Ms[mi], kinds | 4, how); }
    }
    // the source: the all-zero row emits nothing; a full row emits both parts from finite draws
    const slam_fix_sensor off = fix_sensor_default_row();
    const FixSensed e = fix_sense_instance(off, 7ull, 3ull, 11u, 1.0, 2.0, 0.5);
    CHECK(e.kinds == 0 && e.jumped == 0 && e.row[0] == 0.0 && e.row[1] == 0.0 && e.row[2] == 0.0 && e.row[3] == 0.0 && e.row[4] == 0.0);
    slam_fix_sensor on = off;
    on.pos_halfwidth = 0.5; on.yaw_halfwidth = 0.1; on.sigma_pos = 0.3; on.sigma_yaw = 0.06; on.p_jump = 1.0; on.jump_lo = 2.0; on.jump_hi = 3.0; on.kinds = 3;
    CHECK(fix_sensor_bad_field(on) == nullptr && fix_sensor_bad_field(off) == nullptr);
    const FixSensed f = fix_sense_instance(on, 7ull, 3ull, 11u, 1.0, 2.0, 0.5);
    const double jd = sqrt((f.row[0] - 1.0) * (f.row[0] - 1.0) + (f.row[1] - 2.0) * (f.row[1] - 2.0));
    CHECK(f.kinds == 3 && f.jumped == 1 && jd > 2.0 - 0.71 && jd < 3.0 + 0.71 && fabs(f.row[2] - 0.5) <= 0.1 && f.row[3] == 0.3 && f.row[4] == 0.06);
    on.p_miss_pos = 1.0; on.p_miss_yaw = 1.0;
    const FixSensed m = fix_sense_instance(on, 7ull, 3ull, 11u, 1.0, 2.0, 0.5);
    CHECK(m.kinds == 0 && m.jumped == 0 && m.row[0] == 0.0 && m.row[2] == 0.0);
    on.kinds = 4;
    CHECK(fix_sensor_bad_field(on) != nullptr);
    const FixTraffic t0 = fix_traffic(50, 0), t1 = fix_traffic(50, 0x11), t2 = fix_traffic(50, 0x12), t3 = fix_traffic(50, 0x44);
    CHECK(t0.elems == 0 && t3.elems == 0 && t1.elems == 4ull * 103 + 2 + 2ull * 103 + 1 + 2ull * 103 * 103 + 206 && t2.elems == t1.elems && t0.other_bytes == 72);
    printf(failures ? "%d check(s) failed\n" : "fix host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_functions_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "fix_host.cpp"
    exe = tmp_path / "fix_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "fix host driver ok: 864 cases" in out.stdout, out.stdout + out.stderr
