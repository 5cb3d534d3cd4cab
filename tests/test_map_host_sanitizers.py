"""The per-instance functions of map management (live_ekf_slam_amd/csrc/map_kernel.h: the source the kernels compile) in a stand-alone
host program built with AddressSanitizer + UndefinedBehaviorSanitizer: the removal sets none / slot 0 / the last slot / all / alternating /
a single survivor at M = 0, 1, 7, L_max - 1 and L_max, L_max 20, 50 and 66, both element sizes, with and without counters; the tally on
messages of k = 0, 1, 64, 65 and 130 detections with NaN, infinite and out-of-range ids, a negative count and a count beyond the row - on
heap arrays of EXACTLY the sizes the interface states (the slab of n rows at the padded leading dimension, x of n, ids and counters of
L_max, the kept table of M, the message row of k_stride triplets, the id block of 64), so any read or write outside them is reported.  The
program checks the result too, against an out-of-place copy: sub-matrix, zero pads, zeroed tails, counters that follow their slots."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "map_kernel.h"
using namespace slam;

static int failures = 0;
static int g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static unsigned long long rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

template <class T>
static void removal(int M, int L_max, int kind, bool counters) {
    g_case += 1;
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(T));
    // heap blocks of exactly the stated sizes
    std::vector<T> P((size_t)n * ld), x((size_t)n);
    std::vector<int32_t> ids((size_t)L_max), seen, expected, mask((size_t)(M ? M : 1));
    std::vector<uint16_t> kept((size_t)(M ? M : 1));
    if (counters) { seen.resize(L_max); expected.resize(L_max); }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < ld; ++c) P[(size_t)r * ld + c] = c < n ? (T)(1 + r * 4096 + c) : (T)0;
    for (int i = 0; i < n; ++i) x[i] = (T)(900000 + i);
    for (int j = 0; j < L_max; ++j) {
        ids[j] = j < M ? 100 + j : 77;                      // (garbage beyond M: it is zeroed when the instance is touched)
        if (counters) { seen[j] = 1000 + j; expected[j] = 2000 + j; }
    }
    for (int j = 0; j < M; ++j)
        mask[j] = kind == 0 ? 0 : kind == 1 ? j == 0 : kind == 2 ? j == M - 1 : kind == 3 ? 1 : kind == 4 ? (j % 2 == 0) : kind == 5 ? j != M / 2
                                                                                                                        : (int)(rnd() & 1);
    const std::vector<T> P0(P), x0(x);
    const std::vector<int32_t> ids0(ids), seen0(seen), expected0(expected);
    const int Mk = map_remove_instance_host(P.data(), x.data(), ids.data(), counters ? seen.data() : nullptr,
                                            counters ? expected.data() : nullptr, mask.data(), M, L_max, kept.data());
    int want = 0;
    std::vector<int> old;                                    // new state index -> old state index
    for (int i = 0; i < 3; ++i) old.push_back(i);
    for (int j = 0; j < M; ++j)
        if (!mask[j]) { old.push_back(3 + 2 * j); old.push_back(4 + 2 * j); want += 1; }
    CHECK(Mk == want);
    if (Mk == M) {                                           // untouched: not a byte written
        CHECK(P == P0 && x == x0 && ids == ids0 && seen == seen0 && expected == expected0);
        return;
    }
    const int n2 = 3 + 2 * Mk, ld2 = map_ld(n2, (int)sizeof(T));
    for (int r = 0; r < n2; ++r)
        for (int c = 0; c < ld2; ++c) CHECK(P[(size_t)r * ld2 + c] == (c < n2 ? P0[(size_t)old[r] * ld + old[c]] : (T)0));
    for (size_t i = (size_t)n2 * ld2; i < P.size(); ++i) CHECK(P[i] == P0[i]);   // (beyond the new matrix nothing is written)
    for (int i = 0; i < n2; ++i) CHECK(x[i] == x0[old[i]]);
    int p = 0;
    for (int j = 0; j < M; ++j)
        if (!mask[j]) {
            CHECK(ids[p] == ids0[j]);
            if (counters) CHECK(seen[p] == seen0[j] && expected[p] == expected0[j]);
            p += 1;
        }
    for (int j = Mk; j < L_max; ++j) {
        CHECK(ids[j] == 0);
        if (counters) CHECK(seen[j] == 0 && expected[j] == 0);
    }
}

static void tally(int M, int L_max, int k, int count, int k_stride, bool f32) {
    g_case += 1;
    const int n = 3 + 2 * M;
    std::vector<double> x((size_t)n);
    std::vector<int32_t> ids((size_t)(M ? M : 1)), seen((size_t)L_max, 5), expected((size_t)L_max, 9), idbuf(kMapIdBlock);
    std::vector<uint8_t> okbuf(kMapIdBlock);
    std::vector<float> meas((size_t)3 * k_stride);
    x[0] = 0.3; x[1] = -0.2; x[2] = 0.4;
    for (int j = 0; j < M; ++j) {
        const double r = 0.5 + 3.0 * uni(), b = -1.9 + 3.8 * uni();
        x[3 + 2 * j] = x[0] + r * cos(x[2] + b); x[4 + 2 * j] = x[1] + r * sin(x[2] + b);
        ids[j] = 100 + j;
    }
    const float odd[] = {NAN, INFINITY, -INFINITY, 3e9f, -3e9f, -2147483648.0f, 2147483648.0f, 7.0f, 99.5f};
    for (int l = 0; l < k_stride; ++l) {
        meas[3 * l] = (M && (rnd() & 1)) ? (float)ids[rnd() % M] : odd[rnd() % 9];
        meas[3 * l + 1] = 1.0f; meas[3 * l + 2] = 0.1f;
    }
    int kk = count < k_stride ? count : k_stride;
    kk = kk < 0 ? 0 : kk;
    CHECK(kk == (k < 0 ? 0 : k));
    std::vector<int> hit((size_t)(M ? M : 1), 0);
    for (int l = 0; l < kk; ++l)
        for (int j = 0; j < M; ++j)
            if (meas[3 * l] == (float)ids[j]) hit[j] = 1;
    const double* xp = x.data();
    map_tally_instance(MapSeq(), [&](int i) { return f32 ? (double)(float)xp[i] : xp[i]; }, M ? ids.data() : nullptr, M,
                       meas.data(), kk, idbuf.data(), okbuf.data(), 2.7, -1.47, 1.47, seen.data(), expected.data());
    for (int j = 0; j < L_max; ++j) {
        if (j >= M) { CHECK(seen[j] == 5 && expected[j] == 9); continue; }
        CHECK(seen[j] == 5 + hit[j]);
        CHECK(expected[j] == 9 + hit[j] || (!hit[j] && expected[j] == 10));
    }
    bool ok;
    CHECK(map_message_id(-2147483648.0f, &ok) == (-2147483647 - 1) && ok);
    (void)map_message_id(2147483648.0f, &ok); CHECK(!ok);
    (void)map_message_id(NAN, &ok); CHECK(!ok);
}

int main() {
    const int Ls[3] = {20, 50, 66};
    for (int li = 0; li < 3; ++li) {
        const int L_max = Ls[li];
        const int Ms[5] = {0, 1, 7, L_max - 1, L_max};
        for (int mi = 0; mi < 5; ++mi)
            for (int kind = 0; kind < 8; ++kind)
                for (int counters = 0; counters < 2; ++counters) {
                    removal<uint64_t>(Ms[mi], L_max, kind, counters != 0);
                    removal<uint32_t>(Ms[mi], L_max, kind, counters != 0);
                }
        const int ks[5] = {0, 1, 64, 65, 130};
        for (int mi = 0; mi < 5; ++mi)
            for (int ki = 0; ki < 5; ++ki)
                for (int f32 = 0; f32 < 2; ++f32) tally(Ms[mi], L_max, ks[ki], ks[ki], ks[ki] ? ks[ki] : 1, f32 != 0);
        tally(7, L_max, -1, -4, 3, false);                  // a negative count: an empty message
        tally(7, L_max, 3, 9, 3, false);                    // a count beyond the row: clamped to k_stride
    }
    CHECK(map_prune_decide(2, 10, 10, 0.3) && !map_prune_decide(3, 10, 10, 0.3) && !map_prune_decide(0, 9, 10, 0.3) && !map_prune_decide(0, 10, 10, 0.0));
    const MapTraffic t0 = map_traffic(50, 0, 50, 8, false, false), t1 = map_traffic(50, 1, 50, 8, false, false);
    CHECK(t0.moved == 0 && t0.pads == 0 && t0.other_bytes == 4 + 200 + 4 && t1.moved == 101ull * 101ull && t1.pads == 101);
    printf(failures ? "%d check(s) failed\n" : "map host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_functions_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "map_host.cpp"
    exe = tmp_path / "map_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "map host driver ok: 636 cases" in out.stdout, out.stdout + out.stderr
