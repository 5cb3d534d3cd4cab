"""The per-instance functions of landmark merging (live_ekf_slam_amd/csrc/merge_kernel.h: the source the kernels compile) in a
stand-alone host program built with AddressSanitizer + UndefinedBehaviorSanitizer: the find at M = 0, 1, 2, 7, L_max - 1 and L_max, the
pair list of partner rows with entries that are negative, beyond M, beyond L_max, self-referring and not mutual, and the fusion of no pair /
the pair (0, M - 1) / neighbouring pairs / floor(M / 2) pairs, L_max 20, 50 and 66, both storage types, with and without counters - on heap
arrays of EXACTLY the sizes the interface states (the slab of n rows at the padded leading dimension, x of n, the workspace of 4 n + 2,
nn and d2 of M, the pair lists of their length, the mask of M, counters of L_max), so any read or write outside them is reported.  The
program checks the result too, against an out-of-place dense evaluation of the same update.  No Python process is involved in the run."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <vector>
#include "merge_kernel.h"
using namespace slam;

static int failures = 0;
static int g_case = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d (case %d): %s\n", __LINE__, g_case, #c); failures += 1; } } while (0)
static unsigned long long g_s = 88172645463325252ull;
static unsigned long long rnd() { g_s ^= g_s << 13; g_s ^= g_s >> 7; g_s ^= g_s << 17; return g_s; }
static double uni() { return (double)(rnd() >> 11) / 9007199254740992.0; }

// an SPD state of M landmarks in which slot dup_of[s] >= 0 is a noisy copy of that slot
template <class ST>
static void make_state(int M, const std::vector<int>& dup_of, std::vector<ST>& P, std::vector<ST>& x) {
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(ST));
    std::vector<double> A((size_t)n * n), D((size_t)n * n, 0.0), xd((size_t)n);
    for (auto& v : A) v = (uni() - 0.5) * 0.02;
    for (int i = 0; i < n; ++i) xd[i] = i < 3 ? 0.1 * i : 0.5 * (i / 2) + 0.37 * (i & 1);
    for (int s = 0; s < M; ++s)
        if (dup_of[s] >= 0)
            for (int a = 0; a < 2; ++a) {
                for (int c = 0; c < n; ++c) A[(size_t)(3 + 2 * s + a) * n + c] = A[(size_t)(3 + 2 * dup_of[s] + a) * n + c];
                xd[3 + 2 * s + a] = xd[3 + 2 * dup_of[s] + a] + 0.002 * (a ? 0.3 : 0.8);
            }
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            double acc = r == c ? 1.6e-5 : 0.0;
            for (int k = 0; k < n; ++k) acc += A[(size_t)r * n + k] * A[(size_t)c * n + k];
            D[(size_t)r * n + c] = acc;
        }
    P.assign((size_t)n * ld, (ST)0); x.resize((size_t)n);
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) P[(size_t)r * ld + c] = (ST)D[(size_t)r * n + c];
    for (int i = 0; i < n; ++i) x[i] = (ST)xd[i];
}

template <class ST>
static void find_case(int M, int L_max, int n_dups) {
    g_case += 1;
    std::vector<int> dup_of((size_t)M, -1);
    for (int k = 0; k < n_dups && 2 * k + 1 < M; ++k) dup_of[M - 1 - k] = k;
    std::vector<ST> P, x;
    make_state<ST>(M, dup_of, P, x);
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(ST));
    std::vector<int32_t> nn((size_t)M);              // (exactly M; M = 0: empty)
    std::vector<double> d2((size_t)M);
    const ST* Pp = P.data(); const ST* xp = x.data();
    merge_find_instance_host([&](int i) { return (double)xp[i]; }, [&](int r, int c) { return (double)Pp[(size_t)r * ld + c]; }, M, 5.99, 0.0,
                             nn.data(), d2.data());
    int dups = 0;
    for (int s = 0; s < M; ++s) {
        CHECK(nn[s] >= -1 && nn[s] < M && nn[s] != s);
        CHECK((nn[s] < 0) == (d2[s] != d2[s]));
        if (dup_of[s] >= 0) { CHECK(nn[s] == dup_of[s] && nn[dup_of[s]] == s && d2[s] == d2[dup_of[s]]); dups += 1; }
    }
    CHECK(dups == (n_dups < M / 2 ? n_dups : M / 2) || M < 2);
}

static void pairs_case(int M, int L_max) {
    g_case += 1;
    std::vector<int32_t> partner((size_t)L_max, -1);
    std::vector<uint16_t> pi((size_t)(M / 2 ? M / 2 : 1)), pj((size_t)(M / 2 ? M / 2 : 1));
    int want = 0, wild = 0;
    for (int s = 0; s + 1 < M; s += 4) { partner[s] = s + 1; partner[s + 1] = s; want += 1; }           // honoured
    const int32_t odd[] = {-2, -2147483647 - 1, 2147483647, L_max, M, 1000, 65536};
    for (int s = 2; s < L_max; s += 4) { partner[s] = (s / 4) % 8 == 7 ? s : odd[(s / 4) % 7]; wild += 1; }   // ignored, never followed
    if (M >= 4) { partner[3] = 0; wild += 1; }                                                           // not mutual
    int ignored = -1;
    const int np = merge_pairs_host(partner.data(), M, L_max, false, pi.data(), pj.data(), &ignored);
    CHECK(np == want && ignored == wild);
    for (int k = 0; k < np; ++k) CHECK(pi[k] == 4 * k && pj[k] == 4 * k + 1);
    CHECK(merge_pairs_host(partner.data(), M, L_max, true, pi.data(), pj.data(), &ignored) == 0 && ignored == wild + 2 * want);
}

template <class ST>
static void fuse_case(int M, int L_max, int kind, bool counters) {
    g_case += 1;
    // kind 0: no pair, 1: (0, M - 1), 2: neighbours (0, 1), (2, 3), 3: floor(M / 2) pairs (k, M - 1 - k), 4: an exact copy (SINGULAR at sigma = 0)
    std::vector<int> dup_of((size_t)M, -1);
    std::vector<uint16_t> pi, pj;
    if (kind == 1 && M >= 2) { dup_of[M - 1] = 0; pi.push_back(0); pj.push_back((uint16_t)(M - 1)); }
    if (kind == 2) for (int s = 0; s + 1 < M && s < 4; s += 2) { dup_of[s + 1] = s; pi.push_back((uint16_t)s); pj.push_back((uint16_t)(s + 1)); }
    if (kind == 3) for (int k = 0; 2 * k + 1 < M; ++k) { dup_of[M - 1 - k] = k; pi.push_back((uint16_t)k); pj.push_back((uint16_t)(M - 1 - k)); }
    if (kind == 4 && M >= 2) { pi.push_back(0); pj.push_back(1); }
    std::vector<ST> P, x;
    make_state<ST>(M, dup_of, P, x);
    const int n = 3 + 2 * M, ld = map_ld(n, (int)sizeof(ST));
    if (kind == 4 && M >= 2) {                               // slot 1 becomes the exact copy of slot 0
        for (int a = 0; a < 2; ++a) {
            for (int c = 0; c < n; ++c) P[(size_t)(5 + a) * ld + c] = P[(size_t)(3 + a) * ld + c];
            x[5 + a] = x[3 + a];
        }
        for (int a = 0; a < 2; ++a)
            for (int r = 0; r < n; ++r) P[(size_t)r * ld + 5 + a] = P[(size_t)r * ld + 3 + a];
    }
    const int np = (int)pi.size();
    std::vector<uint16_t> pie(pi), pje(pj);                  // heap blocks of exactly np entries
    std::vector<double> ws((size_t)4 * n + 2);
    std::vector<int32_t> remove((size_t)(M ? M : 1), 0), seen, expected;
    if (counters) { seen.resize(L_max); expected.resize(L_max); for (int j = 0; j < L_max; ++j) { seen[j] = 3 + j; expected[j] = 5 + 2 * (j % 7); } }
    const std::vector<ST> P0(P), x0(x);
    const std::vector<int32_t> seen0(seen), expected0(expected);
    const MergeCounts cnt = merge_fuse_instance(MapSeq(), P.data(), x.data(), M, pie.data(), pje.data(), np, 0.0, ws.data(), remove.data(),
                                                counters ? seen.data() : nullptr, counters ? expected.data() : nullptr);
    if (kind == 4 && M >= 2) {
        CHECK(cnt.fused == 0 && cnt.singular == 1 && P == P0 && x == x0 && remove[1] == 0 && seen == seen0 && expected == expected0);
        return;
    }
    CHECK(cnt.fused == np && cnt.singular == 0);
    if (np == 0) { CHECK(P == P0 && x == x0); return; }
    // the same updates out of place, dense
    std::vector<ST> Q(P0), y(x0);
    for (int k = 0; k < np; ++k) {
        const int ii = 3 + 2 * pi[k], jj = 3 + 2 * pj[k];
        std::vector<double> c((size_t)2 * n), g((size_t)2 * n);
        for (int r = 0; r < n; ++r) {
            c[2 * r] = (double)Q[(size_t)r * ld + ii] - (double)Q[(size_t)r * ld + jj];
            c[2 * r + 1] = (double)Q[(size_t)r * ld + ii + 1] - (double)Q[(size_t)r * ld + jj + 1];
            g[2 * r] = (double)Q[(size_t)ii * ld + r] - (double)Q[(size_t)jj * ld + r];
            g[2 * r + 1] = (double)Q[(size_t)(ii + 1) * ld + r] - (double)Q[(size_t)(jj + 1) * ld + r];
        }
        const double S[4] = {c[2 * ii] - c[2 * jj], c[2 * ii + 1] - c[2 * jj + 1], c[2 * ii + 2] - c[2 * jj + 2], c[2 * ii + 3] - c[2 * jj + 3]};
        const double det = S[0] * S[3] - S[1] * S[2];
        const double Si[4] = {S[3] / det, -S[1] / det, -S[2] / det, S[0] / det};
        const double d0 = (double)y[ii] - (double)y[jj], d1 = (double)y[ii + 1] - (double)y[jj + 1];
        for (int r = 0; r < n; ++r) {
            const double k0 = c[2 * r] * Si[0] + c[2 * r + 1] * Si[2], k1 = c[2 * r] * Si[1] + c[2 * r + 1] * Si[3];
            for (int cc = 0; cc < n; ++cc) Q[(size_t)r * ld + cc] = (ST)((double)Q[(size_t)r * ld + cc] - (k0 * g[2 * cc] + k1 * g[2 * cc + 1]));
            y[r] = (ST)((double)y[r] - (k0 * d0 + k1 * d1));
        }
    }
    const double tol = sizeof(ST) == 4 ? 2e-5 : 1e-9;         // (the closed-form inverse against the LU one, on entries below 1e-2 and x of a few units)
    for (int r = 0; r < n; ++r) {
        for (int cc = 0; cc < ld; ++cc) {
            if (cc >= n) CHECK(P[(size_t)r * ld + cc] == (ST)0);   // pad columns stay zero
            else CHECK(fabs((double)P[(size_t)r * ld + cc] - (double)Q[(size_t)r * ld + cc]) <= tol * 1e-2);
        }
        CHECK(fabs((double)x[r] - (double)y[r]) <= tol * 30.0);
    }
    for (int k = 0; k < np; ++k) {                              // the copies coincide afterwards and the mask names slot j
        CHECK(fabs((double)x[3 + 2 * pi[k]] - (double)x[3 + 2 * pj[k]]) <= tol * 30.0);
        CHECK(remove[pj[k]] == 1 && remove[pi[k]] == 0);
        if (counters) {
            const int32_t e2 = expected0[pi[k]] > expected0[pj[k]] ? expected0[pi[k]] : expected0[pj[k]];
            const int32_t s2 = seen0[pi[k]] + seen0[pj[k]];
            CHECK(expected[pi[k]] == e2 && seen[pi[k]] == (s2 < e2 ? s2 : e2));
        }
    }
}

int main() {
    const int Ls[3] = {20, 50, 66};
    for (int li = 0; li < 3; ++li) {
        const int L_max = Ls[li];
        const int Ms[6] = {0, 1, 2, 7, L_max - 1, L_max};
        for (int mi = 0; mi < 6; ++mi) {
            for (int nd = 0; nd < 3; ++nd) { find_case<double>(Ms[mi], L_max, nd); find_case<float>(Ms[mi], L_max, nd); }
            pairs_case(Ms[mi], L_max);
            for (int kind = 0; kind < 5; ++kind)
                for (int counters = 0; counters < 2; ++counters) {
                    fuse_case<double>(Ms[mi], L_max, kind, counters != 0);
                    fuse_case<float>(Ms[mi], L_max, kind, counters != 0);
                }
        }
    }
    double bd = 0.0; int bi = -1;
    merge_consider(3.0, 5, 5.99, &bd, &bi); merge_consider(3.0, 2, 5.99, &bd, &bi); merge_consider(6.0, 0, 5.99, &bd, &bi);
    merge_consider(NAN, 1, 5.99, &bd, &bi); merge_consider(INFINITY, 1, 5.99, &bd, &bi);
    CHECK(bi == 2 && bd == 3.0);
    const MergeTraffic t0 = merge_traffic(50, 0, 0, 0, 50, false), t1 = merge_traffic(50, 1, 1, 1, 50, true);
    CHECK(t0.elems == 0 && t1.elems == 103ull * 103ull + 103ull + 8ull * 103ull + 2ull + 2ull * 103ull * 103ull + 206ull);
    printf(failures ? "%d check(s) failed\n" : "merge host driver ok: %d cases\n", failures ? failures : g_case);
    return failures ? 1 : 0;
}
"""


def test_the_per_instance_functions_under_asan_and_ubsan(tmp_path):
    src = tmp_path / "merge_host.cpp"
    exe = tmp_path / "merge_host"
    src.write_text(DRIVER)
    csrc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", csrc, str(src), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0 and "merge host driver ok: 486 cases" in out.stdout, out.stdout + out.stderr
