"""CPU test of the schedule rules of a pose-graph solve (live_ekf_slam_amd/csrc/host/pgs_schedule.h): the number of solve groups and their
ranges, the streaming share, the lambda lanes, the fused chain + SYRK choice, which kernels a solve's graphs fit, the SYRK kernel, the step of
the segment-length search, the streaming loop's launch bound and hand-over, and the clamps of the tuning values pgs_create reads from the
environment.  pgs_solve (pgs_capi.cpp) decides by these functions and nothing else.

The expected values are written out by hand from the rules as the header's comments (and include/slam_pgs.h) state them - with 256 compute
units for the fused choice and lane switches 16 / 64 - never computed by the code under test.  The driver is built with AddressSanitizer +
UndefinedBehaviorSanitizer (the launch bound is where 32-bit arithmetic would overflow)."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "pgs_schedule.h"

using namespace slam_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures += 1; } } while (0)

static bool range_is(int B, int G, int g, int off, int cnt) { const PgsRange r = pgs_group_range(B, G, g); return r.b_off == off && r.b_cnt == cnt; }
static bool step_is(int SL, int mx, int N, PgsSegStep::Kind kind, int next) {
    const PgsSegStep s = pgs_seg_step(SL, mx, N);
    return s.kind == kind && (kind != PgsSegStep::kTry || s.next == next);
}
static PgsTuning with_env(const char* name, const char* value) {
    setenv(name, value, 1);
    const PgsTuning t = PgsTuning::from_env();
    unsetenv(name);
    return t;
}

int main() {
    static_assert(kPgsMaxGroups == 16 && kPgsRing == 8, "the caps the rules below are written for");
    static_assert(slam::kPgsSegMaxLen == 32 && slam::kPgsSegMaxLm == 63 && slam::kPgsSegMaxSep == 128 && slam::kPgsSyrkInstTiles == 96, "kernel capacities");

    // ---- groups of a solve: (requested, B, profiled)
    CHECK(pgs_groups(0, 127, false) == 1);
    CHECK(pgs_groups(0, 128, false) == 2);
    CHECK(pgs_groups(3, 10, false) == 3);
    CHECK(pgs_groups(16, 10, false) == 10);
    CHECK(pgs_groups(40, 1000, false) == 16);
    CHECK(pgs_groups(0, 1, false) == 1);
    CHECK(pgs_groups(0, 2048, false) == 2);
    CHECK(pgs_groups(0, 2048, true) == 1);
    CHECK(pgs_groups(3, 10, true) == 1);
    CHECK(pgs_groups(40, 1000, true) == 1);

    // ---- range of group g
    CHECK(range_is(10, 3, 0, 0, 4)); CHECK(range_is(10, 3, 1, 4, 4)); CHECK(range_is(10, 3, 2, 8, 2));
    CHECK(range_is(9, 4, 0, 0, 3)); CHECK(range_is(9, 4, 1, 3, 3)); CHECK(range_is(9, 4, 2, 6, 3)); CHECK(range_is(9, 4, 3, 9, 0));
    CHECK(pgs_group_range(9, 4, 3).idle() && !pgs_group_range(9, 4, 2).idle());
    CHECK(range_is(5, 4, 0, 0, 2)); CHECK(range_is(5, 4, 1, 2, 2)); CHECK(range_is(5, 4, 2, 4, 1)); CHECK(range_is(5, 4, 3, 6, -1));
    CHECK(pgs_group_range(5, 4, 3).idle() && !pgs_group_range(5, 4, 2).idle());
    CHECK(range_is(45, 2, 0, 0, 23)); CHECK(range_is(45, 2, 1, 23, 22));
    CHECK(range_is(2048, 1, 0, 0, 2048));

    // ---- streaming share: B 45 in two groups of 23 and 22
    CHECK(pgs_slot_share(44, 2, false) == 22);
    CHECK(pgs_stream_slots(22, 23) == 22);     // group 0 streams with 22
    CHECK(pgs_stream_slots(22, 22) == 0);      // group 1: 22 is not below 22 - lockstep
    CHECK(pgs_slot_share(7, 2, false) == 4);
    CHECK(pgs_stream_slots(4, 23) == 4 && pgs_stream_slots(4, 22) == 4);
    CHECK(pgs_slot_share(64, 2, false) == 32);
    CHECK(pgs_stream_slots(32, 23) == 0 && pgs_stream_slots(32, 22) == 0);
    CHECK(pgs_slot_share(0, 2, false) == 0);
    CHECK(pgs_slot_share(-3, 2, false) == 0);
    CHECK(pgs_stream_slots(0, 23) == 0 && pgs_stream_slots(0, 22) == 0);
    CHECK(pgs_slot_share(44, 2, true) == 0 && pgs_slot_share(7, 1, true) == 0);
    CHECK(pgs_slot_share(8, 3, false) == 3 && pgs_slot_share(7, 1, false) == 7);

    // ---- lanes of the next trial, switches 16 / 64
    PgsTuning t;
    CHECK(t.lanes_switch_all == 16 && t.lanes_switch == 64 && t.lanes == 4);
    CHECK(pgs_lanes_next(t, 16) == 4);
    CHECK(pgs_lanes_next(t, 17) == 2);
    CHECK(pgs_lanes_next(t, 64) == 2);
    CHECK(pgs_lanes_next(t, 65) == 1);
    CHECK(pgs_lanes_next(t, 0) == 4);
    t.lanes = 1;
    CHECK(pgs_lanes_next(t, 1) == 1 && pgs_lanes_next(t, 16) == 1 && pgs_lanes_next(t, 17) == 1 && pgs_lanes_next(t, 64) == 1 && pgs_lanes_next(t, 65) == 1);
    t.lanes = 8;
    CHECK(pgs_lanes_next(t, 10) == 8);
    CHECK(pgs_lanes_next(t, 30) == 2);
    CHECK(pgs_lanes_next(t, 3000) == 1);

    // ---- fused choice: (fused_ok, fused_mode, running slots, 256 compute units)
    CHECK(pgs_fused(true, -1, 1, 256) == 4);
    CHECK(pgs_fused(true, -1, 64, 256) == 4);
    CHECK(pgs_fused(true, -1, 65, 256) == 3);
    CHECK(pgs_fused(true, -1, 85, 256) == 3);
    CHECK(pgs_fused(true, -1, 86, 256) == 2);
    CHECK(pgs_fused(true, -1, 128, 256) == 2);
    CHECK(pgs_fused(true, -1, 129, 256) == 0);
    CHECK(pgs_fused(true, -1, 170, 256) == 0);
    CHECK(pgs_fused(true, -1, 171, 256) == 2);
    CHECK(pgs_fused(true, -1, 256, 256) == 2);
    CHECK(pgs_fused(true, -1, 257, 256) == 0);
    CHECK(pgs_fused(true, 3, 257, 256) == 3);
    CHECK(pgs_fused(true, 2, 64, 256) == 2 && pgs_fused(true, 4, 2048, 256) == 4);
    for (int mode = -1; mode <= 5; ++mode) { CHECK(pgs_fused(false, mode, 64, 256) == 0); CHECK(pgs_fused(false, mode, 257, 256) == 0); }
    const int automatic[3] = {-1, 1, 5};
    for (int mode : automatic) {
        CHECK(pgs_fused(true, mode, 64, 256) == 4); CHECK(pgs_fused(true, mode, 85, 256) == 3); CHECK(pgs_fused(true, mode, 128, 256) == 2);
        CHECK(pgs_fused(true, mode, 170, 256) == 0); CHECK(pgs_fused(true, mode, 171, 256) == 2); CHECK(pgs_fused(true, mode, 257, 256) == 0);
    }

    // ---- whether a solve's graphs fit: (most landmarks, k_per_pose, fused_mode)
    CHECK(pgs_fit(176, 8, -1).fused_ok);             // 352 columns: 11 tile rows, 66 tiles of 72
    CHECK(!pgs_fit(177, 8, -1).fused_ok);            // 354 columns: 12 tile rows, 78 tiles
    CHECK(pgs_fit(176, 32, -1).fused_ok);
    CHECK(!pgs_fit(176, 33, -1).fused_ok);
    CHECK(!pgs_fit(176, 8, 0).fused_ok);
    CHECK(!pgs_fit(1, 8, 0).fused_ok && pgs_fit(1, 8, 3).fused_ok);
    CHECK(pgs_fit(207, 8, -1).syrk_inst_ok);         // 415 columns: 13 tile rows, 91 tiles of 96
    CHECK(!pgs_fit(208, 8, -1).syrk_inst_ok);        // 417 columns: 14 tile rows, 105 tiles
    CHECK(pgs_fit(207, 33, 0).syrk_inst_ok && !pgs_fit(207, 8, -1).fused_ok);   // (the two do not depend on each other)

    // ---- SYRK kernel of a trial: (active, lanes, switch, syrk_inst_ok)
    CHECK(pgs_syrk_kernel(25, 4, 100, true) == 1);
    CHECK(pgs_syrk_kernel(24, 4, 100, true) == 32);
    CHECK(pgs_syrk_kernel(100, 1, 100, true) == 1 && pgs_syrk_kernel(99, 1, 100, true) == 32);
    CHECK(pgs_syrk_kernel(25, 4, 100, false) == 32 && pgs_syrk_kernel(2048, 1, 100, false) == 32);

    // ---- one step of the segment search: (SL, largest seg_umax, poses)
    CHECK(step_is(32, 63, 300, PgsSegStep::kAccept, 0));
    CHECK(step_is(32, 0, 300, PgsSegStep::kAccept, 0));
    CHECK(step_is(32, 64, 300, PgsSegStep::kTry, 16));
    CHECK(step_is(16, 64, 300, PgsSegStep::kTry, 8));
    CHECK(step_is(8, 64, 300, PgsSegStep::kGiveUp, 0));
    CHECK(step_is(32, 0x7fffffff, 300, PgsSegStep::kGiveUp, 0));
    CHECK(step_is(32, 64, 2066, PgsSegStep::kGiveUp, 0));     // 2064 / 16 = 129 separators
    CHECK(step_is(32, 64, 2065, PgsSegStep::kTry, 16));       // 2063 / 16 = 128
    CHECK(step_is(8, 63, 2066, PgsSegStep::kAccept, 0));

    // ---- streaming loop
    CHECK(pgs_stream_launch_bound(45, 2, 8) == 192);          // (22 + 2) x 8
    CHECK(pgs_stream_launch_bound(1 << 20, 1, 400000) == 419431200000LL);   // (1048576 + 2) x 400000: beyond 32 bits
    CHECK(pgs_stream_hands_over(0, 10, 45, 2, 64));           // nothing left
    CHECK(pgs_stream_hands_over(0, 45, 45, 2, 64));
    CHECK(!pgs_stream_hands_over(5, 44, 45, 2, 64));          // a graph still waits
    CHECK(!pgs_stream_hands_over(1, 22, 23, 1, 64));
    CHECK(pgs_stream_hands_over(32, 45, 45, 2, 64));          // nothing waits, 64 of the batch's scale run
    CHECK(!pgs_stream_hands_over(65, 45, 45, 1, 64));         // 65
    CHECK(pgs_stream_hands_over(64, 46, 45, 1, 64));
    CHECK(!pgs_stream_hands_over(13, 45, 45, 5, 64));         // 13 x 5 = 65

    // ---- the tuning values: defaults, then one variable at a time
    const char* names[] = {"SLAM_PGS_MAX_TRIALS", "SLAM_PGS_LANES", "SLAM_PGS_LANES_SWITCH", "SLAM_PGS_LANES_SWITCH_ALL", "SLAM_PGS_SYRK_INST_SWITCH",
                           "SLAM_PGS_TRACE", "SLAM_PGS_HOST_PROF", "SLAM_PGS_FUSED", "SLAM_PGS_SEG", "SLAM_PGS_LIST", "SLAM_PGS_GROUPS", "SLAM_PGS_SLOTS",
                           "SLAM_PGS_STREAM_DEPTH", "SLAM_PGS_SEG_BACK_GLOBAL", "SLAM_PGS_GROUP_PRIO"};
    for (const char* n : names) unsetenv(n);
    const PgsTuning d = PgsTuning::from_env();
    CHECK(d.max_trials == 400 && d.lanes == 4 && d.lanes_switch == 64 && d.lanes_switch_all == 16 && d.syrk_inst_switch == 100);
    CHECK(d.fused_mode == -1 && d.seg_len == 32 && d.use_list && d.groups == 0 && d.slots == 0 && d.stream_depth == 3);
    CHECK(!d.trace && !d.host_prof && d.seg_back_global == 0 && d.group_prio);
    CHECK(with_env("SLAM_PGS_LANES", "0").lanes == 4);
    CHECK(with_env("SLAM_PGS_LANES", "9").lanes == 4);
    CHECK(with_env("SLAM_PGS_LANES", "8").lanes == 8);
    CHECK(with_env("SLAM_PGS_LANES", "1").lanes == 1);
    CHECK(with_env("SLAM_PGS_SEG", "-1").seg_len == 0);
    CHECK(with_env("SLAM_PGS_SEG", "0").seg_len == 0);
    CHECK(with_env("SLAM_PGS_SEG", "1").seg_len == 2);
    CHECK(with_env("SLAM_PGS_SEG", "33").seg_len == 32);
    CHECK(with_env("SLAM_PGS_SEG", "16").seg_len == 16);
    CHECK(with_env("SLAM_PGS_STREAM_DEPTH", "0").stream_depth == 3);
    CHECK(with_env("SLAM_PGS_STREAM_DEPTH", "8").stream_depth == 3);
    CHECK(with_env("SLAM_PGS_STREAM_DEPTH", "7").stream_depth == 7);
    CHECK(with_env("SLAM_PGS_STREAM_DEPTH", "1").stream_depth == 1);
    CHECK(with_env("SLAM_PGS_SLOTS", "-3").slots == 0);
    CHECK(with_env("SLAM_PGS_SLOTS", "44").slots == 44);
    CHECK(with_env("SLAM_PGS_MAX_TRIALS", "0").max_trials == 400);
    CHECK(with_env("SLAM_PGS_MAX_TRIALS", "-2").max_trials == 400);
    CHECK(with_env("SLAM_PGS_MAX_TRIALS", "8").max_trials == 8);
    CHECK(!with_env("SLAM_PGS_GROUP_PRIO", "0").group_prio);
    CHECK(with_env("SLAM_PGS_GROUP_PRIO", "1").group_prio);
    CHECK(with_env("SLAM_PGS_GROUP_PRIO", "2").group_prio);
    // the values taken as they read, and the switches that only need to be set
    CHECK(with_env("SLAM_PGS_LANES_SWITCH", "0").lanes_switch == 0 && with_env("SLAM_PGS_LANES_SWITCH_ALL", "-1").lanes_switch_all == -1);
    CHECK(with_env("SLAM_PGS_SYRK_INST_SWITCH", "1000000000").syrk_inst_switch == 1000000000);
    CHECK(with_env("SLAM_PGS_FUSED", "0").fused_mode == 0 && with_env("SLAM_PGS_FUSED", "3").fused_mode == 3);
    CHECK(with_env("SLAM_PGS_GROUPS", "3").groups == 3 && with_env("SLAM_PGS_SEG_BACK_GLOBAL", "1").seg_back_global == 1);
    CHECK(!with_env("SLAM_PGS_LIST", "0").use_list && with_env("SLAM_PGS_LIST", "1").use_list);
    CHECK(with_env("SLAM_PGS_TRACE", "").trace && with_env("SLAM_PGS_HOST_PROF", "0").host_prof);
    CHECK(with_env("SLAM_PGS_LANES", "8").max_trials == 400);   // (one variable moves one value)
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
"""


def test_pgs_schedule_rules_and_tuning_clamps_under_asan_ubsan(tmp_path):
    src = tmp_path / "pgs_schedule_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "pgs_schedule_driver"
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


def test_the_headers_are_part_of_the_build():
    from live_ekf_slam_amd import build
    assert "host/pgs_schedule.h" in build.HEADERS and "host/pgs_limits.h" in build.HEADERS
