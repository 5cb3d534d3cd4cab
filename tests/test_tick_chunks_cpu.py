"""CPU test of the chunk rule of the per-tick runs (live_ekf_slam_amd/csrc/host/tick_chunks.h): slam_nav_run, slam_monitor_run,
slam_innovation_run and slam_gate_run all cut their T ticks into chunks by slam_host::ticks_per_chunk with the budget of
slam_host::tick_log_budget.

The rule: at most 4096 ticks per chunk; if a tick holds bytes on the device and budget / bytes_per_tick is below that, the quotient
truncated, one tick at least.  The expected values below are written out by hand from that sentence.  The driver is built with
AddressSanitizer + UndefinedBehaviorSanitizer (the float-to-int conversion of the quotient is where the rule could go wrong)."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include "tick_chunks.h"

using slam_host::ticks_per_chunk;
using slam_host::tick_log_budget;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures += 1; } } while (0)

int main() {
    // nothing held per tick: the cap alone, whatever the budget
    CHECK(ticks_per_chunk(1, 0.0, 1.0) == 1);
    CHECK(ticks_per_chunk(4095, 0.0, 1.0) == 4095);
    CHECK(ticks_per_chunk(4096, 0.0, 1.0) == 4096);
    CHECK(ticks_per_chunk(4097, 0.0, 1.0) == 4096);
    CHECK(ticks_per_chunk(100000, 0.0, 1.0) == 4096);
    CHECK(ticks_per_chunk(100000, 0.0, -1.0) == 4096);
    // 1320 bytes per tick (three series of 55 doubles), T = 10: a budget of exactly k ticks, and one byte less
    CHECK(ticks_per_chunk(10, 1320.0, 1320.0) == 1);
    CHECK(ticks_per_chunk(10, 1320.0, 1319.0) == 1);      // less than one tick: one tick all the same
    CHECK(ticks_per_chunk(10, 1320.0, 3960.0) == 3);
    CHECK(ticks_per_chunk(10, 1320.0, 3959.0) == 2);
    CHECK(ticks_per_chunk(10, 1320.0, 3967.0) == 3);      // (3 * per_tick + 7, the budget of the GPU chunking tests)
    CHECK(ticks_per_chunk(10, 1320.0, 1.0) == 1);
    CHECK(ticks_per_chunk(10, 1320.0, 0.0) == 1);
    CHECK(ticks_per_chunk(10, 1320.0, -5.0) == 1);
    CHECK(ticks_per_chunk(10, 1320.0, -1e300) == 1);
    // a budget that holds the whole run, exactly and with room
    CHECK(ticks_per_chunk(10, 1320.0, 13200.0) == 10);
    CHECK(ticks_per_chunk(10, 1320.0, 13201.0) == 10);
    CHECK(ticks_per_chunk(10, 1320.0, 1e300) == 10);
    // the cap and the budget together: 256 MiB hold 33 554 432 ticks of 8 bytes, and 512 ticks of 8 * 65 536 bytes
    CHECK(ticks_per_chunk(100000, 8.0, 268435456.0) == 4096);
    CHECK(ticks_per_chunk(100000, 524288.0, 268435456.0) == 512);
    CHECK(ticks_per_chunk(300, 524288.0, 268435456.0) == 300);
    // the budget: 256 MiB when the variable is unset, else what atof reads (no number: 0, hence one tick per chunk)
    unsetenv("SLAM_MONITOR_LOG_BYTES");
    CHECK(tick_log_budget() == 268435456.0);
    setenv("SLAM_MONITOR_LOG_BYTES", "1", 1);
    CHECK(tick_log_budget() == 1.0);
    CHECK(ticks_per_chunk(10, 8.0, tick_log_budget()) == 1);
    setenv("SLAM_MONITOR_LOG_BYTES", "3967", 1);
    CHECK(tick_log_budget() == 3967.0);
    setenv("SLAM_MONITOR_LOG_BYTES", "not a number", 1);
    CHECK(tick_log_budget() == 0.0);
    CHECK(ticks_per_chunk(10, 8.0, tick_log_budget()) == 1);
    CHECK(ticks_per_chunk(10, 0.0, tick_log_budget()) == 10);
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
"""


def test_ticks_per_chunk_and_the_budget_under_asan_ubsan(tmp_path):
    src = tmp_path / "tick_chunks_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "tick_chunks_driver"
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
