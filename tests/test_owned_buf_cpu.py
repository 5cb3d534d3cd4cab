"""CPU test of slam_host::Buf (live_ekf_slam_amd/csrc/host/owned_buf.h), the owner of every device and pinned buffer of the C ABI.

A small driver is built against the header with AddressSanitizer + UndefinedBehaviorSanitizer and a malloc-backed policy that can be told to
fail its next allocation, so the growth rule - allocate the new block first, keep the old block and capacity when that fails - is checked
without a HIP runtime.  LeakSanitizer reports any block that is never released; ASan reports any block released twice."""
import os
import subprocess

from conftest import ROOT

DRIVER = r"""
#include <stdio.h>
#include <stdlib.h>
#include <utility>
#include "owned_buf.h"

static bool g_fail_next = false;
static int g_live = 0;   // blocks allocated and not yet released
struct MallocAlloc {
    static int alloc(void** p, size_t bytes) {
        if (g_fail_next) { g_fail_next = false; return 2; }
        *p = malloc(bytes);
        if (!*p) return 1;
        g_live += 1;
        return 0;
    }
    static void release(void* p) { g_live -= 1; free(p); }
};
using B = slam_host::Buf<int, MallocAlloc>;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { printf("FAILED line %d: %s\n", __LINE__, #c); failures += 1; } } while (0)

int main() {
    {
        B b;
        CHECK(b.get() == nullptr && b.cap() == 0 && !b);
        CHECK(b.reserve(0) == 0 && b.get() == nullptr);           // nothing to do
        CHECK(b.reserve(16) == 0 && b.get() && b.cap() == 16);    // a grow succeeds
        for (int i = 0; i < 16; ++i) b[i] = i;                    // the whole capacity is writable
        int* p = b.get();
        CHECK(b.reserve(8) == 0 && b.get() == p && b.cap() == 16);   // within the capacity: the same block
        g_fail_next = true;
        CHECK(b.reserve(64) == 2);                                // a failed grow returns the policy's error ...
        CHECK(b.get() == p && b.cap() == 16 && g_live == 1);      // ... and keeps the old block and capacity
        CHECK(b[15] == 15);                                       // (still the caller's: not released)
        CHECK(b.reserve(64) == 0 && b.cap() == 64 && g_live == 1);   // a later grow succeeds and releases the old block
        for (int i = 0; i < 64; ++i) b[i] = -i;
        B c(std::move(b));                                        // moved-from: empty
        CHECK(b.get() == nullptr && b.cap() == 0 && c.cap() == 64 && g_live == 1);
        B d;
        CHECK(d.reserve(4) == 0 && g_live == 2);
        d = std::move(c);                                         // move assignment releases what d held
        CHECK(c.get() == nullptr && c.cap() == 0 && d.cap() == 64 && d[63] == -63 && g_live == 1);
        d = std::move(d);                                         // self-move keeps the block
        CHECK(d.cap() == 64 && g_live == 1);
        B e;
        g_fail_next = true;
        CHECK(e.reserve(3) == 2 && e.get() == nullptr && e.cap() == 0);   // a failed first grow leaves it empty
        d.reset();
        CHECK(d.get() == nullptr && d.cap() == 0 && g_live == 0);
        {
            B f;
            CHECK(f.reserve(5) == 0 && g_live == 1);
        }
        CHECK(g_live == 0);                                       // released by the destructor
        CHECK(d.reserve(7) == 0 && g_live == 1);                  // (d is left holding a block for the destructor below)
    }
    CHECK(g_live == 0);   // every block released exactly once by the destructors
    printf("%d failed\n", failures);
    return failures ? 1 : 0;
}
"""


def test_owned_buf_growth_failure_and_moves_under_asan_ubsan(tmp_path):
    src = tmp_path / "owned_buf_driver.cpp"
    src.write_text(DRIVER)
    exe = tmp_path / "owned_buf_driver"
    inc = os.path.join(ROOT, "live_ekf_slam_amd", "csrc", "host")
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-self-move", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                         "-fno-omit-frame-pointer", "-I", inc, str(src), "-o", str(exe)], capture_output=True, text=True, timeout=300)
    assert cc.returncode == 0, cc.stdout[-3000:] + cc.stderr[-3000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:halt_on_error=1", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300, env=env)
    text = out.stdout + out.stderr
    assert "ERROR: AddressSanitizer" not in text and "runtime error:" not in text and "LeakSanitizer" not in text, text[-3000:]
    assert out.returncode == 0, text[-3000:]
    assert "0 failed" in out.stdout, text[-3000:]
