// tick_chunks.h — how many ticks of a per-tick run (every caller of run_chunked, capi_run.h: slam_nav_run, slam_monitor_run,
// slam_innovation_run and the filtered runs of capi_filter.h) go into one chunk.
// A chunk is what such a run enqueues before it synchronises, reads its events and copies the rows of its ticks out; the rows of one chunk
// live on the device.  Plain C++: needs no HIP runtime (tests/test_tick_chunks_cpu.py).
#pragma once
#include <stdlib.h>

namespace slam_host {

constexpr int kMaxTicksPerChunk = 4096;

// At most 4096 ticks, and what the ticks of a chunk hold on the device - bytes_per_tick each - stays within budget_bytes, one tick at least
// (so a budget of 0, or a negative one, gives 1).  bytes_per_tick = 0: nothing is held per tick and only the cap applies.
inline int ticks_per_chunk(int T, double bytes_per_tick, double budget_bytes) {
    int chunk = T < kMaxTicksPerChunk ? T : kMaxTicksPerChunk;
    if (bytes_per_tick > 0.0) {
        const double fit = budget_bytes / bytes_per_tick;
        if (fit < (double)chunk) chunk = fit >= 1.0 ? (int)fit : 1;
    }
    return chunk;
}

// The budget: SLAM_MONITOR_LOG_BYTES as atof reads it (a text that is no number: 0), 256 MiB when unset.
inline double tick_log_budget() {
    const char* env = getenv("SLAM_MONITOR_LOG_BYTES");
    return env ? atof(env) : 256.0 * 1024 * 1024;
}

}  // namespace slam_host
