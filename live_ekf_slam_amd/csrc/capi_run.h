// capi_run.h — what the per-tick runs (slam_nav_run, slam_monitor_run, slam_innovation_run, slam_gate_run) share: the checks at entry, the
// chunked driver, the source of a tick's command and the slam_last_*_work readers.  Defined in capi_nav.cpp, except the template and TickCmds (here)
// and innovation_supported (capi_innovation.cpp).  Internal, like slam_handle.h.
#pragma once
#include <string.h>

#include "nav_kernel.h"
#include "slam_handle.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// The one place a NavParams is filled from the handle (everything but tick and cmd_log); the commands go to the first row of dcmd_each.
int nav_params(slam_handle* h, slam::NavParams* out);
// the next controller tick on the handle's stream
int nav_launch(slam_handle* h, slam::NavParams& p);

// innovations can be evaluated on this handle: EKF_SLAM with known landmark ids
int innovation_supported(const slam_handle* h);

// What a per-tick run `who` checks once its own arguments are in order: the handle, then its state, then the queued timesteps run.
// ekf_known_ids: the run evaluates innovations (innovation_supported).
int run_enter(slam_handle* h, const char* who, bool need_map, bool need_path, bool ekf_known_ids);

// T ticks in chunks of `chunk`.  Per chunk: before(t0, tc) enqueues the uploads of ticks [t0, t0 + tc); tick(t0, t, mark) enqueues the
// launches of tick t0 + t and passes the one launch group whose time is wanted through mark(launch); then the stream is synchronised and
// after(t0, tc) copies the rows of the chunk out.  The device time of every chunk is summed into times.total_ms and, while `timed`, that of
// every marked group into times.part_ms: an event pair per chunk and per tick of a chunk, from the handle's pool.
template <class Before, class Tick, class After>
int run_chunked(slam_handle* h, int T, int chunk, bool timed, RunTimes& times, Before before, Tick tick, After after) {
    while (h->run_ev.size() < 2 + (timed ? 2 * (size_t)chunk : 0)) {
        hipEvent_t e = nullptr;
        HIP_TRY(hipEventCreate(&e));
        h->run_ev.push_back(e);
    }
    hipEvent_t* const ev = h->run_ev.data();
    times.part_ms = timed ? 0.0 : -1.0; times.total_ms = 0.0;
    for (int t0 = 0; t0 < T; t0 += chunk) {
        const int tc = T - t0 < chunk ? T - t0 : chunk;
        TRY(before(t0, tc));
        HIP_TRY(hipEventRecord(ev[0], h->stream));
        for (int t = 0; t < tc; ++t)
            TRY(tick(t0, t, [&](auto launch) -> int {
                if (timed) HIP_TRY(hipEventRecord(ev[2 + 2 * t], h->stream));
                TRY(launch());
                if (timed) HIP_TRY(hipEventRecord(ev[3 + 2 * t], h->stream));
                return SLAM_OK;
            }));
        HIP_TRY(hipEventRecord(ev[1], h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
        times.total_ms += (double)ms;
        for (int t = 0; timed && t < tc; ++t) {
            HIP_TRY(hipEventElapsedTime(&ms, ev[2 + 2 * t], ev[3 + 2 * t]));
            times.part_ms += (double)ms;
        }
        TRY(after(t0, tc));
    }
    return SLAM_OK;
}

// slam_last_*_work; t: the times of that kind of run, NULL with a NULL handle
int last_work(const RunTimes* t, const char* run, double* part_ms, double* total_ms);

// Where the command of a tick comes from: kShared: row t0 + t of the host array cmds [T][2]; kEach: cmds is [T][B][2] on the host, and the
// rows of a chunk are uploaded to dcmd_each before its ticks; kNav: the controller computes them, one launch per tick.
struct TickCmds {
    enum Source { kShared, kEach, kNav } src;
    const float* cmds;
    slam::NavParams np;

    int init(slam_handle* h, Source s, const float* host_cmds) {
        src = s; cmds = host_cmds;
        memset(&np, 0, sizeof(np));
        return src == kNav ? nav_params(h, &np) : SLAM_OK;
    }
    double bytes_per_tick(const slam_handle* h) const { return src == kEach ? 4.0 * 2.0 * (double)h->B : 0.0; }   // on the device
    int upload(slam_handle* h, int t0, int tc) const { return src == kEach ? upload_cmds_each(h, cmds + (size_t)t0 * 2 * h->B, tc) : SLAM_OK; }
    // tick t of the chunk at t0: the shared command and the device row of per-instance commands (NULL: shared) of its step launch
    int select(slam_handle* h, int t0, int t, const float** cmd, const float** d_each) {
        *cmd = kNoCmd; *d_each = h->each.dcmd_each;
        if (src == kNav) return nav_launch(h, np);
        if (src == kEach) *d_each = h->each.dcmd_each + (size_t)t * 2 * h->B;
        else { *cmd = cmds + 2 * (size_t)(t0 + t); *d_each = nullptr; }
        return SLAM_OK;
    }
};

}  // namespace slam_capi
#pragma GCC visibility pop
