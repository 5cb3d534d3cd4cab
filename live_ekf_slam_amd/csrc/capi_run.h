// capi_run.h — what the per-tick runs share (slam_nav_run, slam_monitor_run, slam_innovation_run and, through run_filtered of capi_filter.h,
// slam_gate_run, slam_associate_run, slam_associate_joint_run, slam_manage_run, slam_manage_merge_run and their _sim forms): the checks at
// entry, the chunked driver, the source of a tick's command, the source of a tick's message and the slam_last_*_work readers.  Defined in
// capi_nav.cpp, except the template and TickCmds (here), innovation_supported (capi_innovation.cpp) and TickMsgs (capi_sense.cpp).
// Internal, like slam_handle.h.
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
// runs_simulator: the run advances the simulator's truth (its step generates the message, or the sensor model does): it needs a true map
// and no sense waiting for its commit.  need_path: the controller issues the commands.  ekf_known_ids: the run evaluates innovations
// (innovation_supported).
int run_enter(slam_handle* h, const char* who, bool runs_simulator, bool need_path, bool ekf_known_ids);

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

// Where the message of a tick comes from, for the runs that step on host-fed messages (slam_gate_run, slam_associate_run,
// slam_associate_joint_run, slam_manage_run, slam_manage_merge_run and their _sim forms).  kLog: the host arrays meas [T][B][k_stride][3] and
// count [T][B], the rows of a chunk uploaded before its ticks.  kSim: the sensor model (sense_kernel.h) writes the tick's message on the
// device from the tick's command, the commit follows the tick's step launch, and the rows the caller's slam_sense_log asks for are held
// per chunk and copied out after it.  Defined in capi_sense.cpp.
struct TickMsgs {
    enum Source { kLog, kSim } src;
    const float* meas; const int32_t* count;   // kLog
    slam_sense_log log;                        // kSim: what is wanted (all NULL: nothing)
    int k_stride; int chunk;

    void init_log(const float* host_meas, const int32_t* host_count, int ks) {
        src = kLog; meas = host_meas; count = host_count; k_stride = ks; chunk = 0;
        memset(&log, 0, sizeof(log));
    }
    void init_sim(const slam_sense_log* want, int ks) {
        src = kSim; meas = nullptr; count = nullptr; k_stride = ks; chunk = 0;
        memset(&log, 0, sizeof(log));
        if (want) log = *want;
    }
    bool sim() const { return src == kSim; }
    double bytes_per_tick(const slam_handle* h, const TickCmds& tcmd) const;   // on the device
    int reserve(slam_handle* h, const TickCmds& tcmd, int ticks);  // once the chunk length is known
    int upload(slam_handle* h, int t0, int tc) const;              // before(): kLog uploads the chunk's messages
    // tick t of the chunk, after TickCmds::select: the device message the tick's launches read (kSim: the sense launch comes first)
    int produce(slam_handle* h, const TickCmds& tcmd, int t, const float cmd[2], const float* d_each, const float** d_meas,
                const int32_t** d_count);
    int commit(slam_handle* h, int t);                             // right after the tick's step launch (kLog: nothing)
    int download(slam_handle* h, const TickCmds& tcmd, int t0, int tc) const;   // after(): the logged rows of the chunk
};

// the `source` argument of a *_run_sim call as a TickCmds source; LOG and unknown values are SLAM_ERR_ARG
int sim_run_source(int source, const float* cmds, TickCmds::Source* out);

}  // namespace slam_capi
#pragma GCC visibility pop
