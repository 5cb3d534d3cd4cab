// capi_filter.h — what the units that rewrite a tick's message before the known-id EKF step consumes it share (capi_gate.cpp: the chi-square
// gate; capi_assoc.cpp, capi_joint.cpp: the associations; capi_map.cpp, capi_merge.cpp: the managed ticks), and capi_innovation.cpp with
// them: the checks and the staging of one message, rows as data, the preamble of the host hooks and run_filtered, the one run of T filtered
// ticks.  The bodies that are no templates are in capi_innovation.cpp.  Internal, like slam_handle.h.
#pragma once
#include <vector>

#include "capi_innovation.h"
#include "capi_run.h"
#include "host/tick_chunks.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// ---- rows as data ---------------------------------------------------------------------------------------------------------------------------
// One output of a call: per_tick elements of elem_bytes per tick, the ticks of a chunk (or the one of a single call) from the head of
// `dev`, every tick of the call in `host` (NULL: not wanted), whose type gives the element size.
struct TickRow {
    const void* dev; void* host; size_t elem_bytes; size_t per_tick;
    template <class T> TickRow(const void* d, T* to, size_t n) : dev(d), host(to), elem_bytes(sizeof(T)), per_tick(n) {}
};
// once the stream has run dry: ticks [t0, t0 + tc) of the wanted rows
int copy_rows(const std::vector<TickRow>& rows, int t0, int tc);
// row r of a [rows][stride] block of per-instance counts, at offset o
inline int32_t* row(int32_t* base, int r, size_t stride, size_t o = 0) { return base + (size_t)r * stride + o; }
inline const int32_t* row(const int32_t* base, int r, size_t stride, size_t o = 0) { return base + (size_t)r * stride + o; }

// ---- one message: arguments, entry, staging -------------------------------------------------------------------------------------------------
// a message on the device
struct DevMsg { float* meas; int32_t* count; };

// the arguments every entry point of one message shares, checked after the config and before the handle is looked at
int message_args(const float* cmds, const void* meas, const void* count, int k_stride, const void* meas_out = nullptr,
                 const void* count_out = nullptr, bool need_out = false);
// the byte ranges [a, a + na) and [b, b + nb) meet
bool ranges_overlap(const void* a, size_t na, const void* b, size_t nb);
// SLAM_ERR_ARG if the output message of a _dev call meets the input (other than in place) or itself
int out_message_overlaps(const slam_handle* h, const float* d_meas, const int32_t* d_count, int k_stride, DevMsg out);
// association can run on this handle: EKF_SLAM with known landmark ids (capi_assoc.cpp; innovation_supported: capi_run.h)
int assoc_supported(const slam_handle* h);
// the handle, once the arguments are in order; the queued timesteps run first
int filter_enter(slam_handle* h, int (*supported)(const slam_handle*));
// a call that steps or edits the map: no shadow filter, no pending prediction stage
int step_state(const slam_handle* h, const char* who);
// Where the launches of one call read its message and commands.  host: the message is uploaded (*meas and *count become the staged
// copies) and so are per-instance commands; else they are the caller's device arrays.  *cmd: the shared command, *d_each: the
// per-instance ones (NULL: shared).
int stage_message(slam_handle* h, bool host, const float* cmds, int cmd_each, const float** meas, const int32_t** count, int k_stride,
                  const float** cmd, const float** d_each);
// the row a host call's filter writes starts as the (staged) input row: slots the kernel does not write keep what the caller gave
int seed_out_message(slam_handle* h, float* d_meas_out, int k_stride);
// what a filtered step hands back: nothing synchronises unless the record or the [B] count at d_n is wanted
int step_outputs(slam_handle* h, double* rec, const int32_t* d_n, int32_t* n);

// the arguments of a *_run call after its configs, and its messages
int run_args_log(const float* cmds, const float* meas, const int32_t* count, int k_stride, int T, TickMsgs* msgs);
// the arguments of a *_run_sim call after its configs, its commands' source and its messages
int run_args_sim(int source, const float* cmds, int k_stride, int T, const slam_sense_log* log, TickCmds::Source* csrc, TickMsgs* msgs);

// ---- the host hooks of one instance (slam_*_instance_host) ----------------------------------------------------------------------------------
// What they share once their config is checked: the checks of the state and the message, the noise as the kernels take it and the loads
// of x and P through the storage type.
struct InstanceHostArgs {
    struct LoadX {
        const double* x; bool f32;
        double operator()(int i) const { return f32 ? (double)(float)x[i] : x[i]; }
    };
    struct LoadP {
        const double* P; int n; bool f32;
        double operator()(int r, int c) const { const double e = P[(size_t)r * n + c]; return f32 ? (double)(float)e : e; }
    };
    slam::InnovNoise nz;
    LoadX load_x;
    LoadP load_P;
    // strided: the message has `count` detections at stride k_stride; else it is dense, count = k of them
    int init(const double* x, const double* P, const int32_t* ids, int M, int L_max, const float cmd[2], const float* meas, int count,
             int k_stride, bool strided, const slam_noise* noise, int f32_storage);
};

// ---- the run of T filtered ticks ------------------------------------------------------------------------------------------------------------
// slam_gate_run, slam_associate_run, slam_associate_joint_run, slam_manage_run, slam_manage_merge_run and their _sim forms once their
// arguments are in order: T ticks with the commands of `csrc` on the messages of `msgs`.  Every tick: the command, the message, the
// feature's filter, the step on the filtered message, the simulator's commit, what the feature does after a step.  The feature `f` gives,
// all of it asked for only once the handle is checked:
//   RunTimes& times()                    where the device times of this kind of run go
//   double bytes_per_tick()              its rows of one tick on the device
//   int reserve(k_stride, chunk)         once the chunk length is known; what it zeroes once per run
//   int chunk_begin()                    what it zeroes per chunk, between the uploads of the commands and of the messages
//   int filter(t, cmd, d_each, d_meas, d_count, k_stride, mark)   tick t of the chunk: the launches that write out()
//   DevMsg out()                         the filtered message
//   int after_step(t_run, t, mark)       after the commit (mark, in either: the one launch group whose time is wanted)
//   int chunk_done(t0, tc)               after the chunk's events and its synchronisation: the traffic sums
//   std::vector<TickRow> rows()          asked once, after reserve
//   int finish()                         after the last chunk
template <class Feature>
int run_filtered(slam_handle* h, const char* who, TickCmds::Source csrc, const float* cmds, TickMsgs& msgs, int T, Feature&& f) {
    const int k_stride = msgs.k_stride;
    TRY(run_enter(h, who, msgs.sim(), csrc == TickCmds::kNav, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    TickCmds tcmd;
    TRY(tcmd.init(h, csrc, cmds));
    // what a tick holds on the device: the feature's rows, those of the commands (cmd_each) and of the messages
    const int chunk = slam_host::ticks_per_chunk(T, f.bytes_per_tick() + tcmd.bytes_per_tick(h) + msgs.bytes_per_tick(h, tcmd),
                                                 slam_host::tick_log_budget());
    TRY(f.reserve(k_stride, chunk));
    TRY(msgs.reserve(h, tcmd, chunk));
    const std::vector<TickRow> rows = f.rows();
    TRY(run_chunked(
        h, T, chunk, h->nav.time_ticks, f.times(),
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            TRY(f.chunk_begin());
            return msgs.upload(h, t0, tc);
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each, *dm;
            const int32_t* dc;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(msgs.produce(h, tcmd, t, cmd, d_each, &dm, &dc));
            TRY(f.filter(t, cmd, d_each, dm, dc, k_stride, mark));
            TRY(launch_step(h, cmd, 0, f.out().meas, f.out().count, k_stride, d_each));
            TRY(msgs.commit(h, t));   // (before anything that edits the map or moves the pose: the simulator's error is taken after the step)
            return f.after_step(t0 + t, t, mark);
        },
        [&](int t0, int tc) -> int {
            TRY(msgs.download(h, tcmd, t0, tc));
            TRY(f.chunk_done(t0, tc));   // (after the chunk's events: the traffic models are no part of the run's times)
            return copy_rows(rows, t0, tc);
        }));
    return f.finish();
}

}  // namespace slam_capi
#pragma GCC visibility pop
