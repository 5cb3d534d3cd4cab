// slam_handle.h — the handle of the filter ABI (include/slam_batch.h) and the host helpers that more than one of its translation units
// uses (slam_capi.cpp: create / configure / init; capi_step.cpp: the steps and their queue; capi_state.cpp: reading the state back;
// capi_consistency.cpp, capi_nav.cpp, capi_monitor.cpp, capi_innovation.cpp, capi_gate.cpp, capi_assoc.cpp, capi_joint.cpp, capi_map.cpp,
// capi_merge.cpp, capi_score.cpp, capi_sense.cpp, capi_fix.cpp: one feature each; capi_run.h: what the per-tick runs share; capi_filter.h: what the features that filter a
// message before the step share).  Not installed, not part of the ABI: the standing of capi_internal.h.
#pragma once
#include "../../include/slam_batch.h"

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "capi_internal.h"
#include "noise_row.h"

namespace slam { struct EkfStepParams; struct UkfStepParams; struct ConsistencyParams; }

// a block of the handle whose (implicit) member functions stay out of the library's export table
#define SLAM_HANDLE_BLOCK __attribute__((visibility("hidden")))

// Device times of the last per-tick run of one kind (run_chunked): part_ms is the sum over the launch group each tick marks, -1 while
// slam_nav_set_timing is off; total_ms is the sum over the chunks, -1 until such a run has run on the handle.
namespace slam_capi {
struct RunTimes { double part_ms = -1.0, total_ms = -1.0; };
// The traffic model of an association (slam_associate*, slam_associate_joint*): its three sums on the device, what the last synchronising
// call read from them and the device times of the last run.
struct Traffic {
    DevBuf<unsigned long long> dwork;
    double bytes = -1.0, lines = -1.0;
    RunTimes times;
};
}

struct slam_handle {
    slam_config cfg;
    int kind, B, L_max, dtype, device;
    int n_max, ld_max, pstride, xstride;
    int waves_per_filter = 0;
    int dbg = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool inited = false;
    uint64_t seed = 2025;
    int64_t inst0 = 0;
    uint32_t step = 0;
    double range_max, fov_min, fov_max;
    // device buffers (released with the handle)
    DevBuf<char> dP, dP2;                      // dP = current P_t; dP2 = second buffer (EKF: layout changes, UKF: ping-pong)
    DevBuf<char> dx; int esz = 8;              // x_t; element size of P / x storage
    DevBuf<double> dscratch;                   // fp32 storage: fp64 slab for P between detection groups
    DevBuf<int32_t> dM, dids, dflags, dts; DevBuf<double> dtruth, derr;
    DevBuf<double> dmap; int L = 0;
    DevBuf<float> dmeas; DevBuf<int32_t> dcount; int k_stride = 0;   // last-measurement dump (slam_get_last_meas); k_stride: what both hold
    // One fill of host messages on its way to the device: pinned staging buffers, their device copies and the events that order the copy
    // stream with the compute stream (copied: the fill is on the device; used: the launch that read it is enqueued, in_use: and may still
    // run), created on first use.
    struct Stage {
        PinnedBuf<float> hmeas; PinnedBuf<int32_t> hcount; PinnedBuf<float> hcmds;   // pinned host (hcmds: the queued fill only)
        DevBuf<float> dmeas; DevBuf<int32_t> dcount;                                 // device
        hipEvent_t copied = nullptr, used = nullptr;
        bool in_use = false;
    };
    // slam_step (host measurements), launched at the call: two fills of one message each, filled on a copy stream while the previous
    // step's kernel runs; no stream synchronisation per step
    Stage stage[2];
    hipStream_t copy_stream = nullptr;
    hipEvent_t shadow_ev = nullptr;
    uint32_t stage_next = 0;
    DevBuf<unsigned long long> dkhist;                         // [8] instance-steps by detection count
    // EKF: consecutive calls of the per-tick entry points (slam_step_sim, slam_step, slam_step_dev) are queued on the host and run as
    // ONE multi-step launch when the queue is full or anything else touches the handle (every other entry point runs it first).  The
    // kernels are asynchronous anyway, and a multi-step launch gives the same bits as single steps, so only the speed changes (one
    // launch per call re-reads x, ids and the thin rows / columns of P and cannot keep update groups open across timesteps).  Steps
    // run in call order, so the queue holds the steps of one source at a time (queue_takes) and one function runs it (flush_lazy).
    struct SLAM_HANDLE_BLOCK StepQueue {
        enum Source { kNone, kSim, kHost, kDev } src = kNone;
        std::vector<float> cmds;                      // [steps][2]
        int ks = 0;                                   // detections per instance of this fill (host and device messages)
        int steps() const { return (int)(cmds.size() / 2); }
        // host messages (slam_step): each call packs its message into one of two pinned fills ([lazy_max][B][ks][3], [lazy_max][B],
        // [lazy_max][2]); the flush copies the fill on the copy stream, so packing the next fill overlaps the launch of the last one
        Stage host[2];
        int host_cur = 0;
        int host_ks = 2;                              // stride of the next host fill: the largest message seen so far
        // device messages (slam_step_dev): copied device-to-device at the call on the compute stream (so the caller may overwrite its
        // buffers in stream order, as with an immediate launch); one buffer suffices, since copies and launches share the stream
        DevBuf<float> dmeas; DevBuf<int32_t> dcount;  // [lazy_max][B][ks][3], [lazy_max][B]
    } q;                                                       // EKF: the queued steps of slam_step_sim, slam_step and slam_step_dev
    int eager_init = 2;                                        // first idle-GPU launch size (SLAM_EAGER_FLUSH, 0 = off)
    int eager_target = 2;                                      // queued steps an idle GPU is given at once (doubles per such launch)
    bool lazy_explicit = false;                                // slam_set_lazy_steps / SLAM_LAZY_STEPS asked for queueing: slam_step_dev queues only then
    int lazy_max = 32;                                         // 0 / 1 = off (SLAM_LAZY_STEPS, slam_set_lazy_steps); per launch a workgroup pays
                                                               // ~25 us of start / drain: 16 -> 61 M, 32 -> 66 M, 64 -> 70 M steps/s (one launch: 73 M)
    // slam_track_instance: instance `tracked` also runs in a one-instance SHADOW filter (same config, seed, map and GLOBAL
    // instance id, hence the same bits: results do not depend on how a batch is partitioned), stepped at once at every step
    // call on its own stream, so that slam_get_state(h, tracked) - the publishState of every tick, localization_node.cpp:139 -
    // does not have to run the batch's queued timesteps first.
    slam_handle* shadow = nullptr; int tracked = -1;
    std::vector<double> hmap;                  // host copy of the map (the shadow needs it)
    DevBuf<double> dscalar;
    DevBuf<unsigned long long> dprof;
    // the UKF kinds only
    struct SLAM_HANDLE_BLOCK Ukf {
        DevBuf<double> dsq; DevBuf<int32_t> dnsq;         // matrix square root scratch + its dimension
        DevBuf<double> dxprev;                            // x_t the last sigma points were drawn around
        DevBuf<double> dvt; DevBuf<int32_t> dvage;        // V^T of the last eigen-decomposition + warm-start age
        DevBuf<double> dbigws;                            // beyond the LDS size classes: [B][2 * pstride] scratch (ukf_big_kernel.hip)
        DevBuf<uint4> drot;                               // n <= 44: pass table of the fast sqrt kernel (launch_ukf_quad_table)
        DevBuf<uint8_t> dchol; bool chol = false;         // SLAM_UKF_SQRT_CHOLESKY is on; [B] "the Cholesky factor succeeded" (ukf_chol_kernel)
        hipStream_t aux_stream[3] = {nullptr, nullptr, nullptr}; hipEvent_t aux_ev[4] = {nullptr, nullptr, nullptr, nullptr};   // run_sim: the other parts of the batch
        int parts = 2;                                    // streams the batch is split over (SLAM_UKF_PARTS, 1..4)
        int split_min = 1024;                             // batch size from which it is used
        bool predicted = false; float pred_cmd[2] = {0.f, 0.f};   // slam_predict done, slam_update_dev pending
        bool pred_each = false;                           // slam_predict_each done, the pending update stage reads each.dcmd_each
        DevBuf<float> dmapf;                              // UKF_LOC: the known map as float32 [id, x, y] triplets
    } ukf;
    DevBuf<float> dcmds;                              // command sequence of a multi-step launch (slam_run_sim)
    int run_chunk = 0;                                // timesteps per launch in slam_run_sim (0 = all of them)
    int base = 3;                                     // state offset of the first landmark: 3 (EKF) or 4 (UKF)
    bool dump_meas = false;
    // per-instance inputs (the slam_*_each entry points).  slam_set_maps: one true map per instance, [B][map_stride][2] and [B] landmark
    // counts; while maps_each is set, L above is the largest count (the size-class and LDS decisions use it) and the kernels read these
    // instead of dmap.  Host copies for the shadow of slam_track_instance.
    struct SLAM_HANDLE_BLOCK Each {
        DevBuf<double> dmaps; DevBuf<int32_t> dLs; int map_stride = 0; bool maps_each = false;
        std::vector<double> hmaps; std::vector<int32_t> hLs;
        DevBuf<float> dcmd_each;                          // per-instance commands of the launches of one call: [T][B][2]
        // slam_set_noise_each: [B] packed rows the step kernels read (noise_each: they are set) and the caller's rows for the shadow
        DevBuf<slam::NoiseRow> dnoise; bool noise_each = false;
        std::vector<slam_noise> hnoise;
        DevBuf<float> dpose_each; DevBuf<double> dstart_each;   // slam_init_each: EKF [B][3] start poses; [B][4] UKF x_t heads + [B][3] true poses
    } each;
    // slam_consistency: [3][B] nees_full, nees_pose, map_rms and [2][B] dof, flags on the device; the packed triangles of one chunk of
    // instances (L_max > 50 only, grown on demand); what the last call had to read and its device time
    struct SLAM_HANDLE_BLOCK Cons {
        DevBuf<double> dcons, dcons_ws; DevBuf<int32_t> dconsi;
        double cons_bytes = 0.0, cons_ms = -1.0;
    } cons;
    // slam_map_score: [3][B] map_rms, max_err, nees_matched and [6][B] n_matched, n_duplicate, n_spurious, dof_matched, flags, slots with a
    // row on the device; [2][B][L_max] lm_err, lm_nees and [4][B][L_max] row, role, the list of MATCHED slots and their true rows; the
    // per-instance records [B][16], their partial records and the record; the two sums of the traffic model, what the last call read from
    // them and its device time.  The factorisation of full = 1 uses the workspace of `cons`.
    struct SLAM_HANDLE_BLOCK Score {
        DevBuf<double> dval, dslot, dinst, dpart, drec; DevBuf<int32_t> dint, dsloti; DevBuf<unsigned long long> dwork;
        double bytes = 0.0, ms = -1.0;
    } score;
    // slam_nav_*: the path (shared [P][2], or [B][stride][2] with [B] lengths), the controller state of every instance, the command log
    // of one chunk of ticks, ticks since the state was reset and the device times of the last slam_nav_run
    struct Nav {
        bool set = false, each = false;
        slam_nav_config cfg;
        int P = 0, stride = 0;
        DevBuf<double> dpath; DevBuf<int32_t> dP;
        DevBuf<int32_t> dhead, dfinish; DevBuf<double> dinteg, derrp;
        DevBuf<float> dlog;
        int tick = 0;
        bool time_ticks = false;   // slam_nav_set_timing: every per-tick run brackets one launch group of each tick with an event pair
        slam_capi::RunTimes times;
    } nav;
    // the events of a per-tick run (run_chunked): one pair per chunk and, while time_ticks is on, one per tick of a chunk.  One pool serves
    // every kind of run: a run returns synchronised, so two never overlap on a handle.
    std::vector<hipEvent_t> run_ev;
    // slam_monitor_*: the per-workgroup partial records of one evaluation, the records and the per-instance series of one chunk of ticks
    // ([series][ticks][B] doubles, [B] flags of slam_monitor_now) and the device times of the last slam_monitor_run
    struct Mon {
        DevBuf<double> dpart, drec, dlog; DevBuf<int32_t> dflags;
        slam_capi::RunTimes times;
    } mon;
    // slam_innovation_*: the staged message and per-instance commands of a host-fed evaluation (one chunk of ticks for the LOG source), the
    // per-instance outputs ([B] nis_sum, [B][12] post, [B][16] contributions, the partial records, the records and the nis_sum series of a
    // chunk; [B][64][6] detection slots when asked for; [3][ticks][B] n_upd, flags, n_new) and the device times of the last run
    struct Inn {
        DevBuf<float> dmeas, dcmd; DevBuf<int32_t> dcount;
        DevBuf<double> dval, ddet, dpart, drec, dlog; DevBuf<int32_t> dint;
        slam_capi::RunTimes times;
    } inn;
    // slam_gate_*: the filtered message of a gated step or of one tick of slam_gate_run ([B][k_stride][3] and [B] counts), [ticks][B] n_rej
    // and [B][64] verdicts, the device times of the last slam_gate_run.  Everything else is staged in `inn`.
    struct Gate {
        DevBuf<float> dmeas; DevBuf<int32_t> dcount, drej, dverdict;
        slam_capi::RunTimes times;
    } gate;
    // slam_associate_*: the labelled message of an associated step or of one tick of slam_associate_run ([B][k_stride][3] and [B] counts),
    // [5][ticks][B] n_match, n_new, n_drop, flags and landmarks compared with, [B][64] verdicts and slots, [B][64][4] detection slots, the three sums of the traffic
    // model, what the last synchronising call read and the device times of the last slam_associate_run.  The incoming message, the
    // per-instance contributions and the records are staged in `inn`.
    struct Assoc : slam_capi::Traffic {
        DevBuf<float> dmeas; DevBuf<int32_t> dcount, dint, dverdict, dslot; DevBuf<double> ddet;
    } assoc;
    // slam_associate_joint_*: as `assoc`, with [7][ticks][B] n_match, n_new, n_drop, flags, landmarks compared with, nodes and on-demand
    // blocks, [ticks][B] d2_joint and [B][64] candidate counts
    struct Joint : slam_capi::Traffic {
        DevBuf<float> dmeas; DevBuf<int32_t> dcount, dint, dverdict, dslot, dncand; DevBuf<double> ddet, dd2;
    } joint;
    // slam_remove_landmarks / slam_map_*: the track counters seen and expected ([B][L_max] each, allocated on first use and outside the
    // checkpoint format; tracked: they exist), the staged mask of a host-pointer removal ([B][L_max]), [2][ticks][B] n_removed and the M
    // before, the record, the three sums of the traffic model (work_set: a removal has filled them) and the device times of the last
    // slam_manage_run
    struct Map {
        DevBuf<int32_t> dseen, dexpected, dmask, dint; DevBuf<double> drec; DevBuf<unsigned long long> dwork;
        bool tracked = false, work_set = false;
        slam_capi::RunTimes times;
    } map;
    // slam_map_duplicates / slam_merge_landmarks / slam_map_merge: the partner row of every slot ([B][L_max]; a staged host array or what the
    // find wrote), the d2 of the slots' best candidates ([B][L_max], when asked for), the mask the fusion writes for the compaction
    // ([B][L_max]), [6][ticks][B] candidates that were not mutual, eligible, pairs fused, pairs attempted, slots removed and the M before,
    // the record, the five sums of the traffic model (work_set: a merge has filled them) and the device times of the last slam_manage_merge_run
    struct Merge {
        DevBuf<int32_t> dpartner, dmask, dint; DevBuf<double> dd2, drec; DevBuf<unsigned long long> dwork;
        bool work_set = false;
        slam_capi::RunTimes times;
    } merge;
    // slam_sense_* and the *_run_sim calls: the [B] sensor rows (rows_set: the kernels read them), the staged true poses [B][3] and the
    // timesteps they were staged at [B], the per-instance records [B][16] with their partial records and the record; pending: a sense
    // waits for its commit, made at RNG step pending_step.  The staged message and labels of slam_sense, and of one chunk of ticks of a
    // run: meas, count, origin, fault, the logged truth, position errors, commands and records.
    struct Sense {
        DevBuf<slam_sensor> drows; bool rows_set = false;
        DevBuf<double> dnext, dinst, dpart, drec; DevBuf<int32_t> dstaged;
        bool pending = false; uint32_t pending_step = 0;
        DevBuf<float> dmeas, dcmd; DevBuf<int32_t> dcount, dorigin, dfault; DevBuf<double> dtruth, derrpos, drecs;
    } sense;
    // slam_fix*: the [B] rows of the simulated source (rows_set: the kernel reads them); the staged rows, kinds, verdicts, nis and jumped
    // flags of a host-pointer call, and of one chunk of ticks of slam_fix_run ([ticks][B] each, the records [ticks][16]); the record; the two
    // sums of the traffic model (work_set: a fix has filled them) and the device times of the last slam_fix_run.  The per-instance
    // contributions and the partial records are staged in `inn`.
    struct Fix {
        DevBuf<slam_fix_sensor> drows; bool rows_set = false;
        DevBuf<double> dfix, dnis, drec, drecs; DevBuf<int32_t> dkinds, dverdict, djumped; DevBuf<unsigned long long> dwork;
        bool work_set = false;
        slam_capi::RunTimes times;
    } fix;
};

#pragma GCC visibility push(hidden)
namespace slam_capi {

using StepQueue = slam_handle::StepQueue;

// Room for n elements in a buffer of the handle that launches in flight may still use: they finish before it is replaced.  A buffer that
// has its size costs a comparison.
template <class T>
int grow(slam_handle* h, DevBuf<T>& buf, size_t n) {
    if (buf.cap() >= n) return SLAM_OK;
    if (buf) HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(buf.reserve(n));
    return SLAM_OK;
}

constexpr float kNoCmd[2] = {0.f, 0.f};   // the shared command of a launch whose commands are per instance (not read)

// slam_set_map or slam_set_maps has given the simulator a true map (inline: every per-tick call asks)
inline bool has_map(const slam_handle* h) { return h->dmap || h->each.maps_each; }

// no slam_sense waits for its slam_sense_commit (checked where a pending prediction stage is): the simulator's truth is staged, so nothing
// else may run the simulator or write a checkpoint
inline int sense_idle(const slam_handle* h, const char* who) {
    return h->sense.pending ? slam_internal_fail(SLAM_ERR_STATE, "a sense is pending: call slam_sense_commit before %s", who) : SLAM_OK;
}

// ---- capi_step.cpp (the functions without a comment here carry it at their definition)
// Every EKF step launch: T = 0 is one timestep with `cmd`; T > 0 is a multi-step launch over the device commands d_cmds, whose first
// command is `cmd`, with the messages of timestep t at meas + t * B * k_stride * 3 / count + t * B.  `sim` = the device-side generator, else
// messages of stride k_stride at meas / count; long_cap > 0: messages may exceed the size class (long_message_cap).
// The maps of slam_set_maps, if set, and per-instance commands d_cmd_each (device, [T][B][2]; NULL = the shared ones).
void fill_ekf_params(slam_handle* h, slam::EkfStepParams& p, const float cmd[2], int sim, int long_cap, const float* meas, const int32_t* count,
                     int k_stride, const float* d_cmds, int T, const float* d_cmd_each = nullptr);
// d_cmd_each: [B][2] per-instance commands of this timestep (device), NULL = cmd
void fill_ukf_params(slam_handle* h, slam::UkfStepParams& p, const float cmd[2], const float* d_cmd_each = nullptr);
int long_message_cap(slam_handle* h, int sim, int k_stride, int* cap_out);
// one timestep, either filter kind; `sim` = device-side measurement generator; d_cmd_each: [B][2] per-instance commands (device) or NULL
int launch_step(slam_handle* h, const float cmd[2], int sim, const float* d_meas, const int32_t* d_count, int k_stride,
                const float* d_cmd_each = nullptr);
int ensure_meas_buffers(slam_handle* h, int k_stride);
int upload_cmds_each(slam_handle* h, const float* cmds, int T);
int flush_lazy(slam_handle* h);

// ---- capi_consistency.cpp
// The launch parameters of launch_consistency at the handle's current state, with its output buffers and workspace reserved; *chunk_out:
// instances per launch of the workspace class.
int consistency_params(slam_handle* h, slam::ConsistencyParams* out, int* chunk_out);

// ---- capi_map.cpp
// slam_init / slam_init_each / slam_load_state: the track counters, where they exist, are zero again, in stream order
int map_track_reset(slam_handle* h);

// ---- capi_nav.cpp
// slam_init / slam_init_each / setting a path: head = 0, integ = err_prev = 0, finish_tick = -1 for every instance, in stream order
int nav_reset(slam_handle* h);

}  // namespace slam_capi
#pragma GCC visibility pop
