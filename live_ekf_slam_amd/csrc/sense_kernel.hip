// sense_kernel.hip — the simulator source with a sensor fault model (slam_sense, slam_sense_commit, the *_run_sim calls): sense_instance()
// of sense_kernel.h mapped to the device, the commit of the simulator's bookkeeping after the step, and the fixed-order sum of the records.
//
// Mapping of the sense kernel: ONE WAVEFRONT PER INSTANCE, four instances per 256-thread workgroup, as the innovation kernels.  The
// wavefront generates the clean message with sim_wave (the step kernels' generator, the step's RNG index) into its slice of LDS, then lane i
// takes the candidates i and i + 64 of the fault model.  Phases are ordered by wavefront fences: the wavefronts of a workgroup share
// nothing, there is no workgroup barrier.  An instance reads its map (16 L bytes), its pose, its noise and sensor rows and writes
// 12 k_stride bytes of message (8 k_stride more with both label rows), its staged pose and a record of 128 bytes.
// Commit: one thread per instance.  Record: launch_record_reduce (record_kernel.h) with the join mask kSenseRecMax, every entry a sum:
// no atomics, the order of every sum depends on the batch size alone.
#include <hip/hip_runtime.h>

#include "aux_device.h"
#include "sense_kernel.h"

namespace slam {
namespace {

static_assert(kSenseFrozen == SLAM_SENSE_INSTANCE_FROZEN && kSenseTooLong == SLAM_SENSE_TOO_LONG, "sense flags are slam_sense_flags");
static_assert(kSenseMaxDet == SLAM_SENSE_MAX_DET && kSenseMaxClutter == SLAM_SENSE_MAX_CLUTTER, "the exported limits");
static_assert(kInnovStatusFrozen == SLAM_INST_INDEX_OOR, "the status bit the step kernel returns on");

constexpr int kSenseWaves = 4;                      // instances per workgroup of the instance kernel
static_assert(kSenseRecLen == kRecLen, "the record launch_record_reduce takes");
static_assert(sizeof(SenseWork) * kSenseWaves <= 64 * 1024, "static LDS of a workgroup");

__global__ __launch_bounds__(64 * kSenseWaves) void sense_instance_kernel(const SenseParams p) {
    __shared__ SenseWork s_ws[kSenseWaves];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kSenseWaves + wave;
    if (b >= p.s.B) return;                          // (the whole wavefront; there is no workgroup barrier below)
    SenseWork& ws = s_ws[wave];
    const InnovWave w = {lane};
    const EkfStepParams& s = p.s;
    const int ks = p.k_stride;
    float* const mo = p.meas_out + (size_t)b * ks * 3;
    int32_t* const org = p.origin ? p.origin + (size_t)b * ks : nullptr;
    int32_t* const flt = p.fault ? p.fault + (size_t)b * ks : nullptr;
    double tx = s.truth[3 * (size_t)b], ty = s.truth[3 * (size_t)b + 1], tth = s.truth[3 * (size_t)b + 2];
    SenseResult v;
    int32_t staged = -2;
    if (s.flags[b] & kInnovStatusFrozen) {
        v = sense_frozen(w, ks, mo, org, flt);
    } else {
        const AuxCommand c = aux_command(s, b);
        const int Lm = sim_map_size(s, b);
        const double* const map = sim_map(s, b);
        const double lmx0 = lane < Lm ? map[2 * lane] : 0.0, lmy0 = lane < Lm ? map[2 * lane + 1] : 0.0;
        const int c_vis = sim_wave<kSenseMaxDet, false>(s, b, lane, c.fwd, c.ang, s.step, map, Lm, tx, ty, tth, lmx0, lmy0, ws.meas, sim_noise(s, b));
        w.sync();
        const slam_sensor row = p.rows ? p.rows[b] : sense_default_row();
        v = sense_instance(w, ws, row, s.seed, (uint64_t)(s.inst0 + b), s.step, c_vis, Lm, s.range_max, s.fov_min, s.fov_max, ks, mo, org, flt);
        staged = s.timestep[b];
    }
    if (lane == 0) {
        p.count_out[b] = v.count;
        p.truth_next[3 * (size_t)b] = tx; p.truth_next[3 * (size_t)b + 1] = ty; p.truth_next[3 * (size_t)b + 2] = tth;
        p.staged_ts[b] = staged;
        double r[kSenseRecLen];
        sense_record(v, ks, r);
#pragma unroll
        for (int i = 0; i < kSenseRecLen; ++i) p.inst_rec[(size_t)b * kSenseRecLen + i] = r[i];
    }
}

template <class ST>
__global__ __launch_bounds__(256) void sense_commit_kernel(const SenseCommitParams p) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const bool commit = p.timestep[b] == p.staged_ts[b] + 1;
    const double* const src = (commit ? p.truth_next : p.truth) + 3 * (size_t)b;
    const double tx = src[0], ty = src[1], tth = src[2];
    double e = 0.0;
    if (commit) {
        const ST* const xb = aux_row<ST>(p.x, b, p.xstride);
        p.truth[3 * (size_t)b] = tx; p.truth[3 * (size_t)b + 1] = ty; p.truth[3 * (size_t)b + 2] = tth;
        e = ekf_position_error((double)xb[0], (double)xb[1], tx, ty);
        p.err_sum[b] = p.err_sum[b] + e;
    }
    if (p.truth_out) { p.truth_out[3 * (size_t)b] = tx; p.truth_out[3 * (size_t)b + 1] = ty; p.truth_out[3 * (size_t)b + 2] = tth; }
    if (p.err_pos) p.err_pos[b] = commit ? e : __builtin_nan("");
    p.inst_rec[(size_t)b * kSenseRecLen + kSenCommitted] = commit ? 1.0 : 0.0;
    p.inst_rec[(size_t)b * kSenseRecLen + kSenErrSum] = e;
}

}  // namespace

hipError_t launch_sense(const SenseParams& p, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    if (s.B <= 0 || p.k_stride <= 0 || !p.meas_out || !p.count_out || !p.truth_next || !p.staged_ts || !p.inst_rec || !s.truth || !s.flags ||
        !s.timestep || (!s.map && !s.map_each) || (p.rec && !p.partials))
        return hipErrorInvalidValue;
    const int groups = (s.B + kSenseWaves - 1) / kSenseWaves;
    (void)hipGetLastError();   // sticky and per thread: only these launches' errors are reported (capi_internal.h)
    hipLaunchKernelGGL(sense_instance_kernel, dim3(groups), dim3(64 * kSenseWaves), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess || !p.rec) return e;
    return launch_record_reduce<kSenseRecMax>(p.inst_rec, s.B, p.partials, p.rec, stream);
}

hipError_t launch_sense_commit(const SenseCommitParams& p, hipStream_t stream) {
    if (p.B <= 0 || !p.x || p.xstride < 3 || !p.timestep || !p.staged_ts || !p.truth || !p.truth_next || !p.err_sum || !p.inst_rec ||
        (p.rec && !p.partials))
        return hipErrorInvalidValue;
    const hipError_t e = aux_launch(p.f32_storage, sense_commit_kernel<float>, sense_commit_kernel<double>, dim3((p.B + 255) / 256), dim3(256), 0,
                                    stream, p);
    if (e != hipSuccess || !p.rec) return e;
    return launch_record_reduce<kSenseRecMax>(p.inst_rec, p.B, p.partials, p.rec, stream);
}

}  // namespace slam
