// assoc_kernel.hip — maximum-likelihood association of the detections of an id-less message with the landmarks of every instance of a
// batch (slam_associate, slam_step_associated, slam_associate_run).  The definition is associate_instance() (assoc_kernel.h); this file
// maps it to the device.
//
// Mapping: ONE WAVEFRONT PER INSTANCE, kAssocWaves instances per workgroup, as innovation_instance_kernel; the message and the
// per-detection results in the wavefront's slice of LDS, phases ordered by wavefront fences, no workgroup barrier.
//   costs      lanes over landmark slots j, 64 at a time.  A lane forms its landmark's predicted 5 x 5 block, H, S and Si once, in
//              registers, from rows 0 - 2 of P (lane j reads the adjacent columns ii, ii + 1: contiguous over the lanes), P[ii .. ii + 1][0 .. 2]
//              (a stride of two rows between lanes: one cache line per row) and the 2 x 2 diagonal block; both triangles are read, since P
//              is symmetric only to rounding and the innovation replay reads both.  Then the lanes walk the message in LDS (every lane the
//              same detection: a broadcast, no bank conflict) and each step ends in a butterfly arg-min over the wavefront with the
//              (value, j) tie-break: cross-lane operations, no atomics on values.
//   decisions  lanes over detections (a message is at most 64): the conflicts from the LDS arrays (lane l element l: consecutive banks;
//              the scan over the other detections reads one element in all lanes: broadcasts), ranks and output positions by ballot and
//              popcount, so message order is preserved without a scan loop.
// The whole message is in LDS before the first write, so the output row may be the input row.
// Record: the per-instance contributions go through launch_record_reduce (record_kernel.h, join mask kAssocRecMax): a fixed order that
// depends on the batch size alone.  The traffic model (slam_last_associate_work) is summed by a launch of its own (launch_work_sum) after
// a call or a chunk of ticks, in integers, from the per-instance counts.  All arithmetic is fp64, unfused.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "assoc_kernel.h"
#include "aux_device.h"

namespace slam {
namespace {

static_assert(kAssocNone == SLAM_ASSOC_NONE && kAssocMatched == SLAM_ASSOC_MATCHED && kAssocNew == SLAM_ASSOC_NEW &&
              kAssocAmbiguous == SLAM_ASSOC_AMBIGUOUS && kAssocConflict == SLAM_ASSOC_CONFLICT && kAssocNoRoom == SLAM_ASSOC_NO_ROOM &&
              kAssocInvalid == SLAM_ASSOC_INVALID, "verdicts are slam_assoc_verdict");

static_assert(kInnovRecLen == kRecLen, "the record launch_record_reduce takes");

constexpr int kAssocWaves = 4;                      // instances per workgroup
static_assert(sizeof(AssocWork) * kAssocWaves <= 64 * 1024, "static LDS of a workgroup");

template <class ST>
__global__ __launch_bounds__(64 * kAssocWaves) void assoc_instance_kernel(const AssocParams p) {
    __shared__ AssocWork s_ws[kAssocWaves];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kAssocWaves + wave;
    const EkfStepParams& s = p.s;
    if (b >= s.B) return;                            // (the whole wavefront; there is no workgroup barrier below)
    AssocWork& ws = s_ws[wave];
    const AssocWave w = {lane};
    const AuxInstance<ST> inst(s, b);
    const AuxMessage msg(s, b);
    msg.stage(lane, ws.meas);
    w.sync();
    const int M = inst.M;
    const size_t bd = (size_t)b * kInnovMaxDet;
    // (every index the loaders see is below 3 + 2 M: a lane's landmark is j < M, or landmark 0 while M > 0)
    const AssocResult v = associate_instance(
        w, ws, inst.load_x(), inst.load_P(), inst.ids, M, s.L_max, inst.status, inst.fwd, inst.ang, msg.k, inst.nz, p.gate_match, p.gate_new,
        nullptr, p.verdict ? p.verdict + bd : nullptr, p.slot ? p.slot + bd : nullptr, p.det ? p.det + bd * kAssocDetLen : nullptr,
        p.meas_out + (size_t)b * s.k_stride_in * 3);
    if (lane == 0) {
        p.count_out[b] = v.count_out;
        if (p.n_match) p.n_match[b] = v.n_match;
        if (p.n_new) p.n_new[b] = v.n_new;
        if (p.n_drop) p.n_drop[b] = v.n_drop;
        if (p.flags) p.flags[b] = v.flags;
        double r[kInnovRecLen];
        assoc_record(v, r);
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) p.inst_rec[(size_t)b * kInnovRecLen + i] = r[i];
        if (p.n_lm) p.n_lm[b] = v.flags ? -1 : M;     // (what the traffic model needs besides the counts)
    }
}

// element i of the traffic model's sum: one instance-tick
struct AssocWorkTerms {
    const int32_t *n_lm, *n_match, *n_new, *n_drop;
    int esz;
    __device__ void operator()(size_t i, unsigned long long (&t)[3]) const {
        // (n_lm < 0: an instance that emits an empty message: the counts; its zeroed row is not known here)
        const AssocTraffic w = n_lm[i] >= 0 ? assoc_traffic(n_lm[i], n_match[i] + n_new[i] + n_drop[i], esz) : AssocTraffic{0ull, 8ull, 0ull};
        t[0] = w.p_elems; t[1] = w.other_bytes; t[2] = w.p_lines;
    }
};

}  // namespace

hipError_t launch_associate_work(const int32_t* n_lm, const int32_t* n_match, const int32_t* n_new, const int32_t* n_drop, size_t n, int esz,
                                 unsigned long long* work, hipStream_t stream) {
    if (!n_lm || !n_match || !n_new || !n_drop) return hipErrorInvalidValue;
    return launch_work_sum<3>(AssocWorkTerms{n_lm, n_match, n_new, n_drop, esz}, n, work, stream);
}

hipError_t launch_associate(const AssocParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    if (!aux_shape_ok(s.B, s.L_max, s.xstride, s.pstride, f32_storage) || !p.inst_rec || !p.partials || !p.rec) return hipErrorInvalidValue;
    if (s.sim || !s.meas_in || !s.meas_count_in || s.k_stride_in <= 0 || !p.meas_out || !p.count_out || !(p.gate_match > 0.0) ||
        !(p.gate_match <= p.gate_new))
        return hipErrorInvalidValue;
    const int groups = (s.B + kAssocWaves - 1) / kAssocWaves;
    const hipError_t e = aux_launch(f32_storage, assoc_instance_kernel<float>, assoc_instance_kernel<double>, dim3(groups), dim3(64 * kAssocWaves), 0,
                                    stream, p);
    if (e != hipSuccess) return e;
    return launch_record_reduce<kAssocRecMax>(p.inst_rec, s.B, p.partials, p.rec, stream);
}

}  // namespace slam
