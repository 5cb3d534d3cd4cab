// gate_kernel.hip — the chi-square gate on the detections of the message the next EKF step will process, for every instance of a batch
// (slam_gate, slam_step_gated, slam_gate_run).  The definition is innovation_instance() with the policy InnovGate
// (innovation_kernel.h) and the output rules of gate_kernel.h; this file maps them to the device.
//
// Mapping: that of innovation_instance_kernel - ONE WAVEFRONT PER INSTANCE, kGateWaves instances per workgroup, the block of P, the
// message and the verdicts in the wavefront's slice of LDS, phases ordered by wavefront fences, no workgroup barrier.  After the replay
// the wavefront writes the filtered message: a message is at most 64 detections, one lane each; the kept mask is the ballot of
// verdict != 2, a kept detection's position the popcount of the mask below its lane, so message order is preserved without a scan loop.
// The whole message is in LDS before the first write, so the output row may be the input row.  Instances that pass through (frozen, would
// freeze, too long) copy their row from global memory when the output is another buffer.
// Record: the per-instance contributions (an innovation record with entry 15 = rejected detections, join mask kInnovRecMax) go through
// launch_record_reduce (record_kernel.h): a fixed order that depends on the batch size alone, no atomics on values.  All arithmetic is
// fp64, unfused.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "gate_kernel.h"

namespace slam {
namespace {

static_assert(kGateNone == SLAM_GATE_NOT_UPDATE && kGateAccepted == SLAM_GATE_ACCEPTED && kGateRejected == SLAM_GATE_REJECTED, "verdicts are slam_gate_verdict");
static_assert(kInnovMaxDet == 64, "one lane per detection of a message");

constexpr int kGateWaves = 4;                       // instances per workgroup
static_assert((sizeof(InnovWork) + sizeof(int32_t) * kInnovMaxDet) * kGateWaves <= 64 * 1024, "static LDS of a workgroup");

template <class ST>
__global__ __launch_bounds__(64 * kGateWaves) void gate_instance_kernel(const GateParams p) {
    __shared__ InnovWork s_ws[kGateWaves];
    __shared__ int32_t s_verdict[kGateWaves][kInnovMaxDet];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kGateWaves + wave;
    const EkfStepParams& s = p.in.s;
    if (b >= s.B) return;                            // (the whole wavefront; there is no workgroup barrier below)
    InnovWork& ws = s_ws[wave];
    const InnovWave w = {lane};
    const AuxInstance<ST> inst(s, b);
    const AuxMessage msg(s, b);
    const int count = msg.count, k = msg.k;
    const float* const src = msg.src;
    float* const dst = p.meas_out + (size_t)b * s.k_stride_in * 3;
    msg.stage(lane, ws.meas);
    w.sync();
    double* const det = p.in.det ? p.in.det + (size_t)b * kInnovMaxDet * kInnovDetLen : nullptr;
    InnovGate g = {p.gate, s_verdict[wave], 0};
    // (every index the loaders see is below 3 + 2 M: the block's landmarks come from ids[0 .. M))
    const InnovResult v = innovation_instance(w, ws, inst.load_x(), inst.load_P(), inst.ids, inst.M, s.L_max, inst.status, inst.fwd, inst.ang, k,
                                              inst.nz, s.lm_from_pred != 0, p.in.nis_lo, p.in.nis_hi, det, &g);
    w.sync();                                        // the verdicts lane 0 wrote
    const int32_t vd = s_verdict[wave][lane];
    if (p.verdict) p.verdict[(size_t)b * kInnovMaxDet + lane] = vd;
    int count_out = count;
    if (gate_passes_through(v.flags)) {              // (wave-uniform: every lane holds the same result)
        if (dst != src)
            for (int i = lane; i < 3 * k; i += 64) dst[i] = src[i];
    } else {                                         // k <= 64 here, and every output index is below 3 k <= 3 k_stride
        const bool keep = lane < k && vd != kGateRejected;
        const unsigned long long mask = __ballot(keep);
        const int pos = __popcll(mask & ((1ull << lane) - 1ull));
        const int kept = __popcll(mask);
        if (keep) {
            dst[3 * pos] = ws.meas[3 * lane]; dst[3 * pos + 1] = ws.meas[3 * lane + 1]; dst[3 * pos + 2] = ws.meas[3 * lane + 2];
        } else if (lane < k) {                       // the rejected lanes zero the tail kept .. k - 1, one triplet each
            const int t = kept + (lane - pos);       // lane - pos = rejected detections below this lane
            dst[3 * t] = 0.0f; dst[3 * t + 1] = 0.0f; dst[3 * t + 2] = 0.0f;
        }
        count_out = kept;
    }
    if (lane == 0) {
        p.count_out[b] = count_out;
        if (p.n_rej) p.n_rej[b] = g.n_rej;
        if (p.in.post)
#pragma unroll
            for (int i = 0; i < 12; ++i) p.in.post[(size_t)b * 12 + i] = v.post[i];
        if (p.in.nis_sum) p.in.nis_sum[b] = v.nis_sum;
        if (p.in.n_upd) p.in.n_upd[b] = v.n_upd;
        if (p.in.n_new) p.in.n_new[b] = v.n_new;
        if (p.in.flags) p.in.flags[b] = v.flags;
        double r[kInnovRecLen];
        gate_record(v, g.n_rej, r);
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) p.in.inst_rec[(size_t)b * kInnovRecLen + i] = r[i];
    }
}

}  // namespace

hipError_t launch_gate(const GateParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.in.s;
    if (!aux_shape_ok(s.B, s.L_max, s.xstride, s.pstride, f32_storage) || !p.in.inst_rec || !p.in.partials || !p.in.rec) return hipErrorInvalidValue;
    if (s.sim || !s.meas_in || !s.meas_count_in || s.k_stride_in <= 0 || !p.meas_out || !p.count_out || !(p.gate > 0.0)) return hipErrorInvalidValue;
    const int groups = (s.B + kGateWaves - 1) / kGateWaves;
    const hipError_t e = aux_launch(f32_storage, gate_instance_kernel<float>, gate_instance_kernel<double>, dim3(groups), dim3(64 * kGateWaves), 0,
                                    stream, p);
    if (e != hipSuccess) return e;
    return launch_record_reduce<kInnovRecMax>(p.in.inst_rec, s.B, p.in.partials, p.in.rec, stream);
}

}  // namespace slam
