// gate_kernel.h — innovation gating of the detections of the message the next EKF step will process (slam_gate, slam_step_gated,
// slam_gate_run; gfx950): the chi-square gate on the individual NIS, with the EKF step kernels untouched.
//
// The replay of innovation_kernel.h runs with the policy InnovGate: an update slot whose nis is finite and exceeds the gate is REJECTED, its
// update is not applied in the replay, and at the end the message is written out with the rejected detections taken out, in message order.
// The unmodified step then consumes the filtered message and computes exactly what the gated replay computed: an update slot is a found
// id, and the insertion, skip and freeze decisions of the plan look only at ids that were not found, so removing an update slot changes no
// other slot's plan; and the replay is exact on any block that contains the J of the filtered message.  A gated step therefore equals,
// byte for byte, a plain step on the host-filtered message.
//
// gate_instance_host() is the host side of the definition (slam_gate_instance_host): innovation_instance() and the compaction as a
// plain loop; the device (gate_kernel.hip) compacts by ballot and popcount, one lane per detection.
// Output message of an instance with count_in = clamp(count, 0, k_stride) detections:
//   gated             the kept detections (verdict != 2) in message order, count_out = their number, the triplets count_out .. count_in - 1
//                     written as 0.0f, nothing from count_in up
//   passed through    (INSTANCE_FROZEN, WOULD_FREEZE, TOO_LONG) the first count_in triplets copied when the output is not the input,
//                     count_out = count as given
#pragma once
#include "innovation_kernel.h"

namespace slam {

constexpr int kGateRej = kInnReserved;   // entry 15 of a gate record: rejected detections

SLAM_HD bool gate_passes_through(int32_t flags) { return (flags & (kInnovFrozen | kInnovWouldFreeze | kInnovTooLong)) != 0; }

// what one instance adds to a gate record: entries 0 - 14 as innovation_record (5 and 7 - 14 over the accepted updates), 15 = n_rej
SLAM_HD void gate_record(const InnovResult& v, int32_t n_rej, double r[kInnovRecLen]) {
    innovation_record(v, r);
    r[kGateRej] = (double)n_rej;
}

// One instance on the host.  meas: the message, count its detection count as given, k_stride the row's capacity (meas holds
// clamp(count, 0, k_stride) triplets); the other arguments as innovation_instance.  meas_out [k_stride][3] may be meas itself.
template <class LX, class LP>
InnovResult gate_instance_host(InnovWork& ws, LX load_x, LP load_P, const int32_t* ids, int M, int L_max, int32_t status, float fwd, float ang,
                               const float* meas, int count, int k_stride, const InnovNoise& nz, bool lm_from_pred, double lo, double hi,
                               double gate, double* det, float* meas_out, int32_t* count_out, int32_t* n_rej, int32_t* verdict) {
    int k = count < k_stride ? count : k_stride;
    k = k < 0 ? 0 : k;
    for (int i = 0; i < 3 * (k < kInnovMaxDet ? k : kInnovMaxDet); ++i) ws.meas[i] = meas[i];
    int32_t vd[kInnovMaxDet];
    InnovGate g = {gate, vd, 0};
    const InnovResult v = innovation_instance(InnovSeq(), ws, load_x, load_P, ids, M, L_max, status, fwd, ang, k, nz, lm_from_pred, lo, hi, det, &g);
    if (gate_passes_through(v.flags)) {
        if (meas_out && meas_out != meas)
            for (int i = 0; i < 3 * k; ++i) meas_out[i] = meas[i];
        if (count_out) *count_out = count;
    } else {
        int kept = 0;
        for (int l = 0; l < k; ++l) {
            if (vd[l] == kGateRejected) continue;
            if (meas_out)
                for (int i = 0; i < 3; ++i) meas_out[3 * kept + i] = ws.meas[3 * l + i];
            kept += 1;
        }
        if (meas_out)
            for (int i = 3 * kept; i < 3 * k; ++i) meas_out[i] = 0.0f;
        if (count_out) *count_out = kept;
    }
    if (n_rej) *n_rej = g.n_rej;
    if (verdict)
        for (int l = 0; l < kInnovMaxDet; ++l) verdict[l] = vd[l];
    return v;
}

#if defined(__HIPCC__)
// One gating of every instance on `stream`: three launches (the instances with their filtered messages, then the record as
// launch_innovation reduces it, join mask kInnovRecMax).  in.s is what the step that follows is launched with, message source meas_in / meas_count_in /
// k_stride_in (never the simulator).  meas_out / count_out may be the input pair itself (in place: the message is in LDS before anything is
// written) and must not overlap it otherwise.
struct GateParams {
    InnovParams in;
    double gate;
    float* meas_out;        // [B][k_stride_in][3]
    int32_t* count_out;     // [B]
    int32_t* n_rej;         // [B] or NULL
    int32_t* verdict;       // [B][kInnovMaxDet] or NULL
};
hipError_t launch_gate(const GateParams& p, int f32_storage, hipStream_t stream);
#endif

}  // namespace slam
