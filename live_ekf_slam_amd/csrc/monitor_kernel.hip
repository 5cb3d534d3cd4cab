// monitor_kernel.hip — one monitor evaluation of every instance of a batch (slam_monitor_now, slam_monitor_run).
//
// Mapping: ONE LANE PER INSTANCE, 256 instances per workgroup.  An instance needs 3 (4) elements of x, the leading 3 x 3 block of P (three
// short reads, pstride apart between instances and one row apart within), the truth, M and the status word: about 150 bytes against the
// 171 KB its timestep moves at L = 50, followed by some fifty dependent fp64 operations with three square roots and six divisions.  There is
// nothing for the lanes of a wavefront to share and nothing to stage, so the kernel is bound by the latency of its loads, and the batch's
// 256 workgroups (B = 65 536) fill the device once.
// Reduction: every workgroup ends in record_block_tree (record_kernel.h) over its 256 consecutive instances and writes one partial record,
// fused with the evaluation; launch_record_total then joins the partials in ascending order.  The join mask is kMonRecMax (entries
// kMonMaxPos and kMonMaxYaw are maxima).  No atomics on values: the order of every sum depends on B alone.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "monitor_kernel.h"

namespace slam {
namespace {

static_assert(kMonFlagPoseNotPd == SLAM_CONSISTENCY_POSE_NOT_PD && kMonFlagFailed == SLAM_CONSISTENCY_INSTANCE_FAILED, "monitor flags are slam_consistency_flags");
static_assert(kMonStatusDead == (SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG), "the status bits that leave an undefined state");
static_assert(kMonRecLen == kRecLen, "the record record_block_tree takes");

template <class ST>
__global__ __launch_bounds__(kRecBlock) void monitor_tick_kernel(const MonitorParams p) {
    __shared__ double s_part[kRecBlock / 64][kRecLen];
    const int b = blockIdx.x * kRecBlock + threadIdx.x;
    double r[kMonRecLen];
#pragma unroll
    for (int i = 0; i < kMonRecLen; ++i) r[i] = 0.0;
    if (b < p.B) {
        const int m = aux_clamp_m(p.M[b], p.L_max);
        const ST* __restrict__ xb = aux_row<ST>(p.x, b, p.xstride);
        double x[4], P3[9], truth[3];
        x[0] = (double)xb[0]; x[1] = (double)xb[1]; x[2] = (double)xb[2];
        x[3] = p.ukf ? (double)xb[3] : 0.0;                                 // (xstride >= 4 for every kind)
#pragma unroll
        for (int i = 0; i < 9; ++i) P3[i] = 0.0;
        if (!p.ukf) {                                                       // rows 0 .. 2 of P_t: 3 <= ld, 3 ld <= pstride
            const int ld = ekf_ld(3 + 2 * m, (int)sizeof(ST));
            const ST* __restrict__ Pb = aux_row<ST>(p.P, b, p.pstride);
#pragma unroll
            for (int i = 0; i < 3; ++i)
#pragma unroll
                for (int j = 0; j < 3; ++j) P3[3 * i + j] = (double)Pb[(size_t)i * ld + j];
        }
        truth[0] = p.truth[3 * (size_t)b]; truth[1] = p.truth[3 * (size_t)b + 1]; truth[2] = p.truth[3 * (size_t)b + 2];
        const MonitorValue v = monitor_instance(x, P3, truth, p.status[b], p.ukf != 0);
        if (p.err_pos) p.err_pos[b] = v.err_pos;
        if (p.err_yaw) p.err_yaw[b] = v.err_yaw;
        if (p.nees_pose) p.nees_pose[b] = v.nees_pose;
        if (p.flags) p.flags[b] = v.flags;
        if (v.flags & kMonFlagFailed) {
            r[kMonFailed] = 1.0;
        } else {
            const double ay = fabs(v.err_yaw);
            r[kMonOk] = 1.0;
            r[kMonSumPos] = v.err_pos; r[kMonSumPos2] = v.err_pos * v.err_pos; r[kMonMaxPos] = v.err_pos;
            r[kMonSumYaw2] = v.err_yaw * v.err_yaw; r[kMonMaxYaw] = ay;
            r[kMonSumM] = (double)m;
            if (v.flags & kMonFlagPoseNotPd) r[kMonPoseNotPd] = 1.0;
            if (mon_finite(v.nees_pose)) {
                r[kMonNees] = 1.0; r[kMonSumNees] = v.nees_pose;
                if (v.nees_pose < p.nees_lo) r[kMonBelow] = 1.0;
                if (v.nees_pose > p.nees_hi) r[kMonAbove] = 1.0;
            }
        }
        if (p.nees_full) {
            const double nf = p.nees_full[b];
            if (mon_finite(nf)) { r[kMonFull] = 1.0; r[kMonSumFull] = nf; r[kMonSumDof] = (double)p.dof[b]; }
        }
    }
    // (a lane past the batch contributes zeros, which change no sum of non-negative terms and no maximum)
    record_block_tree(r, kMonRecMax, s_part, p.partials + (size_t)blockIdx.x * kRecLen);
}

}  // namespace

hipError_t launch_monitor(const MonitorParams& p, int f32_storage, hipStream_t stream) {
    if (p.B <= 0 || !p.partials || !p.rec || p.xstride < 4 || (!p.ukf && p.pstride < 3 * ekf_ld(3 + 2 * p.L_max, f32_storage ? 4 : 8)))
        return hipErrorInvalidValue;
    const int blocks = record_blocks(p.B);
    const hipError_t e = aux_launch(f32_storage, monitor_tick_kernel<float>, monitor_tick_kernel<double>, dim3(blocks), dim3(kRecBlock), 0, stream, p);
    if (e != hipSuccess) return e;
    return launch_record_total<kMonRecMax>(p.partials, blocks, p.rec, stream);
}

}  // namespace slam
