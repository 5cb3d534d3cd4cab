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
// Record: the per-instance contributions go through innovation_reduce_kernel and innovation_sum_kernel (launch_innovation_reduce): a
// fixed order that depends on the batch size alone.  The traffic model (slam_last_associate_work) is summed by a launch of its own after a
// call or a chunk of ticks, in integers, from the per-instance counts.  All arithmetic is fp64, unfused.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "assoc_kernel.h"
#include "ekf_kernel.h"
#include "sim_device.h"

namespace slam {
namespace {

static_assert(kAssocNone == SLAM_ASSOC_NONE && kAssocMatched == SLAM_ASSOC_MATCHED && kAssocNew == SLAM_ASSOC_NEW &&
              kAssocAmbiguous == SLAM_ASSOC_AMBIGUOUS && kAssocConflict == SLAM_ASSOC_CONFLICT && kAssocNoRoom == SLAM_ASSOC_NO_ROOM &&
              kAssocInvalid == SLAM_ASSOC_INVALID, "verdicts are slam_assoc_verdict");

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
    const StepNoise sn = step_noise(s, b);
    const InnovNoise nz = {sn.v_d, sn.v_th, sn.w_r, sn.w_b, sn.V00, sn.V11, sn.W00, sn.W11};
    const int32_t status = s.flags[b];
    const float* const cp = s.cmd_each ? s.cmd_each + 2 * (size_t)b : nullptr;
    const float fwd = cp ? cp[0] : s.fwd, ang = cp ? cp[1] : s.ang;
    const int count = s.meas_count_in[b];
    int k = count < s.k_stride_in ? count : s.k_stride_in;
    k = k < 0 ? 0 : k;
    const float* const src = s.meas_in + (size_t)b * s.k_stride_in * 3;
    if (k <= kInnovMaxDet)
        for (int i = lane; i < 3 * k; i += 64) ws.meas[i] = src[i];
    w.sync();
    int M = s.M[b];
    M = M < 0 ? 0 : (M > s.L_max ? s.L_max : M);
    const int ld = ekf_ld(3 + 2 * M, (int)sizeof(ST));
    const ST* __restrict__ const xb = static_cast<const ST*>(s.x) + (size_t)b * s.xstride;
    const ST* __restrict__ const Pb = static_cast<const ST*>(s.P) + (size_t)b * s.pstride;
    const size_t bd = (size_t)b * kInnovMaxDet;
    // (every index the loaders see is below 3 + 2 M: a lane's landmark is j < M, or landmark 0 while M > 0)
    const AssocResult v = associate_instance(
        w, ws, [&](int i) { return (double)xb[i]; }, [&](int r, int c) { return (double)Pb[(size_t)r * ld + c]; }, s.ids + (size_t)b * s.L_max, M,
        s.L_max, status, fwd, ang, k, nz, p.gate_match, p.gate_new, nullptr, p.verdict ? p.verdict + bd : nullptr, p.slot ? p.slot + bd : nullptr,
        p.det ? p.det + bd * kAssocDetLen : nullptr, p.meas_out + (size_t)b * s.k_stride_in * 3);
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

// The traffic model summed over n instance-ticks, in integers (the order of the additions does not matter): a grid-stride sum per lane,
// a shuffle tree per wavefront, one atomic add per wavefront and sum.
__global__ __launch_bounds__(256) void assoc_work_kernel(const int32_t* __restrict__ n_lm, const int32_t* __restrict__ n_match,
                                                         const int32_t* __restrict__ n_new, const int32_t* __restrict__ n_drop, size_t n, int esz,
                                                         unsigned long long* __restrict__ work) {
    unsigned long long a0 = 0, a1 = 0, a2 = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int M = n_lm[i];
        AssocTraffic t;
        if (M >= 0) t = assoc_traffic(M, n_match[i] + n_new[i] + n_drop[i], esz);
        else t = AssocTraffic{0ull, 8ull, 0ull};   // an instance that emits an empty message: the counts (its zeroed row is not known here)
        a0 += t.p_elems; a1 += t.other_bytes; a2 += t.p_lines;
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        a0 += __shfl_down(a0, off, 64); a1 += __shfl_down(a1, off, 64); a2 += __shfl_down(a2, off, 64);
    }
    if (threadIdx.x % 64 == 0) { atomicAdd(work, a0); atomicAdd(work + 1, a1); atomicAdd(work + 2, a2); }
}

}  // namespace

hipError_t launch_associate_work(const int32_t* n_lm, const int32_t* n_match, const int32_t* n_new, const int32_t* n_drop, size_t n, int esz,
                                 unsigned long long* work, hipStream_t stream) {
    if (!n_lm || !n_match || !n_new || !n_drop || !work || n == 0) return hipErrorInvalidValue;
    const size_t want = (n + 255) / 256;
    hipLaunchKernelGGL(assoc_work_kernel, dim3((unsigned)(want < 256 ? want : 256)), dim3(256), 0, stream, n_lm, n_match, n_new, n_drop, n, esz, work);
    return hipGetLastError();
}

hipError_t launch_associate(const AssocParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    const int n_max = 3 + 2 * s.L_max;
    if (s.B <= 0 || s.L_max < 0 || !p.inst_rec || !p.partials || !p.rec || s.xstride < n_max ||
        (long long)s.pstride < (long long)n_max * ekf_ld(n_max, f32_storage ? 4 : 8))
        return hipErrorInvalidValue;
    if (s.sim || !s.meas_in || !s.meas_count_in || s.k_stride_in <= 0 || !p.meas_out || !p.count_out || !(p.gate_match > 0.0) ||
        !(p.gate_match <= p.gate_new))
        return hipErrorInvalidValue;
    const int groups = (s.B + kAssocWaves - 1) / kAssocWaves;
    (void)hipGetLastError();   // sticky and per thread: only these launches' errors are reported (capi_internal.h)
    if (f32_storage) hipLaunchKernelGGL(assoc_instance_kernel<float>, dim3(groups), dim3(64 * kAssocWaves), 0, stream, p);
    else hipLaunchKernelGGL(assoc_instance_kernel<double>, dim3(groups), dim3(64 * kAssocWaves), 0, stream, p);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_innovation_reduce(p.inst_rec, s.B, p.partials, p.rec, stream);
}

}  // namespace slam
