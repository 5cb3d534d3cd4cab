// innovation_kernel.hip — the innovation statistics of the message the next EKF step will process, for every instance of a batch
// (slam_innovation, slam_innovation_run).  The definition is innovation_instance() in innovation_kernel.h; this file maps it to the device.
//
// Mapping: ONE WAVEFRONT PER INSTANCE, kInnovWaves instances per workgroup.  An instance needs x[J] and the J x J block of P
// (J = pose + the mapped landmarks of its message: 7 x 7 at the mean message of 1.65 detections, at most 35 x 35), its ids and its message:
// about half a kilobyte against the 171 KB its timestep moves at L = 50.  The block lives in the wavefront's slice of LDS (12.3 KB); the
// lanes gather it (element loads: a landmark's pair of columns starts at an odd index, so it is not a 16-byte aligned pair in either
// storage type), look ids up by ballot, and take the columns of H P, the rows of K and the elements of the downdate; the scalar chain of a
// detection (Jacobian entries, atan2, the 2 x 2 inverse) is evaluated by every lane alike.  Phases are ordered by wavefront fences: no
// workgroup barrier, the wavefronts of a workgroup share nothing.  Simulator source: the wavefront first regenerates the message the step
// will generate (sim_wave with the step's RNG index: the generator is counter based) from the instance's truth, which is read, not written.
// Record: every instance leaves its contribution (16 doubles); a second launch reduces 256 consecutive instances per workgroup by a fixed
// tree (shuffles within a wavefront, then the four wavefronts in order), a third adds the partial records in ascending order.  No atomics
// on values: the order of every sum depends on the batch size alone.  Everything is read only, except the outputs.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "ekf_kernel.h"
#include "innovation_kernel.h"
#include "sim_device.h"

namespace slam {
namespace {

static_assert(kInnovFrozen == SLAM_INNOVATION_INSTANCE_FROZEN && kInnovWouldFreeze == SLAM_INNOVATION_WOULD_FREEZE &&
              kInnovSingular == SLAM_INNOVATION_S_SINGULAR && kInnovTooLong == SLAM_INNOVATION_TOO_LONG, "innovation flags are slam_innovation_flags");
static_assert(kInnovStatusFrozen == SLAM_INST_INDEX_OOR, "the status bit the step kernel returns on");
static_assert(kInnovMaxDet == SLAM_INNOV_MAX_DET && kInnovMaxLm == SLAM_INNOV_MAX_LM, "the exported limits");
static_assert(kInnovBlock % 64 == 0, "whole wavefronts");

constexpr int kInnovWaves = 4;                      // instances per workgroup of the instance kernel
constexpr int kRedWaves = kInnovBlock / 64;
static_assert(sizeof(InnovWork) * kInnovWaves <= 64 * 1024, "static LDS of a workgroup");

template <class ST>
__global__ __launch_bounds__(64 * kInnovWaves) void innovation_instance_kernel(const InnovParams p) {
    __shared__ InnovWork s_ws[kInnovWaves];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kInnovWaves + wave;
    if (b >= p.s.B) return;                          // (the whole wavefront; there is no workgroup barrier below)
    InnovWork& ws = s_ws[wave];
    const InnovWave w = {lane};
    const EkfStepParams& s = p.s;
    const StepNoise sn = step_noise(s, b);
    const InnovNoise nz = {sn.v_d, sn.v_th, sn.w_r, sn.w_b, sn.V00, sn.V11, sn.W00, sn.W11};
    const int32_t status = s.flags[b];
    const float* const cp = s.cmd_each ? s.cmd_each + 2 * (size_t)b : nullptr;
    const float fwd = cp ? cp[0] : s.fwd, ang = cp ? cp[1] : s.ang;
    int k = 0;
    if (!(status & kInnovStatusFrozen)) {
        if (s.sim) {
            double tx = s.truth[3 * (size_t)b], ty = s.truth[3 * (size_t)b + 1], tth = s.truth[3 * (size_t)b + 2];
            const int Lm = sim_map_size(s, b);
            const double* const map = sim_map(s, b);
            const double lmx0 = lane < Lm ? map[2 * lane] : 0.0, lmy0 = lane < Lm ? map[2 * lane + 1] : 0.0;
            k = sim_wave<kInnovMaxDet, false>(s, b, lane, fwd, ang, s.step, map, Lm, tx, ty, tth, lmx0, lmy0, ws.meas, sn.sim);
        } else {
            k = s.meas_count_in[b];
            k = k < s.k_stride_in ? k : s.k_stride_in;
            k = k < 0 ? 0 : k;
            if (k <= kInnovMaxDet) {
                const float* const src = s.meas_in + (size_t)b * s.k_stride_in * 3;
                for (int i = lane; i < 3 * k; i += 64) ws.meas[i] = src[i];
            }
        }
        w.sync();
    }
    int M = s.M[b];
    M = M < 0 ? 0 : (M > s.L_max ? s.L_max : M);
    const int ld = ekf_ld(3 + 2 * M, (int)sizeof(ST));
    const ST* __restrict__ const xb = static_cast<const ST*>(s.x) + (size_t)b * s.xstride;
    const ST* __restrict__ const Pb = static_cast<const ST*>(s.P) + (size_t)b * s.pstride;
    double* const det = p.det ? p.det + (size_t)b * kInnovMaxDet * kInnovDetLen : nullptr;
    // (every index the loaders see is below 3 + 2 M: the block's landmarks come from ids[0 .. M))
    const InnovResult v = innovation_instance(
        w, ws, [&](int i) { return (double)xb[i]; }, [&](int r, int c) { return (double)Pb[(size_t)r * ld + c]; },
        s.ids + (size_t)b * s.L_max, M, s.L_max, status, fwd, ang, k, nz, s.lm_from_pred != 0, p.nis_lo, p.nis_hi, det);
    if (lane == 0) {
        if (p.post)
#pragma unroll
            for (int i = 0; i < 12; ++i) p.post[(size_t)b * 12 + i] = v.post[i];
        if (p.nis_sum) p.nis_sum[b] = v.nis_sum;
        if (p.n_upd) p.n_upd[b] = v.n_upd;
        if (p.n_new) p.n_new[b] = v.n_new;
        if (p.flags) p.flags[b] = v.flags;
        double r[kInnovRecLen];
        innovation_record(v, r);
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) p.inst_rec[(size_t)b * kInnovRecLen + i] = r[i];
    }
}

__device__ __forceinline__ double rec_join(int i, double a, double b) { return i == kInnMaxNis ? (b > a ? b : a) : a + b; }

// one lane per instance: the contributions of 256 consecutive instances by a fixed tree into one partial record
__global__ __launch_bounds__(kInnovBlock) void innovation_reduce_kernel(const double* __restrict__ inst_rec, int B, double* __restrict__ partials) {
    __shared__ double s_part[kRedWaves][kInnovRecLen];
    const int b = blockIdx.x * kInnovBlock + threadIdx.x;
    double r[kInnovRecLen];
#pragma unroll
    for (int i = 0; i < kInnovRecLen; ++i) r[i] = b < B ? inst_rec[(size_t)b * kInnovRecLen + i] : 0.0;
    // (a lane past the batch contributes zeros, which change no maximum of non-negative values and add exactly)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) r[i] = rec_join(i, r[i], __shfl_down(r[i], off, 64));
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) s_part[wave][i] = r[i];
    __syncthreads();
    if (threadIdx.x < kInnovRecLen) {
        const int i = threadIdx.x;
        double a = s_part[0][i];
        for (int wv = 1; wv < kRedWaves; ++wv) a = rec_join(i, a, s_part[wv][i]);
        partials[(size_t)blockIdx.x * kInnovRecLen + i] = a;
    }
}

// the partial records in ascending order of their workgroups: one lane per entry
__global__ __launch_bounds__(64) void innovation_sum_kernel(const double* __restrict__ partials, int blocks, double* __restrict__ rec) {
    const int i = threadIdx.x;
    if (i >= kInnovRecLen) return;
    double a = partials[i];
    for (int k = 1; k < blocks; ++k) a = rec_join(i, a, partials[(size_t)k * kInnovRecLen + i]);
    rec[i] = a;
}

}  // namespace

hipError_t launch_innovation(const InnovParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    const int n_max = 3 + 2 * s.L_max;
    if (s.B <= 0 || s.L_max < 0 || !p.inst_rec || !p.partials || !p.rec || s.xstride < n_max ||
        (long long)s.pstride < (long long)n_max * ekf_ld(n_max, f32_storage ? 4 : 8))
        return hipErrorInvalidValue;
    if (s.sim ? (!s.truth || (!s.map && !s.map_each)) : (!s.meas_in || !s.meas_count_in || s.k_stride_in <= 0)) return hipErrorInvalidValue;
    const int groups = (s.B + kInnovWaves - 1) / kInnovWaves;
    (void)hipGetLastError();   // sticky and per thread: only these launches' errors are reported (capi_internal.h)
    if (f32_storage) hipLaunchKernelGGL(innovation_instance_kernel<float>, dim3(groups), dim3(64 * kInnovWaves), 0, stream, p);
    else hipLaunchKernelGGL(innovation_instance_kernel<double>, dim3(groups), dim3(64 * kInnovWaves), 0, stream, p);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_innovation_reduce(p.inst_rec, s.B, p.partials, p.rec, stream);
}

hipError_t launch_innovation_reduce(const double* inst_rec, int B, double* partials, double* rec, hipStream_t stream) {
    const int blocks = innovation_blocks(B);
    hipLaunchKernelGGL(innovation_reduce_kernel, dim3(blocks), dim3(kInnovBlock), 0, stream, inst_rec, B, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(innovation_sum_kernel, dim3(1), dim3(64), 0, stream, partials, blocks, rec);
    return hipGetLastError();
}

}  // namespace slam
