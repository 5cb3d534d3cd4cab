// fix_kernel.hip — absolute position and heading fixes of the EKF batch on the device (slam_fix, slam_fix_sense, slam_fix_run): the
// per-instance functions of fix_kernel.h mapped to gfx950.
//
// fix_instance_kernel: ONE WORKGROUP PER INSTANCE, as merge_fuse_kernel, fix_instance<true> over the 256 lanes: whatever parts a fix
//   carries, P and x are read and written ONCE, in place in the canonical buffer.  The workspace (rows and columns 0, 1, 2 of P, six
//   values per state index, and x[0 .. 2]: 6 n + 3 doubles, 4968 bytes at L_max = 50, 96 KB at L_max = 1000) is dynamic LDS.  The gather of the
//   columns is a column read (one line per row, n rows) beside the n * ld elements the update streams through along rows, 16 bytes
//   per lane and access (two doubles or four floats: fp32 storage needs them to keep as many bytes in flight as fp64).  One barrier,
//   between the gather and the first store; both verdicts, Si, si and K_2 are recomputed by every lane from the workspace (no broadcast).
//   An instance without an applied part leaves after the barrier without a store; one whose parts are absent or invalid by the fix row
//   alone, or whose status skips it, never reads P.  Index arithmetic inside an instance is int; b * pstride is formed in size_t.
// fix_sense_kernel: one lane per instance, fix_sense_instance.
// FixWorkTerms: the traffic model, summed in integers by launch_work_sum outside any timed part.
// Record: launch_record_reduce (record_kernel.h) with the join mask kFixRecMax, every entry a sum.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "fix_kernel.h"
#include "lds_attr.h"

namespace slam {
namespace {

static_assert(kFixRecLen == kRecLen, "the record launch_record_reduce takes");
static_assert((int)kFixApplied == (int)SLAM_FIX_APPLIED && (int)kFixRejected == (int)SLAM_FIX_REJECTED &&
              (int)kFixSingular == (int)SLAM_FIX_SINGULAR && (int)kFixInvalid == (int)SLAM_FIX_INVALID, "the verdicts are slam_fix_verdict");
static_assert(sizeof(slam_fix_sensor) == 80, "nine doubles, one int32 and its padding");

constexpr int kFixThreads = 256;                    // one instance's workgroup

struct FixGroup {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return kFixThreads; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

template <class ST>
__global__ __launch_bounds__(kFixThreads) void fix_instance_kernel(const FixParams p) {
    extern __shared__ double s_ws[];                 // fix_ws_len(3 + 2 L_max) doubles
    const int b = blockIdx.x;                        // (the grid is exactly B workgroups)
    const int tid = threadIdx.x;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    const bool skip = (p.status[b] & kMapStatusSkip) != 0;   // (the whole workgroup: no barrier is passed by a part of it)
    const double gates[2] = {p.gate_pos, p.gate_yaw};
    FixResult o = {0, {__builtin_nan(""), __builtin_nan("")}, 0};
    if (!skip) {
        o = fix_instance<true>(FixGroup(), aux_row<ST>(p.P, b, p.pstride), aux_row<ST>(p.x, b, p.xstride), M, p.fix + (size_t)b * kFixRowLen, p.kinds[b], gates, s_ws);
    }
    if (tid == 0) {
        p.verdict[b] = o.verdict;
        p.nis[2 * (size_t)b] = o.nis[0]; p.nis[2 * (size_t)b + 1] = o.nis[1];
        if (p.rec) {
            double r[kFixRecLen];
            fix_record(o, skip, r);
#pragma unroll
            for (int i = 0; i < kFixRecLen; ++i) p.inst_rec[(size_t)b * kFixRecLen + i] = r[i];
        }
    }
}

__global__ __launch_bounds__(256) void fix_sense_kernel(const FixSenseParams p) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const slam_fix_sensor row = p.rows ? p.rows[b] : fix_sensor_default_row();
    const FixSensed o = fix_sense_instance(row, p.seed, (uint64_t)(p.inst0 + b), p.step, p.truth[3 * (size_t)b], p.truth[3 * (size_t)b + 1],
                                           p.truth[3 * (size_t)b + 2]);
#pragma unroll
    for (int i = 0; i < kFixRowLen; ++i) p.fix[(size_t)b * kFixRowLen + i] = o.row[i];
    p.kinds[b] = o.kinds;
    if (p.jumped) p.jumped[b] = o.jumped;
}

// element i of the traffic model's sum: one instance of one call
struct FixWorkTerms {
    const int32_t *M, *verdict;
    int L_max;
    __device__ void operator()(size_t i, unsigned long long (&t)[2]) const {
        const FixTraffic w = fix_traffic(aux_clamp_m(M[i], L_max), verdict[i]);
        t[0] = w.elems; t[1] = w.other_bytes;
    }
};

}  // namespace

hipError_t launch_fix(const FixParams& p, int f32_storage, hipStream_t stream) {
    const int n_max = 3 + 2 * p.L_max;
    if (!aux_shape_ok(p.B, p.L_max, p.xstride, p.pstride, f32_storage) || p.L_max <= 0 || p.L_max > kMapMaxLandmarks || !p.P || !p.x || !p.M || !p.status || !p.fix || !p.kinds ||
        !p.verdict || !p.nis || (p.rec && (!p.inst_rec || !p.partials)) ||
        reinterpret_cast<uintptr_t>(p.P) % 16 != 0 || ((size_t)p.pstride * (f32_storage ? 4 : 8)) % 16 != 0)   // (the 16-byte accesses of a row)
        return hipErrorInvalidValue;
    const size_t lds = sizeof(double) * (size_t)fix_ws_len(n_max);
    const void* fn = f32_storage ? reinterpret_cast<const void*>(&fix_instance_kernel<float>) : reinterpret_cast<const void*>(&fix_instance_kernel<double>);
    if (lds + 4096 > 64 * 1024) {   // once per device, to the kernel's maximum (lds_attr.h)
        const hipError_t e = slam_allow_full_lds(fn);
        if (e != hipSuccess) return e;
    }
    const hipError_t e = aux_launch(f32_storage, fix_instance_kernel<float>, fix_instance_kernel<double>, dim3(p.B), dim3(kFixThreads), lds, stream, p);
    if (e != hipSuccess || !p.rec) return e;
    return launch_record_reduce<kFixRecMax>(p.inst_rec, p.B, p.partials, p.rec, stream);
}

hipError_t launch_fix_sense(const FixSenseParams& p, hipStream_t stream) {
    if (p.B <= 0 || !p.truth || !p.fix || !p.kinds) return hipErrorInvalidValue;
    (void)hipGetLastError();
    hipLaunchKernelGGL(fix_sense_kernel, dim3((p.B + 255) / 256), dim3(256), 0, stream, p);
    return hipGetLastError();
}

hipError_t launch_fix_work(const int32_t* M, const int32_t* verdict, size_t n, int L_max, unsigned long long* work, hipStream_t stream) {
    if (!M || !verdict) return hipErrorInvalidValue;
    return launch_work_sum<2>(FixWorkTerms{M, verdict, L_max}, n, work, stream);
}

}  // namespace slam
