// record_kernel.hip — the one kernel pair that reduces the per-instance records of every auxiliary EKF batch feature (innovation, gate,
// association, joint association, sense, fix, map, merge; the monitor's sum): record_kernel.h has the order and the join rule.
#include <hip/hip_runtime.h>

#include "record_kernel.h"

namespace slam {
namespace {

// one lane per instance: the records of kRecBlock consecutive instances into one partial record
template <unsigned MAX_MASK>
__global__ __launch_bounds__(kRecBlock) void record_reduce_kernel(const double* __restrict__ inst_rec, int B, double* __restrict__ partials) {
    __shared__ double s_part[kRecBlock / 64][kRecLen];
    const int b = blockIdx.x * kRecBlock + threadIdx.x;
    double r[kRecLen];
#pragma unroll
    for (int i = 0; i < kRecLen; ++i) r[i] = b < B ? inst_rec[(size_t)b * kRecLen + i] : 0.0;
    record_block_tree(r, MAX_MASK, s_part, partials + (size_t)blockIdx.x * kRecLen);
}

// the partial records in ascending order of their workgroups: one lane per entry
template <unsigned MAX_MASK>
__global__ __launch_bounds__(64) void record_sum_kernel(const double* __restrict__ partials, int blocks, double* __restrict__ rec) {
    const int i = threadIdx.x;
    if (i >= kRecLen) return;
    double a = partials[i];
    for (int k = 1; k < blocks; ++k) a = record_join(MAX_MASK, i, a, partials[(size_t)k * kRecLen + i]);
    rec[i] = a;
}

}  // namespace

// (neither clears the sticky error: both follow a launch of the caller's, whose error has been taken)
template <unsigned MAX_MASK>
hipError_t launch_record_reduce(const double* inst_rec, int B, double* partials, double* rec, hipStream_t stream) {
    if (B <= 0 || !inst_rec || !partials || !rec) return hipErrorInvalidValue;
    const int blocks = record_blocks(B);
    hipLaunchKernelGGL(record_reduce_kernel<MAX_MASK>, dim3(blocks), dim3(kRecBlock), 0, stream, inst_rec, B, partials);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return launch_record_total<MAX_MASK>(partials, blocks, rec, stream);
}

template <unsigned MAX_MASK>
hipError_t launch_record_total(const double* partials, int blocks, double* rec, hipStream_t stream) {
    hipLaunchKernelGGL(record_sum_kernel<MAX_MASK>, dim3(1), dim3(64), 0, stream, partials, blocks, rec);
    return hipGetLastError();
}

// the masks in use: entry 8 a maximum (innovation, gate, association, joint association, map, merge); every entry a sum (sense, fix);
// entry 7 a maximum (score); entries 6 and 8 maxima (the monitor, whose kernel runs the tree itself)
template hipError_t launch_record_reduce<1u << 8>(const double*, int, double*, double*, hipStream_t);
template hipError_t launch_record_reduce<0u>(const double*, int, double*, double*, hipStream_t);
template hipError_t launch_record_reduce<1u << 7>(const double*, int, double*, double*, hipStream_t);
template hipError_t launch_record_total<(1u << 6) | (1u << 8)>(const double*, int, double*, hipStream_t);

}  // namespace slam
