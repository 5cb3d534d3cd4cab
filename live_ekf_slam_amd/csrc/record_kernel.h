// record_kernel.h — how the per-instance records of the auxiliary EKF batch features (16 doubles each) become one record, for all of them.
//
// The order is fixed and depends on the batch size alone, so a record has the same bits on every run: kRecBlock = 256 consecutive
// instances per workgroup, lane i joined with lane i + off for off = 32 .. 1 (a lane past the batch contributes 0.0, which changes no
// maximum of non-negative values and adds exactly), then the workgroup's four wavefronts in order, then the workgroups in ascending
// order.  No atomics on values.  An entry is joined by a sum, or by a maximum where its bit is set in the record's JOIN MASK, declared
// beside the record's enum (kInnovRecMax, kMonRecMax, ...): a property of the record, passed by its launcher as a template argument.  (As a
// kernel argument the mask cost the reduction kernel 129 registers against 68, three wavefronts per SIMD against seven, and put a
// select into every step of the final sum's dependent chain, also where every entry is a sum.)
#pragma once
#include <hip/hip_runtime.h>

namespace slam {

constexpr int kRecLen = 16;                          // doubles of one record, of every feature
constexpr int kRecBlock = 256;                       // instances one workgroup of the tree takes
static_assert(kRecBlock % 64 == 0 && kRecLen <= 64, "whole wavefronts; one lane per entry");

inline int record_blocks(int B) { return (B + kRecBlock - 1) / kRecBlock; }

// (a maximum is b > a ? b : a, not fmax: a NaN on the right is dropped, one on the left stays)
__device__ __forceinline__ double record_join(unsigned max_mask, int i, double a, double b) {
    return (max_mask >> i) & 1u ? (b > a ? b : a) : a + b;
}

// The tree of one workgroup of kRecBlock threads, called by all of them: r is the thread's record (zeros past the batch), s_part the
// workgroup's LDS; the joined record goes to partial [kRecLen].  The workgroup barrier inside is the only one.
__device__ __forceinline__ void record_block_tree(double (&r)[kRecLen], unsigned max_mask, double (&s_part)[kRecBlock / 64][kRecLen],
                                                  double* __restrict__ partial) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int i = 0; i < kRecLen; ++i) r[i] = record_join(max_mask, i, r[i], __shfl_down(r[i], off, 64));
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < kRecLen; ++i) s_part[wave][i] = r[i];
    __syncthreads();
    if (threadIdx.x < kRecLen) {
        const int i = threadIdx.x;
        double a = s_part[0][i];
        for (int w = 1; w < kRecBlock / 64; ++w) a = record_join(max_mask, i, a, s_part[w][i]);
        partial[i] = a;
    }
}

// inst_rec [B][kRecLen] -> partials [record_blocks(B)][kRecLen] -> rec [kRecLen]: two launches on `stream`.  Both are instantiated
// in record_kernel.hip for the masks in use.
template <unsigned MAX_MASK>
hipError_t launch_record_reduce(const double* inst_rec, int B, double* partials, double* rec, hipStream_t stream);
// the second of them alone, for a kernel that ends in record_block_tree itself: partials [blocks][kRecLen] -> rec [kRecLen]
template <unsigned MAX_MASK>
hipError_t launch_record_total(const double* partials, int blocks, double* rec, hipStream_t stream);

}  // namespace slam
