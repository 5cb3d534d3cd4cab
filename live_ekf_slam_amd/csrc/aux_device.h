// aux_device.h — what the .hip files of the auxiliary EKF batch features (innovation, gate, assoc, joint, sense, fix, monitor, map,
// merge) share: how a kernel reads instance b of a batch view, the launchers' shape check and launch, and the sum of the traffic model.
// DEVICE BUILD ONLY: the .hip files include it; the *_kernel.h headers, which the host hooks and the stand-alone host programs compile
// without HIP, must not.  The per-instance records are reduced by record_kernel.h.
#pragma once
#include <hip/hip_runtime.h>

#include "ekf_kernel.h"
#include "innovation_kernel.h"
#include "record_kernel.h"
#include "sim_device.h"

namespace slam {

// ---- instance b of a batch view ----

// M as every kernel uses it: clamped to the handle's capacity, so that no index derived from it leaves the instance's slab
__device__ __forceinline__ int aux_clamp_m(int M, int L_max) { return M < 0 ? 0 : (M > L_max ? L_max : M); }

// instance b's part of a buffer of `stride` elements of T per instance (b * stride is formed in size_t)
template <class T> __device__ __forceinline__ T* aux_row(void* base, int b, int stride) { return static_cast<T*>(base) + (size_t)b * stride; }
template <class T> __device__ __forceinline__ const T* aux_row(const void* base, int b, int stride) {
    return static_cast<const T*>(base) + (size_t)b * stride;
}

// the command actually applied to instance b: its own (cmd_each) or the shared one
struct AuxCommand { float fwd, ang; };
__device__ __forceinline__ AuxCommand aux_command(const EkfStepParams& s, int b) {
    const float* const cp = s.cmd_each ? s.cmd_each + 2 * (size_t)b : nullptr;
    return AuxCommand{cp ? cp[0] : s.fwd, cp ? cp[1] : s.ang};
}

// What a wave-per-instance kernel reads of instance b of an EkfStepParams view (ST: the storage type of x and P), alike in every lane.
// Every index the loaders see must be below 3 + 2 M (x) or address an element of the n x n matrix at ld (P): the callers say why.
template <class ST>
struct AuxInstance {
    int32_t status;                                  // slam_instance_flags
    float fwd, ang;                                  // aux_command
    InnovNoise nz;                                   // the filter noise: the instance's row or the shared scalars
    int M, ld;                                       // landmarks (clamped) and the leading dimension of P at n = 3 + 2 M
    const int32_t* ids;                              // [L_max]
    const ST* __restrict__ xb;
    const ST* __restrict__ Pb;

    __device__ __forceinline__ AuxInstance(const EkfStepParams& s, int b)
        : status(s.flags[b]), M(aux_clamp_m(s.M[b], s.L_max)), ld(ekf_ld(3 + 2 * M, (int)sizeof(ST))), ids(s.ids + (size_t)b * s.L_max),
          xb(aux_row<ST>(s.x, b, s.xstride)), Pb(aux_row<ST>(s.P, b, s.pstride)) {
        const FilterNoise f = filter_noise(s, b);
        nz = InnovNoise{f.v_d, f.v_th, f.w_r, f.w_b, f.V00, f.V11, f.W00, f.W11};
        const AuxCommand c = aux_command(s, b);
        fwd = c.fwd; ang = c.ang;
    }
    __device__ __forceinline__ auto load_x() const { return [x = xb](int i) { return (double)x[i]; }; }
    __device__ __forceinline__ auto load_P() const { return [P = Pb, l = ld](int r, int c) { return (double)P[(size_t)r * l + c]; }; }
};

// The host-fed message of instance b (meas_in / meas_count_in / k_stride_in): its count as given and clamped to the row, and the row.
// stage() copies the k triplets into the caller's LDS array of 3 kInnovMaxDet floats, lanes along the row; a longer message is not
// staged (its instance is TOO_LONG, nothing reads the array).  The caller's wavefront fence comes after it.
struct AuxMessage {
    int count, k;
    const float* src;                                // [k_stride_in][3]
    __device__ __forceinline__ AuxMessage(const EkfStepParams& s, int b) : count(s.meas_count_in[b]), src(s.meas_in + (size_t)b * s.k_stride_in * 3) {
        k = count < s.k_stride_in ? count : s.k_stride_in;
        k = k < 0 ? 0 : k;
    }
    __device__ __forceinline__ void stage(int lane, float* meas) const {
        if (k <= kInnovMaxDet)
            for (int i = lane; i < 3 * k; i += 64) meas[i] = src[i];
    }
};

// ---- launchers ----

// the slabs of a handle hold every state up to L_max landmarks: x [>= 3 + 2 L_max], P [>= n_max * ekf_ld(n_max)].  (L_max = 0 passes: the
// innovation family accepts a handle without landmarks; the map family adds its own 0 < L_max <= kMapMaxLandmarks.)
inline bool aux_shape_ok(int B, int L_max, int xstride, int pstride, int f32_storage) {
    const int n_max = 3 + 2 * L_max;
    return B > 0 && L_max >= 0 && xstride >= n_max && (long long)pstride >= (long long)n_max * ekf_ld(n_max, f32_storage ? 4 : 8);
}

// one launch of the kernel's instantiation for fp32 (k32) or fp64 (k64) storage; its error alone
template <class K, class... A>
hipError_t aux_launch(int f32_storage, K k32, K k64, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const A&... args) {
    (void)hipGetLastError();   // sticky and per thread: only this launch's error is reported (capi_internal.h)
    const K k = f32_storage ? k32 : k64;
    hipLaunchKernelGGL(k, grid, block, lds, stream, args...);
    return hipGetLastError();
}

// ---- the traffic model (slam_last_*_work) ----

// work [N] += the N terms f(i, t) of the elements i < n, in integers (the order of the additions does not matter): a grid-stride sum per
// lane, a shuffle tree per wavefront, one atomic add per wavefront and sum.  F: a small struct of pointers and sizes with
// __device__ void operator()(size_t i, unsigned long long (&t)[N]) const, beside the feature's launcher.
template <int N, class F>
__global__ __launch_bounds__(256) void work_sum_kernel(const F f, size_t n, unsigned long long* __restrict__ work) {
    unsigned long long a[N] = {};
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        unsigned long long t[N];
        f(i, t);
#pragma unroll
        for (int j = 0; j < N; ++j) a[j] += t[j];
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1)
#pragma unroll
        for (int j = 0; j < N; ++j) a[j] += __shfl_down(a[j], off, 64);
    if (threadIdx.x % 64 == 0)
#pragma unroll
        for (int j = 0; j < N; ++j) atomicAdd(work + j, a[j]);
}

// (outside any timed part; the caller has checked the functor's pointers)
template <int N, class F>
hipError_t launch_work_sum(const F& f, size_t n, unsigned long long* work, hipStream_t stream) {
    if (!work || n == 0) return hipErrorInvalidValue;
    const size_t want = (n + 255) / 256;
    (void)hipGetLastError();   // sticky and per thread: only this launch's error is reported
    hipLaunchKernelGGL((work_sum_kernel<N, F>), dim3((unsigned)(want < 256 ? want : 256)), dim3(256), 0, stream, f, n, work);
    return hipGetLastError();
}

}  // namespace slam
