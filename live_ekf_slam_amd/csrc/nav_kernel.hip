// nav_kernel.hip — one tick of the pure-pursuit / direct controller for every instance of a batch (slam_nav_run).
//
// Mapping: ONE LANE PER INSTANCE.  The work of an instance is a short, data-dependent loop nest (at most P waypoints x the lookahead radii,
// usually one or two radii over the few segments left in the queue) around scalar fp64 arithmetic with a sqrt and two divisions per segment:
// there is nothing in it for the 64 lanes of a wavefront to share, and a wave per instance would leave 63 lanes idle in the common case of a
// queue of a handful of points while paying a cross-lane reduction for "the last segment with a valid root".  Divergence between the lanes of
// a wave is bounded by the longest queue among 64 neighbours.  The shared path is staged in LDS once per workgroup (16 bytes per waypoint, 16 KB at the cap of 1024
// waypoints), so every lane's walk over it is an LDS read; per-instance paths are read where they lie.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "nav_kernel.h"

namespace slam {
namespace {

constexpr int kNavTPB = 64;

struct LdsPath {
    const double* pts;
    __device__ __forceinline__ double x(int i) const { return pts[2 * i]; }
    __device__ __forceinline__ double y(int i) const { return pts[2 * i + 1]; }
};

template <class ST, bool SHARED>
__global__ __launch_bounds__(kNavTPB) void nav_tick_kernel(const NavParams p) {
    extern __shared__ double s_path[];   // SHARED: 2 * p.P doubles (launch_one sizes it), else none
    if constexpr (SHARED) {
        for (int i = threadIdx.x; i < 2 * p.P; i += kNavTPB) s_path[i] = p.path[i];   // p.P <= kNavMaxWaypoints (checked when the path is set)
        __syncthreads();
    }
    const int b = blockIdx.x * kNavTPB + threadIdx.x;
    if (b >= p.B) return;
    const ST* __restrict__ xb = static_cast<const ST*>(p.x) + (size_t)b * p.xstride;
    // the wire values of the state message: float32 x_v, y_v, yaw_v (EKFState.msg:5-7)
    const double ex = (double)(float)(double)xb[0], ey = (double)(float)(double)xb[1];
    double yaw = (double)xb[2];
    if (p.ukf) yaw = remainder(det_atan2((double)xb[3], (double)xb[2]), kTwoPi);       // ukf.cpp:71
    const double eyaw = (double)(float)yaw;
    const bool frozen = (p.flags[b] & SLAM_INST_INDEX_OOR) != 0;
    NavState s;
    s.head = p.head[b]; s.finish_tick = p.finish_tick[b]; s.integ = p.integ[b]; s.err_prev = p.err_prev[b];
    float cmd[2];
    if constexpr (SHARED) {
        nav_tick(p.c, LdsPath{s_path}, p.P, ex, ey, eyaw, frozen, p.tick, s, cmd);
    } else {
        const int Pb = p.P_each[b];                                                     // 1 <= Pb <= path_stride (checked when the paths are set)
        nav_tick(p.c, NavPathView{p.path + (size_t)b * p.path_stride * 2}, Pb, ex, ey, eyaw, frozen, p.tick, s, cmd);
    }
    p.head[b] = s.head; p.finish_tick[b] = s.finish_tick; p.integ[b] = s.integ; p.err_prev[b] = s.err_prev;
    *reinterpret_cast<float2*>(p.cmd_out + 2 * (size_t)b) = make_float2(cmd[0], cmd[1]);
    if (p.cmd_log) *reinterpret_cast<float2*>(p.cmd_log + 2 * (size_t)b) = make_float2(cmd[0], cmd[1]);
}

template <class ST, bool SHARED>
hipError_t launch_one(const NavParams& p, hipStream_t stream) {
    const int grid = (p.B + kNavTPB - 1) / kNavTPB;
    (void)hipGetLastError();   // sticky and per thread: only this launch's error is reported (capi_internal.h)
    const size_t lds = SHARED ? sizeof(double) * 2 * (size_t)p.P : 0;   // at most 16 KB: P <= kNavMaxWaypoints
    hipLaunchKernelGGL((nav_tick_kernel<ST, SHARED>), dim3(grid), dim3(kNavTPB), lds, stream, p);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_nav_tick(const NavParams& p, int f32_storage, hipStream_t stream) {
    if (p.B <= 0) return hipSuccess;
    const bool shared = p.P_each == nullptr;
    if (shared && (p.P < 1 || p.P > kNavMaxWaypoints)) return hipErrorInvalidValue;
    if (f32_storage) return shared ? launch_one<float, true>(p, stream) : launch_one<float, false>(p, stream);
    return shared ? launch_one<double, true>(p, stream) : launch_one<double, false>(p, stream);
}

}  // namespace slam
