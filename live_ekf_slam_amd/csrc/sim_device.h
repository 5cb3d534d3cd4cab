// sim_device.h — device-side range-bearing measurement generator, a port of get_cmd
// (reference ekf_ws/src/base_pkg/src/sim_node.py:209-250), shared by the EKF and UKF step kernels.
#pragma once
#include <type_traits>
#include <utility>

#include "noise_row.h"
#include "slam_math.h"
#include "slam_rng.h"

namespace slam {

// The noise values of ONE instance as a kernel holds them: the scalars of the parameter block, or the instance's row of
// P::noise_each (slam_set_noise_each).  The instance index is uniform over a wavefront in every step kernel, so the values are
// wave-uniform: the compiler reads the row with scalar loads into scalar registers, where the kernel arguments they stand in for live.
struct SimNoise { double sV00, sV11, sW00, sW11; };                  // simulator: half-widths of get_cmd's uniform draws
struct StepNoise { float v_d, v_th, w_r, w_b; double V00, V11, W00, W11; SimNoise sim; };   // filter (effective V / W) and simulator

template <class P, class = void> struct has_noise_each : std::false_type {};
template <class P> struct has_noise_each<P, std::void_t<decltype(std::declval<const P&>().noise_each)>> : std::true_type {};

// The simulator's half-widths of instance b (a GLOBAL index of the batch, as for cmd_each): its row, or the block's scalars where the
// block has no noise_each (the pose graph's) or the pointer is NULL.  The branch is on a pointer of the parameter block, uniform over
// the launch.  Ordinary loads, read ONCE per instance at kernel entry - not per timestep or detection.
template <class P>
__device__ __forceinline__ SimNoise sim_noise(const P& p, int b) {
    SimNoise s = {p.sV00, p.sV11, p.sW00, p.sW11};
    if constexpr (has_noise_each<P>::value) {
        if (p.noise_each && p.sim) {   // (EXT mode reads only the filter fields)
            const NoiseRow* const r = p.noise_each + (size_t)b;
            s.sV00 = r->sV00; s.sV11 = r->sV11; s.sW00 = r->sW00; s.sW11 = r->sW11;
        }
    }
    return s;
}
// ... and all of the instance's values, for the step kernels (EkfStepParams / UkfStepParams)
template <class P>
__device__ __forceinline__ StepNoise step_noise(const P& p, int b) {
    StepNoise s = {p.v_d, p.v_th, p.w_r, p.w_b, p.V00, p.V11, p.W00, p.W11, {p.sV00, p.sV11, p.sW00, p.sW11}};
    if (p.noise_each) {
        const NoiseRow* const r = p.noise_each + (size_t)b;
        s.v_d = r->v_d; s.v_th = r->v_th; s.w_r = r->w_r; s.w_b = r->w_b;
        s.V00 = r->V00; s.V11 = r->V11; s.W00 = r->W00; s.W11 = r->W11;
        if (p.sim) {   // (EXT mode reads only the filter fields)
            s.sim.sV00 = r->sV00; s.sim.sV11 = r->sV11; s.sim.sW00 = r->sW00; s.sim.sW11 = r->sW11;
        }
    }
    return s;
}

// Executed by ONE wavefront (lane = 0..63).  `P` is a step-parameter struct with the simulator fields
// (seed, inst0, d_max, th_max, range_max, fov_min, fov_max, truth); sn: the instance's half-widths (sim_noise, read by the caller once).
// fwd, ang: the commanded motion; step: RNG step index.  map, L: the instance's true map [L][2] (the shared map or its own,
// slam_set_maps).  tx, ty, tth: the instance's true pose (prefetched), advanced in place; lmx, lmy: prefetched map entry of id = lane.
// Writes the [id, range, bearing] float32 triplets of the visible landmarks (ascending id) to s_meas and returns
// their count (wave-uniform; triplets beyond KCAP are not stored, the caller caps and flags); lane 0 stores the new
// truth pose unless STORE_TRUTH is false (the EKF kernel writes it when it knows whether the instance froze).
template <int KCAP, bool STORE_TRUTH = true, class P>
__device__ __forceinline__ int sim_wave(const P& p, int b, int lane, float fwd, float ang, uint32_t step, const double* map, int L,
                                        double& tx, double& ty, double& tth, double lmx, double lmy, float* s_meas, const SimNoise& sn) {
    const uint64_t inst = (uint64_t)(p.inst0 + b);
    double u0, u1;
    noise_pair(p.seed, inst, step, 0u, &u0, &u1);
    double d = ((double)fwd + (2 * sn.sV00) * u0) - sn.sV00;          // sim_node.py:216
    double hdg = ((double)ang + (2 * sn.sV11) * u1) - sn.sV11;        // :217
    d = (p.d_max < d) ? p.d_max : d;                                 // min(d, d_max)        :219
    d = (0.0 < d) ? d : 0.0;                                         // max(0, .)
    hdg = (p.th_max < hdg) ? p.th_max : hdg;                         // :220
    hdg = (-p.th_max < hdg) ? hdg : -p.th_max;
    double s, c;
    det_sincos(tth, &s, &c);
    tx = tx + d * c;                                                 // :222 (yaw not wrapped)
    ty = ty + d * s;
    tth = tth + hdg;
    int count = 0;
#pragma unroll 1
    for (int base = 0; base < L; base += 64) {
        const int id = base + lane;
        bool vis = false;
        double r = 0.0, beta = 0.0;
        if (id < L) {
            if (base > 0) { lmx = map[2 * id]; lmy = map[2 * id + 1]; }   // ids 0..63 were prefetched
            const double dx = lmx - tx, dy = lmy - ty;
            r = sqrt(dx * dx + dy * dy);
            const double gb = det_atan2(dy, dx);
            beta = rem2pi(gb - tth);
            vis = !(r > p.range_max) && (beta > p.fov_min && beta < p.fov_max);
        }
        const unsigned long long mask = __ballot(vis);
        const int pos = count + __popcll(mask & ((1ull << lane) - 1ull));
        if (vis && pos < KCAP) {  // noise in visible-id order (sim_node.py:245-249), float32 wire format
            double v0, v1;
            noise_pair(p.seed, inst, step, (uint32_t)(1 + pos), &v0, &v1);
            const double rn = (r + (2 * sn.sW00) * v0) - sn.sW00;
            const double bn = (beta + (2 * sn.sW11) * v1) - sn.sW11;
            s_meas[3 * pos] = (float)id;
            s_meas[3 * pos + 1] = (float)rn;
            s_meas[3 * pos + 2] = (float)bn;
        }
        count += __popcll(mask);
    }
    if constexpr (STORE_TRUTH) {   // (a block without `truth` may call the other form)
        if (lane == 0) {
            p.truth[3 * (size_t)b] = tx;
            p.truth[3 * (size_t)b + 1] = ty;
            p.truth[3 * (size_t)b + 2] = tth;
        }
    }
    return count;   // the caller caps at KCAP and flags the overflow
}

// the same with the half-widths the parameter block says (a block without per-instance rows: the pose graph's)
template <int KCAP, bool STORE_TRUTH = true, class P>
__device__ __forceinline__ int sim_wave(const P& p, int b, int lane, float fwd, float ang, uint32_t step, const double* map, int L,
                                        double& tx, double& ty, double& tth, double lmx, double lmy, float* s_meas) {
    return sim_wave<KCAP, STORE_TRUTH>(p, b, lane, fwd, ang, step, map, L, tx, ty, tth, lmx, lmy, s_meas, sim_noise(p, b));
}

// ... and the filter's values alone, for a kernel whose generator reads the simulator's half-widths itself when it runs (the EKF step
// kernel: sim_noise on its cold fields).  Same places and the same branch as the filter part of step_noise.
struct FilterNoise { float v_d, v_th, w_r, w_b; double V00, V11, W00, W11; };
template <class P>
__device__ __forceinline__ FilterNoise filter_noise(const P& p, int b) {
    FilterNoise s = {p.v_d, p.v_th, p.w_r, p.w_b, p.V00, p.V11, p.W00, p.W11};
    if (p.noise_each) {
        const NoiseRow* const r = p.noise_each + (size_t)b;
        s.v_d = r->v_d; s.v_th = r->v_th; s.w_r = r->w_r; s.w_b = r->w_b;
        s.V00 = r->V00; s.V11 = r->V11; s.W00 = r->W00; s.W11 = r->W11;
    }
    return s;
}

// The true map of instance b and its landmark count: its own (slam_set_maps) or the shared one.  The branch is on a pointer of the
// parameter block, uniform over the launch.
template <class P>
__device__ __forceinline__ const double* sim_map(const P& p, int b) { return p.map_each ? p.map_each + (size_t)b * p.map_stride * 2 : p.map; }
template <class P>
__device__ __forceinline__ int sim_map_size(const P& p, int b) { return p.map_each ? p.L_each[b] : p.L; }

}  // namespace slam
