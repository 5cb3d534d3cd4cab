// ukf_kernel.h — parameter block and launchers of the UKF-SLAM step kernels (gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "noise_row.h"
#include "slam_math.h"

namespace slam {

// One timestep of UKF::update (ukf.cpp:161-372) for every instance = two launches:
//   ukf_sqrt_kernel : nearestSPD + matrix square root of P_t (ukf.cpp:106-123,208)      -> sqtP
//   ukf_step_kernel : sigma points, motion model, weighted mean / covariance, landmark updates and insertions
//                     (ukf.cpp:214-372), optionally preceded by the measurement generator (sim_node.py:209-250)
struct UkfStepParams {
    // ---- filter state in HBM ----
    const double* P;    // [B][pstride]  P_t packed row-major n x n, n = 4+2*M[b]
    double* P_out;      // [B][pstride]  next P_t (ping-pong with P)
    double* x;          // [B][xstride]  x_t = [x, y, cos, sin, landmarks...]
    double* sqtP;       // [B][pstride]  scratch: matrix square root, n x n row-major (symmetric)
    int32_t* n_sq;      // [B]           dimension of the matrix currently held in sqtP
    double* Vt_store;   // [B][pstride]  V^T of the last eigen-decomposition (n_sq x n_sq, row p = eigenvector p): warm start
    int32_t* v_age;     // [B]           consecutive warm starts so far, -1 = no usable V
    double* x_prev;     // [B][xstride]  x_t the sigma points were drawn around (UKFState.X = [x, x + sqtP cols, x - sqtP cols])
    int32_t* M;         // [B]
    int32_t* ids;       // [B][L_max]
    int32_t* flags;     // [B]
    int32_t* timestep;  // [B]
    // ---- simulator state ----
    double* truth;      // [B][3]
    double* err_sum;    // [B]
    const double* map;  // [L][2]
    int32_t L;          // landmarks of the map; with map_each: the largest L_each[b] (what the LDS sizing of a launch uses)
    const double* map_each; const int32_t* L_each; int32_t map_stride;   // per-instance maps (slam_set_maps) as in EkfStepParams, NULL = `map`
    // ---- measurements ----
    const float* meas_in; const int32_t* meas_count_in; int32_t k_stride_in;
    float* meas_out; int32_t* meas_count_out; int32_t k_stride_out;
    float fwd, ang;
    const float* cmd_each;   // [B][2] per-instance commands of this timestep, indexed by the GLOBAL instance b; NULL = (fwd, ang)
    // ---- filter config (filter.h:105-121) ----
    float v_d, v_th, w_r, w_b;
    double V00, V11, W00, W11;
    const NoiseRow* noise_each;   // [B] per-instance noise rows (slam_set_noise_each), indexed by the GLOBAL instance b; NULL = the scalars here and below
    int32_t float_trig;  // unqualified cos/sin(float): float overload (1) or double function (0)
    int32_t acc_zest1, yaw_sigma;   // quirk switches ukf_accumulate_zest1 / ukf_sensing_yaw_from_sigma (include/slam_batch.h), 0 = reference
    // ---- simulator config ----
    double sV00, sV11, sW00, sW11, d_max, th_max, range_max, fov_min, fov_max;
    uint64_t seed;
    int64_t inst0;
    uint32_t step;
    int32_t B, L_max, pstride, xstride;
    int32_t b_off, b_cnt;  // the launch covers instances [b_off, b_off + b_cnt) (the batch is split over two streams)
    int32_t sim;
    int32_t loc;          // 1 = FilterChoice::UKF_LOC: every detection updates against the known map (ukf.cpp:146-154)
    unsigned long long* prof;   // optional [B][16] phase timers of the step kernel (debug), NULL otherwise
    const float* mapf;    // [L][3] float32 {id, x, y}: `filter->map` as it arrives on /truth/landmarks
    // Pass table of the fast sqrt kernel (<44, 256>): [nj / 4][pass < 21][thread 256] x 32 bytes, the LDS byte offsets of every operand a thread
    // touches in a pass of two Jacobi rounds at the padded state size nj = 4, 8, .., 44 (built once by launch_ukf_quad_table); the other
    // variants derive them from the schedule themselves
    const uint4* quad_tab;
    // workload statistics (optional): [0..7] instance-steps by detections in the message (7 = seven or more), [8] Jacobi sweeps
    // that rotated something, [9] eigen-decompositions (slam_k_histogram / slam_ukf_sweep_stats)
    unsigned long long* khist;
    // the size class beyond LDS (ukf_big_kernel.hip, n = 4 + 2 L_max > 104): [B][2 * pstride] doubles of scratch per instance (the scaled
    // symmetrised matrix and the warm-start product of the sqrt kernel, then P_pred of the step kernel); NULL for the LDS classes
    double* big_ws;
    // Messages longer than the size class holds (ukf_class_message_capacity).  0: none can occur.  1 (set by the host when one can, with
    // long_cap = that capacity and big_ws allocated): launch_ukf_step pairs the LDS step kernel, which then leaves every instance whose
    // message exceeds long_cap untouched, with ukf_big_step_kernel for exactly those (long_mode = 2 inside that launch); in SIM mode, where the
    // count is not known before the generator has run, the streamed kernel takes the whole launch.  The sqrt kernel is the class's own either way.
    int32_t long_mode, long_cap;
    // SLAM_UKF_SQRT_CHOLESKY (slam_ukf_set_sqrt_mode): [B] per-instance byte, 1 = ukf_chol_kernel factored Y = L L^T this step and
    // wrote sqtP = L^T, 0 = a pivot <= 1e-8 or non-finite, the eigen kernel that follows computes sqtP cold.  NULL = the eigen path
    // (the default, reference-exact): launch_ukf_sqrt then launches exactly what it launched before the mode existed.
    uint8_t* chol_ok;
};
// detections ONE message may hold in the LDS size class of the step kernel (launch_ukf_step picks the class the same way)
inline int ukf_class_message_capacity(int L_max, bool loc, int L_map) { return ((loc && L_map > 20) ? 104 : 4 + 2 * L_max) <= 44 ? 20 : 50; }

static constexpr int kUkfRotThreads = 256;   // threads of the variant with the pass table
// Pass table for ukf_sqrt_kernel<44, 256> at the padded sizes nj = 4, 8, ..., 44: kUkfQuadTabEntries uint4 entries (2 MB), built on the host
static constexpr int kUkfQuadPasses = 21, kUkfQuadSizes = 12;   // block rounds T = 0 .. n / 2 - 2; n / 4 = 0 .. 11
static constexpr size_t kUkfQuadTabEntries = (size_t)kUkfQuadSizes * kUkfQuadPasses * kUkfRotThreads * 2;
hipError_t launch_ukf_quad_table(uint4* tab, hipStream_t stream);

static constexpr int kUkfLdsMaxLandmarks = 50;   // n = 4 + 2L <= 104: the fast kernels keep A, V^T and sqtP of an instance in LDS
static constexpr int kUkfMaxLandmarks = 200;     // beyond: ukf_big_kernel.hip, every n x n object in HBM / L2 (slow, bit-identical)
hipError_t launch_ukf_big_sqrt(const UkfStepParams& p, hipStream_t stream);
hipError_t launch_ukf_big_step(const UkfStepParams& p, hipStream_t stream);

static constexpr float kUkfW0 = 0.2f;        // weight of the central sigma point (filter.h:207)
static constexpr int kUkfWarmMaxAge = 100;   // consecutive warm starts of the eigen-decomposition before one starts cold again

// unqualified cos / sin on a float argument (ukf.cpp:39-42,129-133,183-186,358-359)
__device__ __forceinline__ void tsincos(float a, int float_trig, double* s, double* c) {
    double ss, cc;
    det_sincos((double)a, &ss, &cc);
    *s = float_trig ? (double)(float)ss : ss;
    *c = float_trig ? (double)(float)cc : cc;
}

__device__ __forceinline__ float yaw_of(double c, double s) {  // (float) remainder(atan2(x3, x2), 2 pi)
    return (float)remainder(det_atan2(s, c), kTwoPi);
}

// SLAM_UKF_SQRT_CHOLESKY: khist[kUkfCholSlot] = Cholesky factors that succeeded, khist[kUkfCholSlot + 1] = eigen fallbacks
static constexpr int kUkfCholSlot = 14;
// Eigen mode: ukf_sqrt_kernel.  Cholesky mode (p.chol_ok != NULL, LDS classes only): ukf_chol_kernel, then ukf_sqrt_kernel for the
// instances whose factorisation failed (the others leave at once), in stream order without a host synchronisation.
hipError_t launch_ukf_sqrt(const UkfStepParams& p, hipStream_t stream);
hipError_t launch_ukf_step(const UkfStepParams& p, hipStream_t stream);

struct UkfInitParams {
    double* P; double* x; int32_t* n_sq; int32_t* v_age; int32_t* M; int32_t* flags; int32_t* timestep; double* truth; double* err_sum;
    int32_t B, pstride, xstride;
    double x0, y0, c0, s0;   // x_t = (x_0, y_0, cos(yaw_0), sin(yaw_0)) as the reference stores them (ukf.cpp:33)
    double tx, ty, tyaw;
    const double* x_each;       // [B][4] (x_0, y_0, cos, sin) per instance (slam_init_each; the host applies ukf_float_trig), NULL = the above
    const double* truth_each;   // [B][3] the simulator's true start pose per instance, NULL = (tx, ty, tyaw) for all
};
hipError_t launch_ukf_init(const UkfInitParams& p, hipStream_t stream);

// slam_math_probe2 (include/slam_batch.h): one shared function per launch, selected by `op`, on device arrays a..d[n] -> out[n][out_per_item].
// The kernel lives in ukf_kernel.hip so that a second translation unit (other code generation options than ekf_kernel.hip, which holds
// slam_math_probe's kernel) compiles slam_math.h / slam_rng.h for a probe, and so that tsincos / yaw_of above are within its reach.
enum MathProbeOp {
    kProbeSincos = 0,     // a                  -> det_sincos: sin, cos
    kProbeAtan2 = 1,      // a = y, b = x       -> det_atan2
    kProbeRem2pi = 2,     // a                  -> rem2pi, wrap2pi (the library remainder)
    kProbeArith = 3,      // a, b               -> sqrt(a), a / b, (double)(float)a
    kProbeInv2x2 = 4,     // a..d = S[0..3]     -> Si[0..3], ok
    kProbeAssocAbs = 5,   // a, b = as_int      -> assoc_abs
    kProbeTsincos = 6,    // (float)a, b = float_trig -> tsincos: sin, cos
    kProbeYawOf = 7,      // a = c, b = s       -> yaw_of
    kProbeNoisePair = 8,  // a..d = packed (seed, inst, t, p), see slam_batch.h -> u0, u1
    kProbeOps = 9
};
// inputs read / outputs written per item by each op (the host allocates and checks by these)
static constexpr int kProbeIn[kProbeOps] = {1, 2, 1, 2, 4, 2, 2, 2, 4};
static constexpr int kProbeOut[kProbeOps] = {2, 1, 2, 3, 5, 1, 2, 1, 2};
hipError_t launch_math_probe2(int op, const double* a, const double* b, const double* c, const double* d, double* out, int out_per_item, int n,
                              hipStream_t stream);

}  // namespace slam
