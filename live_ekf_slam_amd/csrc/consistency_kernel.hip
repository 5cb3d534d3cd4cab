// consistency_kernel.hip — NEES = e^T S^-1 e of every EKF instance, S = (P_t + P_t^T) / 2, e = estimate - truth (slam_consistency).
//
// Per instance: the lower triangle of S is packed row by row (row i at i (i + 1) / 2) and e is appended as row n.  A right-looking
// Cholesky over the n + 1 rows then leaves y = L^-1 e in the appended row, one component per column step, so NEES is the running sum
// of y_k^2 and there is no separate solve; the sum after three columns is the NEES of the vehicle pose's marginal.  L itself is never
// stored: the scaled column k lives in a double-buffered LDS vector, and the thread that updates the element (i, k + 1) of the
// trailing triangle writes the scaled column k + 1 at once (every thread forms the next pivot itself from the same two operands), so
// a column step costs ONE barrier.
// Storage policy: the triangle is in LDS (L_max <= 50: 45 KB per instance at n = 103, three workgroups per CU; L_max <= 20: four
// instances of 8.6 KB per workgroup, one wavefront each) or in a device workspace (beyond: slow by design, like ekf_big_kernel.hip).
// All arithmetic is fp64, whatever the storage type of P and x; sums run in a fixed order (no atomics on values), so an instance's
// result does not depend on the batch, the chunk or the call.  Nothing the kernel indexes with is trusted: M is clamped to
// [0, L_max], an id is compared with the instance's map size before the map is read.
// The SEL variant (launch_consistency_selected, slam_map_score with full = 1) is the same factorisation on a principal submatrix: row i
// of S is row src(i) of P, src = (0, 1, 2, then 3 + 2 s, 4 + 2 s for the slots s of the instance's list sel [n_sel], ascending), and the
// landmark truth of list entry k is map[sel_row[k]]; score_kernel.hip wrote the list, decided INSTANCE_FAILED and summed map_rms.  It
// is a compile-time variant (if constexpr): the instantiations behind slam_consistency contain none of it.
#include "consistency_kernel.h"

#include "../../include/slam_batch.h"
#include "ekf_kernel.h"
#include "slam_math.h"

namespace slam {
namespace {

__device__ inline bool pivot_ok(double d) { return d > 0.0 && d < __builtin_inf(); }
__device__ inline bool finite_d(double v) { return fabs(v) < __builtin_inf(); }

// NMAX: largest n of the class; TPI threads per instance, IPW instances per workgroup; G lanes share one row of the trailing update
// (TPI / G rows in flight); WS: the triangle lives in the workspace, else in LDS; ST: storage type of P and x.
template <int NMAX, int TPI, int IPW, int G, bool WS, class ST, bool SEL = false>
__global__ __launch_bounds__(TPI * IPW) void consistency_kernel(const ConsistencyParams p) {
    constexpr int TRI = (NMAX + 1) * (NMAX + 2) / 2;
    constexpr int NG = TPI / G;
    __shared__ double s_tri[WS ? 1 : IPW * TRI];
    __shared__ double s_col[IPW][2][NMAX + 1];
    __shared__ int s_flag[IPW], s_rows[IPW];

    const int inst = threadIdx.x / TPI, t = threadIdx.x % TPI;
    const int g = t / G, l = t % G;
    const int slot = blockIdx.x * IPW + inst;
    const bool live = slot < p.count;
    const int b = p.b0 + (live ? slot : 0);
    double* A = WS ? p.ws + (size_t)slot * p.ws_stride : s_tri + inst * TRI;

    int m = live ? p.M[b] : 0;
    m = m < 0 ? 0 : (m > p.L_max ? p.L_max : m);
    int ld_n = 3 + 2 * m;                            // the n the instance's P is stored at
    if constexpr (SEL) {                             // the selected slots: n_sel of the m (never more: the list has m places)
        const int k = live ? p.n_sel[b] : 0;
        m = k < 0 ? 0 : (k > m ? m : k);
    }
    const int n = 3 + 2 * m;
    const bool failed = live && (SEL ? (p.flags[b] & SLAM_CONSISTENCY_INSTANCE_FAILED) != 0
                                     : (p.status[b] & (SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG)) != 0);
    const ST* x = static_cast<const ST*>(p.x) + (size_t)b * p.xstride;
    const ST* P = static_cast<const ST*>(p.P) + (size_t)b * p.pstride;
    const int ld = ekf_ld(SEL ? ld_n : n, (int)sizeof(ST));
    const int32_t* const sel = SEL ? p.sel + (size_t)b * p.L_max : nullptr;
    const int32_t* const sel_row = SEL ? p.sel_row + (size_t)b * p.L_max : nullptr;
    // row i of S in the stored state (SEL: through the list; every entry is clamped into the instance's slots before it indexes)
    auto src = [&](int i) -> int {
        if constexpr (SEL) {
            if (i < 3) return i;
            int s = sel[(i - 3) >> 1];
            s = s < 0 ? 0 : (s > (ld_n - 3) / 2 - 1 ? (ld_n - 3) / 2 - 1 : s);
            return 3 + 2 * s + ((i - 3) & 1);
        } else {
            return i;
        }
    };
    const double* map = p.map_each ? p.map_each + (size_t)b * p.map_stride * 2 : p.map;
    int Lb = p.map_each ? p.L_each[b] : p.L;
    if (p.map_each && Lb > p.map_stride) Lb = p.map_stride;
    const int32_t* ids = p.ids + (size_t)b * p.L_max;

    // ---- which landmarks have a truth ----
    if (t == 0) s_flag[inst] = (!SEL && !p.id_known && m > 0) ? SLAM_CONSISTENCY_NO_TRUTH : 0;
    __syncthreads();
    if (!SEL && live && !failed && p.id_known)
        for (int j = t; j < m; j += TPI)
            if (ids[j] < 0 || ids[j] >= Lb) atomicOr(&s_flag[inst], SLAM_CONSISTENCY_NO_TRUTH);
    __syncthreads();
    const bool no_truth = (s_flag[inst] & SLAM_CONSISTENCY_NO_TRUTH) != 0;
    // rows of S that are factored: all n, the vehicle's three without a landmark truth, none for a dead slot or a failed instance
    const int nf = (!live || failed) ? 0 : (no_truth ? 3 : n);
    if (t == 0) s_rows[inst] = nf;

    // ---- e into row nf, the lower triangle of P into rows 0 .. nf - 1 ----
    double* E = A + nf * (nf + 1) / 2;
    for (int i = t; i < nf; i += TPI) {
        double e;
        if (i < 3) {
            e = (double)x[i] - p.truth[(size_t)b * 3 + i];
            if (i == 2) e = wrap2pi(e);
        } else if constexpr (SEL) {                  // (a row outside the instance's map reads row 0: the list's writer never gives one)
            const int r = sel_row[(i - 3) >> 1];
            e = (double)x[src(i)] - map[2 * (r < 0 || r >= Lb ? 0 : r) + ((i - 3) & 1)];
        } else {
            e = (double)x[i] - map[2 * ids[(i - 3) >> 1] + ((i - 3) & 1)];
        }
        if (!finite_d(e)) atomicOr(&s_flag[inst], SLAM_CONSISTENCY_INSTANCE_FAILED);
        E[i] = e;
    }
    for (int i = g; i < nf; i += NG)
        for (int j = l; j <= i; j += G) A[i * (i + 1) / 2 + j] = (double)P[(size_t)src(i) * ld + src(j)];
    __syncthreads();
    // the upper triangle, read along its rows like the lower one: S_ji = (P_ji + P_ij) / 2, each element owned by one thread
    for (int i = g; i < nf; i += NG)
        for (int j = i + 1 + l; j < nf; j += G) {
            double* a = A + j * (j + 1) / 2 + i;
            *a = 0.5 * (*a + (double)P[(size_t)src(i) * ld + src(j)]);
        }
    __syncthreads();
    // the landmark part of e, before the factorisation updates row nf in place: slot order, one thread
    double rms = 0.0;
    if (!SEL && t == 0 && nf > 3) {
        for (int j = 3; j < nf; j += 2) rms += E[j] * E[j] + E[j + 1] * E[j + 1];
        rms = sqrt(rms / (double)m);
    }
    int kmax = 0;
#pragma unroll
    for (int q = 0; q < IPW; ++q) kmax = s_rows[q] > kmax ? s_rows[q] : kmax;

    // ---- column 0 ----
    bool bad_full = false, bad_pose = false;
    if (nf > 0) {
        const double d = A[0];
        if (!pivot_ok(d)) bad_full = bad_pose = true;
        const double s = sqrt(d);
        for (int i = 1 + t; i <= nf; i += TPI) s_col[inst][0][i] = A[i * (i + 1) / 2] / s;
    }
    __syncthreads();
    // ---- columns: col = column k of L below its diagonal (col[nf] = y_k); the update forms column k + 1 in coln ----
    double acc = 0.0, acc_pose = 0.0;
    for (int k = 0; k < kmax; ++k) {
        if (k < nf) {
            const double* col = s_col[inst][k & 1];
            double* coln = s_col[inst][(k + 1) & 1];
            if (t == 0) {
                acc += col[nf] * col[nf];
                if (k == 2) acc_pose = acc;
            }
            const int k1 = k + 1;
            if (k1 < nf) {
                const double c1 = col[k1];
                const double dn = A[k1 * (k1 + 1) / 2 + k1] - c1 * c1;
                if (!pivot_ok(dn)) { bad_full = true; if (k1 < 3) bad_pose = true; }
                const double sn = sqrt(dn);
                for (int i = k1 + g; i <= nf; i += NG) {
                    const double li = col[i];
                    double* row = A + i * (i + 1) / 2;
                    const int jmax = i < nf ? i : nf - 1;
                    for (int j = k1 + l; j <= jmax; j += G) {
                        const double a = row[j] - li * col[j];
                        if (j == k1) { if (i > k1) coln[i] = a / sn; }
                        else row[j] = a;
                    }
                }
            }
        }
        __syncthreads();
    }

    if (!live || t != 0) return;
    if constexpr (SEL) {                             // nees_matched, dof_matched, MATCHED_NOT_PD and the record entries 12 - 14
        int fl = p.flags[b];
        const bool dead = failed || (s_flag[inst] & SLAM_CONSISTENCY_INSTANCE_FAILED) != 0;
        const bool fin = !dead && !bad_full && finite_d(acc);
        if (!dead && bad_full) fl |= SLAM_CONSISTENCY_FULL_NOT_PD;
        p.nees_full[b] = (dead || bad_full) ? __builtin_nan("") : acc;
        p.dof[b] = dead ? 0 : n;
        p.flags[b] = fl;
        double* const r = p.inst_rec + (size_t)b * 16;
        r[12] = fin ? 1.0 : 0.0; r[13] = fin ? acc : 0.0; r[14] = fin ? (double)n : 0.0;
        return;
    }
    int fl = s_flag[inst];
    if (failed) fl = SLAM_CONSISTENCY_INSTANCE_FAILED;
    const double nan = __builtin_nan("");
    double out_full = acc, out_pose = acc_pose;
    if (fl & SLAM_CONSISTENCY_INSTANCE_FAILED) {
        fl = SLAM_CONSISTENCY_INSTANCE_FAILED;
        out_full = out_pose = rms = nan;
    } else {
        if (bad_full) fl |= SLAM_CONSISTENCY_FULL_NOT_PD;
        if (bad_pose) fl |= SLAM_CONSISTENCY_POSE_NOT_PD;
        if (no_truth) {
            out_full = rms = nan;
        }
        if (bad_full) out_full = nan;
        if (bad_pose) out_pose = nan;
    }
    p.nees_full[b] = out_full; p.nees_pose[b] = out_pose; p.map_rms[b] = rms; p.dof[b] = n; p.flags[b] = fl;
}

template <int NMAX, int TPI, int IPW, int G, bool WS, bool SEL = false>
hipError_t launch_class(const ConsistencyParams& p, int f32, hipStream_t stream) {
    const dim3 grid((p.count + IPW - 1) / IPW), block(TPI * IPW);
    if (f32) hipLaunchKernelGGL((consistency_kernel<NMAX, TPI, IPW, G, WS, float, SEL>), grid, block, 0, stream, p);
    else hipLaunchKernelGGL((consistency_kernel<NMAX, TPI, IPW, G, WS, double, SEL>), grid, block, 0, stream, p);
    return hipGetLastError();
}

// the classes of launch_consistency, for either variant
template <bool SEL>
hipError_t launch_classes(ConsistencyParams p, int f32, int chunk, hipStream_t stream) {
    if (p.L_max > kEkfMaxLandmarks || p.B <= 0) return hipErrorInvalidValue;
    if (p.L_max <= 20) { p.b0 = 0; p.count = p.B; return launch_class<43, 64, 4, 16, false, SEL>(p, f32, stream); }
    if (p.L_max <= 50) { p.b0 = 0; p.count = p.B; return launch_class<103, 256, 1, 64, false, SEL>(p, f32, stream); }
    if (!p.ws || chunk <= 0 || p.ws_stride < consistency_ws_per_instance(p.L_max)) return hipErrorInvalidValue;
    for (int b0 = 0; b0 < p.B; b0 += chunk) {   // (launches on one stream: the next chunk reuses the workspace after the last one is done)
        p.b0 = b0; p.count = p.B - b0 < chunk ? p.B - b0 : chunk;
        const hipError_t e = launch_class<3 + 2 * kEkfMaxLandmarks, 1024, 1, 64, true, SEL>(p, f32, stream);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace

size_t consistency_ws_per_instance(int L_max) {
    if (L_max <= 50) return 0;
    const size_t n = 3 + 2 * (size_t)L_max;
    return (n + 1) * (n + 2) / 2;
}

hipError_t launch_consistency(ConsistencyParams p, int f32, int chunk, hipStream_t stream) { return launch_classes<false>(p, f32, chunk, stream); }

hipError_t launch_consistency_selected(ConsistencyParams p, int f32, int chunk, hipStream_t stream) {
    if (!p.sel || !p.sel_row || !p.n_sel || !p.inst_rec || !p.flags || !p.nees_full || !p.dof) return hipErrorInvalidValue;
    return launch_classes<true>(p, f32, chunk, stream);
}

}  // namespace slam
