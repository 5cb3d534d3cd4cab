// ekf_big_kernel.hip — EKF::update (reference ekf_ws/src/localization_pkg/src/ekf.cpp:37-179) for states that do NOT fit the LDS size
// classes of ekf_kernel_impl.h (n = 3 + 2 L > 403, up to kEkfBigMaxLandmarks landmarks).  The reference grows its state by two per new
// landmark without limit (ekf.cpp:144-146); the fused kernel keeps an instance's thin rows / columns and its K / H P ring in LDS and
// therefore ends at 200 landmarks.  This kernel is the size class beyond: one workgroup per instance, ONE timestep per launch, the
// covariance streamed through HBM / L2 for every phase.  It follows the reference's loop detection by detection (association, update or
// insertion, in message order) - which also means a message may hold ANY number of detections here (read from the caller's buffer as it is
// walked; no per-message capacity) - and evaluates every element with the same expressions in the same order as the fused kernel and the
// oracle's MODE_FAST (the functions of ekf_model.h, which both kernels call: this file holds the decomposition over 1024 threads, where the
// operands live, the barriers and the flags), so results are bit-identical to both.  It is slow by design (a pass over P per detection instead of one per group of
// deferred updates, a barrier per phase); SLAM_ERR_UNSUPPORTED for a legal reference configuration was the alternative.
//
// Working matrix: the step works on a copy of P in the handle's second buffer with the FIXED leading dimension ekf_ld(3 + 2 L_max) (no
// re-layout when landmarks are inserted); the result is compacted into the first buffer with the leading dimension of the new state size,
// the layout every getter expects.  An instance that freezes (filter.h:5: the reference dies on an out-of-range index) simply does not
// write anything back: its pre-step state is still in the first buffer.
#include "ekf_kernel.h"

#include <stdio.h>
#include <string.h>

#include "../../include/slam_batch.h"
#include "lds_attr.h"
#include "ekf_model.h"
#include "sim_device.h"
#include "slam_rng.h"

namespace slam {

namespace {

constexpr int kBigTpb = 1024;

// LDS layout (dynamic): x_t [np], x_pred [np], K / P H^T [2 np] (interleaved per state index), H P [2 np] (row 0, row 1), scalars [32],
// ints [16], new ids [L_max], message [3 L] floats (SIM mode)
// ST = storage type of x_t and P_t.  double: the streamed size class (L_max > 200) and the long messages of the fp64 LDS classes.  float
// (round 5): the long messages of the fp32-storage classes - x_t / P_t are read as floats, the timestep runs in fp64 in the working matrix
// (the handle's fp64 slab `scratch`, [B][pstride] doubles: n x ld8(n) fits since ld4(n) >= ld8(n)) and the result is rounded to float where it
// is stored: the oracle's STORAGE_F32 (slam_oracle.cpp round_storage: once per timestep), which is what the fp32 LDS kernel computes too.
template <class ST>
__global__ __launch_bounds__(kBigTpb) void ekf_big_step_kernel(const EkfStepParams p, const int t_off, const int multi) {
    constexpr int ESZ = (int)sizeof(ST);
    extern __shared__ double sm[];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
    const StepNoise nz = step_noise(p, b);   // the instance's noise values (its row of slam_set_noise_each or the block's scalars), read once
    const int Lcap = p.L_max, nmax = 3 + 2 * Lcap, np = (nmax + 1) & ~1;
    double* const s_xt = sm;
    double* const s_xp = s_xt + np;
    double* const s_K = s_xp + np;          // [r][2]
    double* const s_HP = s_K + 2 * np;      // [2][np]
    double* const s_sc = s_HP + 2 * np;     // 32 scalars
    int* const s_i = reinterpret_cast<int*>(s_sc + 32);   // 16 ints: 0 association result, 1 freeze, 2 flags raised, 3 detections, 4 non-finite
    int* const s_newid = s_i + 16;                        // ids of the landmarks inserted by this message
    float* const s_meas = reinterpret_cast<float*>(s_newid + ((Lcap + 1) & ~1));

    if (p.long_mode == 2) {   // paired with the LDS kernel's launch: only the instances whose message that kernel cannot hold (ekf_kernel.h)
        const int kk = p.meas_count_in[b];
        if ((kk < p.k_stride_in ? kk : p.k_stride_in) <= p.long_cap) return;
    }
    int flags = p.flags[b];
    if (flags & SLAM_INST_INDEX_OOR) return;   // frozen instance: the state stays as it is
    const int M0 = p.M[b], n0 = 3 + 2 * M0;
    const int ldw = ekf_ld(nmax, 8);           // leading dimension of the working matrix
    const int ld0 = ekf_ld(n0, ESZ);
    const ST* PA = static_cast<const ST*>(p.P) + (size_t)b * p.pstride;
    double* __restrict__ PB = (ESZ == 8 ? static_cast<double*>(p.P_out) : p.scratch) + (size_t)b * p.pstride;
    ST* __restrict__ xb = static_cast<ST*>(p.x) + (size_t)b * p.xstride;
    const int* __restrict__ idsb = p.ids + (size_t)b * p.L_max;

    for (int i = tid; i < np; i += kBigTpb) {
        const double v = i < n0 ? (double)xb[i] : 0.0;
        s_xt[i] = v; s_xp[i] = v;
    }
    if (tid < 16) s_i[tid] = 0;
    // the command array (per-instance, shared multi-step, or none: fwd / ang) is chosen first, then read once (selecting between the
    // three values instead put this kernel's stack in scratch)
    const float* const cp = p.cmd_each ? p.cmd_each + ((size_t)t_off * p.B + b) * 2 : (multi ? p.cmds + 2 * t_off : nullptr);
    const float fwd = cp ? cp[0] : p.fwd;
    const float ang = cp ? cp[1] : p.ang;
    // ---- the message of this timestep ----
    double tx = 0.0, ty = 0.0, tth = 0.0;
    const float* meas = s_meas;
    if (p.sim) {
        if (tid < 64) {
            tx = p.truth[3 * (size_t)b]; ty = p.truth[3 * (size_t)b + 1]; tth = p.truth[3 * (size_t)b + 2];
            const int Lm = sim_map_size(p, b);
            const double* const map = sim_map(p, b);
            const double lmx0 = lane < Lm ? map[2 * lane] : 0.0, lmy0 = lane < Lm ? map[2 * lane + 1] : 0.0;
            const int kr = sim_wave<(1 << 30), false>(p, b, lane, fwd, ang, p.step + (uint32_t)t_off, map, Lm, tx, ty, tth, lmx0, lmy0, s_meas, nz.sim);
            if (lane == 0) { s_i[3] = kr; s_sc[24] = tx; s_sc[25] = ty; s_sc[26] = tth; }
        }
    } else {
        int kk = p.meas_count_in[(size_t)t_off * p.B + b];
        kk = kk < p.k_stride_in ? kk : p.k_stride_in;
        kk = kk < 0 ? 0 : kk;
        if (tid == 0) s_i[3] = kk;
        meas = p.meas_in + ((size_t)t_off * p.B + b) * p.k_stride_in * 3;   // walked where it lies: no per-message capacity
    }
    __syncthreads();
    const int k = s_i[3];
    if (tid == 0 && p.khist != nullptr) atomicAdd(&p.khist[k < 7 ? k : 7], 1ull);
    if (p.sim && p.meas_out != nullptr) {
        for (int i = tid; i < 3 * k && i < 3 * p.k_stride_out; i += kBigTpb) p.meas_out[(size_t)b * p.k_stride_out * 3 + i] = s_meas[i];
        if (tid == 0) p.meas_count_out[b] = k < p.k_stride_out ? k : p.k_stride_out;
    }

    // ---- prediction (ekf.cpp:41-61): x_pred of the vehicle, P_pred = F_x P F_x^T + F_v V F_v^T into the working matrix ----
    {
        const EkfMotion m = ekf_motion(s_xt[0], s_xt[1], s_xt[2], fwd, ang, nz.v_d, nz.v_th, nz.V00);
        __syncthreads();
        if (tid == 0) { s_xp[0] = m.xp0; s_xp[1] = m.xp1; s_xp[2] = m.xp2; }
        const double p22 = (double)PA[(size_t)2 * ld0 + 2];
        for (int e = tid; e < n0 * n0; e += kBigTpb) {
            const int r = e / n0, c = e - r * n0;
            const double p2c = r < 2 ? (double)PA[(size_t)2 * ld0 + c] : 0.0;   // rows 0, 1 of F_x P
            const double pr2 = c < 2 ? (double)PA[(size_t)r * ld0 + 2] : 0.0;   // cols 0, 1 of (F_x P) F_x^T
            const double q_rc = r == 0 ? (c == 0 ? m.q00 : m.q01) : (c == 0 ? m.q10 : m.q11);   // F_v V F_v^T
            PB[(size_t)r * ldw + c] = ekf_predicted((double)PA[(size_t)r * ld0 + c], r, c, p2c, pr2, p22, m.fa, m.fb, q_rc, nz.V11);
        }
    }
    __syncthreads();

    int M = M0, n = n0;
    // ---- detections in message order (ekf.cpp:73): association, then landmark update or insertion ----
#pragma unroll 1
    for (int l = 0; l < k; ++l) {
        const float idf = meas[3 * l], r_m = meas[3 * l + 1], b_m = meas[3 * l + 2];
        // association: first match wins (ekf.cpp:82-108); every thread scans a stride of the landmarks, the lowest hit is kept
        if (tid == 0) s_i[0] = 0x7fffffff;
        __syncthreads();
        int id = M;
        {
            int hit = 0x7fffffff;
            if (p.id_known) {
                id = (int)idf;
                for (int j = tid; j < M; j += kBigTpb) {
                    const int idj = j < M0 ? idsb[j] : s_newid[j - M0];
                    if (idj == id) { hit = j; break; }
                }
            } else {
                double s, c;
                det_sincos(s_xp[2] + (double)b_m, &s, &c);
                const float x_det = (float)(s_xp[0] + (double)r_m * c);
                const float y_det = (float)(s_xp[1] + (double)r_m * s);
                for (int j = tid; j < M; j += kBigTpb) {
                    const float xd = assoc_abs((double)x_det - s_xp[3 + 2 * j], p.abs_is_int);
                    const float yd = assoc_abs((double)y_det - s_xp[3 + 2 * j + 1], p.abs_is_int);
                    if (xd < p.min_sep && yd < p.min_sep) { hit = j; break; }
                }
            }
            if (hit != 0x7fffffff) atomicMin(&s_i[0], hit);
        }
        __syncthreads();
        const int i = s_i[0] == 0x7fffffff ? -1 : s_i[0];
        if (i >= 0) {
            // ---------------- landmark update, ekf.cpp:110-140 ----------------
            const int ii = 2 * i + 3;
            if (ii + 1 >= n0) {   // x_t(ii) out of range (a landmark this message inserted): the reference throws, the instance freezes
                if (tid == 0) s_i[1] = 1;
                __syncthreads();
                break;
            }
            if (tid == 0) {   // the scalar chain: Jacobian entries with the reference's float truncations, innovation
                const double* const xl = p.lm_from_pred ? s_xp : s_xt;   // quirk D-2
                const EkfRange g = ekf_range(xl[ii], xl[ii + 1], s_xp[0], s_xp[1]);
                const EkfH hj = ekf_jacobian(g.dx, g.dy, g.dd, g.d2);
                s_sc[0] = hj.h00; s_sc[1] = hj.h01; s_sc[2] = hj.h03; s_sc[3] = hj.h04;   // H0 at columns 0, 1, ii, ii+1
                s_sc[4] = hj.h10; s_sc[5] = hj.h11; s_sc[6] = hj.h13; s_sc[7] = hj.h14;   // H1 at columns 0, 1, ii, ii+1 (H1[2] = -1)
                const EkfVec2 nu = ekf_innovation(r_m, b_m, g.dist, g.dx, g.dy, s_xp[2], nz.w_r, nz.w_b);
                s_sc[8] = nu.x; s_sc[9] = nu.y;
            }
            __syncthreads();
            const EkfH h = {s_sc[0], s_sc[1], s_sc[2], s_sc[3], s_sc[4], s_sc[5], s_sc[6], s_sc[7]};
            for (int c = tid; c < n; c += kBigTpb) {   // H P (rows of P) and P H^T (columns of P)
                const EkfVec2 g = ekf_hp_col(h, PB[c], PB[(size_t)ldw + c], PB[(size_t)2 * ldw + c], PB[(size_t)ii * ldw + c], PB[(size_t)(ii + 1) * ldw + c]);
                s_HP[c] = g.x;
                s_HP[np + c] = g.y;
                const double* pr = PB + (size_t)c * ldw;
                const EkfVec2 ph = ekf_pht_row(h, pr[0], pr[1], pr[2], pr[ii], pr[ii + 1]);
                s_K[2 * c] = ph.x;
                s_K[2 * c + 1] = ph.y;
            }
            __syncthreads();
            if (tid == 0) {   // S = (H P) H^T + W and its inverse (ekf.cpp:133-135)
                auto col = [&](int c) -> EkfVec2 { return EkfVec2{s_HP[c], s_HP[np + c]}; };
                const EkfS S = ekf_S(h, col(0), col(1), col(2), col(ii), col(ii + 1), nz.W00, nz.W11);
                double Si[4];
                if (!inv2x2_lu(S.s, Si)) s_i[2] |= SLAM_INST_S_SINGULAR;
                s_sc[10] = Si[0]; s_sc[11] = Si[1]; s_sc[12] = Si[2]; s_sc[13] = Si[3];
            }
            __syncthreads();
            {
                const double si0 = s_sc[10], si1 = s_sc[11], si2 = s_sc[12], si3 = s_sc[13], nu0 = s_sc[8], nu1 = s_sc[9];
                for (int r = tid; r < n; r += kBigTpb) {   // K = (P H^T) S^-1, x_pred += K nu
                    const EkfVec2 kk = ekf_gain(EkfVec2{s_K[2 * r], s_K[2 * r + 1]}, si0, si1, si2, si3);
                    s_K[2 * r] = kk.x; s_K[2 * r + 1] = kk.y;
                    s_xp[r] = ekf_state_update(s_xp[r], r, kk.x, kk.y, nu0, nu1);
                }
            }
            __syncthreads();
            {   // P_pred -= K (H P): one pass over the working matrix, a lane owns a 16-byte column pair
                typedef double dbl2_t __attribute__((ext_vector_type(2)));
                const int nv = (n + 1) >> 1;
                for (int e = tid; e < n * nv; e += kBigTpb) {
                    const int r = e / nv, j = e - r * nv, c = 2 * j;
                    const double k0 = s_K[2 * r], k1 = s_K[2 * r + 1];
                    dbl2_t v = *reinterpret_cast<dbl2_t*>(PB + (size_t)r * ldw + c);
                    v.x = ekf_downdate(v.x, k0, k1, s_HP[c], s_HP[np + c]);
                    if (c + 1 < n) v.y = ekf_downdate(v.y, k0, k1, s_HP[c + 1], s_HP[np + c + 1]);
                    *reinterpret_cast<dbl2_t*>(PB + (size_t)r * ldw + c) = v;
                }
            }
            __syncthreads();
        } else {
            // ---------------- landmark insertion, ekf.cpp:141-173 ----------------
            if (M >= Lcap) {   // no room: skipped (the reference has no capacity; here SLAM_INST_CAPACITY)
                if (tid == 0) s_i[2] |= SLAM_INST_CAPACITY;
                __syncthreads();   // (everybody has read this detection's association result before the next one resets it)
                continue;
            }
            const int no = n;
            const EkfInsert g = ekf_insert_geom(s_xp[0], s_xp[1], s_xp[2], r_m, b_m);
            __syncthreads();
            if (tid == 0) {
                s_xp[no] = g.lx;
                s_xp[no + 1] = g.ly;
                s_newid[M - M0] = p.id_known ? id : M;
            }
            for (int j = tid; j < no; j += kBigTpb) {   // new rows G_x P[0:3, :] and new columns P[:, 0:3] G_x^T
                const double r2 = PB[(size_t)2 * ldw + j];
                PB[(size_t)no * ldw + j] = ekf_insert_row(PB[j], g.g02, r2);
                PB[(size_t)(no + 1) * ldw + j] = ekf_insert_row(PB[(size_t)ldw + j], g.g12, r2);
                const double* pr = PB + (size_t)j * ldw;
                const double c0 = pr[0], c1 = pr[1], c2 = pr[2];
                PB[(size_t)j * ldw + no] = ekf_insert_col(c0, c2, g.g02);
                PB[(size_t)j * ldw + no + 1] = ekf_insert_col(c1, c2, g.g12);
            }
            __syncthreads();
            if (tid == 0) {   // corner: (G_x P_vv) G_x^T + (G_z W) G_z^T
                const double* Ra = PB + (size_t)no * ldw;
                const double* Rb = PB + (size_t)(no + 1) * ldw;
                const EkfCorner v = ekf_insert_corner(Ra[0], Ra[1], Ra[2], Rb[0], Rb[1], Rb[2], g.g02, g.g12, g.c, g.s, nz.W00, nz.W11);
                PB[(size_t)no * ldw + no] = v.v00; PB[(size_t)no * ldw + no + 1] = v.v01;
                PB[(size_t)(no + 1) * ldw + no] = v.v10; PB[(size_t)(no + 1) * ldw + no + 1] = v.v11;
            }
            M += 1;
            n += 2;
            __syncthreads();
        }
    }
    __syncthreads();
    flags |= s_i[2];
    if (s_i[1]) {   // frozen in the pre-step state: nothing of this timestep is written (filter.h:5)
        if (tid == 0) p.flags[b] = flags | SLAM_INST_INDEX_OOR;
        return;
    }
    // ---- x_t = x_pred, P_t = P_pred (ekf.cpp:176-177): compact the working matrix into the layout of the new state size ----
    const int ldn = ekf_ld(n, ESZ);
    ST* PAw = const_cast<ST*>(PA);
    int bad = 0;
    for (int e = tid; e < n * ldn; e += kBigTpb) {
        const int r = e / ldn, c = e - r * ldn;
        const ST v = (ST)(c < n ? PB[(size_t)r * ldw + c] : 0.0);   // pad columns stay zero
        bad |= !isfinite(v);
        PAw[e] = v;
    }
    for (int i = tid; i < n; i += kBigTpb) {
        const ST v = (ST)s_xp[i];
        bad |= !isfinite(v);
        xb[i] = v;
    }
    if (bad) s_i[4] = 1;
    for (int q = tid; q < M - M0; q += kBigTpb) p.ids[(size_t)b * p.L_max + M0 + q] = s_newid[q];
    __syncthreads();
    if (tid == 0) {
        if (s_i[4]) flags |= SLAM_INST_NONFINITE;
        p.M[b] = M;
        p.flags[b] = flags;
        p.timestep[b] = p.timestep[b] + 1;
        if (p.sim) {   // plotting_node.py:209-212 with the float32 wire format of EKFState.x_v / y_v
            p.err_sum[b] = p.err_sum[b] + ekf_position_error(s_xp[0], s_xp[1], s_sc[24], s_sc[25]);
            p.truth[3 * (size_t)b] = s_sc[24]; p.truth[3 * (size_t)b + 1] = s_sc[25]; p.truth[3 * (size_t)b + 2] = s_sc[26];
        }
    }
}

size_t big_lds_bytes(int L_max, int L_map) {
    const int nmax = 3 + 2 * L_max, np = (nmax + 1) & ~1;
    return sizeof(double) * (size_t)(6 * np + 32) + sizeof(int) * (size_t)(16 + ((L_max + 1) & ~1)) + sizeof(float) * 3 * (size_t)(L_map > 1 ? L_map : 1) + 16;
}

}  // namespace

hipError_t launch_ekf_big_step(const EkfStepParams& p, hipStream_t stream, int f32_storage) {
    const size_t lds = big_lds_bytes(p.L_max, p.sim ? p.L : 1);
    if (lds > 160 * 1024) return hipErrorInvalidConfiguration;
    if (f32_storage && p.scratch == nullptr) return hipErrorInvalidValue;   // the fp64 working matrix of an fp32-storage handle
    const void* fn = f32_storage ? reinterpret_cast<const void*>(&ekf_big_step_kernel<float>) : reinterpret_cast<const void*>(&ekf_big_step_kernel<double>);
    if (lds > 64 * 1024) {   // once per device, to the kernel's maximum (lds_attr.h)
        const hipError_t e = slam_allow_full_lds(fn);
        if (e != hipSuccess) return e;
    }
    const int multi = (ekf_device_cmds(p) && p.T > 1) ? 1 : 0;
    const int T = multi ? p.T : 1;
    for (int t = 0; t < T; ++t) {   // one launch per timestep: the kernel keeps nothing on chip between steps
        if (f32_storage) hipLaunchKernelGGL(ekf_big_step_kernel<float>, dim3(p.B), dim3(kBigTpb), lds, stream, p, t, multi);
        else hipLaunchKernelGGL(ekf_big_step_kernel<double>, dim3(p.B), dim3(kBigTpb), lds, stream, p, t, multi);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t ekf_big_kernel_info(EkfKernelInfo* out) {
    hipFuncAttributes a;
    const hipError_t e = hipFuncGetAttributes(&a, reinterpret_cast<const void*>(&ekf_big_step_kernel<double>));
    if (e != hipSuccess) return e;
    snprintf(out->name, sizeof(out->name), "ekf_big_step_kernel");
    out->lds_bytes = (int)a.sharedSizeBytes;
    out->vgprs = a.numRegs;
    out->sgprs = 0;
    out->threads = kBigTpb;
    out->wg_per_cu = 1;
    return hipSuccess;
}

}  // namespace slam
