// pgs_factors.h — the factors (whitened residuals / Jacobians of pose_graph.cpp's Prior / Between / BearingRange factors), per-instance views, deterministic block sums, the cost.
// Part of pgs_kernel.hip (round 6: split by phase, pure moves); included there inside namespace slam { namespace {.  DESIGN.md 4.4.
#pragma once

typedef double dbl4_t __attribute__((ext_vector_type(4)));

// ------------------------------------------------------------------------------------------------------------
// factors (whitened residuals / Jacobians); same formulas as the oracle, see there for the GTSAM definitions
// ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void prior_factor(const PgsParams& p, const double* prior, const double* ps, double e[3]) {
    double s, c;
    det_sincos(ps[2], &s, &c);
    const double dx = prior[0] - ps[0], dy = prior[1] - ps[1];
    e[0] = -(c * dx + s * dy) * p.w_prior[0];
    e[1] = -(-s * dx + c * dy) * p.w_prior[1];
    e[2] = -remainder(prior[2] - ps[2], kTwoPi) * p.w_prior[2];
}

template <bool JAC>
__device__ __forceinline__ void between_factor(const PgsParams& p, const double* pa, const double* pb, float fwd, float ang,
                                               double e[3], double J1[9]) {
    double si, ci, sm, cm;
    det_sincos(pa[2], &si, &ci);
    det_sincos((double)ang, &sm, &cm);
    const double dx = pb[0] - pa[0], dy = pb[1] - pa[1];
    const double hx = ci * dx + si * dy, hy = -si * dx + ci * dy, hth = pb[2] - pa[2];
    const double ux = hx - (double)fwd, uy = hy;
    e[0] = (cm * ux + sm * uy) * p.w_btw[0];
    e[1] = (-sm * ux + cm * uy) * p.w_btw[1];
    e[2] = remainder(hth - (double)ang, kTwoPi) * p.w_btw[2];
    if (JAC) {   // -Ad(h^-1)
        double sh, ch;
        det_sincos(hth, &sh, &ch);
        const double xi = -(ch * hx + sh * hy), yi = sh * hx - ch * hy;
        J1[0] = -ch * p.w_btw[0]; J1[1] = -sh * p.w_btw[0]; J1[2] = -yi * p.w_btw[0];
        J1[3] = sh * p.w_btw[1];  J1[4] = -ch * p.w_btw[1]; J1[5] = xi * p.w_btw[1];
        J1[6] = 0.0;              J1[7] = 0.0;              J1[8] = -p.w_btw[2];
    }
}

template <bool JAC>
__device__ __forceinline__ void bearing_range_factor(const PgsParams& p, const double* ps, const double* l, double b, double r,
                                                     double e[2], double Jp[6], double Jl[4]) {
    double s, c, sb, cb;
    det_sincos(ps[2], &s, &c);
    det_sincos(b, &sb, &cb);
    const double dx = l[0] - ps[0], dy = l[1] - ps[1];
    const double qx = c * dx + s * dy, qy = -s * dx + c * dy;
    const double d2 = qx * qx + qy * qy, n = sqrt(d2);
    const double cp = qx / n, sp = qy / n;
    e[0] = det_atan2(cb * sp - sb * cp, cb * cp + sb * sp) * p.w_meas[0];
    e[1] = (n - r) * p.w_meas[1];
    if (JAC) {
        Jp[0] = (qy / d2) * p.w_meas[0]; Jp[1] = (-qx / d2) * p.w_meas[0]; Jp[2] = -p.w_meas[0];
        Jp[3] = (-qx / n) * p.w_meas[1]; Jp[4] = (-qy / n) * p.w_meas[1]; Jp[5] = 0.0;
        Jl[0] = ((-qy / d2) * c + (qx / d2) * (-s)) * p.w_meas[0];
        Jl[1] = ((-qy / d2) * s + (qx / d2) * c) * p.w_meas[0];
        Jl[2] = (dx / n) * p.w_meas[1];
        Jl[3] = (dy / n) * p.w_meas[1];
    }
}

// per-instance views of slot b: its own copy of the graph arrays, and the inputs of the instance it belongs to (slot j B + instance)
struct Inst {
    const int32_t* cnt; const int32_t* mlm; const double* mb; const double* mr;
    const float* cmds;      // BetweenFactor measurement of pose i at cmds[2 i] (the shared row while cmd_stride = 0)
    const double* prior;    // mean of the PriorFactor
};
__device__ __forceinline__ Inst inst_view(const PgsParams& p, int b) {
    Inst v;
    const size_t inst = (size_t)((unsigned)b % (unsigned)p.B);
    v.cmds = p.cmds + inst * p.cmd_stride;
    v.prior = p.prior + 3 * inst;
    v.cnt = p.cnt + (size_t)b * p.N_max;
    v.mlm = p.mlm + (size_t)b * p.N_max * p.KP;
    v.mb = p.mb + (size_t)b * p.N_max * p.KP;
    v.mr = p.mr + (size_t)b * p.N_max * p.KP;
    return v;
}

// deterministic block sum (fixed tree), result valid in every thread
template <int TPB>
__device__ __forceinline__ double block_sum(double v, double* s_buf) {
    const int tid = threadIdx.x;
    __syncthreads();
    s_buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (int off = TPB / 2; off > 0; off >>= 1) {
        if (tid < off) s_buf[tid] = s_buf[tid] + s_buf[tid + off];
        __syncthreads();
    }
    return s_buf[0];
}

// cost of one bearing-range factor with whitened residual e: 0.5 |e|^2, or (RB) rho(|e|) of the handle's robust loss (pgs_robust.h)
template <bool RB>
__device__ __forceinline__ double factor_cost(const PgsParams& p, const double e[2]) {
    const double ss = e[0] * e[0] + e[1] * e[1];
    if (!RB) return 0.5 * ss;
    double rho, w, sw;
    pgs_robust_loss(p.loss_kind, p.loss_k, ss, sqrt(ss), &rho, &w, &sw);
    return rho;
}

// The absolute fixes of slot b (pgs_fix.h): inputs of the instance it belongs to, like cmds and prior.  Only the kernels built with FX ask.
struct FixView { const double* row; const int32_t* kind; };
__device__ __forceinline__ FixView fix_view(const PgsParams& p, int b) {
    const size_t inst = (size_t)((unsigned)b % (unsigned)p.B);
    return FixView{p.fix_row + inst * p.N_max * kPgsFixRowLen, p.fix_kind + inst * p.N_max};
}

// cost of one fix part with squared whitened residual norm ss: 0.5 ss, or (RB) rho of the fix loss
template <bool RB>
__device__ __forceinline__ double fix_part_cost(const PgsParams& p, double ss) {
    if (!RB) return 0.5 * ss;
    double rho, w, sw;
    pgs_robust_loss(p.fix_loss_kind, p.fix_loss_k, ss, sqrt(ss), &rho, &w, &sw);
    return rho;
}

// acc plus the costs of the fix parts stored at pose i with value ps: position, then heading (the order of sums within a pose, everywhere)
template <bool RB>
__device__ __forceinline__ double add_fix_cost(const PgsParams& p, const FixView& f, const double* ps, int i, double acc) {
    const int fk = f.kind[i];
    const double* row = f.row + (size_t)kPgsFixRowLen * i;
    if (fk & kPgsFixPos) {
        double e[2];
        pgs_fix_pos<false>(ps, row, e, nullptr);
        acc = acc + fix_part_cost<RB>(p, e[0] * e[0] + e[1] * e[1]);
    }
    if (fk & kPgsFixYaw) {
        double wy;
        const double e = pgs_fix_yaw(ps, row, &wy);
        acc = acc + fix_part_cost<RB>(p, e * e);
    }
    return acc;
}

// sum of the costs of the factors owned by pose i: 0.5 |whitened e|^2 of the prior (i = 0) and the between (i, i+1), (FX) the fix parts at i,
// factor_cost of the bearing-range at i
template <bool RB, bool FX>
__device__ __forceinline__ double pose_cost(const PgsParams& p, const Inst& g, const double* pose, const double* lm, int i, int N, int b) {
    double acc = 0.0, e[3];
    if (i == 0) {
        prior_factor(p, g.prior, pose, e);
        acc = acc + 0.5 * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
    if (i + 1 < N) {
        between_factor<false>(p, pose + 3 * i, pose + 3 * (i + 1), g.cmds[2 * i], g.cmds[2 * i + 1], e, nullptr);
        acc = acc + 0.5 * ((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
    }
    if (FX) acc = add_fix_cost<RB>(p, fix_view(p, b), pose + 3 * i, i, acc);
    const int kc = g.cnt[i];
    for (int s = 0; s < kc; ++s) {
        const size_t k = (size_t)i * p.KP + s;
        const int j = g.mlm[k] & (kPgsFirstBit - 1);
        bearing_range_factor<false>(p, pose + 3 * i, lm + 2 * j, g.mb[k], g.mr[k], e, nullptr, nullptr);
        acc = acc + factor_cost<RB>(p, e);
    }
    return acc;
}

template <int TPB, bool RB, bool FX>
__device__ __forceinline__ double block_cost(const PgsParams& p, int b, int N, const double* pose, const double* lm, double* s_buf) {
    const Inst g = inst_view(p, b);
    double acc = 0.0;
    for (int i = threadIdx.x; i < N; i += TPB) acc = acc + pose_cost<RB, FX>(p, g, pose, lm, i, N, b);
    return block_sum<TPB>(acc, s_buf);
}
