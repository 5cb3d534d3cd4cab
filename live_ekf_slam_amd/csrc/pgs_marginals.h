// pgs_marginals.h — marginal covariances of every pose and landmark: the diagonal blocks of H^-1, H = J^T J at lambda = 0
// (gtsam::Marginals(graph, values).marginalCovariance(key), pose_graph.cpp:289-294).
// Part of pgs_kernel.hip; included there inside namespace slam { namespace {.  DESIGN.md 4.4 "Marginal covariances".
//
// The factor comes from the solve's own kernels at lambda = 0 in the sequential elimination order (pgs_launch_marginals): the
// linearisation, H_pp = L_p L_p^T (block bidiagonal: Linv_i = L_ii^-1, G_i = L_{i,i-1}), Y = L_p^-1 H_pl, S = H_ll - Y^T Y = R R^T.  Then
//   pgs_marg_inv_kernel    X = R^-T in place over the upper triangle of S (diagonal included); lm_cov[j] = the 2x2 diagonal block of
//                          S^-1 = X X^T
//   pgs_marg_back_kernel   V = L_p^-T Y in place (= H_pp^-1 H_pl; backward recurrence through the chain, one thread per column) and,
//                          on one lane beside the columns, the diagonal blocks of H_pp^-1:
//                          P_i = Linv_i^T Linv_i + K_i P_{i+1} K_i^T,  K_i = Linv_i^T G_{i+1}^T
//   pgs_marg_gram_kernel   Z = V X on v_mfma_f64_16x16x4_f64, 48 rows (16 poses) per workgroup, and pose_cov[i] = P_i + Z_i Z_i^T
//                          (Sigma_pp = H_pp^-1 + V S^-1 V^T); Z is never stored.
// No atomics; every sum has a fixed order that depends on nothing but the instance's own graph.

// values -> pw / lw, the (landmark, time) event lists (what pgs_lm_begin_kernel builds; nothing of the solve's state is touched),
// the slot's flags for the trial kernels and the FLOP model of the instance
__global__ __launch_bounds__(TPB) void pgs_marg_begin_kernel(const PgsParams p, int which, double* flop) {
    __shared__ int s_cnt[TPB];   // L_max <= 255 < TPB
    const int b = blockIdx.x + p.b_off, tid = threadIdx.x;
    const int N = p.N, M = p.M[b];
    double* pw = p.pw + (size_t)b * p.N_max * 3;
    double* lw = p.lw + (size_t)b * p.L_max * 2;
    const double* p0 = (which ? p.pose1 : p.pose0) + (size_t)b * p.N_max * 3;
    const double* l0 = (which ? p.lm1 : p.lm0) + (size_t)b * p.L_max * 2;
    for (int i = tid; i < 3 * N; i += TPB) pw[i] = p0[i];
    for (int i = tid; i < 2 * M; i += TPB) lw[i] = l0[i];
    const int32_t* head = p.lm_head + (size_t)b * p.L_max;
    const int32_t* mnext = p.mnext + (size_t)b * p.N_max * p.KP;
    int32_t* evt_start = p.evt_start + (size_t)b * (p.L_max + 1);
    int32_t* evt_pose = p.evt_pose + (size_t)b * p.N_max * p.KP;
    int32_t* evt_slot = p.evt_slot + (size_t)b * p.N_max * p.KP;
    int32_t* slot_pos = p.slot_pos + (size_t)b * p.N_max * p.KP;
    int c = 0;
    if (tid < M)
        for (int k = head[tid]; k >= 0; k = mnext[k]) ++c;
    s_cnt[tid] = c;
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int j = 0; j < M; ++j) { const int v = s_cnt[j]; s_cnt[j] = run; run += v; }
        evt_start[M] = run;
    }
    __syncthreads();
    if (tid < M) {
        int pos = s_cnt[tid];
        evt_start[tid] = pos;
        for (int k = head[tid]; k >= 0; k = mnext[k]) { evt_pose[pos] = k / p.KP; evt_slot[pos] = k; slot_pos[k] = pos; ++pos; }
    }
    if (tid == 0) {
        p.state[b] = 0; p.lin_ok[b] = 0; p.solve_ok[b] = 1; p.lambda[b] = 0.0;
        // FLOP model: triangular product 3N (2M)^2, recurrence + Gram 3N 2M (3 + 9), R^-1 and its Gram 2 (2M)^3 / 3,
        // and the lambda = 0 factorisation: Schur complement 3N (2M)^2 + Cholesky (2M)^3 / 3
        const double n3 = 3.0 * N, m2 = 2.0 * M;
        flop[b] = n3 * m2 * m2 + n3 * m2 * 12.0 + 2.0 * m2 * m2 * m2 / 3.0 + n3 * m2 * m2 + m2 * m2 * m2 / 3.0;
    }
}

// X = R^-T over the upper triangle of S, row c of X = column c of R^-1: thread r owns column r of X (row r of R^-1) and fills it from
// the diagonal up, X[c][r] = -(sum_{c < k <= r} X[k][r] R[k][c]) / R[c][c]; column c of R is staged in LDS once per step.
// Then lm_cov[j] = (X X^T)_{jj}: a wavefront per landmark, lanes strided over k, a butterfly sum.
constexpr int MI_TPB = 512;
__global__ __launch_bounds__(MI_TPB) void pgs_marg_inv_kernel(const PgsParams p, double* lm_cov, int32_t* status) {
    __shared__ double s_col[MI_TPB];
    const int b = blockIdx.x + p.b_off, tid = threadIdx.x;
    const int LD = p.LD, M = p.M[b], m2 = 2 * M;
    double* out = lm_cov + (size_t)b * p.L_max * 4;
    if (!p.solve_ok[b]) {   // a non-positive or non-finite pivot in the chain or in the Cholesky factorisation of S: singular
        const double nan = __builtin_nan("");
        for (int i = tid; i < 4 * M; i += MI_TPB) out[i] = nan;
        if (tid == 0) status[b] = 1;
        return;
    }
    if (tid == 0) status[b] = 0;
    double* Sb = p.S + (size_t)b * LD * LD;
#pragma unroll 1
    for (int c = m2 - 1; c >= 0; --c) {
        if (tid >= c && tid < m2) s_col[tid] = Sb[(size_t)tid * LD + c];
        __syncthreads();
        if (tid >= c && tid < m2) {
            const double rc = 1.0 / s_col[c];
            double x = rc;
            if (tid > c) {
                // (the entries of X are a memory round trip each: eight loads in flight, four partial sums - an order fixed by (c, r) alone)
                double s[4] = {0.0, 0.0, 0.0, 0.0};
                const double* Xr = Sb + tid;
                int k = c + 1;
#pragma unroll 1
                for (; k + 7 <= tid; k += 8) {
                    double xk[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) xk[u] = Xr[(size_t)(k + u) * LD];
#pragma unroll
                    for (int u = 0; u < 8; ++u) s[u & 3] += xk[u] * s_col[k + u];
                }
                for (; k <= tid; ++k) s[0] += Xr[(size_t)k * LD] * s_col[k];
                x = -((s[0] + s[1]) + (s[2] + s[3])) * rc;
            }
            Sb[(size_t)c * LD + tid] = x;
        }
        __syncthreads();
    }
    const int w = tid >> 6, lane = tid & 63;
    for (int j = w; j < M; j += MI_TPB / 64) {
        const double* Xa = Sb + (size_t)(2 * j) * LD;
        const double* Xb = Xa + LD;
        double s00 = 0.0, s01 = 0.0, s11 = 0.0;
        for (int k = 2 * j + lane; k < m2; k += 64) {
            const double xa = Xa[k], xb = k > 2 * j ? Xb[k] : 0.0;
            s00 += xa * xa; s01 += xa * xb; s11 += xb * xb;
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { s00 += __shfl_xor(s00, o); s01 += __shfl_xor(s01, o); s11 += __shfl_xor(s11, o); }
        if (lane == 0) { out[4 * j] = s00; out[4 * j + 1] = s01; out[4 * j + 2] = s01; out[4 * j + 3] = s11; }
    }
}

// V = L_p^-T Y in place, from the last pose down: V_i = Linv_i^T (Y_i - G_{i+1}^T V_{i+1}).  Thread 64 + c owns column c; the factor of
// 64 poses at a time is staged in LDS by the first wavefront, whose lane 0 runs the 3x3 recursion of the diagonal blocks of H_pp^-1
// beside the columns and leaves them in pose_cov (lower triangle: 6 of the 9 entries; pgs_marg_gram_kernel completes the block).
__global__ __launch_bounds__(1024) void pgs_marg_back_kernel(const PgsParams p, double* pose_cov) {
    __shared__ double s_f[CHAIN_CH][16];   // Linv_i (6), G_{i+1} (9)
    const int b = blockIdx.x + p.b_off, tid = threadIdx.x;
    if (!p.solve_ok[b]) return;
    const int N = p.N, LD = p.LD, m2 = 2 * p.M[b];
    const double* Lb = p.Linv + (size_t)b * p.N_max * 6;
    const double* Gb = p.G + (size_t)b * p.N_max * 9;
    double* Yb = p.Y + (size_t)b * p.y_stride;
    double* Pb = pose_cov + (size_t)b * p.N_max * 9;
    const int c = tid - 64;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    double P[6] = {0, 0, 0, 0, 0, 0};   // P_{i+1}: 00, 10, 11, 20, 21, 22
    const int nch = (N + CHAIN_CH - 1) / CHAIN_CH;
#pragma unroll 1
    for (int ch = nch - 1; ch >= 0; --ch) {
        const int base = ch * CHAIN_CH;
        const int n = (N - base) < CHAIN_CH ? (N - base) : CHAIN_CH;
        __syncthreads();   // the chunk before is read
        if (tid < n) {
            const int i = base + tid;
#pragma unroll
            for (int k = 0; k < 6; ++k) s_f[tid][k] = Lb[6 * (size_t)i + k];
#pragma unroll
            for (int k = 0; k < 9; ++k) s_f[tid][6 + k] = i + 1 < N ? Gb[9 * (size_t)(i + 1) + k] : 0.0;
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll 1
            for (int l = n - 1; l >= 0; --l) {
                const double* o = s_f[l];
                const double I0 = o[0], I1 = o[1], I2 = o[2], I3 = o[3], I4 = o[4], I5 = o[5];
                double K[9];   // K = Linv^T G^T: K[a][r] = sum_m Linv[m][a] G[r][m]
#pragma unroll
                for (int r = 0; r < 3; ++r) {
                    const double g0 = o[6 + 3 * r], g1 = o[7 + 3 * r], g2 = o[8 + 3 * r];
                    K[r] = (I0 * g0 + I1 * g1) + I3 * g2;
                    K[3 + r] = I2 * g1 + I4 * g2;
                    K[6 + r] = I5 * g2;
                }
                const double Pf[9] = {P[0], P[1], P[3], P[1], P[2], P[4], P[3], P[4], P[5]};
                double T[9];   // T = K P
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int q = 0; q < 3; ++q) T[3 * a + q] = (K[3 * a] * Pf[q] + K[3 * a + 1] * Pf[3 + q]) + K[3 * a + 2] * Pf[6 + q];
                // Linv^T Linv (lower triangle) + T K^T
                const double B00 = (I0 * I0 + I1 * I1) + I3 * I3, B10 = I1 * I2 + I3 * I4, B11 = I2 * I2 + I4 * I4;
                const double B20 = I3 * I5, B21 = I4 * I5, B22 = I5 * I5;
                P[0] = B00 + ((T[0] * K[0] + T[1] * K[1]) + T[2] * K[2]);
                P[1] = B10 + ((T[3] * K[0] + T[4] * K[1]) + T[5] * K[2]);
                P[2] = B11 + ((T[3] * K[3] + T[4] * K[4]) + T[5] * K[5]);
                P[3] = B20 + ((T[6] * K[0] + T[7] * K[1]) + T[8] * K[2]);
                P[4] = B21 + ((T[6] * K[3] + T[7] * K[4]) + T[8] * K[5]);
                P[5] = B22 + ((T[6] * K[6] + T[7] * K[7]) + T[8] * K[8]);
                double* Po = Pb + 9 * (size_t)(base + l);
#pragma unroll
                for (int k = 0; k < 6; ++k) Po[k] = P[k];
            }
        } else if (c >= 0 && c < m2) {
            double* Yi = Yb + (size_t)3 * (base + n - 1) * LD + c;
#pragma unroll 2
            for (int l = n - 1; l >= 0; --l) {
                const double* o = s_f[l];
                const double u0 = Yi[0] - ((o[6] * v0 + o[9] * v1) + o[12] * v2);   // (G^T v)_a = sum_r G[r][a] v_r
                const double u1 = Yi[LD] - ((o[7] * v0 + o[10] * v1) + o[13] * v2);
                const double u2 = Yi[2 * LD] - ((o[8] * v0 + o[11] * v1) + o[14] * v2);
                v0 = (o[0] * u0 + o[1] * u1) + o[3] * u2;
                v1 = o[2] * u1 + o[4] * u2;
                v2 = o[5] * u2;
                Yi[0] = v0; Yi[LD] = v1; Yi[2 * LD] = v2;
                Yi -= 3 * LD;
            }
        }
    }
}

// pose_cov[i] = P_i + Z_i Z_i^T, Z = V X.  One workgroup per 16 poses (48 rows of V = three 16-row MFMA tiles) of one instance; wavefront
// w forms the 16-column blocks w, w + 4, ... of Z (k runs over the rows of X up to the block's last column: X is upper triangular),
// passes each block through LDS and adds the products of its pose rows: lane (q, pl) takes pose pl and the block's columns 4 q .. 4 q + 3.
// The lanes' sums meet in LDS and are added in a fixed order.  Operands: lane (kq, cl) feeds the MFMA step s of a 16-k block with
// k = 4 kq + s on both sides (one 32-byte load of V per lane and block), which only permutes the order of the sum.
constexpr int MG_TPB = 256, MG_NW = MG_TPB / 64;
__global__ __launch_bounds__(MG_TPB) void pgs_marg_gram_kernel(const PgsParams p, double* pose_cov, int ntile) {
    __shared__ double s_z[MG_NW][48][17];
    __shared__ double s_red[MG_NW][64][6];
    const int bl = blockIdx.x / ntile, t0 = 16 * (blockIdx.x - bl * ntile);
    const int b = bl + p.b_off, tid = threadIdx.x;
    const int N = p.N, LD = p.LD, m2 = 2 * p.M[b];
    double* Pb = pose_cov + (size_t)b * p.N_max * 9;
    if (!p.solve_ok[b]) {
        const double nan = __builtin_nan("");
        for (int i = tid; i < 16 * 9; i += MG_TPB)
            if (t0 + i / 9 < N) Pb[9 * (size_t)t0 + i] = nan;
        return;
    }
    typedef double dbl4v_t __attribute__((ext_vector_type(4)));
    const int w = tid >> 6, lane = tid & 63, kq = lane >> 4, cl = lane & 15;
    const double* Vb = p.Y + (size_t)b * p.y_stride;
    const double* Xb = p.S + (size_t)b * LD * LD;
    const int r0 = 3 * t0, R3 = 3 * N;
    const double* vrow[3];
    bool vin[3];
#pragma unroll
    for (int s = 0; s < 3; ++s) {
        const int r = r0 + 16 * s + cl;
        vin[s] = r < R3;
        vrow[s] = Vb + (size_t)(vin[s] ? r : 0) * LD + 4 * kq;
    }
    double g[6] = {0, 0, 0, 0, 0, 0};   // pose (lane & 15), columns 4 kq .. of every block: 00, 10, 11, 20, 21, 22
    const int nkb = (m2 + 15) >> 4;
#pragma unroll 1
    for (int kb = w; kb < nkb; kb += MG_NW) {
        dbl4_t acc[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) acc[s] = dbl4_t{0.0, 0.0, 0.0, 0.0};
        const int n = 16 * kb + cl;   // this lane's column of X
#pragma unroll 1
        for (int j0 = 0; j0 <= 16 * kb; j0 += 16) {
            const int jq = j0 + 4 * kq;
            dbl4v_t a[3];
            double x[4];
#pragma unroll
            for (int s = 0; s < 3; ++s) a[s] = vin[s] ? *reinterpret_cast<const dbl4v_t*>(vrow[s] + j0) : dbl4v_t{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int j = jq + q;
                const bool in = j <= n && n < m2;   // (the upper triangle of S holds X, the rest R)
                x[q] = in ? Xb[(size_t)j * LD + n] : 0.0;
#pragma unroll
                for (int s = 0; s < 3; ++s) if (j >= m2) a[s][q] = 0.0;   // (columns of Y beyond the landmarks': the gradient column, then nothing)
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int s = 0; s < 3; ++s) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[s][q], x[q], acc[s], 0, 0, 0);
        }
#pragma unroll
        for (int s = 0; s < 3; ++s)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) s_z[w][16 * s + kq + 4 * r4][cl] = acc[s][r4];   // C/D layout: row = (lane >> 4) + 4 reg, column = lane & 15
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double z0 = s_z[w][3 * cl][4 * kq + q], z1 = s_z[w][3 * cl + 1][4 * kq + q], z2 = s_z[w][3 * cl + 2][4 * kq + q];
            g[0] += z0 * z0; g[1] += z1 * z0; g[2] += z1 * z1; g[3] += z2 * z0; g[4] += z2 * z1; g[5] += z2 * z2;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) s_red[w][lane][k] = g[k];
    __syncthreads();
    if (tid < 16 * 6) {
        const int pl = tid / 6, k = tid - 6 * pl;
        if (t0 + pl < N) {
            double* Po = Pb + 9 * (size_t)(t0 + pl);
            double v = Po[k];
#pragma unroll
            for (int ww = 0; ww < MG_NW; ++ww)
#pragma unroll
                for (int q = 0; q < 4; ++q) v += s_red[ww][16 * q + pl][k];
            s_red[0][pl][k] = v;   // (entry [0][pl][k] was read by this thread alone: q = 0, lane pl)
        }
    }
    __syncthreads();
    if (tid < 16 && t0 + tid < N) {   // the full block, both halves from one value
        const double* v = s_red[0][tid];
        double* Po = Pb + 9 * (size_t)(t0 + tid);
        Po[0] = v[0]; Po[1] = v[1]; Po[2] = v[3];
        Po[3] = v[1]; Po[4] = v[2]; Po[5] = v[4];
        Po[6] = v[3]; Po[7] = v[4]; Po[8] = v[5];
    }
}
