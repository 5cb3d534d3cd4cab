// pgs_fix_phase.h — absolute fixes of the pose graph outside the solve: attaching a fix to the newest pose, the simulated source, the weights.
// Part of pgs_kernel.hip; included there inside namespace slam { namespace {.  The factor itself: pgs_fix.h; its terms in the solve:
// pgs_linearize_kernel, pgs_evaluate_kernel, pose_cost (the FX instantiations).  DESIGN.md 4.4 "Absolute fixes".
#pragma once

// One lane per instance: row b of fix / kinds is validated part by part (pgs_fix_check_*), the STORED parts go to pose N - 1 of the instance's
// fix_row / fix_kind.  A part the call carries replaces that part at that pose, a part it does not carry (or carries INVALID) stays.
__global__ __launch_bounds__(256) void pgs_fix_attach_kernel(const PgsParams p, double* fix_row, int32_t* fix_kind, const double* fix,
                                                             const int32_t* kinds, int32_t* verdict) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const int i = p.N - 1;
    if (i < 0 || i >= p.N_max) return;
    const double* row = fix + (size_t)b * kPgsFixRowLen;
    const int k = kinds[b];
    const int vp = pgs_fix_check_pos(k, row), vy = pgs_fix_check_yaw(k, row);
    double* dst = fix_row + ((size_t)b * p.N_max + i) * kPgsFixRowLen;
    int32_t* dk = fix_kind + (size_t)b * p.N_max + i;
    int have = *dk;
    if (vp == kPgsFixStored) { dst[0] = row[0]; dst[1] = row[1]; dst[3] = row[3]; have |= kPgsFixPos; }
    if (vy == kPgsFixStored) { dst[2] = row[2]; dst[4] = row[4]; have |= kPgsFixYaw; }
    *dk = have;
    if (verdict) verdict[b] = vp | (vy << 4);
}

// The simulated source: fix_sense_instance of fix_kernel.h (the EKF batch's; its pair indices G = 0x50000000 ...) on the pose graph's truth,
// seed, global instance id and the RNG step the next pgs_run_sim tick would use.  One lane per instance; reads state, advances none.
__global__ __launch_bounds__(256) void pgs_fix_sense_kernel(const PgsParams p, const slam_fix_sensor* rows, uint32_t step, double* fix,
                                                            int32_t* kinds, int32_t* jumped) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= p.B) return;
    const slam_fix_sensor row = rows ? rows[b] : fix_sensor_default_row();
    const FixSensed o = fix_sense_instance(row, p.seed, (uint64_t)(p.inst0 + b), step, p.truth[3 * (size_t)b], p.truth[3 * (size_t)b + 1],
                                           p.truth[3 * (size_t)b + 2]);
#pragma unroll
    for (int i = 0; i < kFixRowLen; ++i) fix[(size_t)b * kFixRowLen + i] = o.row[i];
    kinds[b] = o.kinds;
    if (jumped) jumped[b] = o.jumped;
}

// IRLS weight of both parts of the fix at every pose, at initial_estimate (which = 0) / result (1): what the solve believed of each fix.  One
// thread per pose slot; out [B][N_max][2] (position, heading), NaN where the part is not stored and at poses the graph does not have.
__global__ __launch_bounds__(256) void pgs_fix_weights_kernel(const PgsParams p, int which, double* out) {
    const int nb = (p.N_max + 255) / 256;
    const int b = blockIdx.x / nb, i = (blockIdx.x - b * nb) * 256 + threadIdx.x;
    if (b >= p.B || i >= p.N_max) return;
    double w[2] = {__builtin_nan(""), __builtin_nan("")};
    if (i < p.N) {
        const double* ps = (which ? p.pose1 : p.pose0) + (size_t)b * p.N_max * 3 + 3 * i;
        const double* row = p.fix_row + ((size_t)b * p.N_max + i) * kPgsFixRowLen;
        const int fk = p.fix_kind[(size_t)b * p.N_max + i];
        double rho, sw;
        if (fk & kPgsFixPos) {
            double e[2];
            pgs_fix_pos<false>(ps, row, e, nullptr);
            const double ss = e[0] * e[0] + e[1] * e[1];
            pgs_robust_loss(p.fix_loss_kind, p.fix_loss_k, ss, sqrt(ss), &rho, &w[0], &sw);
        }
        if (fk & kPgsFixYaw) {
            double wy;
            const double e = pgs_fix_yaw(ps, row, &wy);
            const double ss = e * e;
            pgs_robust_loss(p.fix_loss_kind, p.fix_loss_k, ss, sqrt(ss), &rho, &w[1], &sw);
        }
    }
    out[((size_t)b * p.N_max + i) * 2] = w[0];
    out[((size_t)b * p.N_max + i) * 2 + 1] = w[1];
}
