// innovation_kernel.hip — the innovation statistics of the message the next EKF step will process, for every instance of a batch
// (slam_innovation, slam_innovation_run).  The definition is innovation_instance() in innovation_kernel.h; this file maps it to the device.
//
// Mapping: ONE WAVEFRONT PER INSTANCE, kInnovWaves instances per workgroup.  An instance needs x[J] and the J x J block of P
// (J = pose + the mapped landmarks of its message: 7 x 7 at the mean message of 1.65 detections, at most 35 x 35), its ids and its message:
// about half a kilobyte against the 171 KB its timestep moves at L = 50.  The block lives in the wavefront's slice of LDS (12.3 KB); the
// lanes gather it (element loads: a landmark's pair of columns starts at an odd index, so it is not a 16-byte aligned pair in either
// storage type), look ids up by ballot, and take the columns of H P, the rows of K and the elements of the downdate; the scalar chain of a
// detection (Jacobian entries, atan2, the 2 x 2 inverse) is evaluated by every lane alike.  Phases are ordered by wavefront fences: no
// workgroup barrier, the wavefronts of a workgroup share nothing.  Simulator source: the wavefront first regenerates the message the step
// will generate (sim_wave with the step's RNG index: the generator is counter based) from the instance's truth, which is read, not written.
// Record: every instance leaves its contribution (16 doubles); launch_record_reduce (record_kernel.h) joins them in a fixed order that
// depends on the batch size alone, entry kInnMaxNis by a maximum (kInnovRecMax).  Everything is read only, except the outputs.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "innovation_kernel.h"

namespace slam {
namespace {

static_assert(kInnovFrozen == SLAM_INNOVATION_INSTANCE_FROZEN && kInnovWouldFreeze == SLAM_INNOVATION_WOULD_FREEZE &&
              kInnovSingular == SLAM_INNOVATION_S_SINGULAR && kInnovTooLong == SLAM_INNOVATION_TOO_LONG, "innovation flags are slam_innovation_flags");
static_assert(kInnovStatusFrozen == SLAM_INST_INDEX_OOR, "the status bit the step kernel returns on");
static_assert(kInnovMaxDet == SLAM_INNOV_MAX_DET && kInnovMaxLm == SLAM_INNOV_MAX_LM, "the exported limits");
static_assert(kInnovRecLen == kRecLen, "the record launch_record_reduce takes");

constexpr int kInnovWaves = 4;                      // instances per workgroup of the instance kernel
static_assert(sizeof(InnovWork) * kInnovWaves <= 64 * 1024, "static LDS of a workgroup");

template <class ST>
__global__ __launch_bounds__(64 * kInnovWaves) void innovation_instance_kernel(const InnovParams p) {
    __shared__ InnovWork s_ws[kInnovWaves];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kInnovWaves + wave;
    if (b >= p.s.B) return;                          // (the whole wavefront; there is no workgroup barrier below)
    InnovWork& ws = s_ws[wave];
    const InnovWave w = {lane};
    const EkfStepParams& s = p.s;
    const AuxInstance<ST> inst(s, b);
    int k = 0;
    if (!(inst.status & kInnovStatusFrozen)) {       // (a frozen instance has no message: nothing is generated or staged, k = 0)
        if (s.sim) {
            double tx = s.truth[3 * (size_t)b], ty = s.truth[3 * (size_t)b + 1], tth = s.truth[3 * (size_t)b + 2];
            const int Lm = sim_map_size(s, b);
            const double* const map = sim_map(s, b);
            const double lmx0 = lane < Lm ? map[2 * lane] : 0.0, lmy0 = lane < Lm ? map[2 * lane + 1] : 0.0;
            k = sim_wave<kInnovMaxDet, false>(s, b, lane, inst.fwd, inst.ang, s.step, map, Lm, tx, ty, tth, lmx0, lmy0, ws.meas, sim_noise(s, b));
        } else {
            const AuxMessage msg(s, b);
            msg.stage(lane, ws.meas);
            k = msg.k;
        }
        w.sync();
    }
    double* const det = p.det ? p.det + (size_t)b * kInnovMaxDet * kInnovDetLen : nullptr;
    // (every index the loaders see is below 3 + 2 M: the block's landmarks come from ids[0 .. M))
    const InnovResult v = innovation_instance(w, ws, inst.load_x(), inst.load_P(), inst.ids, inst.M, s.L_max, inst.status, inst.fwd, inst.ang, k,
                                              inst.nz, s.lm_from_pred != 0, p.nis_lo, p.nis_hi, det);
    if (lane == 0) {
        if (p.post)
#pragma unroll
            for (int i = 0; i < 12; ++i) p.post[(size_t)b * 12 + i] = v.post[i];
        if (p.nis_sum) p.nis_sum[b] = v.nis_sum;
        if (p.n_upd) p.n_upd[b] = v.n_upd;
        if (p.n_new) p.n_new[b] = v.n_new;
        if (p.flags) p.flags[b] = v.flags;
        double r[kInnovRecLen];
        innovation_record(v, r);
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) p.inst_rec[(size_t)b * kInnovRecLen + i] = r[i];
    }
}

}  // namespace

hipError_t launch_innovation(const InnovParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    if (!aux_shape_ok(s.B, s.L_max, s.xstride, s.pstride, f32_storage) || !p.inst_rec || !p.partials || !p.rec) return hipErrorInvalidValue;
    if (s.sim ? (!s.truth || (!s.map && !s.map_each)) : (!s.meas_in || !s.meas_count_in || s.k_stride_in <= 0)) return hipErrorInvalidValue;
    const int groups = (s.B + kInnovWaves - 1) / kInnovWaves;
    const hipError_t e = aux_launch(f32_storage, innovation_instance_kernel<float>, innovation_instance_kernel<double>, dim3(groups),
                                    dim3(64 * kInnovWaves), 0, stream, p);
    if (e != hipSuccess) return e;
    return launch_record_reduce<kInnovRecMax>(p.inst_rec, s.B, p.partials, p.rec, stream);
}

}  // namespace slam
