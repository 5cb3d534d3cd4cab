// joint_kernel.hip — joint-compatibility association (JCBB) of the detections of an id-less message with the landmarks of every instance
// of a batch (slam_associate_joint, slam_step_associated_joint, slam_associate_joint_run).  The definition is joint_instance()
// (joint_kernel.h); this file maps it to the device.
//
// Mapping: ONE WAVEFRONT PER INSTANCE, kJointWaves instances per workgroup, as assoc_instance_kernel; everything an instance holds between
// its phases (JointWork, 24 KB: the message, the candidate lists, H and S of at most 64 candidate landmarks, the packed Cholesky factor
// of 32 x 32 and y, the stack of the search) in the wavefront's slice of LDS, phases ordered by wavefront fences, no workgroup barrier, no
// atomics on values.  Two instances per workgroup take 48 KB of the CU's 160 KB: three workgroups, six wavefronts per CU; the search is
// a chain of dependent LDS round trips, so more wavefronts per SIMD would be welcome and registers are not what limits them.
//   costs      as assoc_instance_kernel (lanes over landmark slots); a lane whose pair passes the individual gate inserts it into the
//              detection's sorted list, the lanes of one detection one after the other in ascending slot (a ballot walk)
//   table      one lane per candidate landmark recomputes H and S with the cost phase's function
//   a node     lanes over the pairings on the stack (at most 15) form the 2 x 2 cross blocks, each from 25 elements of P read on demand
//              through L2 (the cost phase has just pulled the pose rows and columns in); then the two new rows against the factor,
//              right-looking: lane (row, column) holds one element and subtracts in ascending column order, what the sequential policy
//              does too; the corner, y and the distance are summed by every lane alike from LDS broadcasts
//   the search its control state (level, pairs, used set, best) is computed alike in every lane and kept scalar by readfirstlane
// Record (join mask kJointRecMax) and traffic model: as assoc_kernel.hip.  All arithmetic is fp64, unfused.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "joint_kernel.h"

namespace slam {
namespace {

static_assert(kAssocJointUnpaired == SLAM_ASSOC_JOINT_UNPAIRED && kJointMaxCand == SLAM_JOINT_MAX_CAND && kJointMaxPair == SLAM_JOINT_MAX_PAIR &&
              kJointBudget == SLAM_JOINT_BUDGET && kJointSingular == SLAM_JOINT_S_SINGULAR && kJointLmTable == SLAM_JOINT_LM_TABLE,
              "the constants of slam_batch.h");

static_assert(kInnovRecLen == kRecLen, "the record launch_record_reduce takes");

constexpr int kJointWaves = 2;                      // instances per workgroup
static_assert(sizeof(JointWork) * kJointWaves <= 64 * 1024, "static LDS of a workgroup");

template <class ST>
__global__ __launch_bounds__(64 * kJointWaves) void joint_instance_kernel(const JointParams p) {
    __shared__ JointWork s_ws[kJointWaves];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kJointWaves + wave;
    const EkfStepParams& s = p.s;
    if (b >= s.B) return;                            // (the whole wavefront; there is no workgroup barrier below)
    JointWork& ws = s_ws[wave];
    JointWave w;
    w.ln = lane;
    const AuxInstance<ST> inst(s, b);
    const AuxMessage msg(s, b);
    msg.stage(lane, ws.a.meas);
    {   // gate_joint into LDS (constant indices: the kernel arguments stay in scalar registers)
        double g = 0.0;
#pragma unroll
        for (int i = 0; i < kJointMaxPair; ++i) g = lane == i ? p.gate_joint[i] : g;
        if (lane < kJointMaxPair) ws.gj[lane] = g;
    }
    w.sync();
    const int M = inst.M;
    const size_t bd = (size_t)b * kInnovMaxDet;
    // (every index the loaders see is below 3 + 2 M: a landmark of the cost phase is j < M or landmark 0 while M > 0, and the table
    // and the pairings hold slots the cost phase found, j < M)
    const JointResult v = joint_instance(
        w, ws, inst.load_x(), inst.load_P(), inst.ids, M, s.L_max, inst.status, inst.fwd, inst.ang, msg.k, inst.nz, p.gate_match, p.gate_new,
        ws.gj, p.max_nodes, nullptr, p.verdict ? p.verdict + bd : nullptr, p.slot ? p.slot + bd : nullptr,
        p.det ? p.det + bd * kAssocDetLen : nullptr, p.ncand ? p.ncand + bd : nullptr, p.meas_out + (size_t)b * s.k_stride_in * 3);
    if (lane == 0) {
        p.count_out[b] = v.count_out;
        if (p.n_match) p.n_match[b] = v.n_match;
        if (p.n_new) p.n_new[b] = v.n_new;
        if (p.n_drop) p.n_drop[b] = v.n_drop;
        if (p.flags) p.flags[b] = v.flags;
        if (p.nodes) p.nodes[b] = v.nodes;
        if (p.d2_joint) p.d2_joint[b] = v.d2_joint;
        double r[kInnovRecLen];
        joint_record(v, r);
#pragma unroll
        for (int i = 0; i < kInnovRecLen; ++i) p.inst_rec[(size_t)b * kInnovRecLen + i] = r[i];
        if (p.n_lm) p.n_lm[b] = (v.flags & (kInnovFrozen | kInnovTooLong)) ? -1 : M;     // (what the traffic model needs besides the counts)
        if (p.n_blk) p.n_blk[b] = v.blocks;
    }
}

// element i of the traffic model's sum: assoc_kernel.hip's terms plus, per on-demand 2 x 2 block of P, four elements and one 128-byte line
struct JointWorkTerms {
    const int32_t *n_lm, *n_match, *n_new, *n_drop, *n_blk;
    int esz;
    __device__ void operator()(size_t i, unsigned long long (&t)[3]) const {
        const bool some = n_lm[i] >= 0;              // (else: an instance that emits an empty message: the counts)
        const AssocTraffic w = some ? assoc_traffic(n_lm[i], n_match[i] + n_new[i] + n_drop[i], esz) : AssocTraffic{0ull, 8ull, 0ull};
        const unsigned long long blk = some ? (unsigned long long)n_blk[i] : 0ull;
        t[0] = w.p_elems + 4ull * blk; t[1] = w.other_bytes; t[2] = w.p_lines + blk;
    }
};

}  // namespace

hipError_t launch_associate_joint_work(const int32_t* n_lm, const int32_t* n_match, const int32_t* n_new, const int32_t* n_drop, const int32_t* n_blk,
                                       size_t n, int esz, unsigned long long* work, hipStream_t stream) {
    if (!n_lm || !n_match || !n_new || !n_drop || !n_blk) return hipErrorInvalidValue;
    return launch_work_sum<3>(JointWorkTerms{n_lm, n_match, n_new, n_drop, n_blk, esz}, n, work, stream);
}

hipError_t launch_associate_joint(const JointParams& p, int f32_storage, hipStream_t stream) {
    const EkfStepParams& s = p.s;
    if (!aux_shape_ok(s.B, s.L_max, s.xstride, s.pstride, f32_storage) || !p.inst_rec || !p.partials || !p.rec) return hipErrorInvalidValue;
    if (s.sim || !s.meas_in || !s.meas_count_in || s.k_stride_in <= 0 || !p.meas_out || !p.count_out || !(p.gate_match > 0.0) ||
        !(p.gate_match <= p.gate_new) || p.max_nodes < 1 || p.max_nodes > kJointMaxNodes)
        return hipErrorInvalidValue;
    const int groups = (s.B + kJointWaves - 1) / kJointWaves;
    const hipError_t e = aux_launch(f32_storage, joint_instance_kernel<float>, joint_instance_kernel<double>, dim3(groups), dim3(64 * kJointWaves), 0,
                                    stream, p);
    if (e != hipSuccess) return e;
    return launch_record_reduce<kJointRecMax>(p.inst_rec, s.B, p.partials, p.rec, stream);
}

}  // namespace slam
