// score_kernel.hip — the estimated map of every EKF instance matched to its true map by position (slam_map_score): score_instance() of
// score_kernel.h mapped to the device.
//
// Mapping: ONE WAVEFRONT PER INSTANCE on the front end of aux_device.h (aux_clamp_m, aux_row, aux_launch), kScoreWaves(L_max) instances
// per workgroup, phases ordered by wavefront fences, no workgroup barrier.  A lane owns the slots j = lane + 64 k: it walks the true rows
// for each of them (every lane reads the same map row at the same time: one broadcast load per row, the map of an instance stays in L1 /
// L2), writes the slot's claim (row, d2) into the wavefront's slice of LDS, and after the fence compares it with the claims of all slots
// (LDS broadcast reads) - the claims per true row are resolved in LDS, with no table over the true map, whose size the handle's capacity
// does not bound.  Lane 0 then sums up from LDS in slot order (the order of the definition: one addition per slot), and writes the
// compacted list of MATCHED slots the factorisation of nees_matched selects its rows by (consistency_kernel.hip).
// LDS: 24 bytes per slot of the capacity (row, role, d2, lm_nees); four instances per workgroup up to L_max = 640, fewer beyond, so that
// a workgroup stays below 60 KiB.  The kernel reads x, the map and the 2 x 2 diagonal blocks of P only - O(M Lb) arithmetic on O(M + Lb)
// bytes - so it is bound by the fp64 compare-and-select chain of the scan, not by memory; the traffic model (score_traffic) says what it
// reads.
// Record: the per-instance contributions go through launch_record_reduce (record_kernel.h), join mask kScoreRecMax: a fixed order that
// depends on the batch size alone, no atomics on values.  All arithmetic is fp64, unfused.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "score_kernel.h"

namespace slam {
namespace {

static_assert(kScoreRecLen == kRecLen, "the record launch_record_reduce takes");
static_assert((int)kScoreNone == (int)SLAM_SCORE_NONE && (int)kScoreMatched == (int)SLAM_SCORE_MATCHED &&
              (int)kScoreDuplicate == (int)SLAM_SCORE_DUPLICATE && (int)kScoreSpurious == (int)SLAM_SCORE_SPURIOUS, "roles are slam_score_role");
static_assert(kScoreMatchedNotPd == SLAM_SCORE_MATCHED_NOT_PD && kScoreLmNotPd == SLAM_SCORE_LM_NOT_PD && kScoreFailed == SLAM_SCORE_INSTANCE_FAILED,
              "flags are slam_score_flags");
static_assert(kScoreStatusFailed == (SLAM_INST_NONFINITE | SLAM_INST_WATCHDOG), "the status bits of a failed instance");
static_assert(kScoreMatchedNotPd == SLAM_CONSISTENCY_FULL_NOT_PD && kScoreFailed == SLAM_CONSISTENCY_INSTANCE_FAILED, "the factorisation's bits");

constexpr int kScoreSlotBytes = 24;                 // LDS per slot of the capacity: row, role (int32), d2, lm_nees (double)
constexpr int kScoreLdsBytes = 60 * 1024;           // of one workgroup at most

// instances (wavefronts) per workgroup
int score_waves(int L_max) {
    const int fit = kScoreLdsBytes / (kScoreSlotBytes * (L_max > 0 ? L_max : 1));
    return fit >= 4 ? 4 : (fit >= 1 ? fit : 1);
}

// the 64 lanes of one wavefront
struct ScoreWave {
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int width() const { return 64; }
    // LDS written by some lanes is read by others of the same wavefront afterwards
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    __device__ __forceinline__ bool any(bool b) const { return __ballot(b) != 0ull; }   // (called in wave-uniform control flow)
};

template <class ST>
__global__ __launch_bounds__(256) void score_instance_kernel(const ScoreParams p, const int waves, const int cap) {
    extern __shared__ double s_dyn[];                // per wavefront: d2 [cap], lm_nees [cap], row [cap], role [cap]
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * waves + wave;
    if (b >= p.B) return;                            // (the whole wavefront; there is no workgroup barrier below)
    double* const ws_d2 = s_dyn + (size_t)wave * 3 * cap;
    double* const ws_nees = ws_d2 + cap;
    int32_t* const ws_row = reinterpret_cast<int32_t*>(ws_nees + cap);
    int32_t* const ws_role = ws_row + cap;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    const int ld = ekf_ld(3 + 2 * M, (int)sizeof(ST));
    const ST* __restrict__ const xb = aux_row<ST>(p.x, b, p.xstride);
    const ST* __restrict__ const Pb = aux_row<ST>(p.P, b, p.pstride);
    const double* const map = p.map_each ? p.map_each + (size_t)b * p.map_stride * 2 : p.map;
    int Lb = p.map_each ? p.L_each[b] : p.L;
    if (p.map_each && Lb > p.map_stride) Lb = p.map_stride;
    Lb = Lb < 0 ? 0 : Lb;
    const size_t row0 = (size_t)b * p.L_max;
    // (every index the loaders see is below 3 + 2 M: the pose and the slots j < M)
    const ScoreResult v = score_instance(ScoreWave{lane}, [xb](int i) { return (double)xb[i]; },
                                         [Pb, ld](int r, int c) { return (double)Pb[(size_t)r * ld + c]; }, M, p.L_max, p.status[b],
                                         p.truth + (size_t)b * 3, map, Lb, p.r2, p.lm_lo, p.lm_hi, ws_row, ws_role, ws_d2, ws_nees, p.row + row0,
                                         p.role + row0, p.lm_err + row0, p.lm_nees + row0, p.sel + row0, p.sel_row + row0);
    if (lane != 0) return;
    p.n_matched[b] = v.n_matched; p.n_duplicate[b] = v.n_duplicate; p.n_spurious[b] = v.n_spurious; p.flags[b] = v.flags;
    p.map_rms[b] = v.map_rms; p.max_err[b] = v.max_err;
    p.nees_matched[b] = __builtin_nan(""); p.dof_matched[b] = 0;   // (what full = 0 reports; the factorisation overwrites both)
    p.n_with_row[b] = v.n_matched + v.n_duplicate;
    double r[kScoreRecLen];
    score_record(v, r);
#pragma unroll
    for (int i = 0; i < kScoreRecLen; ++i) p.inst_rec[(size_t)b * kScoreRecLen + i] = r[i];
}

// element i of the traffic model's sum: one instance
struct ScoreWorkTerms {
    const int32_t *M, *L_each, *n_with_row, *n_matched, *flags;
    int L, map_stride, L_max, full;
    __device__ void operator()(size_t i, unsigned long long (&t)[2]) const {
        int Lb = L_each ? L_each[i] : L;
        if (L_each && Lb > map_stride) Lb = map_stride;
        const ScoreTraffic w = score_traffic(aux_clamp_m(M[i], L_max), Lb, L_max, n_with_row[i], n_matched[i], (flags[i] & kScoreFailed) != 0, full != 0);
        t[0] = w.elems; t[1] = w.other_bytes;
    }
};

bool score_params_ok(const ScoreParams& p, int f32_storage) {
    return aux_shape_ok(p.B, p.L_max, p.xstride, p.pstride, f32_storage) && p.L_max <= kEkfMaxLandmarks && p.P && p.x && p.M && p.status && p.truth &&
           (p.map_each ? (p.L_each != nullptr && p.map_stride > 0) : (p.map != nullptr && p.L > 0)) && p.n_matched && p.n_duplicate && p.n_spurious &&
           p.flags && p.map_rms && p.max_err && p.nees_matched && p.dof_matched && p.row && p.role && p.lm_err && p.lm_nees && p.sel && p.sel_row &&
           p.n_with_row && p.inst_rec;   // (the config is the caller's to check: r2 may have underflowed to 0, which matches d2 == 0 only)
}

}  // namespace

hipError_t launch_score(const ScoreParams& p, int f32_storage, hipStream_t stream) {
    if (!score_params_ok(p, f32_storage)) return hipErrorInvalidValue;
    const int waves = score_waves(p.L_max), cap = p.L_max > 0 ? p.L_max : 1;
    const size_t lds = (size_t)waves * kScoreSlotBytes * cap;   // (<= 60 KiB: at L_max = 1000 two instances of 24 000 bytes)
    const int groups = (p.B + waves - 1) / waves;
    return aux_launch(f32_storage, score_instance_kernel<float>, score_instance_kernel<double>, dim3(groups), dim3(64 * waves), lds, stream, p, waves,
                      cap);
}

hipError_t launch_score_record(const double* inst_rec, int B, double* partials, double* rec, hipStream_t stream) {
    (void)hipGetLastError();   // sticky and per thread: only these launches' errors are reported
    return launch_record_reduce<kScoreRecMax>(inst_rec, B, partials, rec, stream);
}

hipError_t launch_score_work(const ScoreParams& p, int full, unsigned long long* work, hipStream_t stream) {
    if (!p.M || !p.n_with_row || !p.n_matched || !p.flags) return hipErrorInvalidValue;
    return launch_work_sum<2>(ScoreWorkTerms{p.M, p.map_each ? p.L_each : nullptr, p.n_with_row, p.n_matched, p.flags, p.L, p.map_stride, p.L_max, full},
                              (size_t)p.B, work, stream);
}

}  // namespace slam
