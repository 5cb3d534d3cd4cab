// map_kernel.hip — map management of the EKF batch on the device (slam_remove_landmarks, slam_map_tally, slam_map_prune): the
// per-instance functions of map_kernel.h mapped to gfx950.  Nothing here computes a filter quantity: the compaction moves bits, the
// tally compares ids and runs the simulator's view test on estimates.
//
// map_compact_kernel: ONE WORKGROUP (256 threads) PER INSTANCE, the compaction IN PLACE in the canonical buffer (map_kernel.h gives the
//   argument: chunks of increasing destination offsets, all loads of a chunk, one workgroup barrier, its stores).  Against a pass
//   through the second buffer and back this halves the traffic.
//   decision   every thread reads M and its part of the mask row (or of the two counter rows, for a prune) and the workgroup votes; an
//              instance with nothing to remove leaves here: it has read M and M words (2 M for a prune) and touches no P.
//   kept list  wavefront 0 walks the slots 64 at a time; positions by ballot and popcount, the table (uint16) in LDS.
//   P          lanes run along the destination rows: consecutive lanes take consecutive new columns, whose old columns are consecutive
//              except across a removed pair.  Loads and stores are ELEMENT-granular (8 or 4 bytes per lane): a removed landmark shifts
//              the columns behind it by 16 bytes (fp64) or 8 bytes (fp32), so in fp32 a 16-byte group of the destination is in general
//              not a 16-byte group of the source, and in fp64 the shorter leading dimension changes the alignment of every other row.  A
//              wavefront's 64 element loads of one instruction still fall into 4 - 5 (fp64) or 2 - 3 (fp32) 128-byte lines of one row,
//              or of two rows at a row end, so every line is fetched once; kMapChunk = 8 loads per lane are in flight before the barrier.
// map_tally_kernel: a wavefront per instance, four per workgroup, lanes over slots, the message's ids in the wavefront's slice of LDS,
//   phases ordered by wavefront fences (assoc_kernel.hip's mapping).
// MapWorkTerms: the traffic model, summed in integers from the per-instance counts by launch_work_sum, outside any timed part.
// Record: launch_record_reduce (record_kernel.h) with the join mask kMapRecMax.
#include <hip/hip_runtime.h>

#include "../../include/slam_batch.h"
#include "aux_device.h"
#include "map_kernel.h"

namespace slam {
namespace {

static_assert(kMapRecLen == kRecLen, "the record launch_record_reduce takes");
static_assert(kMapStatusSkip == (SLAM_INST_NONFINITE | SLAM_INST_INDEX_OOR | SLAM_INST_WATCHDOG), "the instances the tally skips");
static_assert(kMapMaxLandmarks == kEkfMaxLandmarks, "the kept table holds every slot");

constexpr int kMapThreads = 256;                    // one instance's workgroup of the compaction
constexpr int kMapTallyWaves = 4;                   // instances per workgroup of the tally

// the 256 threads of one workgroup
struct MapGroup {
    __device__ __forceinline__ int lane() const { return (int)threadIdx.x; }
    __device__ __forceinline__ int width() const { return kMapThreads; }
    __device__ __forceinline__ void sync() const { __syncthreads(); }
};

// the 64 lanes of one wavefront
struct MapWave {
    int ln;
    __device__ __forceinline__ int lane() const { return ln; }
    __device__ __forceinline__ int width() const { return 64; }
    __device__ __forceinline__ void sync() const {
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
};

template <class T>
__global__ __launch_bounds__(kMapThreads) void map_compact_kernel(const MapCompactParams p) {
    __shared__ uint16_t s_kept[kMapMaxLandmarks];
    __shared__ int s_Mk;
    const int b = blockIdx.x;                        // (the grid is exactly B workgroups)
    const int tid = threadIdx.x;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    const size_t row = (size_t)b * p.L_max;
    const int32_t* const remove = p.remove ? p.remove + row : nullptr;
    int32_t* const seen = p.seen ? p.seen + row : nullptr;
    int32_t* const expected = p.expected ? p.expected + row : nullptr;
    auto drops = [&](int j) { return remove ? remove[j] != 0 : map_prune_decide(seen[j], expected[j], p.min_expected, p.min_ratio); };
    bool any = false;
    for (int j = tid; j < M; j += kMapThreads) any = any || drops(j);
    if (!__syncthreads_or(any)) {                    // nothing to remove: no P is touched
        if (tid == 0) {
            p.n_removed[b] = 0; p.m_before[b] = M;
            if (p.rec)
                for (int i = 0; i < kMapRecLen; ++i) p.inst_rec[(size_t)b * kMapRecLen + i] = 0.0;
        }
        return;
    }
    if (tid < 64) {                                  // the kept slots in their old order
        int Mk = 0;
        for (int j0 = 0; j0 < M; j0 += 64) {
            const int j = j0 + tid;
            const bool keep = j < M && !drops(j);
            const unsigned long long mask = __ballot(keep);
            if (keep) s_kept[Mk + __popcll(mask & ((1ull << tid) - 1ull))] = (uint16_t)j;
            Mk += __popcll(mask);
        }
        if (tid == 0) s_Mk = Mk;
    }
    __syncthreads();
    const int Mk = s_Mk;
    map_compact_instance(MapGroup(), aux_row<T>(p.P, b, p.pstride), aux_row<T>(p.x, b, p.xstride), p.ids + row, seen, expected, s_kept, M, Mk, p.L_max);
    if (tid == 0) {
        const int n2 = 3 + 2 * Mk;
        p.M[b] = Mk;
        p.n_removed[b] = M - Mk; p.m_before[b] = M;
        if (p.rec) {
            for (int i = 0; i < kMapRecLen; ++i) p.inst_rec[(size_t)b * kMapRecLen + i] = 0.0;
            p.inst_rec[(size_t)b * kMapRecLen + kMapTouched] = 1.0;
            p.inst_rec[(size_t)b * kMapRecLen + kMapRemoved] = (double)(M - Mk);
            p.inst_rec[(size_t)b * kMapRecLen + kMapMoved] = (double)n2 * (double)n2;
        }
    }
}

template <class ST>
__global__ __launch_bounds__(64 * kMapTallyWaves) void map_tally_kernel(const MapTallyParams p) {
    __shared__ int32_t s_id[kMapTallyWaves][kMapIdBlock];
    __shared__ uint8_t s_ok[kMapTallyWaves][kMapIdBlock];
    const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
    const int b = blockIdx.x * kMapTallyWaves + wave;
    if (b >= p.B) return;                            // (the whole wavefront; there is no workgroup barrier below)
    if (p.status[b] & kMapStatusSkip) return;
    if (p.assoc_flags && p.assoc_flags[b] != 0) return;
    const int M = aux_clamp_m(p.M[b], p.L_max);
    const int count = p.count[b];
    int k = count < p.k_stride ? count : p.k_stride;
    k = k < 0 ? 0 : k;
    const ST* __restrict__ const xb = aux_row<ST>(p.x, b, p.xstride);
    const size_t row = (size_t)b * p.L_max;
    // (every index load_x sees is below 3 + 2 M: only the lanes with j < M read a landmark)
    map_tally_instance(MapWave{lane}, [&](int i) { return (double)xb[i]; }, p.ids + row, M, p.meas + (size_t)b * p.k_stride * 3, k, s_id[wave],
                       s_ok[wave], p.r_lim, p.b_lo, p.b_hi, p.seen + row, p.expected + row);
}

// element i of the traffic model's sum: one instance of one call
struct MapWorkTerms {
    const int32_t *m_before, *n_removed;
    int L_max, esz, from_counters, counters;
    __device__ void operator()(size_t i, unsigned long long (&t)[3]) const {
        const MapTraffic w = map_traffic(m_before[i], n_removed[i], L_max, esz, from_counters != 0, counters != 0);
        t[0] = w.moved; t[1] = w.pads; t[2] = w.other_bytes;
    }
};

}  // namespace

hipError_t launch_map_compact(const MapCompactParams& p, int f32_storage, hipStream_t stream) {
    if (!aux_shape_ok(p.B, p.L_max, p.xstride, p.pstride, f32_storage) || p.L_max <= 0 || p.L_max > kMapMaxLandmarks || !p.P || !p.x || !p.M ||
        !p.ids || !p.n_removed || !p.m_before || (p.rec && (!p.inst_rec || !p.partials)))
        return hipErrorInvalidValue;
    if ((p.seen == nullptr) != (p.expected == nullptr) || (!p.remove && !p.seen)) return hipErrorInvalidValue;
    const hipError_t e = aux_launch(f32_storage, map_compact_kernel<uint32_t>, map_compact_kernel<uint64_t>, dim3(p.B), dim3(kMapThreads), 0, stream, p);
    if (e != hipSuccess || !p.rec) return e;
    return launch_record_reduce<kMapRecMax>(p.inst_rec, p.B, p.partials, p.rec, stream);
}

hipError_t launch_map_tally(const MapTallyParams& p, int f32_storage, hipStream_t stream) {
    if (p.B <= 0 || p.L_max <= 0 || !p.x || !p.M || !p.ids || !p.status || !p.meas || !p.count || p.k_stride <= 0 || !p.seen || !p.expected ||
        p.xstride < 3 + 2 * p.L_max)
        return hipErrorInvalidValue;
    const int groups = (p.B + kMapTallyWaves - 1) / kMapTallyWaves;
    return aux_launch(f32_storage, map_tally_kernel<float>, map_tally_kernel<double>, dim3(groups), dim3(64 * kMapTallyWaves), 0, stream, p);
}

hipError_t launch_map_work(const int32_t* m_before, const int32_t* n_removed, size_t n, int L_max, int esz, int from_counters, int counters,
                           unsigned long long* work, hipStream_t stream) {
    if (!m_before || !n_removed) return hipErrorInvalidValue;
    return launch_work_sum<3>(MapWorkTerms{m_before, n_removed, L_max, esz, from_counters, counters}, n, work, stream);
}

}  // namespace slam
