// map_kernel.h — map management of the EKF batch (slam_remove_landmarks, slam_map_tally, slam_map_prune, slam_step_managed,
// slam_manage_run; gfx950): landmarks leave the map again.  Since slam_associate every detection farther than gate_new from the map
// becomes a landmark; with clutter the state only grows.  Three per-instance functions are defined here, ONCE, for the device kernels
// (map_kernel.hip) and the host test hook (slam_map_instance_host), both compiled with -ffp-contract=off; the arithmetic of the view
// test is the functions of slam_math.h in the order of sim_device.h:84-87.  The step, gate, innovation and association kernels are
// untouched: a removal leaves an ordinary state of fewer landmarks behind.
//
// Removal (map_compact_instance).  In covariance form, dropping a landmark is exact marginalisation: its two entries of x and its two
// rows and columns of P disappear and nothing else changes.  With the kept slots k0 < k1 < ... in their old order, x', ids' and P' are
// the sub-vector and sub-matrix on the state indices {0, 1, 2} u {3 + 2 k, 4 + 2 k}, P' stored at the leading dimension
// ekf_ld(3 + 2 M') of the smaller state, its pad columns zero (the invariant of ekf_kernel.h), M' = M - removed,
// ids[M' .. L_max) and the track counters of those slots zero.  Pure data movement: elements are moved as integers of their size, so
// NaNs keep their payloads.  Status flags, timestep, truth and err_sum are not touched and the status is not consulted; the slab beyond
// n' * ld' elements keeps whatever it held.
//
// Why the compaction of P may run IN PLACE.  Number the elements of the new matrix i' = r' ld' + c' (row-major, pads included) and let
// s(i') = R(r') ld + R(c') be the old offset of the same element, R the increasing map from new to old state indices.
// R(k) >= k and ld >= ld', so s(i') >= i' (*): an element never moves to a higher offset.  Take the destinations in chunks [a, b) of
// increasing offsets, each chunk LOADING all its sources, passing a workgroup barrier and then STORING.  A store of this chunk lands at an offset < b.  The sources of every later chunk lie at s(i'') >= i'' >= b by (*), so no store
// of this chunk can reach them; the sources of this chunk are all in registers when the barrier is passed; the sources of earlier
// chunks were consumed before their own barriers.  Hence one barrier per chunk, between its loads and its stores, is sufficient, and a
// lane may start loading the next chunk while others still store this one: those loads read offsets >= b that no store of this chunk
// writes.  x, ids and the counters move the same way (one row each).
//
// Track evidence (map_tally_instance), after the step that consumed a labelled message: for every slot j < M of the post-step state
//   seen_now = some triplet l < count has (int32)id == ids[j]   (an id column that is NaN or outside int32 matches nothing)
//   in_view  = !(r > range_max * range_shrink) && beta > fov_min + fov_margin && beta < fov_max - fov_margin
// with r, beta of the ESTIMATED landmark from the ESTIMATED pose (the stored x, widened for fp32 storage), as the simulator computes
// them for the true ones; seen[j] += seen_now, expected[j] += seen_now || in_view.  Skipped whole for an instance that is frozen
// (SLAM_INST_INDEX_OOR), failed (NONFINITE, WATCHDOG) or whose association flag is not 0 (it was given an empty message).
// Prune rule (map_prune_decide): slot j goes iff expected[j] >= min_expected && (double)seen[j] < min_ratio * (double)expected[j].
#pragma once
#include <stdint.h>

#include "slam_math.h"

namespace slam {

constexpr int kMapRecLen = 16;                      // doubles of one record
enum MapRec { kMapTouched = 0, kMapRemoved = 1, kMapMoved = 2 };   // instances touched, landmarks removed, elements of P moved; the rest 0
constexpr unsigned kMapRecMax = 1u << 8;             // the entries joined by a maximum (record_kernel.h): entry 8, unused and 0, as it always was
constexpr int32_t kMapStatusSkip = 1 | 4 | 32;      // SLAM_INST_NONFINITE | SLAM_INST_INDEX_OOR | SLAM_INST_WATCHDOG: no tally
constexpr int kMapMaxLandmarks = 1000;              // kEkfMaxLandmarks: what the index table of a workgroup holds
constexpr int kMapChunk = 8;                        // elements a lane holds between the loads and the stores of a chunk (16 floats
                                                    // measured slower than 8: 1.53 against 1.41 ms at L = 50 x 65 536)
constexpr int kMapIdBlock = 64;                     // ids of the message held at once by the tally

// ekf_ld (slam_math.h) under the name the stand-alone host programs of the map, merge and fix tests call it by
SLAM_HD constexpr int map_ld(int n, int elem_bytes) { return ekf_ld(n, elem_bytes); }

// the view test of one estimated landmark from the estimated pose: sim_device.h:84-87 on estimates, with shrunk limits
SLAM_HD bool map_in_view(double px, double py, double pth, double lx, double ly, double r_lim, double b_lo, double b_hi) {
    const double dx = lx - px, dy = ly - py;
    const double r = sqrt(dx * dx + dy * dy);
    const double gb = det_atan2(dy, dx);
    const double beta = rem2pi(gb - pth);
    return !(r > r_lim) && (beta > b_lo && beta < b_hi);
}

// (int32)id of a message's id column as the step reads it, where that is defined; *ok = false otherwise
SLAM_HD int32_t map_message_id(float f, bool* ok) {
    *ok = f >= -2147483648.0f && f < 2147483648.0f;   // (NaN fails both; -2^31 converts exactly)
    return *ok ? (int32_t)f : 0;
}

SLAM_HD bool map_prune_decide(int32_t seen, int32_t expected, int32_t min_expected, double min_ratio) {
    return expected >= min_expected && (double)seen < min_ratio * (double)expected;
}

// The host's execution policy: one lane.  The device's are MapWave (tally) and MapGroup (compaction) in map_kernel.hip.
struct MapSeq {
    int lane() const { return 0; }
    int width() const { return 1; }
    void sync() const {}
};

// One instance's tally.  load_x(i): the stored x widened; ids [M], seen / expected [>= M]; meas: the labelled message, k = its clamped
// count (any length: it is walked in blocks of kMapIdBlock ids through idbuf, LDS on the device).  M is clamped by the caller.
template <class W, class LX>
SLAM_HD void map_tally_instance(const W& w, LX load_x, const int32_t* ids, int M, const float* meas, int k, int32_t* idbuf, uint8_t* okbuf,
                                double r_lim, double b_lo, double b_hi, int32_t* seen, int32_t* expected) {
    const double px = load_x(0), py = load_x(1), pth = load_x(2);
    for (int j0 = 0; j0 < M; j0 += w.width()) {     // (uniform trip count: every lane reaches every sync)
        const int j = j0 + w.lane();
        const bool mine = j < M;
        const int32_t id = mine ? ids[j] : 0;
        bool seen_now = false;
        for (int l0 = 0; l0 < k; l0 += kMapIdBlock) {
            const int kb = k - l0 < kMapIdBlock ? k - l0 : kMapIdBlock;
            w.sync();                                // (the block before this one has been read by every lane)
            for (int l = w.lane(); l < kb; l += w.width()) {
                bool ok;
                idbuf[l] = map_message_id(meas[3 * (size_t)(l0 + l)], &ok);
                okbuf[l] = ok ? 1 : 0;
            }
            w.sync();
            for (int l = 0; l < kb; ++l) seen_now = seen_now || (okbuf[l] && idbuf[l] == id);   // (every lane the same l: broadcasts)
        }
        if (mine) {
            const bool in_view = map_in_view(px, py, pth, load_x(3 + 2 * j), load_x(4 + 2 * j), r_lim, b_lo, b_hi);
            seen[j] += seen_now ? 1 : 0;
            expected[j] += (seen_now || in_view) ? 1 : 0;
        }
    }
}

// A row of `total` destination elements gathered from src_of(i) in chunks: all loads of a chunk, the barrier, its stores (see the
// argument at the top; dst may be the source array).  src_of(i) < 0: the destination is written as zero.
template <class W, class T, class F>
SLAM_HD void map_gather_chunks(const W& w, T* dst, const T* src, int total, F src_of) {
    constexpr int U = kMapChunk;
    const int step = w.width() * U;
    for (int base = 0; base < total; base += step) {
        T v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * w.width() + w.lane();
            int s = -1;
            if (i < total) s = src_of(i);
            v[u] = s >= 0 ? src[s] : (T)0;
        }
        w.sync();
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int i = base + u * w.width() + w.lane();
            if (i < total) dst[i] = v[u];
        }
    }
}

// One instance's compaction once the kept slots are known: kept[0 .. Mk) ascending (LDS on the device), M the old count.  T: an
// unsigned integer of the element size.  seen / expected may be NULL.  Every lane of the policy calls it; the lanes share the work.
template <class W, class T>
SLAM_HD void map_compact_instance(const W& w, T* P, T* x, int32_t* ids, int32_t* seen, int32_t* expected, const uint16_t* kept, int M, int Mk,
                                  int L_max) {
    const int n = 3 + 2 * M, n2 = 3 + 2 * Mk;
    const int ld = ekf_ld(n, (int)sizeof(T)), ld2 = ekf_ld(n2, (int)sizeof(T));
    auto old_index = [&](int k) { return k < 3 ? k : 3 + 2 * (int)kept[(k - 3) >> 1] + ((k - 3) & 1); };   // R
    map_gather_chunks(w, P, P, n2 * ld2, [&](int i) -> int {
        const int r = i / ld2, c = i - r * ld2;
        return c < n2 ? old_index(r) * ld + old_index(c) : -1;                                 // (a pad column: zero)
    });
    map_gather_chunks(w, x, x, n2, [&](int i) -> int { return old_index(i); });
    auto slot_of = [&](int j) -> int { return j < Mk ? (int)kept[j] : -1; };                                  // (the tail up to L_max: zero)
    map_gather_chunks(w, ids, ids, L_max, slot_of);
    if (seen) map_gather_chunks(w, seen, seen, L_max, slot_of);
    if (expected) map_gather_chunks(w, expected, expected, L_max, slot_of);
}

// The traffic model of one instance of a removal (slam_last_map_work): elements of P moved (read and written once each), elements of
// P written as pads, and the bytes of everything else: M and the mask row (or the two counter rows of a prune) read by every
// instance; for a touched one x read and written, ids and - with counters - their rows read for the kept slots and written to L_max,
// M and n_removed written.
struct MapTraffic { unsigned long long moved, pads, other_bytes; };
SLAM_HD MapTraffic map_traffic(int M, int removed, int L_max, int esz, bool from_counters, bool counters) {
    const unsigned long long m = (unsigned long long)M, e = (unsigned long long)esz;
    MapTraffic t = {0ull, 0ull, 4ull + (from_counters ? 8ull : 4ull) * m + 4ull};   // M, the decision's inputs, n_removed
    if (removed <= 0) return t;
    const unsigned long long mk = m - (unsigned long long)removed, n2 = 3ull + 2ull * mk;
    const unsigned long long ld2 = (unsigned long long)ekf_ld((int)n2, esz);
    t.moved = n2 * n2;
    t.pads = n2 * (ld2 - n2);
    t.other_bytes += 2ull * n2 * e + (counters ? 3ull : 1ull) * 4ull * (mk + (unsigned long long)L_max) + 4ull;
    return t;
}

// One instance on the host (slam_map_instance_host): the kept list from a mask as the kernel forms it, then the compaction.
// remove [>= M] (nonzero: drop).  Returns M'.
template <class T>
int map_remove_instance_host(T* P, T* x, int32_t* ids, int32_t* seen, int32_t* expected, const int32_t* remove, int M, int L_max,
                             uint16_t* kept) {
    int Mk = 0;
    for (int j = 0; j < M; ++j)
        if (!remove[j]) kept[Mk++] = (uint16_t)j;
    if (Mk < M) map_compact_instance(MapSeq(), P, x, ids, seen, expected, kept, M, Mk, L_max);
    return Mk;
}

#if defined(__HIPCC__)
// One removal of every instance on `stream`: the compaction launch, then - when rec is wanted - the record as
// launch_record_reduce sums it (two more launches).
struct MapCompactParams {
    void* P; void* x;                 // [B][pstride], [B][xstride] in elements of the storage type; compacted in place
    int32_t *M, *ids;                 // [B], [B][L_max]
    int32_t *seen, *expected;         // [B][L_max] or both NULL
    const int32_t* remove;            // [B][L_max] mask, or NULL: the prune rule on seen / expected
    int32_t min_expected; double min_ratio;
    int32_t *n_removed, *m_before;    // [B] each: what the instance dropped and the M it had (the traffic model reads both)
    double* inst_rec;                 // [B][kMapRecLen]
    double* partials;                 // [record_blocks(B)][kMapRecLen]
    double* rec;                      // [kMapRecLen], or NULL: no record, and inst_rec / partials are not used
    int32_t B, L_max, pstride, xstride;
};
hipError_t launch_map_compact(const MapCompactParams& p, int f32_storage, hipStream_t stream);

struct MapTallyParams {
    const void* x; const int32_t *M, *ids, *status;
    const float* meas; const int32_t* count; int32_t k_stride;
    const int32_t* assoc_flags;       // [B] or NULL
    int32_t *seen, *expected;         // [B][L_max]
    double r_lim, b_lo, b_hi;         // range_max * range_shrink, fov_min + fov_margin, fov_max - fov_margin
    int32_t B, L_max, xstride;
};
hipError_t launch_map_tally(const MapTallyParams& p, int f32_storage, hipStream_t stream);

// work [3] += the sums of map_traffic over n instances (m_before, n_removed as launch_map_compact wrote them)
hipError_t launch_map_work(const int32_t* m_before, const int32_t* n_removed, size_t n, int L_max, int esz, int from_counters, int counters,
                           unsigned long long* work, hipStream_t stream);
#endif

}  // namespace slam
