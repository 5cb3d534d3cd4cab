// capi_map.h — the pieces of capi_map.cpp that landmark merging (capi_merge.cpp) checks its arguments, enters the handle and launches
// its tally and its compaction with, and the managed tick its run composes.  Internal.
#pragma once
#include "capi_assoc.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int map_config(const slam_map_config* cfg, slam_map_config* out);
// the handle, once the arguments are in order; the queued timesteps run first
int map_enter(slam_handle* h, const char* who);
// the track counters exist (zero when they are new)
int map_track(slam_handle* h);
// the rows of map.dint, [kMapRows][ticks][B]
enum MapRow { kMapRemoved = 0, kMapMBefore = 1, kMapRows = 2 };
// the rows of `ticks` removals, the record, the sums of the traffic model, the per-instance contributions
int map_reserve(slam_handle* h, size_t ticks);
int map_zero_work(slam_handle* h);
// one removal on the handle's stream: by the mask d_remove, or (NULL) by the prune rule of c on the counters
int map_compact_launch(slam_handle* h, const int32_t* d_remove, const slam_map_config& c, int32_t* d_n_removed, int32_t* d_m_before, bool with_rec);
int map_sum_work(slam_handle* h, const int32_t* d_n_removed, const int32_t* d_m_before, bool from_counters);
// the tally of one message that is on the device, on the handle's stream
int tally_now(slam_handle* h, const slam_map_config& c, const float* d_meas, const int32_t* d_count, int k_stride, const int32_t* d_flags);

// slam_manage_run as run_filtered's feature: the association's tick, after the step the tally and, every prune_every ticks, the prune,
// which is the marked group.  slam_manage_merge_run puts its merge between the two and marks that.
struct ManageTicks {
    AssocTicks a; const slam_map_config& mc; int32_t* n_removed;
    int k_stride = 0;

    RunTimes& times() const { return a.h->map.times; }
    double bytes_per_tick() const { return a.bytes_per_tick() + kMapRows * 4.0 * (double)a.h->B; }
    int reserve(int ks, int chunk) {
        k_stride = ks;
        TRY(a.reserve(ks, chunk));
        TRY(map_reserve(a.h, (size_t)chunk));
        TRY(map_track(a.h));
        return map_zero_work(a.h);
    }
    int chunk_begin() {   // (n_removed of the ticks without a prune)
        HIP_TRY(hipMemsetAsync(a.h->map.dint, 0, sizeof(int32_t) * kMapRows * a.cb, a.h->stream));
        return SLAM_OK;
    }
    DevMsg out() const { return a.out(); }
    template <class Mark>
    int filter(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int ks, Mark) {
        return a.launch(t, cmd, d_each, dm, dc, ks);
    }
    int32_t* at(MapRow r, int t) const { return row(a.h->map.dint, r, a.cb, (size_t)t * a.B); }
    bool prunes_after(int t_run) const { return (t_run + 1) % mc.prune_every == 0; }
    int tally(int t) { return tally_now(a.h, mc, out().meas, out().count, k_stride, a.at(kAssocFlags, t)); }
    int prune(int t_run, int t) {
        return prunes_after(t_run) ? map_compact_launch(a.h, nullptr, mc, at(kMapRemoved, t), at(kMapMBefore, t), false) : SLAM_OK;
    }
    template <class Mark>
    int after_step(int t_run, int t, Mark mark) {
        TRY(tally(t));
        // (the marked group of a tick without a prune is empty: its event pair brackets nothing)
        return mark([&]() -> int { return prune(t_run, t); });
    }
    int sum_work(int t_run, int t) { return prunes_after(t_run) ? map_sum_work(a.h, at(kMapRemoved, t), at(kMapMBefore, t), true) : SLAM_OK; }
    int chunk_done(int t0, int tc) {
        for (int t = 0; t < tc; ++t) TRY(sum_work(t0 + t, t));
        return SLAM_OK;
    }
    std::vector<TickRow> rows() const {
        std::vector<TickRow> r = a.rows();
        r.push_back({at(kMapRemoved, 0), n_removed, a.B});
        return r;
    }
    int finish() {
        HIP_TRY(hipStreamSynchronize(a.h->stream));
        return SLAM_OK;
    }
};

}  // namespace slam_capi
#pragma GCC visibility pop
