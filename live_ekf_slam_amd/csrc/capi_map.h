// capi_map.h — the pieces of capi_map.cpp that landmark merging (capi_merge.cpp) checks its arguments, enters the handle and launches
// its tally and its compaction with.  Internal.
#pragma once
#include "slam_handle.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int map_config(const slam_map_config* cfg, slam_map_config* out);
// the handle, once the arguments are in order; the queued timesteps run first
int map_enter(slam_handle* h, const char* who);
// the track counters exist (zero when they are new)
int map_track(slam_handle* h);
// n_removed and the M before of `ticks` removals ([2][ticks][B]), the record, the sums of the traffic model, the per-instance contributions
int map_reserve(slam_handle* h, size_t ticks);
int map_zero_work(slam_handle* h);
// one removal on the handle's stream: by the mask d_remove, or (NULL) by the prune rule of c on the counters
int map_compact_launch(slam_handle* h, const int32_t* d_remove, const slam_map_config& c, int32_t* d_n_removed, int32_t* d_m_before, bool with_rec);
int map_sum_work(slam_handle* h, const int32_t* d_n_removed, const int32_t* d_m_before, bool from_counters);
// the tally of one message that is on the device, on the handle's stream
int tally_now(slam_handle* h, const slam_map_config& c, const float* d_meas, const int32_t* d_count, int k_stride, const int32_t* d_flags);
// what a managed step or run checks at entry
int managed_enter(slam_handle* h, const char* who);

}  // namespace slam_capi
#pragma GCC visibility pop
