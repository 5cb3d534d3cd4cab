// capi_assoc.h — the pieces of capi_assoc.cpp that the joint association (capi_joint.cpp) and the managed ticks (capi_map.cpp,
// capi_merge.cpp) check their arguments, launch their association and read their traffic with.  Internal.
#pragma once
#include "capi_filter.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int assoc_config(const slam_assoc_config* cfg, slam_assoc_config* out);

// the rows of assoc.dint, [kAssocRows][ticks][B]; joint.dint begins with the same five
enum AssocRow { kAssocMatch = 0, kAssocNew = 1, kAssocDrop = 2, kAssocFlags = 3, kAssocLm = 4, kAssocRows = 5 };

// the per-instance outputs of one association on the device (counts, flags and landmarks; the detection slots when asked for)
struct AssocDev { int32_t *n_match, *n_new, *n_drop, *flags, *n_lm, *verdict, *slot; double* det; };

// the association launches of one message on the handle's stream
int assoc_launch(slam_handle* h, const slam_assoc_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
                 int k_stride, float* d_meas_out, int32_t* d_count_out, double* d_rec, const AssocDev& d);
// the labelled message of one tick, the records and the counts of `ticks` ticks, the contributions and the traffic sums (zeroed in stream order)
int assoc_reserve(slam_handle* h, int k_stride, size_t ticks);

// after a synchronisation: the sums of the traffic model since they were zeroed
int read_traffic(slam_handle* h, Traffic& w);
// slam_last_associate_work and slam_last_joint_work; w: NULL with a NULL handle, calls: what has to have run
int last_traffic_work(const Traffic* w, const char* calls, double* bytes, double* part_ms, double* total_ms);

// slam_associate_run as run_filtered's feature; the managed ticks reserve and launch their association and copy its rows with it
struct AssocTicks {
    slam_handle* h; const slam_assoc_config& c;
    double* recs; int32_t *n_match, *n_new, *n_drop, *flags;
    size_t B = 0, cb = 0;   // (set by reserve: the handle is checked by then)

    RunTimes& times() const { return h->assoc.times; }
    double bytes_per_tick() const { return kAssocRows * 4.0 * (double)h->B; }
    int reserve(int k_stride, int chunk) {
        B = (size_t)h->B; cb = (size_t)chunk * B;
        return assoc_reserve(h, k_stride, (size_t)chunk);
    }
    int chunk_begin() { return SLAM_OK; }
    DevMsg out() const { return {h->assoc.dmeas, h->assoc.dcount}; }
    int32_t* at(AssocRow r, int t) const { return row(h->assoc.dint, r, cb, (size_t)t * B); }
    int launch(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int k_stride) {
        return assoc_launch(h, c, cmd, d_each, dm, dc, k_stride, out().meas, out().count, h->inn.drec + (size_t)t * slam::kInnovRecLen,
                            {at(kAssocMatch, t), at(kAssocNew, t), at(kAssocDrop, t), at(kAssocFlags, t), at(kAssocLm, t), nullptr, nullptr, nullptr});
    }
    template <class Mark>
    int filter(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int k_stride, Mark mark) {
        return mark([&] { return launch(t, cmd, d_each, dm, dc, k_stride); });
    }
    template <class Mark> int after_step(int, int, Mark) { return SLAM_OK; }
    int chunk_done(int t0, int tc);   // the traffic of the chunk's ticks
    std::vector<TickRow> rows() const {
        return {{h->inn.drec, recs, slam::kInnovRecLen}, {at(kAssocMatch, 0), n_match, B}, {at(kAssocNew, 0), n_new, B},
                {at(kAssocDrop, 0), n_drop, B}, {at(kAssocFlags, 0), flags, B}};
    }
    int finish();                     // synchronised, the traffic read
};

}  // namespace slam_capi
#pragma GCC visibility pop
