// capi_assoc.h — the pieces of capi_assoc.cpp that the managed tick (capi_map.cpp) checks its arguments and launches its association
// with.  Internal.
#pragma once
#include "slam_handle.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// *out = *cfg (NULL: the defaults), checked
int assoc_config(const slam_assoc_config* cfg, slam_assoc_config* out);
// the arguments every entry point of one message shares, checked before the handle is looked at
int assoc_args(const slam_assoc_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride, const float* meas_out,
               const int32_t* count_out, bool need_out, slam_assoc_config* c);
// the byte ranges [a, a + na) and [b, b + nb) meet
bool assoc_overlap(const void* a, size_t na, const void* b, size_t nb);
int assoc_supported(const slam_handle* h);
// the handle, once the arguments are in order; the queued timesteps run first
int assoc_enter(slam_handle* h);
int assoc_step_state(const slam_handle* h, const char* who);

// the per-instance outputs of one association on the device ([5][ticks][B] counts, flags and landmarks; the detection slots when asked for)
struct AssocDev { int32_t *n_match, *n_new, *n_drop, *flags, *n_lm, *verdict, *slot; double* det; };

// the association launches of one message on the handle's stream
int assoc_launch(slam_handle* h, const slam_assoc_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
                 int k_stride, float* d_meas_out, int32_t* d_count_out, double* d_rec, const AssocDev& d);
// the labelled message of one tick, the records and the counts of `ticks` ticks, the contributions and the traffic sums (zeroed in stream order)
int assoc_reserve(slam_handle* h, int k_stride, size_t ticks);

}  // namespace slam_capi
#pragma GCC visibility pop
