// capi_innovation.h — the pieces of capi_innovation.cpp that the gate (capi_gate.cpp) evaluates with, and the staging buffers every unit
// over capi_filter.h uploads its messages and commands to.  Internal.
#pragma once
#include "innovation_kernel.h"
#include "slam_handle.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// the per-instance buffers of one evaluation; det: the detection slots are wanted
int innovation_reserve(slam_handle* h, bool det);

// the launch parameters of one evaluation of the step launch_step(h, cmd, sim, d_meas, d_count, k_stride, d_cmd_each) would run now
slam::InnovParams innovation_params(slam_handle* h, const slam_innovation_config& c, const float cmd[2], int sim, const float* d_meas,
                                    const int32_t* d_count, int k_stride, const float* d_cmd_each);

// The outputs of one evaluation (slam_innovation*, slam_gate*): on the device they have fixed places in the handle's buffers.
struct InnovOut { double *rec, *nis_sum, *post, *det; int32_t *n_upd, *flags, *n_new; };

int innovation_outputs(slam_handle* h, bool det, InnovOut* d);

// once the stream has run dry: the outputs the caller wants (non-NULL in `to`) from their device places
int innovation_download(slam_handle* h, const InnovOut& d, const InnovOut& to);

// n floats from the host into the handle's staging buffer for per-instance commands, in stream order
int innovation_upload_cmds(slam_handle* h, const float* cmds, size_t n);

// the host messages of `ticks` ticks into the handle's staging buffers ([ticks][B][k_stride][3] and [ticks][B]), in stream order
int upload_messages(slam_handle* h, const float* meas, const int32_t* count, int k_stride, size_t ticks);

}  // namespace slam_capi
#pragma GCC visibility pop
