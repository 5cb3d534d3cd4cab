// capi_sense.h — the launches of capi_sense.cpp that the per-tick runs reach through TickMsgs (capi_run.h).  Internal.
#pragma once
#include "slam_handle.h"

#pragma GCC visibility push(hidden)
namespace slam_capi {

// the staged rows, the per-instance records and the record of one tick
int sense_reserve(slam_handle* h);

// The sense launch for the step launch_step(h, cmd, 0, d_meas, d_count, k_stride, d_cmd_each) is about to run, at the handle's RNG step,
// on the handle's stream; d_origin, d_fault may be NULL; d_rec NULL: no reduction of the records.
int sense_launch(slam_handle* h, const float cmd[2], const float* d_cmd_each, float* d_meas, int32_t* d_count, int k_stride, int32_t* d_origin,
                 int32_t* d_fault, double* d_rec);

// The commit launch after that step; d_err_pos [B], d_truth_out [B][3] (the truth after the commit) and d_rec [16] may be NULL.
int sense_commit_launch(slam_handle* h, double* d_err_pos, double* d_truth_out, double* d_rec);

}  // namespace slam_capi
#pragma GCC visibility pop
