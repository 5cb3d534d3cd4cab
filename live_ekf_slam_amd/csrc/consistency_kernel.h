// consistency_kernel.h — NEES consistency statistics of every EKF instance at the handle's current state (slam_consistency, gfx950).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace slam {

// Everything is read only, except the five outputs and the workspace.
struct ConsistencyParams {
    const void* P;          // [B][pstride] P_t as the step kernels leave it: row-major, leading dimension ekf_ld(n, esz), fp64 or fp32
    const void* x;          // [B][xstride] x_t
    const int32_t* M;       // [B]
    const int32_t* ids;     // [B][L_max] lm_IDs
    const int32_t* status;  // [B] slam_instance_flags
    const double* truth;    // [B][3] the simulator's true pose
    const double* map;      // [L][2] shared true map ...
    int32_t L;
    const double* map_each; // ... or one per instance (slam_set_maps): map_each + b * map_stride * 2, L_each[b] landmarks
    const int32_t* L_each;
    int32_t map_stride;
    int32_t B, L_max, pstride, xstride;
    int32_t id_known;       // landmark_id_is_known: ids[j] is the row of the true map (else it says nothing: NO_TRUTH)
    // outputs, device, [B] each
    double* nees_full; double* nees_pose; double* map_rms; int32_t* dof; int32_t* flags;
    // the class beyond the LDS: packed triangles of the instances of one chunk, ws_stride doubles apart
    double* ws; size_t ws_stride;
    int32_t b0, count;      // the instances [b0, b0 + count) of this launch (set by launch_consistency)
    // launch_consistency_selected only: the slots whose rows of S are factored, ascending, and the true row of each ([B][L_max] each, n_sel
    // [B] entries in use); nees_full and dof are then nees_matched and dof_matched, flags is read (INSTANCE_FAILED as the list's writer
    // decided it) and written, nees_pose and map_rms are not written, entries 12 - 14 of inst_rec [B][16] are
    const int32_t* sel; const int32_t* sel_row; const int32_t* n_sel;
    double* inst_rec;
};

// doubles of workspace ONE instance needs (0: the LDS classes, L_max <= 50)
size_t consistency_ws_per_instance(int L_max);
// All instances, in chunks of `chunk` (the workspace class; ws holds chunk * consistency_ws_per_instance doubles) on `stream`.
hipError_t launch_consistency(ConsistencyParams p, int f32_storage, int chunk, hipStream_t stream);
// The same factorisation on the principal submatrix of S that the pose and the listed slots select (slam_map_score: score_kernel.h
// writes the list), with the landmark truth through the list; the classes, the workspace and the chunks are those of launch_consistency.
hipError_t launch_consistency_selected(ConsistencyParams p, int f32_storage, int chunk, hipStream_t stream);

}  // namespace slam
