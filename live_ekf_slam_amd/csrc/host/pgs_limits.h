// pgs_limits.h — the capacities of the pose-graph kernels that the host's schedule rules (host/pgs_schedule.h) decide by.  One definition of
// each, for the kernels (pgs_kernel.h includes this file) and for the host.  Plain C++: needs no HIP header.
#pragma once

namespace slam {

static constexpr int kPgsSegMaxLen = 32;      // poses a segment holds at most (seg_len <= this)
static constexpr int kPgsSegMaxLm = 63;       // landmarks a segment's column set may hold for the segmented path (2 * 63 + 1 = 127 columns)
static constexpr int kPgsSegMaxSep = 128;     // separators the separator kernel stages in LDS
static constexpr int kPgsSyrkInstTiles = 96;  // 32x32 tiles of S_ext pgs_syrk_inst_kernel holds per instance (16 wavefronts x SI_NB x SI_NS)

}  // namespace slam
