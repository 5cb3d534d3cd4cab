// pgs_schedule.h — the rules that decide the schedule of a pose-graph solve (pgs_solve in pgs_capi.cpp): how many solve groups run and which
// instances each owns, whether a group streams, how many lambda lanes a trial may hand out, which chain / SYRK kernels a trial runs, the next
// segment length to try, when the streaming loop hands over to the lockstep loop; and the tuning values of a handle with their clamps.
// Every rule is arithmetic on a few integers.  Plain C++: needs no HIP header (tests/test_pgs_schedule_cpu.py).
#pragma once
#include <stdlib.h>

#include "pgs_limits.h"

namespace slam_host {

constexpr int kPgsMaxGroups = 16;   // solve groups of a solve at most
constexpr int kPgsRing = 8;         // trials of a streaming group whose counters wait in pinned memory for the host at most

// The tuning values of a handle; from_env: what pgs_create reads, once per handle.
struct PgsTuning {
    int max_trials = 400;          // SLAM_PGS_MAX_TRIALS: lambda trials a graph consumes at most (> 0, else ignored)
    int lanes = 4;                 // SLAM_PGS_LANES: slots per instance for speculative lambda lanes, 1 .. 8 (else ignored), 1 = off
    int lanes_switch = 64;         // SLAM_PGS_LANES_SWITCH: active instances (of the whole batch) from which down two lanes are used ...
    int lanes_switch_all = 16;     // SLAM_PGS_LANES_SWITCH_ALL: ... and from which down all of them
    int syrk_inst_switch = 100;    // SLAM_PGS_SYRK_INST_SWITCH: running slots from which the instance-resident SYRK runs (else the tile kernel)
    int fused_mode = -1;           // SLAM_PGS_FUSED: 0 = chain and SYRK as two launches, 2 | 3 | 4 = fused on that many workgroups, else fused when it pays
    int seg_len = 32;              // SLAM_PGS_SEG: poses per segment of the segmented elimination, 2 .. kPgsSegMaxLen; <= 0: 0 = the sequential chain
    bool use_list = true;          // SLAM_PGS_LIST=0: full-size grids, inactive workgroups return
    int groups = 0;                // SLAM_PGS_GROUPS / pgs_set_groups: solve groups, 0 = choose from the batch (pgs_groups)
    int slots = 0;                 // SLAM_PGS_SLOTS / pgs_set_slots: graphs in flight at most, 0 (and below) = lockstep: all of them
    int stream_depth = 3;          // SLAM_PGS_STREAM_DEPTH: trials a streaming group enqueues ahead of the host, 1 .. kPgsRing - 1 (else ignored)
    bool trace = false;            // SLAM_PGS_TRACE (set): print the active-instance count after every trial
    bool host_prof = false;        // SLAM_PGS_HOST_PROF (set): host clock spent enqueuing trials / waiting for their counters
    int seg_back_global = 0;       // SLAM_PGS_SEG_BACK_GLOBAL: PgsParams::seg_back_global
    bool group_prio = true;        // SLAM_PGS_GROUP_PRIO=0: the groups' streams all at the default priority

    static PgsTuning from_env() {
        PgsTuning t;
        auto num = [](const char* name, int* v) { const char* e = getenv(name); if (e) *v = atoi(e); return e != nullptr; };
        int v = 0;
        if (num("SLAM_PGS_MAX_TRIALS", &v) && v > 0) t.max_trials = v;
        if (num("SLAM_PGS_LANES", &v) && v >= 1 && v <= 8) t.lanes = v;
        num("SLAM_PGS_LANES_SWITCH", &t.lanes_switch);
        num("SLAM_PGS_LANES_SWITCH_ALL", &t.lanes_switch_all);
        num("SLAM_PGS_SYRK_INST_SWITCH", &t.syrk_inst_switch);
        t.trace = getenv("SLAM_PGS_TRACE") != nullptr;
        t.host_prof = getenv("SLAM_PGS_HOST_PROF") != nullptr;
        num("SLAM_PGS_FUSED", &t.fused_mode);
        if (num("SLAM_PGS_SEG", &v)) t.seg_len = v <= 0 ? 0 : (v < 2 ? 2 : (v > slam::kPgsSegMaxLen ? slam::kPgsSegMaxLen : v));
        if (num("SLAM_PGS_LIST", &v)) t.use_list = v != 0;
        num("SLAM_PGS_GROUPS", &t.groups);
        if (num("SLAM_PGS_SLOTS", &v)) t.slots = v > 0 ? v : 0;
        if (num("SLAM_PGS_STREAM_DEPTH", &v) && v >= 1 && v < kPgsRing) t.stream_depth = v;
        num("SLAM_PGS_SEG_BACK_GLOBAL", &t.seg_back_global);
        if (num("SLAM_PGS_GROUP_PRIO", &v)) t.group_prio = v != 0;
        return t;
    }
};

// Solve groups of a solve of B instances: what the caller asked for, else two from 128 instances on and one below; at most kPgsMaxGroups and
// at most one per instance.  A profiled solve runs one (per-kernel timing wants the kernels of one stream back to back).
inline int pgs_groups(int requested, int B, bool profile) {
    int G = requested > 0 ? requested : (B >= 128 ? 2 : 1);
    if (G > kPgsMaxGroups) G = kPgsMaxGroups;
    if (G > B) G = B;
    return profile ? 1 : G;
}

// Group g of G owns the instances [b_off, b_off + b_cnt): ceil(B / G) each, the last ones what is left.  b_cnt <= 0: the group is idle - it
// launches nothing and nothing waits for it.
struct PgsRange { int b_off, b_cnt; bool idle() const { return b_cnt <= 0; } };
inline PgsRange pgs_group_range(int B, int G, int g) {
    const int per = (B + G - 1) / G;
    return {g * per, B - g * per < per ? B - g * per : per};
}

// Streaming: `slots` graphs in flight over all groups, ceil(slots / G) per group (0: no streaming - none asked for, or a profiled solve) ...
inline int pgs_slot_share(int slots, int G, bool profile) { return slots > 0 && !profile ? (slots + G - 1) / G : 0; }
// ... and a group of b_cnt instances streams with its share iff that does not cover them (0: it runs lockstep, every graph from the first trial on).
inline int pgs_stream_slots(int share, int b_cnt) { return share > 0 && share < b_cnt ? share : 0; }

// Lambda lanes the decide step of a trial may hand out, from the active instances (of the whole batch) before it.  Few instances left: the
// per-trial latency counts and spare slots cost little - two lanes from lanes_switch down (the common streak is one failure, then a success
// at 10 lambda), all of them from lanes_switch_all down.
inline int pgs_lanes_next(const PgsTuning& t, int active) {
    return active <= t.lanes_switch_all ? t.lanes : (active <= t.lanes_switch ? (t.lanes < 2 ? t.lanes : 2) : 1);
}

// Workgroups per slot of the fused chain + SYRK launch of a trial of `run` slots on `cus` compute units, 0 = chain and SYRK as two launches.
// Each workgroup is alone on a CU.  With idle CUs to spare the chain is replicated on up to four of them so that a workgroup's share of the
// tiles stays in the shadow of the recursion; between one and two rounds of two workgroups the two-launch path (instance-resident SYRK) is
// faster; a full batch of 2 x cus workgroups is two clean rounds.  fused_mode 2 | 3 | 4 forces that many.
inline int pgs_fused(bool fused_ok, int fused_mode, int run, int cus) {
    if (!fused_ok) return 0;
    if (fused_mode >= 2 && fused_mode <= 4) return fused_mode;
    if (4 * run <= cus) return 4;
    if (3 * run <= cus) return 3;
    if (2 * run <= cus) return 2;
    return run > (cus * 2) / 3 && run <= cus ? 2 : 0;
}

// Whether the graphs of a solve on the sequential chain (asked only with LD <= 448: a column of Y per lane) fit the fused kernel and the
// instance-resident SYRK; mx = the most landmarks of any instance.  Fused: the lower triangle of S (2 mx columns) within the 72 wavefront
// tiles of pgs_chain_syrk_kernel and a pose's factors within its event staging (32).  Instance-resident: the lower triangle of S_ext (the z
// column included) within kPgsSyrkInstTiles tiles, mx <= 207; beyond, the tile kernel takes the solve.
struct PgsFit { bool fused_ok, syrk_inst_ok; };
inline PgsFit pgs_fit(int mx, int KP, int fused_mode) {
    const int nt = (2 * mx + 31) / 32, nti = (2 * mx + 1 + 31) / 32;
    return {fused_mode != 0 && KP <= 32 && nt * (nt + 1) / 2 <= 72, nti * (nti + 1) / 2 <= slam::kPgsSyrkInstTiles};
}

// SYRK kernel of a trial (PgsParams::syrk_wave_tile): instance-resident accumulators (1) from syrk_inst_switch running slots - an upper
// bound, active instances x lanes - while they hold every graph of the solve, else 32 x 32 wavefront tiles (32).
inline int pgs_syrk_kernel(int active, int lanes, int syrk_inst_switch, bool syrk_inst_ok) {
    return active * lanes >= syrk_inst_switch && syrk_inst_ok ? 1 : 32;
}

// One step of the search for a solve's segment length: the plan for segments of SL poses reported mx, the most landmarks any segment sees
// (0x7fffffff: more separators than pgs_sep_kernel stages - shorter segments only add separators); the graph has N poses.  Accept SL, try
// `next` = SL / 2 (not below 8 poses, nor more separators than kPgsSegMaxSep), or give up: the sequential chain.
struct PgsSegStep { enum Kind { kAccept, kTry, kGiveUp } kind; int next; };
inline PgsSegStep pgs_seg_step(int SL, int mx, int N) {
    if (mx <= slam::kPgsSegMaxLm) return {PgsSegStep::kAccept, SL};
    const int next = SL / 2;
    if (mx == 0x7fffffff || next < 8 || (N - 2) / next > slam::kPgsSegMaxSep) return {PgsSegStep::kGiveUp, 0};
    return {PgsSegStep::kTry, next};
}

// Streaming loop of a group of b_cnt instances on `cap` slots.  Launches at most: the trial cap is per graph (pgs_decide_kernel applies it),
// the launches only need a bound that cannot bind first.
inline long long pgs_stream_launch_bound(int b_cnt, int cap, int max_trials) { return ((long long)b_cnt / cap + 2) * max_trials; }
// It hands over to the lockstep loop once nothing is left, or nothing waits (the cursor next_waiting stands behind the group's range, which
// ends before `range_end`) and few enough run that the lambda lanes pay; `active` = the group's running graphs, scaled to the batch by G.
inline bool pgs_stream_hands_over(int active, int next_waiting, int range_end, int G, int lanes_switch) {
    return active == 0 || (next_waiting >= range_end && active * G <= lanes_switch);
}

}  // namespace slam_host
