// sense_kernel.h — a simulator source with a sensor fault model for the robust runs of the EKF batch (slam_sense, slam_sense_commit and the
// *_run_sim calls; gfx950).  The step kernels are untouched: one side kernel writes the message the unmodified known-id step (or a gate,
// an association, a managed step in front of it) is then given, a second one commits the simulator's bookkeeping after that step.
//
// sense_instance() below is THE definition of the fault model: the device kernel (sense_kernel.hip) and the host test hook
// (slam_sense_instance_host) compile this one function, with -ffp-contract=off on both sides, so the two give the same bits.  The clean
// message is sim_wave of sim_device.h on the device and sense_clean_seq(), its lane-by-lane restatement, on the host.
//
// Instance b (global id g = inst0 + b) at RNG step s, the step slam_step_sim would use:
//   0. clean message   sim_wave: pair 0 for the motion, pair 1 + v for the v-th visible landmark in ascending id; the true pose advances
//                      into a STAGED row, not into the handle's truth.  c_vis visible, the first c = min(c_vis, 64) are kept; more sets
//                      TOO_LONG.  An instance whose status carries SLAM_INST_INDEX_OOR is skipped: count 0, nothing staged, FROZEN.
//   1. fault draws     pair indices the clean generator never uses, F = 0x40000000:
//                        (a_v, b_v) = noise_pair(seed, g, s, F + v)       (m_v, k_v) = noise_pair(seed, g, s, F + 64 + v)        v < c
//                        (ur_j, ub_j) = noise_pair(.., F + 128 + j)       (e_j, kc_j) = noise_pair(.., F + 136 + j)              j < n_clutter <= 8
//   2. dropout         detection v is missed iff a_v < p_miss
//   3. range spike     a detection that was not missed is spiked iff b_v < p_spike: r_out = (float)((double)r_f32 + (spike_lo + (spike_hi - spike_lo) * m_v)),
//                      r_f32 the clean float the generator wrote
//   4. clutter         slot j is present iff e_j < p_clutter: r = (float)(clutter_r_min + (range_max - clutter_r_min) * ur_j),
//                      beta = (float)(fov_min + (fov_max - fov_min) * ub_j), id = (float)(L_b + j), L_b the instance's map size
//   5. order           shuffle = 0: survivors in ascending v, then present clutter in ascending j; shuffle = 1: all of them ascending by
//                      (key, position in the shuffle = 0 order), keys k_v / kc_j
//   6. erase_ids = 1   the id column is the quiet NaN 0x7FC00000
//   7. output          n_out detections, the first min(n_out, k_stride) written, the rest of the row up to k_stride written as 0.0f,
//                      count = n_out; origin (true map row, -1 for clutter and for the slots beyond) and fault (1 spiked, else 0)
//   8. record          16 doubles (SenseRec), per instance; the sum over the batch in the fixed order of the innovation record
// Every expression is evaluated as parenthesised, in fp64, without contraction.  Plain loads and stores, no atomics, no inline assembly.
#pragma once
#include <stdint.h>

#include "../../include/slam_batch.h"
#include "innovation_kernel.h"
#include "slam_rng.h"

namespace slam {

constexpr int kSenseMaxDet = 64;                                  // SLAM_SENSE_MAX_DET: clean detections of one message
constexpr int kSenseMaxClutter = 8;                               // SLAM_SENSE_MAX_CLUTTER
constexpr int kSenseItems = kSenseMaxDet + kSenseMaxClutter;      // candidates of one message: lane i takes i and i + 64
constexpr int kSenseRecLen = 16;
constexpr uint32_t kSenseFaultPair = 0x40000000u;                 // F: the first pair index of the fault draws
constexpr uint32_t kSenseNanBits = 0x7FC00000u;                   // the erased id
constexpr int32_t kSenseFrozen = 1, kSenseTooLong = 2;            // slam_sense_flags
static_assert(kSenseMaxDet == kInnovMaxDet, "one message limit");

// indices of a record (counts are stored as doubles)
enum SenseRec {
    kSenSensed = 0, kSenFrozen = 1, kSenTooLong = 2, kSenClean = 3, kSenMissed = 4, kSenSpiked = 5, kSenClutter = 6, kSenOut = 7,
    kSenOverflow = 8, kSenSpikeSum = 9, kSenCommitted = 10, kSenErrSum = 11
};
constexpr unsigned kSenseRecMax = 0u;                               // no entry is joined by a maximum (record_kernel.h): every one is a sum

// the simulator's configuration of one instance: what sim_wave reads from its parameter block and the instance's half-widths
struct SenseSim { uint64_t seed; uint64_t g; double d_max, th_max, range_max, fov_min, fov_max, sV00, sV11, sW00, sW11; };

// everything one instance holds between its phases: LDS on the device (one per wavefront), plain memory on the host
struct SenseWork {
    float meas[3 * kSenseMaxDet];                    // the clean message
    double key[kSenseItems], amt[kSenseItems];       // per candidate: shuffle key, spike amount
    double ckey[kSenseItems];                        // the keys of the present candidates in the shuffle = 0 order
    float id[kSenseItems], r[kSenseItems], b[kSenseItems];
    int32_t pres[kSenseItems], org[kSenseItems], flt[kSenseItems];
};

struct SenseResult {
    int32_t flags, count;                            // slam_sense_flags; n_out
    int32_t c, n_miss, n_spike, n_clutter;
    double spike_sum;                                // the spike amounts in ascending v, from 0.0
};

// The all-off row and the value checks of a row; what: NULL, or the name of the first bad field.
SLAM_HD slam_sensor sense_default_row() { return slam_sensor{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0, 0, 0}; }
inline const char* sense_bad_field(const slam_sensor& r, double range_max) {
    auto prob = [](double p) { return innov_finite(p) && p >= 0.0 && p <= 1.0; };
    if (!prob(r.p_miss)) return "p_miss";
    if (!prob(r.p_spike)) return "p_spike";
    if (!prob(r.p_clutter)) return "p_clutter";
    if (!innov_finite(r.spike_lo)) return "spike_lo";
    if (!innov_finite(r.spike_hi) || r.spike_lo > r.spike_hi) return "spike_hi";
    if (r.n_clutter < 0 || r.n_clutter > kSenseMaxClutter) return "n_clutter";
    if (!innov_finite(r.clutter_r_min) || r.clutter_r_min < 0.0 || r.clutter_r_min > range_max) return "clutter_r_min";
    return nullptr;
}

SLAM_HD float sense_erased_id() {
    const uint32_t bits = kSenseNanBits;
    float f;
    __builtin_memcpy(&f, &bits, sizeof(f));
    return f;
}

// sim_wave (sim_device.h) by one lane: the same expressions on the same operands in the order of the visible ids.  Advances the true pose
// in place, writes the first kSenseMaxDet triplets to meas and returns the number of visible landmarks.
SLAM_HD int sense_clean_seq(const SenseSim& sc, float fwd, float ang, uint32_t step, const double* map, int L, double& tx, double& ty, double& tth,
                            float* meas) {
    double u0, u1;
    noise_pair(sc.seed, sc.g, step, 0u, &u0, &u1);
    double d = ((double)fwd + (2 * sc.sV00) * u0) - sc.sV00;
    double hdg = ((double)ang + (2 * sc.sV11) * u1) - sc.sV11;
    d = (sc.d_max < d) ? sc.d_max : d;
    d = (0.0 < d) ? d : 0.0;
    hdg = (sc.th_max < hdg) ? sc.th_max : hdg;
    hdg = (-sc.th_max < hdg) ? hdg : -sc.th_max;
    double s, c;
    det_sincos(tth, &s, &c);
    tx = tx + d * c;
    ty = ty + d * s;
    tth = tth + hdg;
    int count = 0;
    for (int id = 0; id < L; ++id) {
        const double dx = map[2 * id] - tx, dy = map[2 * id + 1] - ty;
        const double r = sqrt(dx * dx + dy * dy);
        const double gb = det_atan2(dy, dx);
        const double beta = rem2pi(gb - tth);
        if (!(!(r > sc.range_max) && (beta > sc.fov_min && beta < sc.fov_max))) continue;
        if (count < kSenseMaxDet) {
            double v0, v1;
            noise_pair(sc.seed, sc.g, step, (uint32_t)(1 + count), &v0, &v1);
            const double rn = (r + (2 * sc.sW00) * v0) - sc.sW00;
            const double bn = (beta + (2 * sc.sW11) * v1) - sc.sW11;
            meas[3 * count] = (float)id;
            meas[3 * count + 1] = (float)rn;
            meas[3 * count + 2] = (float)bn;
        }
        count += 1;
    }
    return count;
}

// One instance that is not frozen.  ws.meas holds the first min(c_vis, kSenseMaxDet) clean triplets already (the policy's sync() has run).
// w: the execution policy of innovation_kernel.h (InnovSeq on the host, InnovWave on the device); s: the RNG step; L_b: the instance's map
// size.  meas_out [k_stride][3]; origin, fault [k_stride] or NULL.  Every lane returns the same result; the lanes share the writes.
template <class W>
SLAM_HD SenseResult sense_instance(const W& w, SenseWork& ws, const slam_sensor& row, uint64_t seed, uint64_t g, uint32_t s, int c_vis, int L_b,
                                   double range_max, double fov_min, double fov_max, int k_stride, float* meas_out, int32_t* origin,
                                   int32_t* fault) {
    SenseResult o;
    const int c = c_vis < kSenseMaxDet ? (c_vis < 0 ? 0 : c_vis) : kSenseMaxDet;
    const int nclut = row.n_clutter < 0 ? 0 : (row.n_clutter > kSenseMaxClutter ? kSenseMaxClutter : row.n_clutter);
    o.flags = c_vis > kSenseMaxDet ? kSenseTooLong : 0;
    o.c = c;
    // ---- every candidate: the draws, whether it is present, its values ----
    for (int q = w.lane(); q < kSenseItems; q += w.width()) {
        bool pres = false;
        float id = 0.f, rr = 0.f, bb = 0.f;
        int32_t org = -1, flt = 0;
        double key = 0.0, amt = 0.0;
        if (q < kSenseMaxDet) {
            if (q < c) {
                double a_v, b_v, m_v, k_v;
                noise_pair(seed, g, s, kSenseFaultPair + (uint32_t)q, &a_v, &b_v);
                noise_pair(seed, g, s, kSenseFaultPair + 64u + (uint32_t)q, &m_v, &k_v);
                pres = !(a_v < row.p_miss);
                id = ws.meas[3 * q]; rr = ws.meas[3 * q + 1]; bb = ws.meas[3 * q + 2];
                org = (int32_t)id;
                key = k_v;
                if (pres && b_v < row.p_spike) {
                    amt = row.spike_lo + (row.spike_hi - row.spike_lo) * m_v;
                    rr = (float)((double)rr + amt);
                    flt = 1;
                }
            }
        } else if (q - kSenseMaxDet < nclut) {
            const int j = q - kSenseMaxDet;
            double ur, ub, e_j, kc_j;
            noise_pair(seed, g, s, kSenseFaultPair + 128u + (uint32_t)j, &ur, &ub);
            noise_pair(seed, g, s, kSenseFaultPair + 136u + (uint32_t)j, &e_j, &kc_j);
            pres = e_j < row.p_clutter;
            rr = (float)(row.clutter_r_min + (range_max - row.clutter_r_min) * ur);
            bb = (float)(fov_min + (fov_max - fov_min) * ub);
            id = (float)(L_b + j);
            key = kc_j;
        }
        ws.pres[q] = pres ? 1 : 0; ws.org[q] = org; ws.flt[q] = flt;
        ws.id[q] = id; ws.r[q] = rr; ws.b[q] = bb; ws.key[q] = key; ws.amt[q] = amt;
    }
    w.sync();
    // ---- the counts (every lane alike) and the keys in the shuffle = 0 order ----
    int n_out = 0, n_miss = 0, n_spike = 0, n_cl = 0;
    double spike_sum = 0.0;
    for (int q = 0; q < kSenseItems; ++q) {
        const int pr = ws.pres[q];
        if (q < c) {
            n_miss += 1 - pr;
            if (ws.flt[q]) { n_spike += 1; spike_sum = spike_sum + ws.amt[q]; }
        } else {
            n_cl += pr;
        }
        if (pr && (n_out % w.width()) == w.lane()) ws.ckey[n_out] = ws.key[q];
        n_out += pr;
    }
    w.sync();
    o.count = n_out; o.n_miss = n_miss; o.n_spike = n_spike; o.n_clutter = n_cl; o.spike_sum = spike_sum;
    // ---- where every present candidate goes ----
    const float erased = sense_erased_id();
    for (int q = w.lane(); q < kSenseItems; q += w.width()) {
        if (!ws.pres[q]) continue;
        int pos0 = 0;
        for (int i = 0; i < q; ++i) pos0 += ws.pres[i];
        int rank = pos0;
        if (row.shuffle) {
            const double key = ws.key[q];
            rank = 0;
            for (int i = 0; i < n_out; ++i) rank += (ws.ckey[i] < key || (ws.ckey[i] == key && i < pos0)) ? 1 : 0;
        }
        if (rank < k_stride) {
            meas_out[3 * rank] = row.erase_ids ? erased : ws.id[q];
            meas_out[3 * rank + 1] = ws.r[q];
            meas_out[3 * rank + 2] = ws.b[q];
            if (origin) origin[rank] = ws.org[q];
            if (fault) fault[rank] = ws.flt[q];
        }
    }
    for (int e = n_out + w.lane(); e < k_stride; e += w.width()) {
        meas_out[3 * e] = 0.f; meas_out[3 * e + 1] = 0.f; meas_out[3 * e + 2] = 0.f;
        if (origin) origin[e] = -1;
        if (fault) fault[e] = 0;
    }
    return o;
}

// the row of a frozen instance: count 0, the whole row zero
template <class W>
SLAM_HD SenseResult sense_frozen(const W& w, int k_stride, float* meas_out, int32_t* origin, int32_t* fault) {
    SenseResult o;
    o.flags = kSenseFrozen; o.count = 0; o.c = o.n_miss = o.n_spike = o.n_clutter = 0; o.spike_sum = 0.0;
    for (int e = w.lane(); e < k_stride; e += w.width()) {
        meas_out[3 * e] = 0.f; meas_out[3 * e + 1] = 0.f; meas_out[3 * e + 2] = 0.f;
        if (origin) origin[e] = -1;
        if (fault) fault[e] = 0;
    }
    return o;
}

// what one instance adds to a record (entries 10 and 11 belong to the commit)
SLAM_HD void sense_record(const SenseResult& v, int k_stride, double r[kSenseRecLen]) {
    for (int i = 0; i < kSenseRecLen; ++i) r[i] = 0.0;
    if (v.flags & kSenseFrozen) { r[kSenFrozen] = 1.0; return; }
    r[kSenSensed] = 1.0;
    if (v.flags & kSenseTooLong) r[kSenTooLong] = 1.0;
    r[kSenClean] = (double)v.c; r[kSenMissed] = (double)v.n_miss; r[kSenSpiked] = (double)v.n_spike; r[kSenClutter] = (double)v.n_clutter;
    r[kSenOut] = (double)v.count; r[kSenOverflow] = (double)(v.count > k_stride ? v.count - k_stride : 0);
    r[kSenSpikeSum] = v.spike_sum;
}

#if defined(__HIPCC__)
// One tick of the model for every instance on `stream`: the instance kernel and, with rec != NULL, the reduction of the per-instance
// records.  The handle's state is read only; written are the caller's message and labels, the staged rows and the records.
struct SenseParams {
    EkfStepParams s;             // as the simulator step that would follow is launched (sim = 1): status, timestep, truth, maps, noise rows,
                                 // the command or cmd_each, seed, inst0 and the RNG step
    const slam_sensor* rows;     // [B], NULL: the all-off row
    float* meas_out;             // [B][k_stride][3]
    int32_t* count_out;          // [B]
    int32_t k_stride;
    int32_t* origin;             // [B][k_stride] or NULL
    int32_t* fault;              // [B][k_stride] or NULL
    double* truth_next;          // [B][3] staged true pose (a frozen instance: its pose as it is)
    int32_t* staged_ts;          // [B] the timestep the message was made at (a frozen instance: -2, which no step reaches)
    double* inst_rec;            // [B][kSenseRecLen]
    double* partials;            // [record_blocks(B)][kSenseRecLen]
    double* rec;                 // [kSenseRecLen] or NULL: no reduction
};
hipError_t launch_sense(const SenseParams& p, hipStream_t stream);

// After the step: instance b with timestep[b] == staged_ts[b] + 1 takes its staged true pose and adds the position error of the stored
// estimate to its error sum; any other instance is left alone.  Entries 10 and 11 of the per-instance records are written, then the
// records are reduced into rec (if not NULL).
struct SenseCommitParams {
    const void* x; int32_t xstride, f32_storage, B;
    const int32_t* timestep; const int32_t* staged_ts;
    double* truth; const double* truth_next; double* err_sum;
    double* err_pos;             // [B] or NULL: the value added, NaN where not committed
    double* truth_out;           // [B][3] or NULL: the true pose after the commit, committed or not
    double* inst_rec; double* partials; double* rec;
};
hipError_t launch_sense_commit(const SenseCommitParams& p, hipStream_t stream);
#endif

}  // namespace slam
