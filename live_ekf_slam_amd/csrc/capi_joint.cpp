// capi_joint.cpp — C ABI: joint-compatibility association (JCBB) of detections without ids (joint_kernel.hip).  The argument checks, the
// handle's entry and the staging are those of capi_assoc.cpp.
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_assoc.h"
#include "capi_innovation.h"
#include "capi_run.h"
#include "ekf_kernel.h"
#include "host/noise_pack.h"
#include "host/tick_chunks.h"
#include "joint_kernel.h"

using namespace slam_capi;

namespace {

static_assert(sizeof(((slam_joint_config*)0)->gate_joint) == sizeof(double) * slam::kJointMaxPair, "one gate per pairing count");

// *out = *cfg (NULL: the defaults), checked
int joint_config(const slam_joint_config* cfg, slam_joint_config* out) {
    if (cfg) *out = *cfg; else slam_joint_config_default(out);
    const slam_assoc_config ac = {out->gate_match, out->gate_new};
    slam_assoc_config checked;
    TRY(assoc_config(&ac, &checked));
    for (int i = 0; i < slam::kJointMaxPair; ++i) {
        const double g = out->gate_joint[i];
        if (isnan(g) || !(g > 0.0) || (i > 0 && g < out->gate_joint[i - 1]))
            return slam_internal_fail(SLAM_ERR_ARG, "joint config: gate_joint[%d] = %g is NaN, not positive or below its predecessor (+inf is allowed)", i, g);
    }
    if (out->max_nodes < 1 || out->max_nodes > slam::kJointMaxNodes)
        return slam_internal_fail(SLAM_ERR_ARG, "joint config: max_nodes = %d is not in 1 .. %d", (int)out->max_nodes, slam::kJointMaxNodes);
    return SLAM_OK;
}

// the arguments every entry point of one message shares, checked before the handle is looked at
int joint_args(const slam_joint_config* cfg, const float* cmds, const float* meas, const int32_t* count, int k_stride, const float* meas_out,
               const int32_t* count_out, bool need_out, slam_joint_config* c) {
    TRY(joint_config(cfg, c));
    const slam_assoc_config ac = {c->gate_match, c->gate_new};
    slam_assoc_config checked;
    return assoc_args(&ac, cmds, meas, count, k_stride, meas_out, count_out, need_out, &checked);
}

// the per-instance outputs of one joint association on the device ([7][ticks][B] ints; the detection slots when asked for)
struct JointDev { int32_t *n_match, *n_new, *n_drop, *flags, *n_lm, *nodes, *n_blk; double* d2; int32_t *verdict, *slot, *ncand; double* det; };

// the joint launches of one message on the handle's stream
int joint_launch(slam_handle* h, const slam_joint_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
                 int k_stride, float* d_meas_out, int32_t* d_count_out, double* d_rec, const JointDev& d) {
    slam::JointParams p;
    memset(&p, 0, sizeof(p));
    fill_ekf_params(h, p.s, cmd, 0, 0, d_meas, d_count, k_stride, nullptr, 0, d_cmd_each);
    p.gate_match = c.gate_match; p.gate_new = c.gate_new; p.max_nodes = c.max_nodes;
    for (int i = 0; i < slam::kJointMaxPair; ++i) p.gate_joint[i] = c.gate_joint[i];
    p.meas_out = d_meas_out; p.count_out = d_count_out;
    p.n_match = d.n_match; p.n_new = d.n_new; p.n_drop = d.n_drop; p.flags = d.flags; p.n_lm = d.n_lm; p.nodes = d.nodes; p.n_blk = d.n_blk;
    p.d2_joint = d.d2; p.verdict = d.verdict; p.slot = d.slot; p.ncand = d.ncand; p.det = d.det;
    p.inst_rec = h->inn.dval + 13 * (size_t)h->B;   // (the places innovation_reserve gives the contributions and the partial records)
    p.partials = h->inn.dpart;
    p.rec = d_rec;
    HIP_TRY(slam::launch_associate_joint(p, h->esz == 4, h->stream));
    return SLAM_OK;
}

// the labelled message of one tick, the records and the counts of `ticks` ticks, the contributions and the traffic sums (zeroed in stream order)
int joint_reserve(slam_handle* h, int k_stride, size_t ticks) {
    const size_t B = (size_t)h->B;
    TRY(grow(h, h->joint.dmeas, 3 * (size_t)k_stride * B));
    TRY(grow(h, h->joint.dcount, B));
    TRY(grow(h, h->joint.dint, 7 * ticks * B));
    TRY(grow(h, h->joint.dd2, ticks * B));
    TRY(grow(h, h->joint.dwork, 3));
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, ticks * slam::kInnovRecLen));
    HIP_TRY(hipMemsetAsync(h->joint.dwork, 0, 3 * sizeof(unsigned long long), h->stream));
    return SLAM_OK;
}

// the [7][stride] rows of dint at tick offset o
JointDev joint_rows(slam_handle* h, size_t stride, size_t o) {
    int32_t* const di = h->joint.dint;
    return JointDev{di + o, di + stride + o, di + 2 * stride + o, di + 3 * stride + o, di + 4 * stride + o, di + 5 * stride + o, di + 6 * stride + o,
                    h->joint.dd2 + o, nullptr, nullptr, nullptr, nullptr};
}

// the traffic model of `ticks` associations whose counts are in dint, summed on the stream
int joint_sum_work(slam_handle* h, size_t ticks, size_t stride) {
    const int32_t* const di = h->joint.dint;
    HIP_TRY(slam::launch_associate_joint_work(di + 4 * stride, di, di + stride, di + 2 * stride, di + 6 * stride, ticks * (size_t)h->B, h->esz,
                                              h->joint.dwork, h->stream));
    return SLAM_OK;
}

// after a synchronisation: the sums since joint_reserve
int joint_read_work(slam_handle* h) {
    unsigned long long wk[3];
    HIP_TRY(hipMemcpy(wk, h->joint.dwork, sizeof(wk), hipMemcpyDeviceToHost));
    h->joint.bytes = (double)wk[0] * h->esz + (double)wk[1];
    h->joint.lines = 128.0 * (double)wk[2] + (double)wk[1];
    return SLAM_OK;
}

struct JointOut { double* rec; int32_t *n_match, *n_new, *n_drop, *flags, *verdict, *slot; double* det; double* d2; int32_t *nodes, *ncand; };

// slam_associate_joint / slam_associate_joint_dev once the message and the commands are on the device
int joint_now(slam_handle* h, const slam_joint_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas, const int32_t* d_count,
              int k_stride, float* d_meas_out, int32_t* d_count_out, const JointOut& to) {
    const size_t B = (size_t)h->B, nd = B * slam::kInnovMaxDet;
    if (to.verdict) TRY(grow(h, h->joint.dverdict, nd));
    if (to.slot) TRY(grow(h, h->joint.dslot, nd));
    if (to.ncand) TRY(grow(h, h->joint.dncand, nd));
    if (to.det) TRY(grow(h, h->joint.ddet, nd * slam::kAssocDetLen));
    JointDev d = joint_rows(h, B, 0);
    d.verdict = to.verdict ? h->joint.dverdict.get() : nullptr; d.slot = to.slot ? h->joint.dslot.get() : nullptr;
    d.ncand = to.ncand ? h->joint.dncand.get() : nullptr; d.det = to.det ? h->joint.ddet.get() : nullptr;
    TRY(joint_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out, h->inn.drec, d));
    TRY(joint_sum_work(h, 1, B));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(joint_read_work(h));
    if (to.rec) HIP_TRY(hipMemcpy(to.rec, h->inn.drec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (to.n_match) HIP_TRY(hipMemcpy(to.n_match, d.n_match, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_new) HIP_TRY(hipMemcpy(to.n_new, d.n_new, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.n_drop) HIP_TRY(hipMemcpy(to.n_drop, d.n_drop, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.flags) HIP_TRY(hipMemcpy(to.flags, d.flags, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.nodes) HIP_TRY(hipMemcpy(to.nodes, d.nodes, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    if (to.d2) HIP_TRY(hipMemcpy(to.d2, d.d2, sizeof(double) * B, hipMemcpyDeviceToHost));
    if (to.verdict) HIP_TRY(hipMemcpy(to.verdict, d.verdict, sizeof(int32_t) * nd, hipMemcpyDeviceToHost));
    if (to.slot) HIP_TRY(hipMemcpy(to.slot, d.slot, sizeof(int32_t) * nd, hipMemcpyDeviceToHost));
    if (to.ncand) HIP_TRY(hipMemcpy(to.ncand, d.ncand, sizeof(int32_t) * nd, hipMemcpyDeviceToHost));
    if (to.det) HIP_TRY(hipMemcpy(to.det, d.det, sizeof(double) * nd * slam::kAssocDetLen, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

// one jointly associated timestep once the message and the commands are on the device
int step_joint_now(slam_handle* h, const slam_joint_config& c, const float cmd[2], const float* d_cmd_each, const float* d_meas,
                   const int32_t* d_count, int k_stride, double* rec, int32_t* n_drop) {
    const size_t B = (size_t)h->B;
    TRY(joint_reserve(h, k_stride, 1));
    JointDev d = joint_rows(h, B, 0);
    int32_t* const drop = d.n_drop;
    d = JointDev{nullptr, nullptr, drop, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    TRY(joint_launch(h, c, cmd, d_cmd_each, d_meas, d_count, k_stride, h->joint.dmeas, h->joint.dcount, h->inn.drec, d));
    TRY(launch_step(h, cmd, 0, h->joint.dmeas, h->joint.dcount, k_stride, d_cmd_each));
    if (!rec && !n_drop) return SLAM_OK;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (rec) HIP_TRY(hipMemcpy(rec, h->inn.drec, sizeof(double) * slam::kInnovRecLen, hipMemcpyDeviceToHost));
    if (n_drop) HIP_TRY(hipMemcpy(n_drop, drop, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

}  // namespace

extern "C" {

int slam_joint_config_default(slam_joint_config* c) {
    if (!c) return slam_internal_fail(SLAM_ERR_ARG, "cfg is NULL");
    memset(c, 0, sizeof(*c));
    c->gate_match = -2.0 * log(0.01);
    c->gate_new = -2.0 * log(1e-6);
    // the 0.99 quantiles of chi-square with 2, 4, ..., 32 degrees of freedom (mpmath, 50 digits, rounded to nearest)
    static const double q[slam::kJointMaxPair] = {
        9.210340371976184, 13.276704135987625, 16.81189382977093, 20.090235029663233, 23.20925115895436, 26.21696730553585,
        29.141237740672796, 31.99992690881518, 34.80530573470507, 37.56623478662505, 40.289360437593864, 42.97982013935164,
        45.64168266628315, 48.2782357703155, 50.89218131151709, 53.485771836235365};
    for (int i = 0; i < slam::kJointMaxPair; ++i) c->gate_joint[i] = q[i];
    c->gate_joint[0] = c->gate_match;   // (the same quantile as the closed form has it, one ulp below the literal)
    c->max_nodes = 2048;
    return SLAM_OK;
}

int slam_associate_joint(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                         int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, int32_t* verdict,
                         int32_t* slot, double* det, float* meas_out, int32_t* count_out, double* d2_joint, int32_t* nodes, int32_t* ncand) {
    slam_joint_config c;
    TRY(joint_args(cfg, cmds, meas, count, k_stride, meas_out, count_out, false, &c));
    TRY(assoc_enter(h));
    const size_t B = (size_t)h->B, nm = 3 * (size_t)k_stride * B;
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * B));
    TRY(joint_reserve(h, k_stride, 1));
    // (slots the kernel does not write keep what the caller gave: the output row starts as the input row)
    HIP_TRY(hipMemcpyAsync(h->joint.dmeas, h->inn.dmeas, sizeof(float) * nm, hipMemcpyDeviceToDevice, h->stream));
    TRY(joint_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, h->joint.dmeas,
                  h->joint.dcount, {rec, n_match, n_new, n_drop, flags, verdict, slot, det, d2_joint, nodes, ncand}));
    if (meas_out) HIP_TRY(hipMemcpy(meas_out, h->joint.dmeas, sizeof(float) * nm, hipMemcpyDeviceToHost));
    if (count_out) HIP_TRY(hipMemcpy(count_out, h->joint.dcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost));
    return SLAM_OK;
}

int slam_associate_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                             int32_t* verdict, int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out, double* d2_joint, int32_t* nodes,
                             int32_t* ncand) {
    slam_joint_config c;
    TRY(joint_args(cfg, cmds, d_meas, d_count, k_stride, d_meas_out, d_count_out, true, &c));
    TRY(assoc_enter(h));
    const size_t B = (size_t)h->B, bm = sizeof(float) * 3 * (size_t)k_stride * B, bc = sizeof(int32_t) * B;
    if ((d_meas_out != d_meas && assoc_overlap(d_meas_out, bm, d_meas, bm)) || (d_count_out != d_count && assoc_overlap(d_count_out, bc, d_count, bc)) ||
        assoc_overlap(d_meas_out, bm, d_count, bc) || assoc_overlap(d_count_out, bc, d_meas, bm) || assoc_overlap(d_meas_out, bm, d_count_out, bc))
        return slam_internal_fail(SLAM_ERR_ARG, "the output message overlaps the input (only d_meas_out == d_meas with d_count_out == d_count is allowed) or itself");
    TRY(joint_reserve(h, 1, 1));
    return joint_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, d_meas_out, d_count_out,
                     {rec, n_match, n_new, n_drop, flags, verdict, slot, det, d2_joint, nodes, ncand});
}

int slam_step_associated_joint(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas,
                               const int32_t* count, int k_stride, double rec[16], int32_t* n_drop) {
    slam_joint_config c;
    TRY(joint_args(cfg, cmds, meas, count, k_stride, nullptr, nullptr, false, &c));
    TRY(assoc_enter(h));
    TRY(assoc_step_state(h, "a jointly associated step"));
    TRY(upload_messages(h, meas, count, k_stride, 1));
    if (cmd_each) TRY(innovation_upload_cmds(h, cmds, 2 * (size_t)h->B));
    return step_joint_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? h->inn.dcmd.get() : nullptr, h->inn.dmeas, h->inn.dcount, k_stride, rec, n_drop);
}

int slam_step_associated_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                                   const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop) {
    slam_joint_config c;
    TRY(joint_args(cfg, cmds, d_meas, d_count, k_stride, nullptr, nullptr, false, &c));
    TRY(assoc_enter(h));
    TRY(assoc_step_state(h, "a jointly associated step"));
    return step_joint_now(h, c, cmd_each ? kNoCmd : cmds, cmd_each ? cmds : nullptr, d_meas, d_count, k_stride, rec, n_drop);
}

}  // extern "C"

namespace {

// slam_associate_joint_run and its _sim form once their arguments are in order: T ticks with the commands of `csrc` on the messages of `msgs`
int joint_run(slam_handle* h, const char* who, const slam_joint_config& c, TickCmds::Source csrc, const float* cmds, TickMsgs& msgs, int T,
              double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint, int32_t* nodes) {
    const int k_stride = msgs.k_stride;
    TRY(run_enter(h, who, msgs.sim(), csrc == TickCmds::kNav, true));
    if (T == 0) return SLAM_OK;
    HIP_TRY(hipSetDevice(h->device));
    const size_t B = (size_t)h->B;
    TickCmds tcmd;
    TRY(tcmd.init(h, csrc, cmds));
    // what a tick holds on the device: its rows of the counts and distances, of the commands (cmd_each) and of the messages
    const double per_tick = (7.0 * 4.0 + 8.0) * (double)B + tcmd.bytes_per_tick(h) + msgs.bytes_per_tick(h, tcmd);
    const int chunk = slam_host::ticks_per_chunk(T, per_tick, slam_host::tick_log_budget());
    TRY(joint_reserve(h, k_stride, (size_t)chunk));
    TRY(msgs.reserve(h, tcmd, chunk));
    const size_t cb = (size_t)chunk * B;
    const int rc = run_chunked(
        h, T, chunk, h->nav.time_ticks, h->joint.times,
        [&](int t0, int tc) -> int {
            TRY(tcmd.upload(h, t0, tc));
            return msgs.upload(h, t0, tc);
        },
        [&](int t0, int t, auto mark) -> int {
            const float *cmd, *d_each, *dm;
            const int32_t* dc;
            TRY(tcmd.select(h, t0, t, &cmd, &d_each));
            TRY(msgs.produce(h, tcmd, t, cmd, d_each, &dm, &dc));
            const size_t o = (size_t)t * B;
            TRY(mark([&] {
                return joint_launch(h, c, cmd, d_each, dm, dc, k_stride, h->joint.dmeas, h->joint.dcount,
                                    h->inn.drec + (size_t)t * slam::kInnovRecLen, joint_rows(h, cb, o));
            }));
            TRY(launch_step(h, cmd, 0, h->joint.dmeas, h->joint.dcount, k_stride, d_each));
            return msgs.commit(h, t);
        },
        [&](int t0, int tc) -> int {
            const size_t nb = sizeof(int32_t) * (size_t)tc * B, o = (size_t)t0 * B;
            TRY(msgs.download(h, tcmd, t0, tc));
            const int32_t* const di = h->joint.dint;
            TRY(joint_sum_work(h, (size_t)tc, cb));   // (after the chunk's events: it is no part of the run's times)
            if (recs) HIP_TRY(hipMemcpy(recs + (size_t)t0 * slam::kInnovRecLen, h->inn.drec, sizeof(double) * (size_t)tc * slam::kInnovRecLen, hipMemcpyDeviceToHost));
            if (n_match) HIP_TRY(hipMemcpy(n_match + o, di, nb, hipMemcpyDeviceToHost));
            if (n_new) HIP_TRY(hipMemcpy(n_new + o, di + cb, nb, hipMemcpyDeviceToHost));
            if (n_drop) HIP_TRY(hipMemcpy(n_drop + o, di + 2 * cb, nb, hipMemcpyDeviceToHost));
            if (flags) HIP_TRY(hipMemcpy(flags + o, di + 3 * cb, nb, hipMemcpyDeviceToHost));
            if (nodes) HIP_TRY(hipMemcpy(nodes + o, di + 5 * cb, nb, hipMemcpyDeviceToHost));
            if (d2_joint) HIP_TRY(hipMemcpy(d2_joint + o, h->joint.dd2, sizeof(double) * (size_t)tc * B, hipMemcpyDeviceToHost));
            return SLAM_OK;
        });
    TRY(rc);
    HIP_TRY(hipStreamSynchronize(h->stream));
    return joint_read_work(h);
}

}  // namespace

extern "C" {

int slam_associate_joint_run(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                             int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint,
                             int32_t* nodes) {
    slam_joint_config c;
    TRY(joint_config(cfg, &c));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (!cmds) return slam_internal_fail(SLAM_ERR_ARG, "cmds is NULL");
    if (!meas || !count) return slam_internal_fail(SLAM_ERR_ARG, "meas or meas_count is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_log(meas, count, k_stride);
    return joint_run(h, "slam_associate_joint_run", c, cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T, recs, n_match, n_new, n_drop, flags,
                     d2_joint, nodes);
}

int slam_associate_joint_run_sim(slam_handle* h, const slam_joint_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                                 int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint, int32_t* nodes,
                                 const slam_sense_log* log) {
    slam_joint_config c;
    TickCmds::Source csrc;
    TRY(joint_config(cfg, &c));
    TRY(sim_run_source(source, cmds, &csrc));
    if (T < 0) return slam_internal_fail(SLAM_ERR_ARG, "T = %d is negative", T);
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    TickMsgs msgs;
    msgs.init_sim(log, k_stride);
    return joint_run(h, "slam_associate_joint_run_sim", c, csrc, cmds, msgs, T, recs, n_match, n_new, n_drop, flags, d2_joint, nodes);
}

int slam_last_joint_work(slam_handle* h, double* bytes, double* joint_ms, double* total_ms) {
    if (!h) return slam_internal_fail(SLAM_ERR_ARG, "NULL handle");
    if (h->joint.bytes < 0.0)
        return slam_internal_fail(SLAM_ERR_STATE, "slam_associate_joint, slam_associate_joint_dev or slam_associate_joint_run has not run on this handle");
    if (bytes) { bytes[0] = h->joint.bytes; bytes[1] = h->joint.lines; }
    if (joint_ms) *joint_ms = h->joint.times.part_ms;
    if (total_ms) *total_ms = h->joint.times.total_ms;
    return SLAM_OK;
}

int slam_associate_joint_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                       const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                       const slam_joint_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                                       double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out, double* d2_joint,
                                       int32_t* nodes, int32_t* ncand) {
    (void)lm_from_pred;   // (no update precedes a cost: x_pred and x_t hold the same landmark positions)
    slam_joint_config c;
    TRY(joint_config(cfg, &c));
    if (!x || !P || !cmd || !noise) return slam_internal_fail(SLAM_ERR_ARG, "NULL argument");
    if (L_max < 0 || M < 0 || M > L_max) return slam_internal_fail(SLAM_ERR_ARG, "M = %d is not in [0, L_max = %d]", M, L_max);
    if (M > 0 && !ids) return slam_internal_fail(SLAM_ERR_ARG, "ids is NULL");
    if (k_stride <= 0) return slam_internal_fail(SLAM_ERR_ARG, "k_stride = %d is not positive", k_stride);
    if (count > 0 && !meas) return slam_internal_fail(SLAM_ERR_ARG, "meas is NULL");
    if (const char* f = slam_host::noise_bad_field(*noise)) return slam_internal_fail(SLAM_ERR_ARG, "noise: %s is not finite", f);
    const slam::InnovNoise nz = {noise->v_d, noise->v_th, noise->w_r, noise->w_b, noise->V_00, noise->V_11, noise->W_00, noise->W_11};
    const int n = 3 + 2 * M;
    std::vector<slam::JointWork> ws(1);
    const bool f32 = f32_storage != 0;
    const slam::JointResult v = slam::joint_instance_host(
        ws[0], [&](int i) { return f32 ? (double)(float)x[i] : x[i]; },
        [&](int r, int cc) { const double e = P[(size_t)r * n + cc]; return f32 ? (double)(float)e : e; }, ids, M, L_max, status, cmd[0], cmd[1], meas,
        count, k_stride, nz, c.gate_match, c.gate_new, c.gate_joint, c.max_nodes, cost, verdict, slot, det, ncand, meas_out, count_out);
    if (rec) slam::joint_record(v, rec);
    if (n_match) *n_match = v.n_match;
    if (n_new) *n_new = v.n_new;
    if (n_drop) *n_drop = v.n_drop;
    if (flags) *flags = v.flags;
    if (d2_joint) *d2_joint = v.d2_joint;
    if (nodes) *nodes = v.nodes;
    return SLAM_OK;
}

}  // extern "C"
