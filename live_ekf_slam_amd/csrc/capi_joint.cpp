// capi_joint.cpp — C ABI: joint-compatibility association (JCBB) of detections without ids (joint_kernel.hip).  The argument checks, the
// handle's entry and the staging are those of capi_filter.h, the traffic readers those of capi_assoc.h.
#include <math.h>
#include <string.h>

#include <vector>

#include "capi_assoc.h"
#include "ekf_kernel.h"
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

// the rows of joint.dint, [kJointRows][ticks][B]: the association's five, the nodes and the on-demand blocks
enum JointRow { kJointNodes = kAssocRows, kJointBlk = kAssocRows + 1, kJointRows = kAssocRows + 2 };

// the per-instance outputs of one joint association on the device (the rows, [ticks][B] distances; the detection slots when asked for)
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
    TRY(grow(h, h->joint.dint, kJointRows * ticks * B));
    TRY(grow(h, h->joint.dd2, ticks * B));
    TRY(grow(h, h->joint.dwork, 3));
    TRY(innovation_reserve(h, false));
    TRY(grow(h, h->inn.drec, ticks * slam::kInnovRecLen));
    HIP_TRY(hipMemsetAsync(h->joint.dwork, 0, 3 * sizeof(unsigned long long), h->stream));
    return SLAM_OK;
}

// the [kJointRows][stride] rows of dint and the distances at tick offset o
JointDev joint_rows(slam_handle* h, size_t stride, size_t o) {
    int32_t* const di = h->joint.dint;
    return JointDev{row(di, kAssocMatch, stride, o), row(di, kAssocNew, stride, o), row(di, kAssocDrop, stride, o), row(di, kAssocFlags, stride, o),
                    row(di, kAssocLm, stride, o), row(di, kJointNodes, stride, o), row(di, kJointBlk, stride, o), h->joint.dd2 + o,
                    nullptr, nullptr, nullptr, nullptr};
}

// the traffic model of `ticks` associations whose counts are in dint, summed on the stream
int joint_sum_work(slam_handle* h, size_t ticks, size_t stride) {
    const JointDev d = joint_rows(h, stride, 0);
    HIP_TRY(slam::launch_associate_joint_work(d.n_lm, d.n_match, d.n_new, d.n_drop, d.n_blk, ticks * (size_t)h->B, h->esz, h->joint.dwork, h->stream));
    return SLAM_OK;
}

struct JointOut { double* rec; int32_t *n_match, *n_new, *n_drop, *flags, *verdict, *slot; double* det; double* d2; int32_t *nodes, *ncand; };

// slam_associate_joint (host: the message and per-instance commands are host arrays) and slam_associate_joint_dev
int associate_joint(slam_handle* h, bool host, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                    int k_stride, float* meas_out, int32_t* count_out, const JointOut& to) {
    slam_joint_config c;
    const float *cmd, *d_each;
    TRY(joint_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride, meas_out, count_out, !host));
    TRY(filter_enter(h, assoc_supported));
    DevMsg out = {meas_out, count_out};
    if (!host) TRY(out_message_overlaps(h, meas, count, k_stride, out));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(joint_reserve(h, host ? k_stride : 1, 1));
    if (host) {
        out = {h->joint.dmeas, h->joint.dcount};
        TRY(seed_out_message(h, out.meas, k_stride));
    }
    const size_t B = (size_t)h->B, nd = B * slam::kInnovMaxDet, nm = 3 * (size_t)k_stride * B;
    if (to.verdict) TRY(grow(h, h->joint.dverdict, nd));
    if (to.slot) TRY(grow(h, h->joint.dslot, nd));
    if (to.ncand) TRY(grow(h, h->joint.dncand, nd));
    if (to.det) TRY(grow(h, h->joint.ddet, nd * slam::kAssocDetLen));
    JointDev d = joint_rows(h, B, 0);
    d.verdict = to.verdict ? h->joint.dverdict.get() : nullptr; d.slot = to.slot ? h->joint.dslot.get() : nullptr;
    d.ncand = to.ncand ? h->joint.dncand.get() : nullptr; d.det = to.det ? h->joint.ddet.get() : nullptr;
    TRY(joint_launch(h, c, cmd, d_each, meas, count, k_stride, out.meas, out.count, h->inn.drec, d));
    TRY(joint_sum_work(h, 1, B));
    HIP_TRY(hipStreamSynchronize(h->stream));
    TRY(read_traffic(h, h->joint));
    return copy_rows({{h->inn.drec, to.rec, slam::kInnovRecLen}, {d.n_match, to.n_match, B}, {d.n_new, to.n_new, B}, {d.n_drop, to.n_drop, B},
                      {d.flags, to.flags, B}, {d.nodes, to.nodes, B}, {d.d2, to.d2, B}, {d.verdict, to.verdict, nd}, {d.slot, to.slot, nd},
                      {d.ncand, to.ncand, nd}, {d.det, to.det, nd * slam::kAssocDetLen}, {out.meas, host ? meas_out : nullptr, nm},
                      {out.count, host ? count_out : nullptr, B}}, 0, 1);
}

// slam_step_associated_joint (host: as above) and its _dev form: one jointly associated timestep
int step_joint(slam_handle* h, bool host, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
               int k_stride, double* rec, int32_t* n_drop) {
    slam_joint_config c;
    const float *cmd, *d_each;
    TRY(joint_config(cfg, &c));
    TRY(message_args(cmds, meas, count, k_stride));
    TRY(filter_enter(h, assoc_supported));
    TRY(step_state(h, "a jointly associated step"));
    TRY(stage_message(h, host, cmds, cmd_each, &meas, &count, k_stride, &cmd, &d_each));
    TRY(joint_reserve(h, k_stride, 1));
    JointDev d = {};
    d.n_drop = joint_rows(h, (size_t)h->B, 0).n_drop;
    TRY(joint_launch(h, c, cmd, d_each, meas, count, k_stride, h->joint.dmeas, h->joint.dcount, h->inn.drec, d));
    TRY(launch_step(h, cmd, 0, h->joint.dmeas, h->joint.dcount, k_stride, d_each));
    return step_outputs(h, rec, d.n_drop, n_drop);
}

// slam_associate_joint_run as run_filtered's feature
struct JointTicks {
    slam_handle* h; const slam_joint_config& c;
    double* recs; int32_t *n_match, *n_new, *n_drop, *flags; double* d2_joint; int32_t* nodes;
    size_t B = 0, cb = 0;   // (set by reserve: the handle is checked by then)

    RunTimes& times() const { return h->joint.times; }
    double bytes_per_tick() const { return (kJointRows * 4.0 + 8.0) * (double)h->B; }
    int reserve(int k_stride, int chunk) {
        B = (size_t)h->B; cb = (size_t)chunk * B;
        return joint_reserve(h, k_stride, (size_t)chunk);
    }
    int chunk_begin() { return SLAM_OK; }
    DevMsg out() const { return {h->joint.dmeas, h->joint.dcount}; }
    template <class Mark>
    int filter(int t, const float* cmd, const float* d_each, const float* dm, const int32_t* dc, int k_stride, Mark mark) {
        return mark([&] {
            return joint_launch(h, c, cmd, d_each, dm, dc, k_stride, out().meas, out().count, h->inn.drec + (size_t)t * slam::kInnovRecLen,
                                joint_rows(h, cb, (size_t)t * B));
        });
    }
    template <class Mark> int after_step(int, int, Mark) { return SLAM_OK; }
    int chunk_done(int, int tc) { return joint_sum_work(h, (size_t)tc, cb); }
    std::vector<TickRow> rows() const {
        const JointDev d = joint_rows(h, cb, 0);
        return {{h->inn.drec, recs, slam::kInnovRecLen}, {d.n_match, n_match, B}, {d.n_new, n_new, B}, {d.n_drop, n_drop, B}, {d.flags, flags, B},
                {d.nodes, nodes, B}, {d.d2, d2_joint, B}};
    }
    int finish() {
        HIP_TRY(hipStreamSynchronize(h->stream));
        return read_traffic(h, h->joint);
    }
};

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
    return associate_joint(h, true, cfg, cmds, cmd_each, meas, count, k_stride, meas_out, count_out,
                           {rec, n_match, n_new, n_drop, flags, verdict, slot, det, d2_joint, nodes, ncand});
}

int slam_associate_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                             const int32_t* d_count, int k_stride, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                             int32_t* verdict, int32_t* slot, double* det, float* d_meas_out, int32_t* d_count_out, double* d2_joint, int32_t* nodes,
                             int32_t* ncand) {
    return associate_joint(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, d_meas_out, d_count_out,
                           {rec, n_match, n_new, n_drop, flags, verdict, slot, det, d2_joint, nodes, ncand});
}

int slam_step_associated_joint(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas,
                               const int32_t* count, int k_stride, double rec[16], int32_t* n_drop) {
    return step_joint(h, true, cfg, cmds, cmd_each, meas, count, k_stride, rec, n_drop);
}

int slam_step_associated_joint_dev(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* d_meas,
                                   const int32_t* d_count, int k_stride, double rec[16], int32_t* n_drop) {
    return step_joint(h, false, cfg, cmds, cmd_each, d_meas, d_count, k_stride, rec, n_drop);
}

int slam_associate_joint_run(slam_handle* h, const slam_joint_config* cfg, const float* cmds, int cmd_each, const float* meas, const int32_t* count,
                             int k_stride, int T, double* recs, int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint,
                             int32_t* nodes) {
    slam_joint_config c;
    TickMsgs msgs;
    TRY(joint_config(cfg, &c));
    TRY(run_args_log(cmds, meas, count, k_stride, T, &msgs));
    return run_filtered(h, "slam_associate_joint_run", cmd_each ? TickCmds::kEach : TickCmds::kShared, cmds, msgs, T,
                        JointTicks{h, c, recs, n_match, n_new, n_drop, flags, d2_joint, nodes});
}

int slam_associate_joint_run_sim(slam_handle* h, const slam_joint_config* cfg, int source, const float* cmds, int k_stride, int T, double* recs,
                                 int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags, double* d2_joint, int32_t* nodes,
                                 const slam_sense_log* log) {
    slam_joint_config c;
    TickCmds::Source csrc;
    TickMsgs msgs;
    TRY(joint_config(cfg, &c));
    TRY(run_args_sim(source, cmds, k_stride, T, log, &csrc, &msgs));
    return run_filtered(h, "slam_associate_joint_run_sim", csrc, cmds, msgs, T, JointTicks{h, c, recs, n_match, n_new, n_drop, flags, d2_joint, nodes});
}

int slam_last_joint_work(slam_handle* h, double* bytes, double* joint_ms, double* total_ms) {
    return last_traffic_work(h ? &h->joint : nullptr, "slam_associate_joint, slam_associate_joint_dev or slam_associate_joint_run", bytes, joint_ms,
                             total_ms);
}

int slam_associate_joint_instance_host(const double* x, const double* P, const int32_t* ids, int M, int L_max, int32_t status, const float cmd[2],
                                       const float* meas, int count, int k_stride, const slam_noise* noise, int lm_from_pred, int f32_storage,
                                       const slam_joint_config* cfg, double rec[16], int32_t* n_match, int32_t* n_new, int32_t* n_drop, int32_t* flags,
                                       double* cost, int32_t* verdict, int32_t* slot, double* det, float* meas_out, int32_t* count_out, double* d2_joint,
                                       int32_t* nodes, int32_t* ncand) {
    (void)lm_from_pred;   // (no update precedes a cost: x_pred and x_t hold the same landmark positions)
    slam_joint_config c;
    InstanceHostArgs a;
    TRY(joint_config(cfg, &c));
    TRY(a.init(x, P, ids, M, L_max, cmd, meas, count, k_stride, true, noise, f32_storage));
    std::vector<slam::JointWork> ws(1);
    const slam::JointResult v = slam::joint_instance_host(ws[0], a.load_x, a.load_P, ids, M, L_max, status, cmd[0], cmd[1], meas, count, k_stride, a.nz,
                                                          c.gate_match, c.gate_new, c.gate_joint, c.max_nodes, cost, verdict, slot, det, ncand,
                                                          meas_out, count_out);
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
