// nav_kernel.h — the pure-pursuit / direct controller of the reference's goal_pursuit_node, one tick for every instance (slam_nav_run, gfx950).
//
// A restatement of PurePursuit.get_next_cmd, pare_path, choose_lookahead_pt, cmd_loose, cmd_tight and direct_nav
// (ekf_ws/src/planning_pkg/src/pure_pursuit.py:17-161) as goal_pursuit_node.py:23-50 calls them for nav_method "pp" and "direct".
// nav_tick() below is THE definition: the device kernel (nav_kernel.hip) and every host caller compile this one function, with
// -ffp-contract=off on both sides, so the two give the same bits; live_ekf_slam_amd/navigation.py restates it once more in numpy.
//
// Arithmetic is fp64 throughout.  Python's `x**2` on floats is the exact product and `**(1/2)` is taken as sqrt; the higher powers are
// multiplication chains (x^4 = (x x)(x x), x^12 = x^8 x^4 by squaring, the cube of direct_nav x x x); atan2 is slam::det_atan2 (the
// library's one atan2, slam_math.h) and the heading error is IEEE remainder(., 2 pi).
//
// The queue of the reference (goal_queue, a Python list the controller deletes from) is always a suffix of the path it was given, since
// pare_path deletes [0, i] for the first i within 0.15 m and direct_nav pops the front: `head` is the index of the first waypoint still
// queued, and the queue is path[head .. P).
//
// Guards the reference lacks:
//   * consecutive equal waypoints (the reference divides by a = 0 in choose_lookahead_pt) are refused when the path is set;
//   * a non-finite estimate, or an instance frozen by SLAM_INST_INDEX_OOR, gets the command (0, 0) and its controller state is not touched
//     (the reference node would have died with the filter).
#pragma once
#include <stdint.h>

#include "slam_math.h"

namespace slam {

constexpr int kNavMaxWaypoints = 1024;   // P of one path (the shared path is staged in 16 KB of LDS)
constexpr int kNavMaxRadii = 64;         // lookahead radii a config may ask for (the reference's defaults give 11)
constexpr double kNavPareRadius = 0.15;  // pure_pursuit.py:91,159

enum NavMethod { kNavPP = 0, kNavDirect = 1 };
enum NavControl { kNavLoose = 0, kNavTight = 1 };

// controller state of one instance (pure_pursuit.py:11-14)
struct NavState {
    int32_t head;         // first waypoint still queued; == P: the queue is empty
    int32_t finish_tick;  // first tick whose command was issued with an empty queue, -1 before
    double integ, err_prev;
};

struct NavConsts {
    double dt, la_init, la_max, d_max, th_max;
    int32_t method, control;
};

// Command.msg: float32 fwd, ang after the clamps of pure_pursuit.py:79-80 / 156-157 (max(lo, min(v, hi)) with Python's argument order)
SLAM_HD void nav_clamp(double fwd, double ang, const NavConsts& c, float* out) {
    const double f = c.d_max < fwd ? c.d_max : fwd;
    const double a = c.th_max < ang ? c.th_max : ang;
    out[0] = (float)(f > 0.0 ? f : 0.0);
    out[1] = (float)(a > -c.th_max ? a : -c.th_max);
}

// One tick.  (ex, ey, eyaw): the wire values of the state message (float32 x_v, y_v, yaw_v) as doubles; path: P points (x, y);
// tick: the number of this tick since the controller state was reset.  Writes the float32 command.
template <class Path>
SLAM_HD void nav_tick(const NavConsts& c, const Path& path, int P, double ex, double ey, double eyaw, bool frozen, int tick, NavState& s, float* cmd) {
    cmd[0] = 0.f; cmd[1] = 0.f;
    if (frozen || !(fabs(ex) <= 1.79769313486231570815e308) || !(fabs(ey) <= 1.79769313486231570815e308) || !(fabs(eyaw) <= 1.79769313486231570815e308)) return;
    const double tau = kTwoPi, pi = 3.141592653589793;
    if (c.method == kNavDirect) {                                         // direct_nav, pure_pursuit.py:135-161
        if (s.head >= P) { if (s.finish_tick < 0) s.finish_tick = tick; return; }
        const double gx = path.x(s.head), gy = path.y(s.head);
        const double rx = ex - gx, ry = ey - gy;
        const double r = sqrt(rx * rx + ry * ry);
        const double gb = det_atan2(gy - ey, gx - ex);
        const double beta = remainder(gb - eyaw, tau);
        double fwd = 0.0;
        if (r > 0.1) { const double y = 1.0 - fabs(beta) / c.th_max; fwd = 1.0 * (y * y * y) + 0.05; }
        nav_clamp(fwd, beta, c, cmd);
        if (r < kNavPareRadius) { s.head += 1; if (s.head >= P && s.finish_tick < 0) s.finish_tick = tick + 1; }
        return;
    }
    // pare_path, pure_pursuit.py:85-94: cut up to the FIRST queued waypoint within 0.15 m, whichever it is
    for (int i = s.head; i < P; ++i) {
        const double dx = ex - path.x(i), dy = ey - path.y(i);
        if (sqrt(dx * dx + dy * dy) < kNavPareRadius) { s.head = i + 1; break; }
    }
    if (s.head >= P) { if (s.finish_tick < 0) s.finish_tick = tick; return; }   // pure_pursuit.py:49-51
    // lookahead point, pure_pursuit.py:54-63 and choose_lookahead_pt 98-131
    const int head = s.head;
    double lx = path.x(head), ly = path.y(head);                          // one queued point, or nothing found: the head waypoint
    if (P - head > 1) {
        bool found = false;
        double dist = c.la_init;
        while (!found && dist <= c.la_max) {
            double px = path.x(head), py = path.y(head);
            for (int i = head + 1; i < P; ++i) {                          // the last segment with a valid root wins
                const double qx = path.x(i), qy = path.y(i);
                const double dfx = qx - px, dfy = qy - py;
                const double vx = px - ex, vy = py - ey;
                const double a = dfx * dfx + dfy * dfy;
                const double b = 2.0 * (vx * dfx + vy * dfy);
                const double cc = vx * vx + vy * vy - dist * dist;
                const double arg = b * b - 4.0 * a * cc;
                if (!(arg < 0.0)) {                                       // math.sqrt raises for a negative argument only: `continue`
                    const double discr = sqrt(arg);
                    const double q0 = (-b - discr) / (2.0 * a), q1 = (-b + discr) / (2.0 * a);
                    if (q0 >= 0.0 && q0 <= 1.0) { lx = px + q0 * dfx; ly = py + q0 * dfy; found = true; }
                    else if (q1 >= 0.0 && q1 <= 1.0) { lx = px + q1 * dfx; ly = py + q1 * dfy; found = true; }
                }
                px = qx; py = qy;
            }
            dist *= 1.25;
        }
        if (!found) { lx = path.x(head); ly = path.y(head); }
    }
    const double gb = det_atan2(ly - ey, lx - ex);
    const double beta = remainder(gb - eyaw, tau);
    s.integ += beta * c.dt;
    const double x = 1.0 - fabs(beta / pi);
    const double x2 = x * x, x4 = x2 * x2;
    double fwd, ang;
    if (c.control == kNavTight) {                                         // cmd_tight, pure_pursuit.py:28-37
        const double Pt = 0.5 * beta, I = 0.0 * s.integ, D = 0.0 * (beta - s.err_prev) / c.dt;
        ang = Pt + I + D;
        const double x8 = x4 * x4;
        fwd = 0.02 * (x8 * x4) + 0.01;
    } else {                                                              // cmd_loose, pure_pursuit.py:17-26
        const double Pt = 0.9 * beta, I = 0.01 * s.integ, D = 0.4 * (beta - s.err_prev) / c.dt;
        ang = Pt + I + D;
        fwd = x4 + 0.05;
    }
    s.err_prev = beta;
    nav_clamp(fwd, ang, c, cmd);
}

// a path as nav_tick reads it: interleaved (x, y) doubles
struct NavPathView {
    const double* pts;
    SLAM_HD double x(int i) const { return pts[2 * i]; }
    SLAM_HD double y(int i) const { return pts[2 * i + 1]; }
};

#if defined(__HIPCC__)
// One controller tick of every instance on `stream`.  Reads x_t straight from the handle's state buffer, writes [B][2] commands.
struct NavParams {
    const void* x;            // [B][xstride] x_t, fp64 or fp32 storage
    const int32_t* flags;     // [B] slam_instance_flags
    const double* path;       // shared: [P][2]; per instance: [B][path_stride][2]
    const int32_t* P_each;    // per instance: [B] waypoints; NULL = the shared path of P points
    int32_t P, path_stride;
    int32_t B, xstride;
    int32_t ukf;              // x_t = (x, y, cos yaw, sin yaw, ...): yaw_v as ukf.cpp:71
    int32_t tick;
    NavConsts c;
    // controller state, [B] each
    int32_t* head; int32_t* finish_tick; double* integ; double* err_prev;
    float* cmd_out;           // [B][2], read by the step launch that follows
    float* cmd_log;           // [B][2] row of the log, or NULL
};
hipError_t launch_nav_tick(const NavParams& p, int f32_storage, hipStream_t stream);
#endif

}  // namespace slam
