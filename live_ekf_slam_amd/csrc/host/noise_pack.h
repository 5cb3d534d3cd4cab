// noise_pack.h - host side of slam_set_noise_each: validation of the caller's rows and their packing into what the step kernels read.
// No HIP: included by the C ABI units (slam_capi.cpp, capi_innovation.cpp, capi_gate.cpp) and by a stand-alone sanitizer driver (tests/test_noise_each_capi.py).
#pragma once
#include <math.h>
#include <stddef.h>

#include "../../../include/slam_batch.h"
#include "../noise_row.h"

namespace slam_host {

// the row that reproduces a handle without rows: filter and simulator fields both from the config
inline void noise_from_config(const slam_config& c, slam_noise* out) {
    out->v_d = c.v_d; out->v_th = c.v_th; out->w_r = c.w_r; out->w_b = c.w_b;
    out->V_00 = c.V_00; out->V_11 = c.V_11; out->W_00 = c.W_00; out->W_11 = c.W_11;
    out->sim_V_00 = c.V_00; out->sim_V_11 = c.V_11; out->sim_W_00 = c.W_00; out->sim_W_11 = c.W_11;
}

// name of the first non-finite field of a row, NULL if every field is finite (the only value check: the reference has none)
inline const char* noise_bad_field(const slam_noise& r) {
    static const char* const names[12] = {"v_d", "v_th", "w_r", "w_b", "V_00", "V_11", "W_00", "W_11", "sim_V_00", "sim_V_11", "sim_W_00", "sim_W_11"};
    const double v[12] = {r.v_d, r.v_th, r.w_r, r.w_b, r.V_00, r.V_11, r.W_00, r.W_11, r.sim_V_00, r.sim_V_11, r.sim_W_00, r.sim_W_11};
    for (int i = 0; i < 12; ++i)
        if (!isfinite(v[i])) return names[i];
    return nullptr;
}

// One row as the kernels read it: the EFFECTIVE V / W, mapped as fill_ekf_params / fill_ukf_params map slam_config (filter.h:116-117:
// with the quirk W_00 / W_11 land in V and W stays I2).
inline slam::NoiseRow noise_pack_row(const slam_noise& r, int replicate_vw_quirk) {
    slam::NoiseRow o;
    if (replicate_vw_quirk) { o.V00 = r.W_00; o.V11 = r.W_11; o.W00 = 1.0; o.W11 = 1.0; }
    else { o.V00 = r.V_00; o.V11 = r.V_11; o.W00 = r.W_00; o.W11 = r.W_11; }
    o.sV00 = r.sim_V_00; o.sV11 = r.sim_V_11; o.sW00 = r.sim_W_00; o.sW11 = r.sim_W_11;
    o.v_d = r.v_d; o.v_th = r.v_th; o.w_r = r.w_r; o.w_b = r.w_b;
    return o;
}

// rows [n] -> out [n].  0 = packed; 1 = row *bad_inst has the non-finite field *bad_field (out is then unspecified)
inline int noise_pack(const slam_noise* rows, size_t n, int replicate_vw_quirk, slam::NoiseRow* out, size_t* bad_inst, const char** bad_field) {
    for (size_t b = 0; b < n; ++b) {
        if (const char* f = noise_bad_field(rows[b])) { *bad_inst = b; *bad_field = f; return 1; }
        out[b] = noise_pack_row(rows[b], replicate_vw_quirk);
    }
    return 0;
}

}  // namespace slam_host
