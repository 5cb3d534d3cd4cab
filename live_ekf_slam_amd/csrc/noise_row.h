// noise_row.h - one instance's row of slam_set_noise_each as the step kernels read it (EkfStepParams / UkfStepParams::noise_each).
#pragma once

namespace slam {

// Packed by the host (host/noise_pack.h) from a slam_noise: V / W are the EFFECTIVE values (replicate_vw_quirk applied, as for the
// scalars of the parameter blocks), so no kernel has a quirk branch.  80 bytes, 8-byte aligned.
struct NoiseRow {
    double V00, V11, W00, W11;       // filter: effective process / measurement noise
    double sV00, sV11, sW00, sW11;   // simulator: half-widths of get_cmd's uniform draws (sim_node.py:216-217,247-248)
    float v_d, v_th, w_r, w_b;       // filter: noise means
};

}  // namespace slam
