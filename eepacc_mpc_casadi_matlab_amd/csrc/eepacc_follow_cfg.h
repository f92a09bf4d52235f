// What the vehicle-following / cost key-figure kernel (eepacc_follow.hip) reads of a settings class.  Plain data, no HIP:
// the host translation of the settings (eepacc_cfg.cpp) fills it, eepacc_follow.h hands it to the kernel.
#ifndef EEPACC_FOLLOW_CFG_H
#define EEPACC_FOLLOW_CFG_H

namespace eepacc {

// A table of the handle's own, FollowCfg[n_classes], beside DevCfg and KpiCfg (whose layouts and the kernels that take them
// stay as they are).
struct FollowCfg {
    double Ts;                    // Tvec[0]
    double h_min, tau_min;        // minimum-headway policy max(h_min, v tau_min), ABO/Main.m:687
    double phi;                   // rpm = 30 / pi * v * phi
    double b5[21];                // fifth-order power surface
    double w[3][7];               // [EEPACC_FKPI_W_*][w_P, w_a, w_j, w_v, w_h, w_s, w_f]
};

}  // namespace eepacc
#endif
