// What the key-figure kernel (eepacc_kpis.hip) reads of a settings class.  Plain data, no HIP: the host translation of the
// settings (eepacc_cfg.cpp) fills it, eepacc_kpis.h hands it to the kernel.
#ifndef EEPACC_KPIS_CFG_H
#define EEPACC_KPIS_CFG_H

#include <stdint.h>
#include "eepacc_device.h"

namespace eepacc {

// A table of the handle's own, KpiCfg[n_classes], beside DevCfg (whose layout and the kernels that take it stay as they are).
struct KpiCfg {
    double Ts;                    // Tvec[0]
    double phi;                   // rpm = 30 / pi * v * phi
    double b5[21];                // fifth-order power surface
    double lm, F0, F2, R_w;       // wheel torque TW = max(0, (lambda m a + F0 + F2 v^2) R_w); lm = lambda * m
    double p00, p10, p01;         // fuel flow FC = max(0.25, p00 + p10 v + p01 TW) [g/s]
    int32_t n_speedLim, pad;
    double s_speedLim[kMaxKnots], v_speedLim[kMaxKnots];
};

}  // namespace eepacc
#endif
