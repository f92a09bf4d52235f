// What the route-compliance key-figure kernel (eepacc_route.hip) reads of a settings class.  Plain data, no HIP: the host
// translation of the settings (eepacc_cfg.cpp) fills it, eepacc_route.h hands it to the kernel.
#ifndef EEPACC_ROUTE_CFG_H
#define EEPACC_ROUTE_CFG_H

#include <stdint.h>
#include "eepacc_device.h"        // kMaxKnots, kMaxStops, kMaxTL

namespace eepacc {

// A table of the handle's own, RouteCfg[n_classes], beside DevCfg, KpiCfg and FollowCfg (whose layouts and the kernels that
// take them stay as they are).
struct RouteCfg {
    double Ts;                                               // Tvec[0]
    int32_t n_speedLim, n_curv, n_stop, n_TL;
    int32_t bl_mode, pad;                                    // != 0: the comfort envelope of the baseline controllers
    double s_speedLim[kMaxKnots], v_speedLim[kMaxKnots];
    double s_curv[kMaxKnots], vcurv_tab[kMaxKnots];          // alpha_TTL |curvature|^(-1/3), as DevCfg has it
    double stopLoc[kMaxStops];
    double TLLoc[kMaxTL * 4];                                // per light: position, offset, red time, green time
    double stopRefDist, stopRefVelSlope, stopVel, TLstopVel, TLStopRegionSize;
    double bl_aLo, bl_aHi, bl_jLo, bl_jHi;                   // BL_a_LimLowVel, BL_a_LimHighVel, BL_j_LimLowVel, BL_j_LimHighVel
};

}  // namespace eepacc
#endif
