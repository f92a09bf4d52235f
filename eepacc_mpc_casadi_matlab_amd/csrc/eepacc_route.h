// Host interface of the route-compliance key-figure kernel (eepacc_route.hip): whether every instance of a closed-loop run
// obeyed its route -- the speed limit, the curve policy, the stop profile and the lights that ABO/Main.m:374-433 and :486-534
// draw for one run -- and the comfort envelope of EstimateRouteAndComfortBounds.m:154-189, on the device.
#ifndef EEPACC_ROUTE_H
#define EEPACC_ROUTE_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eepacc_kpis.h"
#include "eepacc_route_cfg.h"     // RouteCfg: what the operator reads of a settings class

namespace eepacc {

// Geometry of k_kpis (kKpiWaves, kKpiMinSlice, kpi_slice_len).  A slice hands the join 10 doubles (nine maxima, one minimum)
// and 11 ints (two first indices, nine counts) per lane through LDS.
constexpr int kRouteRecDoubles = 10;
constexpr int kRouteRecInts = 11;
constexpr size_t kRouteLdsBytes = (size_t)kKpiWaves * 64 * (kRouteRecDoubles * sizeof(double) + kRouteRecInts * sizeof(int32_t));

// dR: RouteCfg[n_classes]; class_of: the device map [B] of a handle of eepacc_create_classes, null otherwise (every
// instance then reads dR[0], through scalar loads); tol: v_tol, a_tol, j_tol, checked by the caller.  rkpi [EEPACC_RKPI_N][B];
// limits [n_steps][EEPACC_RLIM_N][B] or null.
hipError_t launch_route_kpis(const RouteCfg* dR, const int32_t* class_of, int B, int n_steps, double t_start, double v_tol,
                             double a_tol, double j_tol, const double* traj, double* rkpi, double* limits, hipStream_t stream);

}  // namespace eepacc
#endif
