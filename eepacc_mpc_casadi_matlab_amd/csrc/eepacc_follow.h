// Host interface of the vehicle-following / cost key-figure kernel (eepacc_follow.hip): per-instance headway figures of
// ABO/Main.m:679-771 and final cost_* of ABO/RunOpt_ABMPC.m:382-404 / ABO/RunOpt_FBMPC.m:373-397, on the device.
#ifndef EEPACC_FOLLOW_H
#define EEPACC_FOLLOW_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eepacc_kpis.h"
#include "eepacc_follow_cfg.h"    // FollowCfg: what the operator reads of a settings class

namespace eepacc {

// Geometry of k_kpis (kKpiWaves, kKpiMinSlice, kpi_slice_len).  A slice hands the join 12 doubles (four minima, one
// maximum, seven sums) and 3 ints (first index of the smallest gap, two counts) per lane through LDS.
constexpr int kFollowRecDoubles = 12;
constexpr int kFollowRecInts = 3;
constexpr size_t kFollowLdsBytes = (size_t)kKpiWaves * 64 * (kFollowRecDoubles * sizeof(double) + kFollowRecInts * sizeof(int32_t));

// dF: FollowCfg[n_classes]; class_of: the device map [B] of a handle of eepacc_create_classes, null otherwise (every
// instance then reads dF[0]); weights: EEPACC_FKPI_W_*, checked by the caller.  fkpi [EEPACC_FKPI_N][B].
hipError_t launch_follow_kpis(const FollowCfg* dF, const int32_t* class_of, int weights, int B, int n_steps, const double* traj,
                              const double* s_tv, const double* v_tv, double* fkpi, hipStream_t stream);

}  // namespace eepacc
#endif
