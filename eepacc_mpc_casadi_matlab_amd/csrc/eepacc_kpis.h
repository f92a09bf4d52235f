// Host interface of the key-figure kernel (eepacc_kpis.hip): per-instance figures of ABO/Main.m:131-263 and
// ABO/Custom_plots.m:73-107 from a closed-loop trajectory, on the device.
#ifndef EEPACC_KPIS_H
#define EEPACC_KPIS_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eepacc_device.h"
#include "eepacc_kpis_cfg.h"      // KpiCfg: what the key figures read of a settings class

namespace eepacc {

// Geometry: a workgroup of kKpiWaves waves serves 64 consecutive instances (lane = instance); wave w reduces the steps
// [w Ls, (w + 1) Ls), Ls = max(kKpiMinSlice, ceil(n_steps / kKpiWaves)).
constexpr int kKpiWaves = 16;
constexpr int kKpiMinSlice = 8;
constexpr int kKpiRecDoubles = 12;   // doubles per lane and slice handed to the join through LDS

inline int kpi_slice_len(int n_steps) {
    const int per = (n_steps + kKpiWaves - 1) / kKpiWaves;
    return per > kKpiMinSlice ? per : kKpiMinSlice;
}

// dK: KpiCfg[n_classes]; class_of: the device map [B] of a handle of eepacc_create_classes, null otherwise (every
// instance then reads dK[0] and cut[0]); cut: device, one cut-off distance per class.  kpi [EEPACC_KPI_N][B].
hipError_t launch_kpis(const KpiCfg* dK, const int32_t* class_of, const double* cut, int B, int n_steps, const double* traj,
                       const int32_t* status, double* kpi, hipStream_t stream);

}  // namespace eepacc
#endif
