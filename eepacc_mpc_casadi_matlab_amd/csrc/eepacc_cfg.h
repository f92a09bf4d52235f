// eepacc_cfg.h -- translation of the reference settings (include/eepacc.h) into what the kernels read: validation, the
// move-blocking maps, the objective constants and the inverse of the condensed Hessian.  Host only, no HIP: eepacc_cfg.cpp
// compiles with a plain C++17 compiler, so this one-time mathematics can be called and tested without a device.
#ifndef EEPACC_CFG_H
#define EEPACC_CFG_H

#include <string>
#include <vector>
#include "eepacc_device.h"
#include "eepacc_kpis_cfg.h"
#include "eepacc_follow_cfg.h"
#include "eepacc_route_cfg.h"
#include "../../include/eepacc.h"

namespace eepacc {

// Records the message of a refusal and returns code.  Defined once per program: by eepacc_capi.cpp in libeepacc (the text
// behind eepacc_last_error), by the harness in a host test.
int set_error(int code, const std::string& msg);

// symmetric positive definite inverse in place (Gauss-Jordan in long double; N <= 63); false: a pivot was not positive
bool spd_inverse(std::vector<long double>& A, int n);

// Checks S and V and fills C (zeroed first; the device pointers Hinv, pred and hb stay null) and Hinv [N][N].  Returns
// EEPACC_OK or the code of the first refusal, its text through set_error.
int build_cfg(const eepacc_settings* S, const eepacc_vehicle* V, DevCfg& C, std::vector<double>& Hinv);

// The tables of eepacc_run_abmpc_preview, [N] each, of a Tvec that build_cfg has accepted (positive entries): stage k of a
// step reads the lead trace idx[k] + frac[k] rows after the step's own, frac in [0, 1) and 0 where the stage falls on a sample.
void preview_tables(const double* Tvec, int N, int32_t* idx, double* frac);

// Of settings that build_cfg has accepted.
KpiCfg build_kpi_cfg(const eepacc_settings* S, const eepacc_vehicle* V);
FollowCfg build_follow_cfg(const eepacc_settings* S, const eepacc_vehicle* V);
RouteCfg build_route_cfg(const eepacc_settings* S, const eepacc_vehicle* V);

}  // namespace eepacc
#endif
