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

// Whether a handle serves the FBMPC entries with supplied horizon guesses (who: the entry's name).  n_classes, C: the handle's;
// structured: its FBMPC steps run through the structured kernels; needs_structured: the entry is the step or the preview loop
// (the builder serves dense-path handles too).  EEPACC_OK, or EEPACC_ENOTSUP with the cause through set_error.
int fb_est_refusal(const std::string& who, int n_classes, const DevCfg& C, bool structured, bool needs_structured);

// What the structured FBMPC solver does not represent of C: the settings field with the reason, or NULL where it runs C
// (eepacc::fbs_supported is this test).
const char* fbs_unsupported_field(const DevCfg& C);

// Whether eepacc_classes_fb_step / eepacc_run_classes_fbmpc (who) serve a call.  Of the handle: n_classes (0: one of
// eepacc_create), bl_mode and N of class 0, unsupported [n_classes] = fbs_unsupported_field of every class, the LDS a block of
// the kernels needs at N and may have, max_batch and the B of the last eepacc_set_classes (0: none).  Of the call: B, n_steps
// (the step entry passes 1) and the name of its first required buffer that is NULL (or NULL).  EEPACC_OK (also for B = 0 or
// n_steps = 0, before the buffers are looked at), EEPACC_ENOTSUP for the handle, EEPACC_EINVAL for the call; text through set_error.
struct ClassesFbCall {
    int n_classes, bl_mode, N;
    const char* const* unsupported;
    size_t smem_bytes, smem_budget;
    int max_batch, classes_B, B, n_steps;
    const char* null_buffer;
};
int classes_fb_refusal(const std::string& who, const ClassesFbCall& c);

// Of settings that build_cfg has accepted.
KpiCfg build_kpi_cfg(const eepacc_settings* S, const eepacc_vehicle* V);
FollowCfg build_follow_cfg(const eepacc_settings* S, const eepacc_vehicle* V);
RouteCfg build_route_cfg(const eepacc_settings* S, const eepacc_vehicle* V);

// The row catalogue of eepacc_classes_build_qp, for a handle's launcher and eepacc_classes_qp_rows alike.  What it depends on of
// a class that create_classes has accepted (no move blocking; N and bl_mode agree over the classes of a handle):
struct QpRowsCfg { int32_t N, bl_mode, ab_route_rows; };
QpRowsCfg qp_rows_cfg(const DevCfg& C);
// Rows of a class's own problem: 14 N + 2 or 18 N + 2 (ABMPC without / with ab_route_rows), 13 N + 2 (bl_mode 1), 11 N (2)
int classes_qp_num_rows(const QpRowsCfg& c);
// nC of the handle: the largest of its classes, the leading row dimension of every instance's A, lba, uba
int classes_qp_max_rows(const QpRowsCfg* c, int n_classes);
// stage, type [nC of the handle]: the rows of class cls as eepacc_ab_qp_rows / eepacc_bl_qp_rows order them, then -1 in both
// for the padding rows up to nC.  EEPACC_EINVAL (through set_error): cls outside [0, n_classes).
int classes_qp_rows(const QpRowsCfg* c, int n_classes, int cls, int32_t* stage, int32_t* type);

}  // namespace eepacc
#endif
