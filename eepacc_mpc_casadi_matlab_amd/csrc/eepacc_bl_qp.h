// eepacc_bl_qp.h -- the condensed QP of one BLMPC or TVMPC step as data (eepacc_bl_qp.hip): row catalogue and launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eepacc_device.h"
#include "eepacc_ab.h"
#include "../../include/eepacc.h"

namespace eepacc {

// The values of EEPACC_BL_ROW_* ascend in the order in which CreateQP_BL.m:217-296 appends the rows of a stage, so a stage's
// rows are the present types in ascending order.  CreateQP_TV.m:215-284 (bl_mode = 2) has the same rows without the two
// safe-distance rows and without terminal rows.  Host (eepacc_bl_qp_rows) and kernel share this.
__host__ __device__ inline bool bl_row_present(int type, int bl_mode) {
    return bl_mode != 2 || type < EEPACC_BL_ROW_SAFE1;
}

__host__ __device__ inline int bl_rows_per_stage(int bl_mode) { return bl_mode == 2 ? EEPACC_BL_ROW_SAFE1 : EEPACC_BL_ROW_N; }

inline int bl_qp_num_rows(const DevCfg& C) { return bl_rows_per_stage(C.bl_mode) * C.N + (C.bl_mode == 2 ? 0 : 2); }

// B workgroups of 256 threads; every entry of H [B][nV*nV], g [B][nV], A [B][nV][nC], lba, uba [B][nC] is written.  The lead
// arrays are not read for a bl_mode = 2 configuration.
hipError_t launch_bl_qp(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                        const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream);

// the same on supplied guesses (eepacc_bl_qp_est.hip, eepacc_bl_build_qp_est): cfg has bl_mode = 1
hipError_t launch_bl_qp_est(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                            const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                            double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                            const AbSupplied& sup);

// the same on a handle with settings classes (eepacc_bl_qp_cls.hip, eepacc_classes_build_qp): cfg is the class array, class_of
// the device map [B]; the classes share bl_mode and so nC.  The members of sup may be null, and are with bl_mode = 2.
hipError_t launch_bl_qp_cls(const DevCfg* cfg, const int32_t* class_of, int N, int nC, int B, const double* s, const double* v,
                            const double* a_prev, const double* t0, const double* s_tv, const double* v_tv,
                            const double* a_tv_prev, double* H, double* g, double* A, double* lba, double* uba,
                            hipStream_t stream, const AbSupplied& sup);

}  // namespace eepacc
