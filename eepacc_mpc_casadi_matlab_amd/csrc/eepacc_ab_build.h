// eepacc_ab_build.h -- the condensed QP of one ABMPC step as data (eepacc_ab_build.hip): row catalogue and launcher.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "eepacc_device.h"
#include "eepacc_ab.h"
#include "../../include/eepacc.h"

namespace eepacc {

// The values of EEPACC_AB_ROW_* ascend in the order in which CreateQP_AB.m:256-371 (with the four ORIG rows :307-329)
// appends the rows of a stage, so a stage's rows are the present types in ascending order: the blocked-move row only on a
// stage with Mb = 1 (:283-289), the four speed caps only with ab_route_rows.  Host (eepacc_ab_qp_rows) and kernel share this.
__host__ __device__ inline bool ab_row_present(int type, int route_rows, int blocked) {
    if (type == EEPACC_AB_ROW_BLOCKED) return blocked != 0;
    if (type >= EEPACC_AB_ROW_V_LIM && type <= EEPACC_AB_ROW_V_TL) return route_rows != 0;
    return true;
}

inline int ab_qp_num_rows(const DevCfg& C) {
    int nC = (C.ab_route_rows ? 18 : 14) * C.N + 2;
    for (int k = 0; k < C.N; ++k) nC += C.mb_mask[k] ? 1 : 0;
    return nC;
}

// B workgroups of 256 threads; every entry of H [B][nV*nV], g [B][nV], A [B][nV][nC], lba, uba [B][nC] is written.
hipError_t launch_ab_build(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                           const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                           double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                           const AbSupplied* sup = nullptr);      // sup: supplied horizon guesses (eepacc_ab_build_qp_est)

// the same on supplied guesses (eepacc_ab_build_est.hip); launch_ab_build goes there when sup is given
hipError_t launch_ab_build_est(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                               const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                               double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                               const AbSupplied& sup);

// the same on a handle with settings classes (eepacc_ab_build_cls.hip, eepacc_classes_build_qp): cfg is the class array,
// class_of the device map [B], nC the row count of the largest class (classes_qp_num_rows, eepacc_cfg.h): the leading row
// dimension of A, lba, uba, padding rows behind an instance's own.  The members of sup may be null.
hipError_t launch_ab_build_cls(const DevCfg* cfg, const int32_t* class_of, int N, int nC, int B, const double* s, const double* v,
                               const double* a_prev, const double* t0, const double* s_tv, const double* v_tv,
                               const double* a_tv_prev, double* H, double* g, double* A, double* lba, double* uba,
                               hipStream_t stream, const AbSupplied& sup);

}  // namespace eepacc
