// eepacc_bl_qp_cls.hip -- the condensed QP of one BLMPC or TVMPC step as data (eepacc_bl_qp.hip) on a handle with settings
// classes: eepacc_classes_build_qp for a handle of eepacc_create_classes_bl.  cfg is the class array and class_of the map of
// eepacc_set_classes; a workgroup builds the problem of its instance with the settings of the instance's class.  The classes
// of such a handle share bl_mode and N_hor and so the row count: no instance has padding rows.  s_est, v_est, s_tv_est are the
// supplied horizon guesses of eepacc_bl_build_qp_est, each null or not for the whole launch (a wave-uniform branch); all null
// gives the estimators of the instance's class, and bl_mode = 2 classes are launched with the three null and with null lead
// inputs, which they do not read.  The kernel is eepacc_bl_qp_kernel.inc compiled once more, in a unit of its own so that
// k_bl_qp and k_bl_qp_est keep their code (profiles/classes_build_codegen.txt).
#include "eepacc_bl_qp.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_BL_QP_KERNEL k_bl_qp_cls
#define EEPACC_BL_QP_CLASSES
#define EEPACC_BL_QP_MORE_PARAMS , const int32_t* __restrict__ class_of, const double* __restrict__ s_est, const double* __restrict__ v_est, const double* __restrict__ s_tv_est
#define EEPACC_BL_QP_SUPPLIED supplied_estimates(k, N, gridDim.x, b, s_est, v_est, s_tv_est, se, ve, st);
#include "eepacc_bl_qp_kernel.inc"

}  // namespace

hipError_t launch_bl_qp_cls(const DevCfg* cfg, const int32_t* class_of, int N, int nC, int B, const double* s, const double* v,
                            const double* a_prev, const double* t0, const double* s_tv, const double* v_tv,
                            const double* a_tv_prev, double* H, double* g, double* A, double* lba, double* uba,
                            hipStream_t stream, const AbSupplied& sup) {
    hipLaunchKernelGGL(k_bl_qp_cls, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba, class_of, sup.s_est, sup.v_est, sup.s_tv_est);
    return hipGetLastError();
}

}  // namespace eepacc
