// eepacc_ab_build_cls.hip -- the condensed QP of one ABMPC step as data (eepacc_ab_build.hip) on a handle with settings
// classes: eepacc_classes_build_qp for a handle of eepacc_create_classes.  cfg is the class array and class_of the map of
// eepacc_set_classes; a workgroup builds the problem of its instance with the settings of the instance's class.  Classes may
// differ in ab_route_rows and so in their row count (14 or 18 rows a stage): nC is the count of the largest class, the leading
// row dimension of A, lba and uba for every instance, and an instance of a smaller class gets padding rows behind its own
// (A exactly 0.0, lba = -inf, uba = +inf), written by the walks that write the other rows.  s_est, v_est, s_tv_est are the
// supplied horizon guesses of eepacc_ab_build_qp_est, each null or not for the whole launch (a wave-uniform branch); all null
// gives the estimators of the instance's class.  The kernel is eepacc_ab_build_kernel.inc compiled once more, in a unit of its
// own so that k_ab_build and k_ab_build_est keep their code (profiles/classes_build_codegen.txt); sums and products keep the
// order and the no-contraction rule stated at the head of eepacc_ab_build.hip.
#include "eepacc_ab_build.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_AB_BUILD_KERNEL k_ab_build_cls
#define EEPACC_AB_BUILD_CLASSES
#define EEPACC_AB_BUILD_MORE_PARAMS , const int32_t* __restrict__ class_of, const double* __restrict__ s_est, const double* __restrict__ v_est, const double* __restrict__ s_tv_est
#define EEPACC_AB_BUILD_SUPPLIED supplied_estimates(k, N, gridDim.x, b, s_est, v_est, s_tv_est, se, ve, st);
#include "eepacc_ab_build_kernel.inc"
}  // namespace

hipError_t launch_ab_build_cls(const DevCfg* cfg, const int32_t* class_of, int N, int nC, int B, const double* s, const double* v,
                               const double* a_prev, const double* t0, const double* s_tv, const double* v_tv,
                               const double* a_tv_prev, double* H, double* g, double* A, double* lba, double* uba,
                               hipStream_t stream, const AbSupplied& sup) {
    hipLaunchKernelGGL(k_ab_build_cls, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba, class_of, sup.s_est, sup.v_est, sup.s_tv_est);
    return hipGetLastError();
}

}  // namespace eepacc
