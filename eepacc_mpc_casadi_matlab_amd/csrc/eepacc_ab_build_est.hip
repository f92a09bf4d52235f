// eepacc_ab_build_est.hip -- the condensed QP of one ABMPC step as data (eepacc_ab_build.hip) on horizon guesses that the
// caller supplies: eepacc_ab_build_qp_est.  s_est, v_est, s_tv_est [N_hor+1][B] stand where CreateQP_AB(OPTsettings, n_x, n_u,
// s_0, v_0, s_est, v_est, s_tv_est, t_0, a_minus1) takes them as inputs; a null array keeps the estimator's guess.  The kernel
// is eepacc_ab_build_kernel.inc compiled once more, in a unit of its own so that k_ab_build keeps its code.
#include "eepacc_ab_build.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_AB_BUILD_KERNEL k_ab_build_est
#define EEPACC_AB_BUILD_MORE_PARAMS , const double* __restrict__ s_est, const double* __restrict__ v_est, const double* __restrict__ s_tv_est
#define EEPACC_AB_BUILD_SUPPLIED supplied_estimates(k, N, gridDim.x, b, s_est, v_est, s_tv_est, se, ve, st);
#include "eepacc_ab_build_kernel.inc"
}  // namespace

hipError_t launch_ab_build_est(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                               const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                               double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                               const AbSupplied& sup) {
    hipLaunchKernelGGL(k_ab_build_est, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba, sup.s_est, sup.v_est, sup.s_tv_est);
    return hipGetLastError();
}

}  // namespace eepacc
