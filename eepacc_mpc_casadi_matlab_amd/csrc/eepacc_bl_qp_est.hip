// eepacc_bl_qp_est.hip -- the condensed QP of one BLMPC step as data (eepacc_bl_qp.hip) on horizon guesses that the caller
// supplies: eepacc_bl_build_qp_est, bl_mode = 1 only.  s_est, v_est, s_tv_est [N_hor+1][B] stand where CreateQP_BL(OPTsettings,
// n_x, n_u, s_0, v_0, s_est, v_est, s_tv_est, t_0, a_minus1) takes them as inputs (RunOpt_BLMPC.m:56,182): s_est and v_est reach
// the problem through the route and comfort bounds alone (CreateQP_BL.m:46), s_tv_est through the upper bounds of the two
// safe-distance rows of a stage and of the terminal stage (:291,295,309,313); a null array keeps the estimator's guess.  The
// kernel is eepacc_bl_qp_kernel.inc compiled once more, in a unit of its own so that k_bl_qp keeps its code.
#include "eepacc_bl_qp.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_BL_QP_KERNEL k_bl_qp_est
#define EEPACC_BL_QP_MORE_PARAMS , const double* __restrict__ s_est, const double* __restrict__ v_est, const double* __restrict__ s_tv_est
#define EEPACC_BL_QP_SUPPLIED supplied_estimates(k, N, gridDim.x, b, s_est, v_est, s_tv_est, se, ve, st);
#include "eepacc_bl_qp_kernel.inc"

}  // namespace

hipError_t launch_bl_qp_est(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                            const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                            double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                            const AbSupplied& sup) {
    hipLaunchKernelGGL(k_bl_qp_est, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba, sup.s_est, sup.v_est, sup.s_tv_est);
    return hipGetLastError();
}

}  // namespace eepacc
