// eepacc_fb_qp_est.hip -- the condensed QP of one FBMPC step as data (eepacc_fb_qp.hip) on horizon guesses that the caller
// supplies: eepacc_fb_build_qp_est.  s_est, v_est, s_tv_est [N_hor+1][B] stand where CreateQP_FB(OPTsettings, ..., s_est,
// v_est, s_tv_est, ...) takes them as inputs (RunOpt_FBMPC.m:215).  v_est reaches the problem through the drag terms of the
// objective, the acceleration and jerk rows, the headway row with FBuseTaylor = 1, the comfort bounds, and through the model:
// entry k == k_step of A(k), D(k) is made of v_est(N_hor) (RunOpt_FBMPC.m:247-259), every D(k) with FBuseTaylor = 0.  s_est
// reaches it through the route bounds, s_tv_est through the three headway rows of a stage and the two terminal rows.  A null
// array keeps the estimator's guess.  The kernel is eepacc_fb_qp_kernel.inc compiled once more, in a unit of its own so that
// k_fb_qp keeps its code.
#include "eepacc_fb_qp.h"
// first of the three: it switches contraction off, also for the rows and the arithmetic as this file compiles them
#include "eepacc_qp_build.h"
#include "eepacc_fb_condense.h"
#include "eepacc_fb_rows.h"

namespace eepacc {
namespace {

#define EEPACC_FB_QP_KERNEL k_fb_qp_est
#define EEPACC_FB_QP_MORE_PARAMS , const double* __restrict__ s_est, const double* __restrict__ v_est, const double* __restrict__ s_tv_est
#define EEPACC_FB_QP_SUPPLIED supplied_estimates(k, N, B, b, s_est, v_est, s_tv_est, se, ve, st);
#include "eepacc_fb_qp_kernel.inc"

}  // namespace

hipError_t launch_fb_qp_est(const fb_qp_args& a, int N, hipStream_t stream, const double* s_est, const double* v_est,
                            const double* s_tv_est) {
    const size_t smem = qp_build_smem_bytes(N, a.nC, 2);
    if (fb_qp_smem_bytes(N, a.nC) > kLdsMax) return hipErrorInvalidValue;
    // (the largest size always, as launch_fb_qp sets it)
    const hipError_t e = hipFuncSetAttribute((const void*)k_fb_qp_est, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kLdsMax - sizeof(Stages)));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fb_qp_est, dim3(a.B), dim3(BT), smem, stream, a, s_est, v_est, s_tv_est);
    return hipGetLastError();
}

}  // namespace eepacc
