// eepacc_ab_build.hip -- the condensed QP of one ABMPC step, written out as data: H, g, A, lba, uba in the layout the
// dense QP operator reads.  The closed-loop kernels never form this problem; this kernel is the
// boundary for callers who want it: to read multipliers row by row, to hand it to another solver, to differentiate it.
//
// Reference: ABO/RunOpt_ABMPC.m:193-252 with solverToUse = 1: estimators (EstimateVehicleTrajectory.m:55-88), bounds
// (EstimateRouteAndComfortBounds.m:63-171), objective and rows of ABO/Functions/MPCs/CreateQP_AB.m:150-387 (zero rows
// trimmed, RunOpt_ABMPC.m:229-233) and the condensing of TransformToDenseFormulation.m:30-91.
//
// No dense product with Psi is formed.  With A_k = [1 T_k; 0 1], B_k = [T_k^2/2; T_k] on the acceleration only,
//   v_k = v_0 + sum_{i<k} T_i a_i,   s_k = d_s[k] + sum_{i<k} Ss[k][i] a_i,   Ss[k][i] = T_i^2/2 + T_i (T_{k-1} + .. + T_{i+1}),
// the sparse-form Hessian is diagonal in v_k and xi_h and tridiagonal in a_k, and a row touches s_k, v_k, a_k, a_{k-1} and
// one slack.  Every output entry is assembled from these pieces, which are put into LDS once.  Sums run in the order of
// the reference's loops (the inner sum of Ss from stage k-1 downwards, the entries of g over ascending stages) and
// products are not contracted into fused multiply-adds, so that an entry of A, lba, uba and g has the reference's
// roundings; the a-a entries of H take the suffix sums of the speed curvature instead of a loop per entry.
//
// Dense variable order per stage (5): a, xi_v, xi_h, xi_s, xi_f.  Rows: eepacc_ab_build.h.  The geometry of the kernel, the
// row list and the walks over H, the bounds and A are eepacc_qp_build.h's, shared with k_fb_qp and k_bl_qp; the stage
// quantities, the rows and the entries of H and g are eepacc_ab_build_kernel.inc's, which eepacc_ab_build_est.hip compiles once
// more for horizon guesses that the caller supplies (eepacc_ab_build_qp_est).
#include "eepacc_ab_build.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_AB_BUILD_KERNEL k_ab_build
#define EEPACC_AB_BUILD_MORE_PARAMS
#define EEPACC_AB_BUILD_SUPPLIED
#include "eepacc_ab_build_kernel.inc"
}  // namespace

hipError_t launch_ab_build(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                           const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                           double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream,
                           const AbSupplied* sup) {
    if (sup) return launch_ab_build_est(cfg, N, nC, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, H, g, A, lba, uba, stream, *sup);
    hipLaunchKernelGGL(k_ab_build, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba);
    return hipGetLastError();
}

}  // namespace eepacc
