// eepacc_bl_qp.hip -- the condensed QP of one BLMPC step (bl_mode = 1) or TVMPC step (bl_mode = 2), written out as data:
// H, g, A, lba, uba in the layout the dense QP operator reads.  The closed-loop kernels never form this problem; this
// kernel is the boundary for callers who want it: to compare objective values on the faces of the LP, to read which
// speed-limit, stop or headway row is tight, to hand the problem to another solver.  The geometry of the kernel (one workgroup
// of 256 threads per instance, stage quantities into LDS once), the row list, the walks over H, the bounds and A, and the
// double-integrator pieces it has in common with k_ab_build (the row type, Ss, the entry of A) are eepacc_qp_build.h's; the
// stage quantities, the rows and the entries of H and g are this file's.
//
// Reference, bl_mode = 1: ABO/RunOpt_BLMPC.m:182-230 with solverToUse = 1: estimators (EstimateVehicleTrajectory.m:55-88),
// bounds (EstimateRouteAndComfortBounds.m:63-143,173-189), objective and rows of ABO/Functions/MPCs/CreateQP_BL.m:99-314
// and the condensing of TransformToDenseFormulation.m:30-91.  bl_mode = 2: ABO/RunOpt_TVMPC.m:161-208 with CreateQP_TV.m:
// the same rows without the headway rows (:288-292: no terminal rows either), 0.8 of the speed-limit and curve caps
// (:265,271) and the comfort limits of a zero speed estimate (:44-45).
//
// With A_k = [1 T_k; 0 1], B_k = [T_k^2/2; T_k] on the acceleration only,
//   v_k = v_0 + sum_{i<k} T_i a_i,   s_k = d_s[k] + sum_{i<k} Ss[k][i] a_i,   Ss[k][i] = T_i^2/2 + T_i (T_{k-1} + .. + T_{i+1}).
// The sparse-form objective has no curvature on s_k, v_k: H is the tridiagonal of the w_a and w_j terms on the
// accelerations (both zero with the reference's weights: a linear program), and g carries the travel incentive -w_v on
// v_0 .. v_N through the speed sensitivities.  CreateQP_BL.m:31 takes Ts = Tvec(1) for the jerk terms at every stage; the
// dynamics take Tvec(k).  Sums run in the order of the reference's loops and products are not contracted into fused
// multiply-adds, so that an entry of A, lba, uba and g has the reference's roundings.
//
// Dense variable order per stage (2): a, xi_f.  Rows: eepacc_bl_qp.h.  The kernel itself is eepacc_bl_qp_kernel.inc's, which
// eepacc_bl_qp_est.hip compiles once more for horizon guesses that the caller supplies (eepacc_bl_build_qp_est).
#include "eepacc_bl_qp.h"
#include "eepacc_qp_build.h"

namespace eepacc {
namespace {

#define EEPACC_BL_QP_KERNEL k_bl_qp
#define EEPACC_BL_QP_MORE_PARAMS
#define EEPACC_BL_QP_SUPPLIED
#include "eepacc_bl_qp_kernel.inc"

}  // namespace

hipError_t launch_bl_qp(const DevCfg* cfg, int N, int nC, int B, const double* s, const double* v, const double* a_prev,
                        const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        double* H, double* g, double* A, double* lba, double* uba, hipStream_t stream) {
    hipLaunchKernelGGL(k_bl_qp, dim3(B), dim3(BT), qp_build_smem_bytes(N, nC, 1), stream, cfg, nC, s, v, a_prev, t0,
                       s_tv, v_tv, a_tv_prev, H, g, A, lba, uba);
    return hipGetLastError();
}

}  // namespace eepacc
