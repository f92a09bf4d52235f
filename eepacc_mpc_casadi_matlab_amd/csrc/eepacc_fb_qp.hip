// eepacc_fb_qp.hip -- the condensed QP of one FBMPC step, written out as data: H, g, A, lba, uba in the layout the dense QP
// operator reads.  The structured FBMPC kernels (eepacc_fbs.hip) never form this problem; the build kernel of the dense
// path (k_fb_build, eepacc_fb.hip) forms it, but inside a pipeline that measures the plant and updates the carried model.
// This kernel is the boundary for callers who want the problem itself: it takes the step's inputs and the model A(k), D(k)
// as arguments and writes nothing but its outputs.
//
// Reference: ABO/RunOpt_FBMPC.m:204-264: estimators (EstimateVehicleTrajectory.m:55-88), bounds
// (EstimateRouteAndComfortBounds.m:63-171), objective and rows of ABO/Functions/MPCs/CreateQP_FB.m:158-489, the model of
// RunOpt_FBMPC.m:78-90, 247-259 and the condensing of TransformToDenseFormulation.m:30-91.  The condensing arithmetic is
// eepacc_fb_condense.h, which k_fb_build calls too; the geometry of the kernel, the row list and the walks over H, the bounds
// and A are eepacc_qp_build.h's, shared with k_ab_build and k_bl_qp.
//
// No dense product with Psi is formed.  With B_k = T_k/(lambda m) [0 0; 1 1] only the state rows of Psi are dense: the
// columns Sv[.,i], Ss[.,i] of the speed / position sensitivities to the force of stage i.  The sparse-form Hessian is block
// tridiagonal in (v, Fm, Fb)_k (diagonal blocks D_k, coupling blocks O_k between stages k-1 and k), and a row touches s_k,
// v_k, the forces of stages k and k-1 and one slack.  Every output entry is assembled from these pieces, which are put into
// LDS once.  Products are not contracted into fused multiply-adds, so that an entry carries the roundings of its products.
//
// Dense variable order per stage (6): Fm, Fb, xi_v, xi_h, xi_s, xi_f.  Rows: eepacc_fb_rows.h.
#include "eepacc_fb_qp.h"
// first of the three: it switches contraction off, also for the rows and the arithmetic as this file compiles them
#include "eepacc_qp_build.h"
#include "eepacc_fb_condense.h"
#include "eepacc_fb_rows.h"

namespace eepacc {
namespace {

#define EEPACC_FB_QP_KERNEL k_fb_qp
#define EEPACC_FB_QP_MORE_PARAMS
#define EEPACC_FB_QP_SUPPLIED
#include "eepacc_fb_qp_kernel.inc"

}  // namespace

size_t fb_qp_smem_bytes(int N, int nC) { return sizeof(Stages) + qp_build_smem_bytes(N, nC, 2); }

hipError_t launch_fb_qp(const fb_qp_args& a, int N, hipStream_t stream) {
    const size_t smem = qp_build_smem_bytes(N, a.nC, 2);
    if (fb_qp_smem_bytes(N, a.nC) > kLdsMax) return hipErrorInvalidValue;
    // The attribute belongs to the kernel, not to the handle: always the largest size, so that launches of handles with
    // different horizons on different host threads cannot lower it under one another.
    const hipError_t e = hipFuncSetAttribute((const void*)k_fb_qp, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kLdsMax - sizeof(Stages)));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fb_qp, dim3(a.B), dim3(BT), smem, stream, a);
    return hipGetLastError();
}

}  // namespace eepacc
