// eepacc_fbs_est.hip -- structured FBMPC kernels (gfx950) on horizon guesses that the caller supplies: eepacc_fb_step_est
// (s_est, v_est, s_tv_est [N_hor+1][B] stand where CreateQP_FB takes them as inputs, RunOpt_FBMPC.m:215) and
// eepacc_run_fbmpc_preview (the lead's guess of every step read from the launch's lead traces).  The kernels are the two
// templates of eepacc_fbs.hip instantiated with further arguments, in a unit of their own so that the kernels of
// eepacc_fbs.hip keep their code (profiles/fb_est_codegen.txt).  Same handle state, same scratch, same grids.
#undef EEPACC_FBS_TIMING        // the phase counters belong to eepacc_fbs.hip (one definition of the device symbol)
#define EEPACC_FBS_KERNELS_ONLY // the templates without that unit's host-side launchers
#include "eepacc_fbs.hip"

namespace eepacc {

namespace {
using P = const double*;
using I = const int32_t*;
}

hipError_t fbs_est_set_max_smem() {
    const void* fns[4] = {reinterpret_cast<const void*>(&fbs::k_fbs_step<kFMMaxSmall, kFNSSmall, kFWpbSmall, P, P, P>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_step<kFMMaxLarge, kFNSLarge, kFWpbLarge, P, P, P>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_run<kFMMaxSmall, kFNSSmall, kFWpbSmall, I, P, int>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_run<kFMMaxLarge, kFNSLarge, kFWpbLarge, I, P, int>)};
    for (int i = 0; i < 4; ++i) {
        hipError_t e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFbsLdsBudget);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_fbs_step_est(const fbs_step_args& a, int N, hipStream_t stream, const double* s_est, const double* v_est,
                               const double* s_tv_est) {
    const size_t smem = fbs_smem_bytes(N);
    if (N > kFNSSmall)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_step<kFMMaxLarge, kFNSLarge, kFWpbLarge, P, P, P>), dim3((a.B + kFWpbLarge - 1) / kFWpbLarge),
                           dim3(64 * kFWpbLarge), smem, stream, a, s_est, v_est, s_tv_est);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_step<kFMMaxSmall, kFNSSmall, kFWpbSmall, P, P, P>), dim3((a.B + kFWpbSmall - 1) / kFWpbSmall),
                           dim3(64 * kFWpbSmall), smem, stream, a, s_est, v_est, s_tv_est);
    return hipGetLastError();
}

hipError_t launch_fbs_run_preview(fbs_run_args a, int N, int num_cus, hipStream_t stream, const int32_t* idx, const double* frac,
                                  int n_lead) {
    const bool large = N > kFNSSmall;
    UnitsLaunch ul;
    hipError_t e = begin_units(a.work_counter, a.done, a.iters_total, a.B, a.n_steps, a.chunk_steps,
                               large ? kFWpbLarge : kFWpbSmall, fbs_run_max_grid(N, num_cus), stream, ul);
    if (e != hipSuccess) return e;
    a.spin_limit = ul.spin_limit;
    const size_t smem = fbs_smem_bytes(N);
    if (large)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_run<kFMMaxLarge, kFNSLarge, kFWpbLarge, I, P, int>), dim3(ul.grid), dim3(64 * kFWpbLarge), smem,
                           stream, a, idx, frac, n_lead);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_run<kFMMaxSmall, kFNSSmall, kFWpbSmall, I, P, int>), dim3(ul.grid), dim3(64 * kFWpbSmall), smem,
                           stream, a, idx, frac, n_lead);
    return hipGetLastError();
}

}  // namespace eepacc
