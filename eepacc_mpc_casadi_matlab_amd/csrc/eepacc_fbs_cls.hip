// eepacc_fbs_cls.hip -- structured FBMPC kernels (gfx950) on a handle with settings classes: eepacc_classes_fb_step and
// eepacc_run_classes_fbmpc (a handle of eepacc_create_classes; every instance runs with the DevCfg of its class).  The kernels
// are the two templates of eepacc_fbs.hip instantiated with one further argument, the class map of the launch: cfg_of there
// binds the instance's DevCfg per wave (step) and per work unit (closed loop), from a wave-uniform index.  A unit of their own,
// as eepacc_fbs_est.hip is, so that the kernels of the other two units keep their code (profiles/classes_fb_codegen.txt).
// Same scratch and grids as eepacc_fbs.hip; a.cfg is the handle's class array, whose head gives N and Tvec.
#undef EEPACC_FBS_TIMING        // the phase counters belong to eepacc_fbs.hip (one definition of the device symbol)
#define EEPACC_FBS_KERNELS_ONLY // the templates without that unit's host-side launchers
#define EEPACC_FBS_CLASS_MAP    // k_fbs_run binds the DevCfg of the unit's instance inside the unit's body (EEPACC_FBS_UNIT_CFG)
#include "eepacc_fbs.hip"

namespace eepacc {

namespace {
using I = const int32_t*;
}

hipError_t fbs_cls_set_max_smem() {
    const void* fns[4] = {reinterpret_cast<const void*>(&fbs::k_fbs_step<kFMMaxSmall, kFNSSmall, kFWpbSmall, I>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_step<kFMMaxLarge, kFNSLarge, kFWpbLarge, I>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_run<kFMMaxSmall, kFNSSmall, kFWpbSmall, I>),
                          reinterpret_cast<const void*>(&fbs::k_fbs_run<kFMMaxLarge, kFNSLarge, kFWpbLarge, I>)};
    for (int i = 0; i < 4; ++i) {
        hipError_t e = hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int)kFbsLdsBudget);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

hipError_t launch_fbs_step_cls(const fbs_step_args& a, int N, hipStream_t stream, const int32_t* class_of) {
    const size_t smem = fbs_smem_bytes(N);
    if (N > kFNSSmall)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_step<kFMMaxLarge, kFNSLarge, kFWpbLarge, I>), dim3((a.B + kFWpbLarge - 1) / kFWpbLarge),
                           dim3(64 * kFWpbLarge), smem, stream, a, class_of);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_step<kFMMaxSmall, kFNSSmall, kFWpbSmall, I>), dim3((a.B + kFWpbSmall - 1) / kFWpbSmall),
                           dim3(64 * kFWpbSmall), smem, stream, a, class_of);
    return hipGetLastError();
}

hipError_t launch_fbs_run_cls(fbs_run_args a, int N, int num_cus, hipStream_t stream, const int32_t* class_of) {
    const bool large = N > kFNSSmall;
    UnitsLaunch ul;
    hipError_t e = begin_units(a.work_counter, a.done, a.iters_total, a.B, a.n_steps, a.chunk_steps,
                               large ? kFWpbLarge : kFWpbSmall, fbs_run_max_grid(N, num_cus), stream, ul);
    if (e != hipSuccess) return e;
    a.spin_limit = ul.spin_limit;
    const size_t smem = fbs_smem_bytes(N);
    if (large)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_run<kFMMaxLarge, kFNSLarge, kFWpbLarge, I>), dim3(ul.grid), dim3(64 * kFWpbLarge), smem,
                           stream, a, class_of);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(fbs::k_fbs_run<kFMMaxSmall, kFNSSmall, kFWpbSmall, I>), dim3(ul.grid), dim3(64 * kFWpbSmall), smem,
                           stream, a, class_of);
    return hipGetLastError();
}

}  // namespace eepacc
