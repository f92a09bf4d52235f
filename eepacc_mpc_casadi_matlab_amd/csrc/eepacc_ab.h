// Host interface of the ABMPC kernels (eepacc_kernels.hip).
#ifndef EEPACC_AB_H
#define EEPACC_AB_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "eepacc_device.h"

namespace eepacc {

// One instantiation of eepacc_ab_impl.inc each; EEPACC_AB_VARIANTS (eepacc_kernels.hip) gives namespace and switches.
enum class AbVariant { Plain, MoveBlocking, Baseline, Ice, IceMoveBlocking, TargetVehicle, Classes, ClassesBL, ClassesTV, Est, BlEst, ClassesEst, ClassesBlEst };

// The further arguments of the est and blest kernels.  No handle has AbVariant::Est or BlEst: eepacc_ab_step_est and
// eepacc_run_abmpc_preview run a handle of AbVariant::Plain through the est kernels, eepacc_bl_step_est and
// eepacc_run_blmpc_preview one of AbVariant::Baseline through the blest kernels, on the handle's own state.
// Nor has one AbVariant::ClassesEst or ClassesBlEst: eepacc_classes_step_est and eepacc_run_classes_preview run a handle of
// AbVariant::Classes through the clsest kernels and one of AbVariant::ClassesBL through the blclsest kernels, whose pack
// holds the class map first and these arguments behind it.
struct AbSupplied { const double *s_est, *v_est, *s_tv_est; };            // device arrays [N+1][B]; s_est and v_est both or neither
struct AbPreview { const int32_t* idx; const double* frac; int n_lead; };   // device tables [N] (preview_tables, eepacc_cfg.h)

// kernel variant of a handle: the baseline controllers (bl_mode) come before the ICE-map fuel term and move blocking.
// AbVariant::Classes, ClassesBL and ClassesTV cannot be told from a DevCfg: a handle of eepacc_create_classes /
// eepacc_create_classes_bl carries that choice itself (ClassesBL: bl_mode = 1 in every class, ClassesTV: bl_mode = 2).
inline AbVariant ab_variant(const DevCfg& C) {
    if (C.bl_mode) return C.bl_mode == 2 ? AbVariant::TargetVehicle : AbVariant::Baseline;
    if (C.ab_fuel_term == 2) return C.mb_any ? AbVariant::IceMoveBlocking : AbVariant::Ice;
    return C.mb_any ? AbVariant::MoveBlocking : AbVariant::Plain;
}

size_t ab_smem_bytes(int N);
size_t ab_hb_doubles(int N, int B, int num_cus);
hipError_t set_max_smem();
int pick_chunk_steps(int n_steps, int B, int resident_waves);
// s_tv, v_tv, a_tv_prev: null for AbVariant::TargetVehicle, whose kernels read no lead inputs.
// AbVariant::Classes, ClassesBL, ClassesTV: dC is the class array DevCfg[n_classes] and class_of the device map [B] of the
// launch (ClassesTV takes null lead inputs like TargetVehicle); every other variant reads dC[0] alone and takes class_of = null (launch_postprocess: null selects the one-config kernel).
// sup / pv: not null launches the est kernels (variant AbVariant::Plain) or the blest kernels (AbVariant::Baseline) with
// these further arguments, and with class_of not null the clsest kernels (AbVariant::Classes) or the blclsest kernels
// (AbVariant::ClassesBL); no other variant has such kernels.
hipError_t launch_ab_step(const DevCfg* dC, const int32_t* class_of, int N, AbVariant variant, int B, const double* s, const double* v,
                          const double* a_prev, const double* t0, const double* s_tv, const double* v_tv,
                          const double* a_tv_prev, unsigned long long* codes, double* out, double* s_pred, double* v_pred,
                          int32_t* status, int32_t* iters, hipStream_t stream, const AbSupplied* sup = nullptr);
hipError_t launch_run_abmpc(const DevCfg* dC, const int32_t* class_of, int N, AbVariant variant, int B, int k_start, int n_steps, const double* s0,
                            const double* v0, const double* a_m1, const double* s_tv, const double* v_tv,
                            double* carry, unsigned long long* codes, double* traj,
                            int32_t* status, int32_t* iters_total, int* work_counter, int* done, int* err_word, int num_cus,
                            hipStream_t stream, const AbPreview* pv = nullptr);
hipError_t launch_postprocess(const DevCfg* dC, const int32_t* class_of, int B, int n_steps, const double* traj, double* rpm, double* Tm,
                              double* P, double* E, hipStream_t stream);

}  // namespace eepacc
#endif
