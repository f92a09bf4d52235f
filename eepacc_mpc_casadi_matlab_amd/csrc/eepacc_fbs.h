// Internal interface of the structured FBMPC kernels (eepacc_fbs.hip).
#ifndef EEPACC_FBS_H
#define EEPACC_FBS_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "eepacc_device.h"

namespace eepacc {

// per-instance state the structured FBMPC path carries between launches (HBM, instance-major)
constexpr int kFbsStateDoubles = 64 + 64 + 64 + 64 + 64;   // codes | A22 | D2 | s_pred | v_pred

struct fbs_step_args {          // B2: one step (ABO/RunOpt_FBMPC.m:204-320)
    const DevCfg* cfg;
    int B, k_step;
    const double *s, *v, *a_prev, *t0, *s_tv, *v_tv, *a_tv_prev;   // [B]
    double* state;              // [B][kFbsStateDoubles]
    double* hb;                 // [waves of the launch][NS*NS] scratch: base inverse Hessian of the step
    double *out, *s_pred, *v_pred;
    int32_t *status, *iters;
};

struct fbs_run_args {           // B1: closed loop (ABO/RunOpt_FBMPC.m:161-331)
    const DevCfg* cfg;
    int B, k_start, n_steps;
    const double *s0, *v0, *a_m1, *s_tv, *v_tv;
    double* carry;              // [6][B]: s, v, Fm, Fb of the previous step, previous lead speed, t_0
    double* state;              // [B][kFbsStateDoubles]
    double* hb;                 // [waves of the launch][NS*NS] scratch
    double* traj;
    int32_t *status, *iters_total;
    int *work_counter, *done, *err_word;
    int chunk_steps, spin_limit;    // spin_limit: set by launch_fbs_run
    int cold;                   // debug: 1 = no working-set warm start between MPC steps
};

// the two size classes of the kernels (eepacc_fbs.hip and eepacc_fbs_est.hip instantiate the same two)
constexpr int kFMMaxSmall = 32, kFNSSmall = 32, kFWpbSmall = 7;     // N <= 32: 21.7 KB of LDS per wave, one block of 7 waves per CU
                                                                    // (working-set rows are independent in the N-dimensional u-space: m <= N)
constexpr int kFMMaxLarge = 66, kFNSLarge = 64, kFWpbLarge = 1;     // N <= 63

// dynamic LDS a block may ask for: 160 KB per CU minus the kernels' static index table (one ushort per packed entry of P)
constexpr size_t kFbsLdsBudget = 160 * 1024 - 4608;

const char* fbs_unsupported_field(const DevCfg& C);     // eepacc_cfg.cpp (declared in eepacc_cfg.h too): NULL, or what the solver lacks
bool fbs_supported(const DevCfg& C);
size_t fbs_smem_bytes(int N);
int fbs_run_max_grid(int N, int num_cus);           // blocks of a chip-filling closed-loop launch
size_t fbs_hb_doubles(int N, int B, int num_cus);   // scratch a launch for B instances needs
hipError_t fbs_set_max_smem();
// Resident waves that eepacc_run_fbmpc sizes its work units for (pick_chunk_steps): the N <= 32 kernel's one block of 7 waves
// per CU, which is what launch_fbs_run's grid gives there.  The same 7 per CU is used at N > 32, where one-wave blocks share
// the LDS and fewer waves are resident: the units of a short launch come out shorter there than the rule intends.  Kept as it
// is, since the unit length enters the results' launch geometry.
inline int fbs_run_chunking_waves(int /*N*/, int num_cus) { return num_cus * 7; }
hipError_t launch_fbs_step(const fbs_step_args& a, int N, hipStream_t stream);
hipError_t launch_fbs_run(fbs_run_args a, int N, int num_cus, hipStream_t stream);

// The kernels with horizon guesses from the caller (eepacc_fbs_est.hip), on the same state, scratch and grids.
// Step: device arrays [N+1][B]; s_est and v_est both or neither, a null array keeps the estimator's guess of that side.
// Closed loop: a.s_tv, a.v_tv are [n_lead][B] and the lead's guess of every step is read from them through the handle's
// preview tables idx, frac [N] (eepacc::preview_tables); the ego estimator stays the handle's.
hipError_t fbs_est_set_max_smem();
hipError_t launch_fbs_step_est(const fbs_step_args& a, int N, hipStream_t stream, const double* s_est, const double* v_est,
                               const double* s_tv_est);
hipError_t launch_fbs_run_preview(fbs_run_args a, int N, int num_cus, hipStream_t stream, const int32_t* idx, const double* frac,
                                  int n_lead);

// The kernels of a handle with settings classes (eepacc_fbs_cls.hip), on the same scratch and grids.  a.cfg is the handle's
// class array DevCfg[n_classes] (N and Tvec are those of its head) and class_of [a.B] the class of every instance, on the device.
hipError_t fbs_cls_set_max_smem();
hipError_t launch_fbs_step_cls(const fbs_step_args& a, int N, hipStream_t stream, const int32_t* class_of);
hipError_t launch_fbs_run_cls(fbs_run_args a, int N, int num_cus, hipStream_t stream, const int32_t* class_of);

}  // namespace eepacc
#endif
