// eepacc_fb_qp.h -- the condensed QP of one FBMPC step as data (eepacc_fb_qp.hip): arguments and launcher.  The row
// catalogue is eepacc_fb_rows.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include "eepacc_device.h"

namespace eepacc {

// An array of the carried FBMPC state as the builder reads it: entry k of instance b is p[k * sk + b * sb].  The structured
// path keeps it instance-major (fbs_state), the dense path and a caller's arrays stage-major ([N][B]).
struct FbCarried {
    const double* p;
    size_t sk, sb;
    __host__ __device__ double at(int k, size_t b) const { return p[(size_t)k * sk + b * sb]; }
};

struct fb_qp_args {
    const DevCfg* cfg;
    int B, nC;
    // k_step >= 0: the model of MPC step k_step from the carried entries (RunOpt_FBMPC.m:78-90, 247-259; A22.p == NULL at
    // step 0, where none is read).  k_step < 0: A22, D2 are the model as it is.  Neither is read with FBuseTaylor = 0.
    int k_step;
    const double *s, *v, *a_prev, *t0, *s_tv, *v_tv, *a_tv_prev;   // [B]
    FbCarried A22, D2;
    FbCarried sp, vp;           // predictions of the previous step (paramEstSetting 2), k = 0 .. N; p == NULL: zeros
    double *H, *g, *A, *lba, *uba;      // [B][nV*nV], [B][nV], [B][nV][nC], [B][nC], [B][nC]
    double *A22_used, *D2_used;         // [N][B] or NULL
};

// B workgroups of 256 threads; every entry of the outputs is written.  Nothing else is.
hipError_t launch_fb_qp(const fb_qp_args& a, int N, hipStream_t stream);
// The same on the caller's horizon guesses (eepacc_fb_qp_est.hip): device arrays [N+1][B], s_est and v_est both or neither,
// a null array keeps the estimator's guess.  All three null: the arrays of launch_fb_qp.
hipError_t launch_fb_qp_est(const fb_qp_args& a, int N, hipStream_t stream, const double* s_est, const double* v_est,
                            const double* s_tv_est);
size_t fb_qp_smem_bytes(int N, int nC);     // static + dynamic LDS of a workgroup

}  // namespace eepacc
