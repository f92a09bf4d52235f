// eepacc_fb.hip -- FBMPC per-step pipeline around the dense QP
// operator: measurement block + estimators + bounds + CreateQP_FB + condensing in one kernel
// (one workgroup per instance), then eepacc_qp_dense.hip, then extraction / plant carry.
//
// Reference: ABO/RunOpt_FBMPC.m:161-331 (loop), ABO/Functions/MPCs/CreateQP_FB.m:158-489 (QP),
// ABO/Functions/MPCs/TransformToDenseFormulation.m:30-91 (condensing).  The condensing is not
// done as literal dense products: with B_k = T_k/(lambda m) [0 0; 1 1] only the state rows of Psi
// are dense, and they are the columns Sv[.,i], Ss[.,i] of the speed / position sensitivities to
// the force of stage i; the sparse-form Hessian is block tridiagonal in (v,Fm,Fb)_k.  Each
// entry of the dense H, g, A is assembled directly from those pieces (O(N) work per entry), by the
// device functions of eepacc_fb_condense.h, which k_fb_qp (eepacc_fb_qp.hip) calls too.  The model
// update and the measurement block are this kernel's own.
//
// Dense variable order per stage (6): Fm, Fb, xi_v, xi_h, xi_s, xi_f.  Rows per stage: 26, in the
// order of CreateQP_FB.m:311-473, plus the two terminal rows :478-489.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "eepacc_fb.h"
#include "eepacc_fb_condense.h"
#include "eepacc_fb_rows.h"
#include "eepacc_stage.h"
#include "../../include/eepacc.h"

namespace eepacc {
namespace {

constexpr int FT = 256;
constexpr int kRowsPerStage = 26;

struct StageData {      // per-stage scalars in LDS
    double *s_est, *v_est, *stv_est, *v_lim, *v_curv, *v_stop, *v_TL, *a_min, *a_max, *j_min, *j_max;
    double *A22, *D2, *ds, *dv, *Dblk, *Oblk, *cs, *tmp, *Sv, *Ss, *scal;
};

__device__ void carve(StageData& S, double* p, int N) {
    const int n1 = N + 1;
    S.s_est = p; p += n1; S.v_est = p; p += n1; S.stv_est = p; p += n1;
    S.v_lim = p; p += n1; S.v_curv = p; p += n1; S.v_stop = p; p += n1; S.v_TL = p; p += n1;
    S.a_min = p; p += n1; S.a_max = p; p += n1; S.j_min = p; p += n1; S.j_max = p; p += n1;
    S.A22 = p; p += n1; S.D2 = p; p += n1; S.ds = p; p += n1; S.dv = p; p += n1;
    S.Dblk = p; p += 9 * n1; S.Oblk = p; p += 9 * n1; S.cs = p; p += 3 * n1; S.tmp = p; p += 3 * n1;
    S.Sv = p; p += (size_t)n1 * N; S.Ss = p; p += (size_t)n1 * N; S.scal = p; p += 16;
}

__global__ void __launch_bounds__(FT) k_fb_build(eepacc_fb_args a) {
    extern __shared__ __align__(16) double smem_d[];
    const DevCfg& C = *a.cfg;
    const int N = C.N, B = a.B, b = a.b0 + blockIdx.x, tid = threadIdx.x;
    const int nV = 6 * N, nC = fb_qp_num_rows(C);
    StageData S;
    carve(S, smem_d, N);
    const double Ts = C.Tvec[0];
    const double lm = C.lambda * C.m, za = C.zeta_a;
    const double zeta_rg = C.m * C.g * (C.c_r * C.cos_theta0 + C.sin_theta0);
    // ---- measurement block (ABO/RunOpt_FBMPC.m:165-200)
    if (tid == 0) {
        double s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, vtvm = 0.0;
        if (a.mode == 0) {
            s = a.s[b]; v = a.v[b]; a_prev = a.a_prev[b]; t0 = a.t0[b];
            s_tv = a.s_tv[b]; v_tv = a.v_tv[b]; a_tv_prev = a.a_tv_prev[b];
        } else if (a.k_step == 0) {
            s = a.s[b]; v = a.v[b]; a_prev = a.a_prev[b]; t0 = 0.0;
            s_tv = a.s_tv[b]; v_tv = 0.0; a_tv_prev = 0.0; vtvm = 0.0;
        } else {
            const double s_prev = a.carry[0 * (size_t)B + b], v_prev = a.carry[1 * (size_t)B + b];
            const double Fm = a.carry[2 * (size_t)B + b], Fb = a.carry[3 * (size_t)B + b];
            const double vtv_prev = a.carry[4 * (size_t)B + b];
            plant_rk4(C, s_prev, v_prev, Fm + Fb, s, v);                                // :188
            a_prev = (v - v_prev) / Ts;
            t0 = a.k_step * Ts;
            s_tv = a.s_tv[b];
            vtvm = a.v_tv[b];
            v_tv = vtvm;
            a_tv_prev = (vtvm - vtv_prev) / Ts;
            S.scal[8] = v_prev;
        }
        S.scal[0] = s; S.scal[1] = v; S.scal[2] = a_prev; S.scal[3] = t0;
        S.scal[4] = s_tv; S.scal[5] = v_tv; S.scal[6] = a_tv_prev; S.scal[7] = vtvm;
    }
    __syncthreads();
    const double s_0 = S.scal[0], v_0 = S.scal[1], a_minus1 = S.scal[2], t_0 = S.scal[3];
    // ---- estimators and bounds (A2, A3)
    if (tid <= N) {
        double se, ve, st, vt;
        if (C.paramEstSetting == 2) {
            // EstimateVehicleTrajectory.m:81-88: [x_curr; prev(3:end); prev(end) + Ts v_prev(end)]
            const int idx = tid < N ? tid + 1 : N;
            const double ps = a.sp_prev[(size_t)idx * B + b], pv = a.vp_prev[(size_t)idx * B + b];
            se = tid == 0 ? s_0 : (tid < N ? ps : ps + C.Tvec[N - 1] * pv);
            ve = tid == 0 ? v_0 : pv;
        } else {
            estimate_traj(C, C.paramEstSetting, C.tConstACC_ego, s_0, v_0, a_minus1, tid, se, ve);
        }
        estimate_traj(C, C.TVestSetting, C.tConstACC_tar, S.scal[4], S.scal[5], S.scal[6], tid, st, vt);
        S.s_est[tid] = se; S.v_est[tid] = ve; S.stv_est[tid] = st;
        if (tid < N)
            route_bounds(C, se, ve, t_0, tid, S.v_lim[tid], S.v_curv[tid], S.v_stop[tid], S.v_TL[tid],
                         S.a_min[tid], S.a_max[tid], S.j_min[tid], S.j_max[tid]);
    }
    __syncthreads();
    // ---- state-space model with the A(k)/D(k) index quirk (ABO/RunOpt_FBMPC.m:78-90, 247-259)
    if (tid < N) {
        const int k = tid;
        double A22 = a.A22[(size_t)k * B + b], D2 = a.D2[(size_t)k * B + b];
        if (a.k_step == 0) {
            if (C.FBuseTaylor) { A22 = 1.0 - 2.0 * C.Tvec[k] * za * v_0 * v_0 / lm; D2 = C.Tvec[k] / lm * (za * v_0 * v_0); }
            else { A22 = 1.0; D2 = C.Tvec[k] / lm * (-za * v_0 * v_0); }
        }
        if (C.FBuseTaylor) {
            if (k == a.k_step) {
                const int i = N - 1;
                const double vi = S.v_est[i];
                A22 = 1.0 - 2.0 * C.Tvec[i] * za * vi / lm;
                D2 = C.Tvec[i] / lm * (za * vi * vi - zeta_rg);
            }
        } else {
            const double vi = S.v_est[k];
            D2 = C.Tvec[k] / lm * (-za * vi * vi - zeta_rg);
        }
        a.A22[(size_t)k * B + b] = A22; a.D2[(size_t)k * B + b] = D2;
        S.A22[k] = A22; S.D2[k] = D2;
    }
    __syncthreads();
    // ---- sensitivities of (s_k, v_k) to the force of stage i, and the free response d (eepacc_fb_condense.h)
    if (tid < N) fb_sens_column(C, S, S.Sv, S.Ss, N, tid, lm);
    else if (tid == N) fb_free_response(C, S, s_0, v_0);
    // ---- block-tridiagonal sparse-form Hessian over (v,Fm,Fb)_k and linear term (CreateQP_FB.m:181-215)
    if (tid <= N) fb_hessian_blocks(C, S, tid, v_0, a_minus1, lm, za, zeta_rg);
    __syncthreads();
    // tmp = Hs d + cs on the (v,Fm,Fb) rows
    if (tid < 3 * N) fb_tmp_entry(C, S, tid);
    __syncthreads();
    const size_t lb_ = blockIdx.x;                         // index inside the chunk the QP arrays hold
    double* Hd = a.H + lb_ * nV * nV;
    double* gd = a.g + lb_ * nV;
    double* Ad = a.A + lb_ * nC * nV;
    // ---- g, H
    const double h_xih = 2.0 * C.fb_w[4];
    for (int col = tid; col < nV; col += FT) gd[col] = fb_g_entry(C, S, S.Sv, N, N, col);
    for (int idx = tid; idx < nV * nV; idx += FT) Hd[idx] = fb_H_entry(S, S.Sv, N, N, h_xih, idx / nV, idx % nV);
    // ---- A (column-major nC x nV), lba, uba
    for (int r = tid; r < nC; r += FT) {
        // stage of row r (stages own 26 rows, 28 with the two blocked-move rows CreateQP_FB.m:346-356 after the bounds)
        int k = r / kRowsPerStage < N ? r / kRowsPerStage : N;
        while (k > 0 && r < C.fb_row0[k]) --k;
        while (k < N && r >= C.fb_row0[k + 1]) ++k;
        int t = r - C.fb_row0[k];
        RowDesc R;
        if (k < N && C.mb_mask[k] && (t == 8 || t == 9)) {
            R.as = R.av = R.aFm = R.aFb = R.aFmp = R.aFbp = R.sc = 0.0;
            R.slack = -1; R.lb = 0.0; R.ub = 0.0;
            if (t == 8) { R.aFmp = 1.0; R.aFm = -1.0; } else { R.aFbp = 1.0; R.aFb = -1.0; }
        } else {
            if (k < N && C.mb_mask[k] && t > 9) t -= 2;
            R = fb_row(C, S, k, t, s_0, v_0, a_minus1);
        }
        const double shift = R.as * S.ds[k] + R.av * S.dv[k];
        a.lba[lb_ * nC + r] = R.lb - shift;
        a.uba[lb_ * nC + r] = R.ub - shift;
        for (int i = 0; i < N; ++i) {
            double cF[2];
            fb_A_entry(R, S.Ss + (size_t)k * N, S.Sv + (size_t)k * N, k, i, cF);
            Ad[(size_t)(6 * i + 0) * nC + r] = cF[0];
            Ad[(size_t)(6 * i + 1) * nC + r] = cF[1];
#pragma unroll
            for (int c = 0; c < 4; ++c) Ad[(size_t)(6 * i + 2 + c) * nC + r] = (i == k && c == R.slack) ? R.sc : 0.0;
        }
    }
    if (tid == 0) {
        a.meas[0 * (size_t)B + b] = s_0;
        a.meas[1 * (size_t)B + b] = v_0;
        a.meas[2 * (size_t)B + b] = S.s_est[N] - s_0;          // DistHor (:208)
        a.meas[3 * (size_t)B + b] = S.scal[7];                 // lead speed carried to the next step
        a.meas[4 * (size_t)B + b] = (a.mode == 1 && a.k_step > 0) ? (v_0 - S.scal[8]) / Ts : 0.0;   // a_opt(k) (:316-318)
    }
}

// extraction (ABO/RunOpt_FBMPC.m:291-318) and closed-loop carry; thread per instance
__global__ void k_fb_apply(eepacc_fb_apply_args a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const DevCfg& C = *a.cfg;
    const int N = C.N, B = a.B, nV = 6 * N;
    const double* x = a.x + (size_t)b * nV;
    const double s = a.meas[0 * (size_t)B + b], v = a.meas[1 * (size_t)B + b];
    double* o = a.out;
    o[(size_t)EEPACC_OUT_S * B + b] = s;
    o[(size_t)EEPACC_OUT_V * B + b] = v;
    o[(size_t)EEPACC_OUT_FM * B + b] = x[0];
    o[(size_t)EEPACC_OUT_FB * B + b] = x[1];
    o[(size_t)EEPACC_OUT_A * B + b] = a.meas[4 * (size_t)B + b];
    o[(size_t)EEPACC_OUT_XI_V * B + b] = x[2];
    o[(size_t)EEPACC_OUT_XI_H * B + b] = x[3];
    o[(size_t)EEPACC_OUT_XI_S * B + b] = x[4];
    o[(size_t)EEPACC_OUT_XI_F * B + b] = x[5];
    o[(size_t)EEPACC_OUT_COST * B + b] = a.cost[b];
    o[(size_t)EEPACC_OUT_DISTHOR * B + b] = a.meas[2 * (size_t)B + b];
    o[(size_t)EEPACC_OUT_AQP * B + b] = 0.0;
    if (a.status) a.status[b] = a.qp_status[b];
    if (a.s_pred && a.v_pred) {
        const double lm = C.lambda * C.m;
        double ss = s, sv = v;
        a.s_pred[b] = ss; a.v_pred[b] = sv;
        for (int k = 0; k < N; ++k) {
            const double T = C.Tvec[k];
            const double ns = ss + T * sv;
            sv = a.A22[(size_t)k * B + b] * sv + T / lm * (x[6 * k] + x[6 * k + 1]) + a.D2[(size_t)k * B + b];
            ss = ns;
            a.s_pred[(size_t)(k + 1) * B + b] = ss; a.v_pred[(size_t)(k + 1) * B + b] = sv;
        }
    }
    if (a.carry) {
        a.carry[0 * (size_t)B + b] = s; a.carry[1 * (size_t)B + b] = v;
        a.carry[2 * (size_t)B + b] = x[0]; a.carry[3 * (size_t)B + b] = x[1];
        a.carry[4 * (size_t)B + b] = a.meas[3 * (size_t)B + b];
    }
}

}  // namespace

size_t fb_build_smem_bytes(int N) {
    const size_t n1 = (size_t)N + 1;
    return (15 * n1 + 18 * n1 + 6 * n1 + 2 * n1 * N + 16) * sizeof(double);
}

hipError_t launch_fb_build(const eepacc_fb_args& a, int N, hipStream_t stream) {
    const size_t smem = fb_build_smem_bytes(N);
    hipError_t e = hipFuncSetAttribute((const void*)k_fb_build, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fb_build, dim3(a.nb), dim3(FT), smem, stream, a);
    return hipGetLastError();
}

hipError_t launch_fb_apply(const eepacc_fb_apply_args& a, hipStream_t stream) {
    hipLaunchKernelGGL(k_fb_apply, dim3((a.B + 255) / 256), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace eepacc
