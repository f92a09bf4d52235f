// eepacc_fb_rows.h -- the row catalogue of the FBMPC QP (CreateQP_FB.m:311-489), shared by the build kernel of the dense
// FBMPC path (eepacc_fb.hip) and the kernel that writes the problem out as data (eepacc_fb_qp.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_device.h"
#include "../../include/eepacc.h"

namespace eepacc {

struct RowDesc {
    double as, av, aFm, aFb, aFmp, aFbp, sc;   // coefficients; sc = slack coefficient
    int slack;                                  // 0..3 = xi_v, xi_h, xi_s, xi_f ; -1 none
    double lb, ub;
};

// row t of stage k among the 26 every stage has (k == N: terminal rows t = 0,1).  SD: the per-stage estimates and bounds of
// the step, indexable members v_est, stv_est, v_lim, v_curv, v_stop, v_TL, a_min, a_max, j_min, j_max.
template <class SD>
__device__ RowDesc fb_row(const DevCfg& C, const SD& S, int k, int t, double s_0, double v_0, double a_minus1) {
    RowDesc R;
    R.as = R.av = R.aFm = R.aFb = R.aFmp = R.aFbp = R.sc = 0.0;
    R.slack = -1; R.lb = -INFINITY; R.ub = INFINITY;
    const int N = C.N;
    const double lm = C.lambda * C.m, za = C.zeta_a;
    const double zeta_rg = C.m * C.g * (C.c_r * C.cos_theta0 + C.sin_theta0);
    if (k == N) {                                           // CreateQP_FB.m:478-489
        R.as = 1.0;
        if (t == 0) R.ub = S.stv_est[N - 1] - C.h_min;
        else { R.av = C.tau_min; R.ub = S.stv_est[N - 1]; }
        return R;
    }
    const double ve = S.v_est[k], Tp = C.Tvec[k];
    const double base = za * ve * ve + zeta_rg;
    switch (t) {
    case 0: R.as = 1.0; R.lb = s_0; R.ub = C.s_goal; break;                       // :311-342
    case 1: R.av = 1.0; R.lb = 0.0; R.ub = C.v_max; break;
    case 2: R.aFm = 1.0; R.lb = -1e4; R.ub = 1e4; break;
    case 3: R.aFb = 1.0; R.lb = -1e4; R.ub = 0.0; break;
    case 4: R.slack = 0; R.sc = 1.0; R.lb = 0.0; break;
    case 5: R.slack = 1; R.sc = 1.0; R.lb = 0.0; break;
    case 6: R.slack = 2; R.sc = 1.0; R.lb = 0.0; break;
    case 7: R.slack = 3; R.sc = 1.0; R.lb = 0.0; break;
    case 8: {                                                                       // :359-366
        double cv = C.phi * C.T_m_max * C.T_m_max / 4.0 / C.P_m_max;
        R.av = -cv; R.aFm = C.eta_TF / C.phi; R.slack = 3; R.sc = 1.0; R.lb = -C.T_m_max; break; }
    case 9: {
        double cv = C.phi * C.T_m_max * C.T_m_max / 4.0 / C.P_m_max;
        R.av = cv; R.aFm = 1.0 / C.eta_TF / C.phi; R.slack = 3; R.sc = -1.0; R.ub = C.T_m_max; break; }
    case 10: {                                                                      // :369-377
        double zeta_w = C.m * C.g * (C.L_f * C.cos_theta0 + C.h_g * C.sin_theta0);
        R.aFm = C.L / C.mu + C.h_g; R.aFb = C.h_g; R.slack = 3; R.sc = 1.0; R.lb = -zeta_w + C.h_g * zeta_rg; break; }
    case 11: {
        double zeta_w = C.m * C.g * (C.L_f * C.cos_theta0 + C.h_g * C.sin_theta0);
        R.aFm = C.L / C.mu - C.h_g; R.aFb = -C.h_g; R.slack = 3; R.sc = -1.0; R.ub = zeta_w - C.h_g * zeta_rg; break; }
    case 12: R.aFm = 1.0; R.aFb = 1.0; R.slack = 3; R.sc = -1.0; R.ub = C.mu * C.m * C.g * C.cos_theta0; break;   // :380-387
    case 13: R.aFm = 1.0; R.aFb = 1.0; R.slack = 3; R.sc = 1.0; R.lb = -C.mu * C.m * C.g * C.cos_theta0; break;
    case 14: R.aFm = 1.0; R.aFb = 1.0; R.slack = 3; R.sc = -1.0; R.ub = lm * S.a_max[k] + base; break;            // :390-397
    case 15: R.aFm = 1.0; R.aFb = 1.0; R.slack = 3; R.sc = 1.0; R.lb = lm * S.a_min[k] + base; break;
    case 16: case 17: {                                                             // :400-418
        R.aFm = 1.0; R.aFb = 1.0; R.slack = 3;
        double rhs_j = (t == 16) ? S.j_max[k] : S.j_min[k], rhs;
        if (k == 0) rhs = lm * (Tp * rhs_j + a_minus1) + base;
        else {
            double vp = S.v_est[k - 1];
            R.aFmp = -1.0; R.aFbp = -1.0;
            rhs = lm * Tp * rhs_j + za * (ve * ve - vp * vp);      // + Dzeta_rg = 0: slope_est is constant
        }
        if (t == 16) { R.sc = -1.0; R.ub = rhs; } else { R.sc = 1.0; R.lb = rhs; }
        break; }
    case 18: R.av = 1.0; R.slack = 3; R.sc = -1.0; R.ub = S.v_lim[k]; break;        // :421-442
    case 19: R.av = 1.0; R.slack = 3; R.sc = -1.0; R.ub = S.v_curv[k]; break;
    case 20: R.av = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.v_stop[k]; break;
    case 21: R.av = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.v_TL[k]; break;
    case 22: R.av = 1.0; R.slack = 0; R.sc = 1.0; R.lb = fmin(S.v_lim[k], S.v_curv[k]); break;   // :445-448
    case 23: R.as = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.stv_est[k] - C.h_min; break;        // :451-458
    case 24: R.as = 1.0; R.av = C.tau_min; R.slack = 2; R.sc = -1.0; R.ub = S.stv_est[k]; break;
    default: {                                                                      // :461-473
        const double T_hwp = 2.0, A_hwp = 2.0, G_hwp = -0.0246 * T_hwp + 0.010819;
        R.as = 1.0; R.slack = 1; R.sc = -1.0;
        if (C.FBuseTaylor) { R.av = T_hwp + 2.0 * G_hwp * ve; R.ub = S.stv_est[k] - A_hwp + G_hwp * ve * ve; }
        else { R.av = T_hwp + G_hwp * ve; R.ub = S.stv_est[k] - A_hwp; }
        break; }
    }
    return R;
}

// The values of EEPACC_FB_ROW_* ascend in the order in which CreateQP_FB.m:311-473 appends the rows of a stage: the 26 rows
// above with the two blocked-move rows (:346-356, only on a stage with Mb = 1) after the eight bounds.  Host
// (eepacc_fb_qp_rows) and kernel share this.
__host__ __device__ inline bool fb_row_present(int type, int blocked) {
    return (type != EEPACC_FB_ROW_BLOCKED_FM && type != EEPACC_FB_ROW_BLOCKED_FB) || blocked != 0;
}

// Rows of the problem: those of the stages and the two terminal rows
__host__ __device__ inline int fb_qp_num_rows(const DevCfg& C) { return C.fb_row0[C.N] + 2; }

// Row `type` (EEPACC_FB_ROW_*) of stage k; k == N: the two terminal rows, EEPACC_FB_ROW_SAFE1 and _SAFE2
template <class SD>
__device__ RowDesc fb_row_typed(const DevCfg& C, const SD& S, int k, int type, double s_0, double v_0, double a_minus1) {
    if (k == C.N) return fb_row(C, S, k, type == EEPACC_FB_ROW_SAFE1 ? 0 : 1, s_0, v_0, a_minus1);
    if (type == EEPACC_FB_ROW_BLOCKED_FM || type == EEPACC_FB_ROW_BLOCKED_FB) {
        RowDesc R;
        R.as = R.av = R.aFm = R.aFb = R.aFmp = R.aFbp = R.sc = 0.0;
        R.slack = -1; R.lb = 0.0; R.ub = 0.0;
        if (type == EEPACC_FB_ROW_BLOCKED_FM) { R.aFmp = 1.0; R.aFm = -1.0; } else { R.aFbp = 1.0; R.aFb = -1.0; }
        return R;
    }
    return fb_row(C, S, k, type < EEPACC_FB_ROW_BLOCKED_FM ? type : type - 2, s_0, v_0, a_minus1);
}

}  // namespace eepacc
