// eepacc_cfg.cpp -- the one-time host mathematics behind every kernel variant: what the settings are refused for, the tau
// prefix sums, the move-blocking maps, the objective constants, the condensed a-space Hessian and its inverse, and the tables
// of the key-figure kernels.  Host only (eepacc_cfg.h); the C-ABI (eepacc_capi.cpp) uploads what this unit returns.
#include <math.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include "eepacc_cfg.h"

namespace eepacc {

static int fail(int code, const std::string& msg) { return set_error(code, msg); }

// symmetric positive definite inverse (Gauss-Jordan in long double; N <= 63)
bool spd_inverse(std::vector<long double>& A, int n) {
    std::vector<long double> I((size_t)n * n, 0.0L);
    for (int i = 0; i < n; ++i) I[(size_t)i * n + i] = 1.0L;
    for (int k = 0; k < n; ++k) {
        long double d = A[(size_t)k * n + k];
        if (!(d > 0.0L)) return false;
        for (int j = 0; j < n; ++j) { A[(size_t)k * n + j] /= d; I[(size_t)k * n + j] /= d; }
        for (int i = 0; i < n; ++i) {
            if (i == k) continue;
            long double f = A[(size_t)i * n + k];
            if (f == 0.0L) continue;
            for (int j = 0; j < n; ++j) { A[(size_t)i * n + j] -= f * A[(size_t)k * n + j]; I[(size_t)i * n + j] -= f * I[(size_t)k * n + j]; }
        }
    }
    A.swap(I);
    return true;
}

int build_cfg(const eepacc_settings* S, const eepacc_vehicle* V, DevCfg& C, std::vector<double>& Hinv) {
    memset(&C, 0, sizeof(C));
    const int N = S->N_hor;
    if (N < 2 || N > eepacc::kMaxN) return fail(EEPACC_EINVAL, "N_hor must be in [2, 63]");
    if (!S->Tvec) return fail(EEPACC_EINVAL, "Tvec is NULL");
    // solverToUse 0 (sparse qpOASES) states the same QP as 1 (dense qpOASES) with the dynamics kept as
    // equality rows (CreateQP_AB.m:227-246): same feasible set and objective, hence the same minimiser and
    // the same kernels.  2 (HPIPM) is a different problem (hard bounds a in [-8, 8], :79-99).
    if (S->solverToUse != 0 && S->solverToUse != 1)
        return fail(EEPACC_ENOTSUP, "solverToUse == 2 (HPIPM formulation, ABO/Settings.m:114) is not built");
    if (S->paramEstSetting < 0 || S->paramEstSetting > 2) return fail(EEPACC_EINVAL, "paramEstSetting must be 0, 1 or 2");
    if (S->TVestSetting != 0 && S->TVestSetting != 1) return fail(EEPACC_EINVAL, "TVestSetting must be 0 or 1");
    if (S->n_speedLim < 1 || S->n_speedLim > eepacc::kMaxKnots || S->n_curv < 1 || S->n_curv > eepacc::kMaxKnots ||
        S->n_slope < 1 || S->n_slope > eepacc::kMaxKnots || S->n_stop < 0 || S->n_stop > eepacc::kMaxStops ||
        S->n_TL < 0 || S->n_TL > eepacc::kMaxTL)
        return fail(EEPACC_EINVAL, "route table sizes out of range");
    if (S->N_integratePlant < 1) return fail(EEPACC_EINVAL, "N_integratePlant < 1");
    if (S->ab_fuel_term < 0 || S->ab_fuel_term > 2) return fail(EEPACC_EINVAL, "ab_fuel_term must be 0, 1 or 2");
    if (S->ab_fuel_term == 2 && !S->bl_mode) {
        // ICE-map fuel term (CreateQP_AB.m:154-159): step-varying Hessian, built (folded for Mb) and inverted in LDS by its
        // own kernel variant, at every N and with or without move blocking
        if (!(V->tau_fd > 0.0) || !(V->eta_drive > 0.0) || !(V->R_w > 0.0))
            return fail(EEPACC_EINVAL, "ab_fuel_term == 2 needs V.tau_fd, V.eta_drive, V.R_w > 0 (SetVehicleParameters.m:92,100-101)");
        for (int g2 = 0; g2 < 8; ++g2) if (!(V->tau_gb[g2] > 0.0)) return fail(EEPACC_EINVAL, "ab_fuel_term == 2 needs positive gear ratios V.tau_gb");
        for (int g2 = 1; g2 < 7; ++g2) if (!(V->upSpd[g2] >= V->upSpd[g2 - 1])) return fail(EEPACC_EINVAL, "V.upSpd must ascend");
    }
    C.N = N;
    C.ab_fuel_term = S->ab_fuel_term; C.ab_route_rows = S->ab_route_rows;
    C.paramEstSetting = S->paramEstSetting; C.TVestSetting = S->TVestSetting;
    C.N_integratePlant = S->N_integratePlant;
    C.max_iter = 60 * N + 200;
    C.const_T = 1;
    C.tau[0] = 0.0;
    for (int k = 0; k < N; ++k) {
        if (!(S->Tvec[k] > 0.0)) return fail(EEPACC_EINVAL, "Tvec entries must be positive");
        C.Tvec[k] = S->Tvec[k];
        C.tau[k + 1] = C.tau[k] + S->Tvec[k];
        if (S->Tvec[k] != S->Tvec[0]) C.const_T = 0;
        if (S->Mb && S->Mb[k] != 0) C.mb_any = 1;
    }
    if (C.mb_any) {
        // block structure: stage k with Mb[k] = 1 repeats the acceleration of the previous stage
        if (S->Mb[0] != 0) return fail(EEPACC_EINVAL, "Mb[0] must be 0 (the first stage has no predecessor in the horizon)");
        int maxlen = 1;
        for (int k = 0, lead = 0; k < N; ++k) {
            if (S->Mb[k] != 0 && S->Mb[k] != 1) return fail(EEPACC_EINVAL, "Mb entries must be 0 or 1");
            if (S->Mb[k] == 0) lead = k;
            C.mb_lead[k] = lead;
            C.mb_end[lead] = k;
            if (k - lead + 1 > maxlen) maxlen = k - lead + 1;
        }
        for (int k = 0; k < N; ++k) if (C.mb_lead[k] != k) C.mb_end[k] = k;
        C.mb_lead[N] = N; C.mb_end[N] = N;
        C.mb_maxlen = maxlen;
    } else {
        for (int k = 0; k <= N; ++k) { C.mb_lead[k] = k; C.mb_end[k] = k; }
        C.mb_maxlen = 1;
    }
    C.fb_row0[0] = 0;
    for (int k = 0; k < N; ++k) {
        C.mb_mask[k] = (S->Mb && S->Mb[k] == 1) ? 1 : 0;
        C.fb_row0[k + 1] = C.fb_row0[k] + 26 + 2 * C.mb_mask[k];
    }
    C.mb_mask[N] = 0;
    C.w_FC = S->ab_fuel_term ? S->W_AB[0] : 0.0;
    C.w_a = S->W_AB[1]; C.w_j = S->W_AB[2]; C.w_v = S->W_AB[3]; C.w_h = S->W_AB[4]; C.w_s = S->W_AB[5]; C.w_f = S->W_AB[6];
    // default: above the noise level of the closed loop at standstill -- ABMPC 1e-10; the baseline LP (solved with the
    // curvature 1e-4) leaves 2e-9 on plain stops and up to 1.5e-6 when its slack is in play (use case 12)
    C.state_tol = S->state_bound_tol > 0.0 ? S->state_bound_tol : (S->bl_mode ? 1e-5 : 1e-9);
    double bl_travel = 0.0;
    if (S->bl_mode) {
        // the LP needs about 13 working-set changes per warm step and 3N from cold (871 saved steps at N = 20 as cold QPs:
        // mean 58, 99th percentile 113, maximum 270); a solve that is still going after 15N + 60 is cycling on a degenerate
        // vertex and is cut off there
        C.max_iter = 15 * N + 60;
        if (const char* ev = getenv("EEPACC_DEBUG_BL_MAX_ITER")) C.max_iter = atoi(ev);
        // RunOpt_BLMPC: CreateQP_BL.m:36-39,131-148  W_BL = [w_v (travel incentive), w_a, w_j, w_f]
        // bl_mode = 2: RunOpt_TVMPC, CreateQP_TV.m:36-39 W_TV = [w_v, w_a, w_j, w_f] in W_BL, TV_*_Lim* in BL_*_Lim*
        if (S->bl_mode != 1 && S->bl_mode != 2) return fail(EEPACC_EINVAL, "bl_mode must be 0, 1 (RunOpt_BLMPC) or 2 (RunOpt_TVMPC)");
        if (C.mb_any) return fail(EEPACC_ENOTSUP, "the baseline controller has no move blocking (RunOpt_BLMPC.m)");
        if (S->bl_mode == 2 && !C.const_T)
            return fail(EEPACC_EINVAL, "bl_mode = 2: Tvec must be uniform (TV_Ts, CreateQP_TV.m:29)");
        if (S->W_BL[0] < 0 || S->W_BL[1] < 0 || S->W_BL[2] < 0 || !(S->W_BL[3] > 0))
            return fail(EEPACC_EINVAL, "W_BL weights must be non-negative (w_f positive)");
        C.bl_mode = S->bl_mode;
        C.ab_fuel_term = 0; C.ab_route_rows = 1;            // CreateQP_BL.m:264-288: the four speed caps are always present
        C.w_FC = 0.0; C.w_a = S->W_BL[1]; C.w_j = S->W_BL[2]; C.w_f = S->W_BL[3];
        C.w_v = 0.0; C.w_s = 0.0; C.w_h = 1.0;              // groups that do not exist in the baseline QP
        bl_travel = S->W_BL[0];
        C.bl_eps = (C.w_a == 0.0 && C.w_j == 0.0) ? (S->bl_lp_eps > 0.0 ? S->bl_lp_eps : 0.1) : 0.0;
        if (const char* ev = getenv("EEPACC_DEBUG_BL_EPS")) { if (C.bl_eps > 0.0 && atof(ev) > 0.0) C.bl_eps = atof(ev); }
        C.bl_prox_max = C.bl_eps > 0.0 ? (S->bl_prox_iter == 0 ? 40 : (S->bl_prox_iter < 0 ? 0 : S->bl_prox_iter)) : 0;
        C.bl_aLo = S->BL_a_LimLowVel; C.bl_aHi = S->BL_a_LimHighVel; C.bl_jLo = S->BL_j_LimLowVel; C.bl_jHi = S->BL_j_LimHighVel;
        if (!(C.bl_aLo > 0) || !(C.bl_aHi > 0) || !(C.bl_jLo > 0) || !(C.bl_jHi > 0))
            return fail(EEPACC_EINVAL, "baseline acceleration / jerk limits must be positive");
    } else if (!(C.w_a > 0.0) || !(C.w_h > 0.0) || C.w_v < 0 || C.w_s < 0 || C.w_f < 0 || C.w_j < 0)
        return fail(EEPACC_EINVAL, "W_AB weights must be positive (w_a, w_h) / non-negative");
    C.tau_min = S->tau_min; C.h_min = S->h_min; C.s_goal = S->s_goal;
    C.tConstACC_ego = S->tConstACC_ego; C.tConstACC_tar = S->tConstACC_tar;
    C.m = V->m; C.lambda = V->lambda; C.g = V->g; C.zeta_a = V->zeta_a; C.c_r = V->c_r; C.mu = V->mu; C.L = V->L;
    C.L_f = V->L_f; C.h_g = V->h_g; C.phi = V->phi; C.T_m_max = V->T_m_max; C.P_m_max = V->P_m_max;
    C.eta_TF = V->eta_TF; C.omega_m_r = V->omega_m_r; C.v_max = V->v_max;
    C.p01 = V->p01; C.p10 = V->p10; C.F2 = V->F2;
    C.cq = C.w_FC * V->p01 * V->F2;
    C.glin_v = C.bl_mode ? -bl_travel : C.w_FC * V->p10;
    C.glin_a = C.w_FC * V->p01 * V->lambda * V->m;
    if (C.ab_fuel_term == 2) {
        // per stage: cq_k = ice_cq / tau_k, lv_k = ice_lv tau_k, la_k = ice_la / tau_k (CreateQP_AB.m:154-159)
        C.cq = 0.0; C.glin_v = 0.0; C.glin_a = 0.0;
        C.ice_cq = C.w_FC * V->k01 * V->F2 * V->R_w / V->tau_fd / V->eta_drive;
        C.ice_lv = C.w_FC * V->k10 / V->R_w * V->tau_fd;
        C.ice_la = C.w_FC * V->k01 * V->lambda * V->m * V->R_w / V->tau_fd / V->eta_drive;
        for (int g2 = 0; g2 < 7; ++g2) C.ice_up[g2] = V->upSpd[g2];
        for (int g2 = 0; g2 < 8; ++g2) C.ice_gb[g2] = V->tau_gb[g2];
    }
    C.n_speedLim = S->n_speedLim; C.n_curv = S->n_curv; C.n_slope = S->n_slope; C.n_stop = S->n_stop; C.n_TL = S->n_TL;
    for (int i = 0; i < S->n_speedLim; ++i) { C.s_speedLim[i] = S->s_speedLim[i]; C.v_speedLim[i] = S->v_speedLim[i]; }
    const double alpha = S->alpha_TTL;
    for (int i = 0; i < S->n_curv; ++i) {
        C.s_curv[i] = S->s_curv[i];
        C.vcurv_tab[i] = alpha * pow(fabs(S->curvature[i]), -1.0 / 3.0);   // EstimateRouteAndComfortBounds.m:106,108
    }
    C.const_slope = 1;
    for (int i = 0; i < S->n_slope; ++i) {
        C.s_slope[i] = S->s_slope[i]; C.slope[i] = S->slope[i];
        if (S->slope[i] != S->slope[0]) C.const_slope = 0;
    }
    C.theta0 = S->slope[0]; C.sin_theta0 = sin(C.theta0); C.cos_theta0 = cos(C.theta0);
    for (int i = 0; i < S->n_stop; ++i) C.stopLoc[i] = S->stopLoc[i];
    for (int i = 0; i < 4 * S->n_TL; ++i) C.TLLoc[i] = S->TLLoc[i];
    C.stopRefDist = S->stopRefDist; C.stopRefVelSlope = S->stopRefVelSlope; C.stopVel = S->stopVel;
    C.TLstopVel = S->TLstopVel; C.TLStopRegionSize = S->TLStopRegionSize;
    for (int i = 0; i < 21; ++i) C.b5[i] = S->b_fifthOrder[i];
    for (int i = 0; i < 7; ++i) C.fb_w[i] = S->W_FB[i];
    for (int i = 0; i < 6; ++i) C.b_quadr[i] = S->b_quadr[i];
    C.FBuseTaylor = S->FBuseTaylor ? 1 : 0;
    // a-space Hessian of the condensed objective (step invariant for AB):
    //   H = 2 cq Sv'Sv + 2 w_a I + jerk tridiagonal (CreateQP_AB.m:162-180 through Psi)
    std::vector<long double> H((size_t)N * N, 0.0L);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j) {
            // sum over stages k = max(i,j)+1 .. N-1 of T_i T_j
            int cnt = N - 1 - (i > j ? i : j);
            if (cnt > 0) H[(size_t)i * N + j] += 2.0L * C.cq * C.Tvec[i] * C.Tvec[j] * cnt;
        }
    for (int k = 0; k < N; ++k) {
        H[(size_t)k * N + k] += 2.0L * C.w_a + (long double)C.bl_eps;
        long double qj = 2.0L * C.w_j / ((long double)C.Tvec[k] * C.Tvec[k]);
        H[(size_t)k * N + k] += qj;
        if (k > 0) {
            H[(size_t)(k - 1) * N + (k - 1)] += qj;
            H[(size_t)k * N + (k - 1)] -= qj;
            H[(size_t)(k - 1) * N + k] -= qj;
        }
    }
    if (C.mb_any) {
        // reduced variables (one acceleration per block): Hbar = E'HE on the leaders, identity on the rest
        std::vector<long double> Hb((size_t)N * N, 0.0L);
        for (int i = 0; i < N; ++i)
            for (int j = 0; j < N; ++j)
                Hb[(size_t)C.mb_lead[i] * N + C.mb_lead[j]] += H[(size_t)i * N + j];
        for (int k = 0; k < N; ++k) if (C.mb_lead[k] != k) Hb[(size_t)k * N + k] = 1.0L;
        H.swap(Hb);
    }
    if (!spd_inverse(H, N)) return fail(EEPACC_EINVAL, "condensed Hessian is not positive definite");
    Hinv.assign((size_t)N * N, 0.0);
    for (int i = 0; i < N; ++i)
        for (int j = 0; j < N; ++j)
            Hinv[(size_t)i * N + j] = (double)(0.5L * (H[(size_t)i * N + j] + H[(size_t)j * N + i]));
    return EEPACC_OK;
}

// Where stage k of a horizon that starts at a row of a trace sampled every Tvec[0] looks into that trace: at row
// + idx[k] + frac[k], with tau_k = sum_{i<k} Tvec[i] and p = tau_k / Tvec[0] in long double.  A stage that falls on a sample
// up to rounding (|p - round(p)| < 1e-9, as with Tvec[k] / Ts a whole number and Ts = 0.3) gets that sample: frac = 0.
void preview_tables(const double* Tvec, int N, int32_t* idx, double* frac) {
    long double tau = 0.0L;
    for (int k = 0; k < N; ++k) {
        const long double p = tau / (long double)Tvec[0];
        long double i = floorl(p), f = p - i;
        if (f < 1e-9L) f = 0.0L;
        else if (f > 1.0L - 1e-9L) { i += 1.0L; f = 0.0L; }
        idx[k] = (int32_t)i;
        frac[k] = (double)f;
        tau += (long double)Tvec[k];
    }
}

// eepacc_fb_step_est, eepacc_fb_build_qp_est, eepacc_run_fbmpc_preview: what they refuse of a handle (header: EEPACC_ENOTSUP).
int fb_est_refusal(const std::string& who, int n_classes, const DevCfg& C, bool structured, bool needs_structured) {
    if (n_classes)
        return set_error(EEPACC_ENOTSUP, who + ": a handle of eepacc_create_classes / eepacc_create_classes_bl has no FBMPC variant, with or without supplied horizon guesses");
    if (C.bl_mode != 0)
        return set_error(EEPACC_ENOTSUP, who + ": the handle was created with bl_mode = " + std::to_string(C.bl_mode) +
                                         "; supplied horizon guesses for FBMPC are built for a handle with bl_mode = 0 (the baseline controller has eepacc_bl_step_est, eepacc_bl_build_qp_est and eepacc_run_blmpc_preview)");
    if (!needs_structured || structured) return EEPACC_OK;
    std::string cause = "EEPACC_FB_DENSE=1 was set when the handle was created, or its horizon does not fit the structured kernels";
    for (int k = 0; k < C.N; ++k)
        if (C.mb_mask[k]) { cause = "Mb[" + std::to_string(k) + "] != 0 (blocked moves)"; break; }
    if (!C.mb_any && C.b_quadr[3] != 0.0) cause = "b_quadr(4) != 0 (the Fm^2 term of the power fit)";
    return set_error(EEPACC_ENOTSUP, who + ": the FBMPC steps of this handle go through the dense path: " + cause +
                                     "; supplied horizon guesses are built for the structured kernels only.  eepacc_fb_build_qp_est still builds the problem of such a handle");
}

// What the structured FBMPC solver (eepacc_fbs.hip) does not represent of a DevCfg: the field, with the reason, or NULL.
const char* fbs_unsupported_field(const DevCfg& C) {
    if (C.mb_any) return "Mb != 0 (blocked moves keep their equality rows, CreateQP_FB.m:346-356)";
    if (C.b_quadr[3] != 0.0) return "b_quadr(4) != 0 (the Fm^2 term of the power fit would give the friction-brake share its own curvature)";
    const double Kr = (30.0 / 3.14159265358979323846) * C.phi;
    if (!(C.fb_w[0] * Kr * C.b_quadr[4] > 0.0)) return "W_FB(1) * b_quadr(5) is not positive (the price of the friction-brake share must rise with speed)";
    if (!(C.fb_w[4] > 0.0) || C.fb_w[3] < 0.0 || C.fb_w[5] < 0.0 || C.fb_w[6] < 0.0 || !(C.fb_w[1] > 0.0))
        return "W_FB (W_FB(2) and W_FB(5) must be positive, W_FB(4), W_FB(6) and W_FB(7) not negative)";
    return nullptr;
}

// eepacc_classes_fb_step, eepacc_run_classes_fbmpc: what they refuse of a handle and of a call (header: EEPACC_ENOTSUP for a handle
// that has no FBMPC class kernels to run, EEPACC_EINVAL for the arguments of a call on one that has).
int classes_fb_refusal(const std::string& who, const ClassesFbCall& c) {
    if (!c.n_classes)
        return set_error(EEPACC_ENOTSUP, who + ": this handle has no settings classes (it was created by eepacc_create); eepacc_fb_step / eepacc_run_fbmpc run FBMPC on such a handle");
    if (c.bl_mode != 0)
        return set_error(EEPACC_ENOTSUP, who + ": a handle of eepacc_create_classes_bl holds classes of the baseline or target-vehicle controller (bl_mode = " +
                                         std::to_string(c.bl_mode) + "); FBMPC classes are those of eepacc_create_classes (bl_mode = 0)");
    for (int k = 0; k < c.n_classes; ++k)
        if (c.unsupported[k])
            return set_error(EEPACC_ENOTSUP, who + ": class " + std::to_string(k) + ": " + c.unsupported[k] +
                                             "; the structured FBMPC kernels do not represent it, and classes have no dense path");
    if (c.smem_bytes > c.smem_budget)
        return set_error(EEPACC_ENOTSUP, who + ": class 0: N_hor = " + std::to_string(c.N) + " needs " + std::to_string(c.smem_bytes) + " bytes of LDS per block, above the " +
                                         std::to_string(c.smem_budget) + " of the structured FBMPC kernels; classes have no dense path");
    if (c.B < 0 || c.B > c.max_batch)
        return set_error(EEPACC_EINVAL, who + ": B = " + std::to_string(c.B) + " is outside [0, max_batch = " + std::to_string(c.max_batch) + "]");
    if (c.n_steps < 0) return set_error(EEPACC_EINVAL, who + ": n_steps = " + std::to_string(c.n_steps) + " is negative");
    if (c.B == 0 || c.n_steps == 0) return EEPACC_OK;
    if (c.null_buffer) return set_error(EEPACC_EINVAL, who + ": " + c.null_buffer + " is NULL");
    if (!c.classes_B) return set_error(EEPACC_EINVAL, who + ": eepacc_set_classes has not been called on this handle");
    if (c.B != c.classes_B)
        return set_error(EEPACC_EINVAL, who + ": B = " + std::to_string(c.B) + " differs from the B = " + std::to_string(c.classes_B) + " of the last eepacc_set_classes");
    return EEPACC_OK;
}

// What eepacc_kpis reads of a class (validated by build_cfg before): the power fit and driveline of the energy, the fuel
// map and coast-down terms of ABO/Custom_plots.m:73-107 and the speed-limit table of ABO/Main.m:133.
KpiCfg build_kpi_cfg(const eepacc_settings* S, const eepacc_vehicle* V) {
    KpiCfg K;
    memset(&K, 0, sizeof(K));
    K.Ts = S->Tvec[0]; K.phi = V->phi;
    for (int i = 0; i < 21; ++i) K.b5[i] = S->b_fifthOrder[i];
    K.lm = V->lambda * V->m; K.F0 = V->F0; K.F2 = V->F2; K.R_w = V->R_w;
    K.p00 = V->p00; K.p10 = V->p10; K.p01 = V->p01;
    K.n_speedLim = S->n_speedLim;
    for (int i = 0; i < S->n_speedLim; ++i) { K.s_speedLim[i] = S->s_speedLim[i]; K.v_speedLim[i] = S->v_speedLim[i]; }
    return K;
}

// What eepacc_follow_kpis reads of a class: the minimum-headway policy of ABO/Main.m:687, the power surface of cost_P and
// the weights of the reference's cost_* series, one row per EEPACC_FKPI_W_*, in the order w_P, w_a, w_j, w_v, w_h, w_s, w_f.
// RunOpt_ABMPC.m:383-388 takes W(1..5) of the user's W_AB with w_f = W(5); ORIG's six entries are stored behind a leading
// zero (ab_fuel_term = 0), ABO's seven as they are, so that W(1) is w_FC there, as in the reference's own cost_a.
FollowCfg build_follow_cfg(const eepacc_settings* S, const eepacc_vehicle* V) {
    FollowCfg F;
    memset(&F, 0, sizeof(F));
    F.Ts = S->Tvec[0]; F.h_min = S->h_min; F.tau_min = S->tau_min; F.phi = V->phi;
    for (int i = 0; i < 21; ++i) F.b5[i] = S->b_fifthOrder[i];
    const double* W = S->W_AB + (S->ab_fuel_term ? 0 : 1);
    for (int i = 0; i < 5; ++i) F.w[EEPACC_FKPI_W_AB][1 + i] = W[i];
    F.w[EEPACC_FKPI_W_AB][6] = W[4];
    for (int i = 0; i < 7; ++i) F.w[EEPACC_FKPI_W_FB][i] = S->W_FB[i];
    for (int i = 1; i < 7; ++i) F.w[EEPACC_FKPI_W_NONE][i] = 1.0;
    return F;
}

// What eepacc_route_kpis reads of a class: Tvec[0], the speed-limit and curve-speed tables as DevCfg has them
// (EstimateRouteAndComfortBounds.m:106,108 for the curve speed), the stops and lights with their five constants, and the
// comfort limits of the baseline controllers (meaningful where bl_mode != 0, copied as given otherwise).
RouteCfg build_route_cfg(const eepacc_settings* S, const eepacc_vehicle*) {
    RouteCfg R;
    memset(&R, 0, sizeof(R));
    R.Ts = S->Tvec[0];
    R.n_speedLim = S->n_speedLim; R.n_curv = S->n_curv; R.n_stop = S->n_stop; R.n_TL = S->n_TL;
    R.bl_mode = S->bl_mode;
    for (int i = 0; i < S->n_speedLim; ++i) { R.s_speedLim[i] = S->s_speedLim[i]; R.v_speedLim[i] = S->v_speedLim[i]; }
    for (int i = 0; i < S->n_curv; ++i) {
        R.s_curv[i] = S->s_curv[i];
        R.vcurv_tab[i] = S->alpha_TTL * pow(fabs(S->curvature[i]), -1.0 / 3.0);
    }
    for (int i = 0; i < S->n_stop; ++i) R.stopLoc[i] = S->stopLoc[i];
    for (int i = 0; i < 4 * S->n_TL; ++i) R.TLLoc[i] = S->TLLoc[i];
    R.stopRefDist = S->stopRefDist; R.stopRefVelSlope = S->stopRefVelSlope; R.stopVel = S->stopVel;
    R.TLstopVel = S->TLstopVel; R.TLStopRegionSize = S->TLStopRegionSize;
    R.bl_aLo = S->BL_a_LimLowVel; R.bl_aHi = S->BL_a_LimHighVel; R.bl_jLo = S->BL_j_LimLowVel; R.bl_jHi = S->BL_j_LimHighVel;
    return R;
}

// ---- the row catalogue of eepacc_classes_build_qp.  A class has the rows of the plain builder of its controller
// (eepacc_ab_qp_rows, eepacc_bl_qp_rows): per stage the present types in ascending order, then the two terminal rows where the
// controller has a lead.  Class handles have no move blocking, so EEPACC_AB_ROW_BLOCKED is never present.
QpRowsCfg qp_rows_cfg(const DevCfg& C) { return QpRowsCfg{C.N, C.bl_mode, C.ab_route_rows}; }

static bool class_row_present(const QpRowsCfg& c, int type) {
    if (c.bl_mode) return c.bl_mode != 2 || type < EEPACC_BL_ROW_SAFE1;
    if (type == EEPACC_AB_ROW_BLOCKED) return false;
    if (type >= EEPACC_AB_ROW_V_LIM && type <= EEPACC_AB_ROW_V_TL) return c.ab_route_rows != 0;
    return true;
}

int classes_qp_num_rows(const QpRowsCfg& c) {
    if (c.bl_mode) return c.bl_mode == 2 ? 11 * c.N : 13 * c.N + 2;
    return (c.ab_route_rows ? 18 : 14) * c.N + 2;
}

int classes_qp_max_rows(const QpRowsCfg* c, int n_classes) {
    int nC = 0;
    for (int k = 0; k < n_classes; ++k) nC = std::max(nC, classes_qp_num_rows(c[k]));
    return nC;
}

int classes_qp_rows(const QpRowsCfg* c, int n_classes, int cls, int32_t* stage, int32_t* type) {
    if (cls < 0 || cls >= n_classes)
        return fail(EEPACC_EINVAL, "eepacc_classes_qp_rows: cls = " + std::to_string(cls) + " is outside [0, " + std::to_string(n_classes) + ")");
    const QpRowsCfg& q = c[cls];
    const int nC = classes_qp_max_rows(c, n_classes);
    const int n_types = q.bl_mode ? (int)EEPACC_BL_ROW_N : (int)EEPACC_AB_ROW_N;
    int r = 0;
    for (int k = 0; k < q.N; ++k)
        for (int t = 0; t < n_types; ++t)
            if (class_row_present(q, t)) { stage[r] = k; type[r] = t; ++r; }
    if (q.bl_mode != 2) {
        stage[r] = q.N; type[r] = q.bl_mode ? (int)EEPACC_BL_ROW_SAFE1 : (int)EEPACC_AB_ROW_SAFE1; ++r;
        stage[r] = q.N; type[r] = q.bl_mode ? (int)EEPACC_BL_ROW_SAFE2 : (int)EEPACC_AB_ROW_SAFE2; ++r;
    }
    for (; r < nC; ++r) stage[r] = type[r] = -1;
    return EEPACC_OK;
}

}  // namespace eepacc
