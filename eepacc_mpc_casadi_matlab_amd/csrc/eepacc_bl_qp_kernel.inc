// eepacc_bl_qp_kernel.inc -- the kernel that writes the condensed QP of a BLMPC or TVMPC step, with what it alone uses.
// Included into an anonymous namespace by eepacc_bl_qp.hip (k_bl_qp: the estimators' horizon guesses) and by
// eepacc_bl_qp_est.hip (k_bl_qp_est: the guesses of the caller, bl_mode = 1 only), with three macros, and by
// eepacc_bl_qp_cls.hip (k_bl_qp_cls: a handle with settings classes) with a fourth:
//   EEPACC_BL_QP_KERNEL       the kernel's name
//   EEPACC_BL_QP_MORE_PARAMS  its parameters after uba (with the leading comma), empty in k_bl_qp
//   EEPACC_BL_QP_SUPPLIED     the statement that puts the caller's guesses of stage k in place of the estimates, empty there
//   EEPACC_BL_QP_CLASSES      defined: cfg is the class array and class_of (among the further parameters) the class of every
//                             instance; the workgroup takes the settings of its instance's class.  The classes of a handle share
//                             bl_mode and N and so the row count: there are no padding rows
// One kernel per translation unit, as eepacc_ab_build_kernel.inc: k_bl_qp is to keep its code (profiles/blest_codegen.txt).
struct Stages {                      // per-stage quantities of the step, static LDS
    double T[kS], stv[kS], ds[kS];
    double v_lim[kS], v_curv[kS], v_stop[kS], v_TL[kS], a_min[kS], a_max[kS], j_min[kS], j_max[kS];
};

// Row `type` (EEPACC_BL_ROW_*) of stage k; k == N: the two terminal rows (CreateQP_BL.m:306-314).  The one slack of a stage
// is xi_f, index 0
__device__ inline Row bl_row(const DevCfg& C, const Stages& S, int k, int type, double a_minus1) {
    Row R = di_row_blank(k, 0);
    if (k == C.N) { di_row_terminal(R, C, S.stv, type == EEPACC_BL_ROW_SAFE1); return R; }
    const double Ts = C.Tvec[0];                                                                    // :31
    switch (type) {
    case EEPACC_BL_ROW_S: R.as = 1.0; R.lb = 0.0; R.ub = C.s_goal; break;                           // :217-228
    case EEPACC_BL_ROW_V: R.av = 1.0; R.lb = 0.0; R.ub = C.v_max; break;
    case EEPACC_BL_ROW_XI_F: R.sc = 1.0; R.lb = 0.0; break;
    case EEPACC_BL_ROW_A_MIN: R.ga = 1.0; R.sc = 1.0; R.lb = S.a_min[k]; break;                     // :232-239
    case EEPACC_BL_ROW_A_MAX: R.ga = 1.0; R.sc = -1.0; R.ub = S.a_max[k]; break;
    case EEPACC_BL_ROW_J_MIN:                                                                       // :242-261
        R.ga = 1.0; R.sc = 1.0;
        if (k > 0) { R.de = -1.0; R.lb = Ts * S.j_min[k]; } else R.lb = Ts * S.j_min[k] + a_minus1;
        break;
    case EEPACC_BL_ROW_J_MAX:
        R.ga = 1.0; R.sc = -1.0;
        if (k > 0) { R.de = -1.0; R.ub = Ts * S.j_max[k]; } else R.ub = Ts * S.j_max[k] + a_minus1;
        break;
    case EEPACC_BL_ROW_V_LIM: R.av = 1.0; R.sc = -1.0; R.ub = S.v_lim[k]; break;                    // :265-286
    case EEPACC_BL_ROW_V_CURV: R.av = 1.0; R.sc = -1.0; R.ub = S.v_curv[k]; break;
    case EEPACC_BL_ROW_V_STOP: R.av = 1.0; R.sc = -1.0; R.ub = S.v_stop[k]; break;
    case EEPACC_BL_ROW_V_TL: R.av = 1.0; R.sc = -1.0; R.ub = S.v_TL[k]; break;
    case EEPACC_BL_ROW_SAFE1: R.as = 1.0; R.sc = -1.0; R.ub = S.stv[k] - C.h_min; break;            // :289-296
    default: R.as = 1.0; R.av = C.tau_min; R.sc = -1.0; R.ub = S.stv[k]; break;
    }
    return R;
}

__global__ void __launch_bounds__(BT) EEPACC_BL_QP_KERNEL(const DevCfg* __restrict__ cfg, int nC, const double* __restrict__ s,
                                              const double* __restrict__ v, const double* __restrict__ a_prev,
                                              const double* __restrict__ t0, const double* __restrict__ s_tv,
                                              const double* __restrict__ v_tv, const double* __restrict__ a_tv_prev,
                                              double* __restrict__ H, double* __restrict__ g, double* __restrict__ A,
                                              double* __restrict__ lba, double* __restrict__ uba EEPACC_BL_QP_MORE_PARAMS) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ Stages S;
#ifdef EEPACC_BL_QP_CLASSES
    const DevCfg& C = cfg[class_of[blockIdx.x]];            // uniform over the workgroup: the settings stay scalar loads
#else
    const DevCfg& C = *cfg;
#endif
    const int N = C.N, nV = 2 * N, tid = threadIdx.x;
    const bool tv = C.bl_mode == 2;
    const size_t b = blockIdx.x;
    const int ld = N | 1;
    double* Ss = reinterpret_cast<double*>(smem);           // [N+1][ld]
    unsigned short* rows = qp_build_rows(Ss, N, 1);         // [nC]
    const double s_0 = s[b], v_0 = v[b], a_minus1 = a_prev[b], t_0 = t0[b];
    const double Ts = C.Tvec[0];                                                // CreateQP_BL.m:31, CreateQP_TV.m:29
    const double q = 2.0 * C.w_j / (Ts * Ts);                                   // jerk curvature, CreateQP_BL.m:138-145

    // ---- estimators and bounds per stage (EstimateVehicleTrajectory.m, EstimateRouteAndComfortBounds.m)
    if (tid <= N) {
        const int k = tid;
        double se, ve, st = 0.0, vt;
        const double* predp = C.pred + b * 128;
        ego_estimate(C, s_0, v_0, a_minus1, k, [&](int idx, double& ps, double& pv) { ps = predp[idx]; pv = predp[64 + idx]; },
                     se, ve);
        // (target-vehicle MPC: no lead vehicle, RunOpt_TVMPC.m:157 estimates its own trajectory only)
        if (!tv) estimate_traj(C, C.TVestSetting, C.tConstACC_tar, s_tv[b], v_tv[b], a_tv_prev[b], k, st, vt);
        EEPACC_BL_QP_SUPPLIED
        S.stv[k] = st;
        double T = 0.0;
        if (k < N) {
            T = C.Tvec[k];
            // CreateQP_TV.m:44-45 hands the bounds a zero speed estimate: the low-speed comfort limits at every stage
            route_bounds(C, se, tv ? 0.0 : ve, t_0, k, S.v_lim[k], S.v_curv[k], S.v_stop[k], S.v_TL[k], S.a_min[k], S.a_max[k],
                         S.j_min[k], S.j_max[k]);
            if (tv) { S.v_lim[k] *= 0.8; S.v_curv[k] *= 0.8; }                  // CreateQP_TV.m:265,271
        }
        S.T[k] = T;
    }
    __syncthreads();

    // ---- position sensitivities and free response; the row catalogue
    if (tid <= N) {
        const int k = tid;
        S.ds[k] = di_position_row(S.T, Ss, ld, k, s_0, v_0);
        if (k < N) {
            fill_stage_rows(rows, bl_rows_per_stage(C.bl_mode) * k, k, EEPACC_BL_ROW_N,
                            [&](int type, int) { return bl_row_present(type, C.bl_mode); });
        } else if (!tv) {
            fill_terminal_rows(rows, nC, N, EEPACC_BL_ROW_SAFE1, EEPACC_BL_ROW_SAFE2);
        }
    }
    __syncthreads();

    // ---- H
    write_H(H + b * (size_t)nV * nV, nV, tid, [&](int ra, int rb) {
        double h = 0.0;
        if (((ra | rb) & 1) == 0) {                                             // a_i, a_j: CreateQP_BL.m:134-145
            const int i = ra >> 1, j = rb >> 1;
            if (i == j) { h = 2.0 * C.w_a + q; if (i + 1 < N) h += q; }
            else if (i == j + 1 || j == i + 1) h = 0.0 - q;
        }
        return h;
    });
    // ---- g: Psi' cs, the sum over ascending stages: -w_v on v_{i+1} .. v_N (:131,304), the jerk term of stage 0 (:141), w_f (:148)
    for (int col = tid; col < nV; col += BT) {
        const int i = col >> 1;
        double gv;
        if ((col & 1) == 0) {
            gv = i == 0 ? 0.0 - 2.0 * C.w_j / Ts * a_minus1 : 0.0;
            const double Ti = S.T[i];
            for (int k = i + 1; k <= N; ++k) gv += Ti * C.glin_v;
        } else {
            gv = C.w_f;
        }
        g[b * (size_t)nV + col] = gv;
    }
    // ---- lba, uba, A
    const auto decode = [&](int e) { return bl_row(C, S, row_stage(e), row_type(e), a_minus1); };
    write_bounds(lba + b * (size_t)nC, uba + b * (size_t)nC, rows, nC, tid,
                 [&](int e) { return di_bounds(decode(e), S.ds, v_0); });
    write_A<1, 1>(A + b * (size_t)nV * nC, rows, N, nC, tid, decode,
                  [&](const Row& R, int k, int i, double* x) { x[0] = di_A_entry(R, Ss, ld, S.T, k, i); });
}
