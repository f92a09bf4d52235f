// eepacc_ab_build_kernel.inc -- the kernel that writes the condensed QP of an ABMPC step, with what it alone uses.  Included
// into an anonymous namespace by eepacc_ab_build.hip (k_ab_build: the estimators' horizon guesses) and by
// eepacc_ab_build_est.hip (k_ab_build_est: the guesses of the caller), with three macros, and by eepacc_ab_build_cls.hip
// (k_ab_build_cls: a handle with settings classes) with a fourth:
//   EEPACC_AB_BUILD_KERNEL       the kernel's name
//   EEPACC_AB_BUILD_MORE_PARAMS  its parameters after uba (with the leading comma), empty in k_ab_build
//   EEPACC_AB_BUILD_SUPPLIED     the statement that puts the caller's guesses of stage k in place of the estimates, empty there
//   EEPACC_AB_BUILD_CLASSES      defined: cfg is the class array and class_of (among the further parameters) the class of every
//                                instance; the workgroup takes the settings of its instance's class, nC is the row count of the
//                                largest class and the rows behind the class's own are padding (eepacc_qp_build.h)
// One kernel per translation unit: a second caller of the helpers below in the same unit changes what the compiler inlines
// into the first, and k_ab_build is to keep its code (profiles/est_codegen.txt).
struct Stages {                      // per-stage quantities of the step, static LDS
    double T[kS], stv[kS], chw[kS], ds[kS];
    double v_lim[kS], v_curv[kS], v_stop[kS], v_TL[kS], a_min[kS], a_max[kS], j_min[kS], j_max[kS];
    double hv[kS];                   // curvature of v_k in the sparse-form objective (CreateQP_AB.m:154-166)
    double tv[kS];                   // (Hs d + cs) on v_k
    double ta[kS];                   // (Hs d + cs) on a_k
    double hsuf[kS + 1];             // hsuf[m] = sum_{k >= m} hv[k], stages below N
    double q[kS];                    // jerk curvature 2 w_j / T_k^2 (:173-180)
    double hd[kS];                   // diagonal of the a-a block
};

// Row `type` (EEPACC_AB_ROW_*) of stage k; k == N: the two terminal rows (CreateQP_AB.m:376-387).  Slack 0..3 = xi_v, xi_h,
// xi_s, xi_f
__device__ inline Row ab_row(const DevCfg& C, const Stages& S, int k, int type, double a_minus1) {
    Row R = di_row_blank(k, -1);
    if (k == C.N) { di_row_terminal(R, C, S.stv, type == EEPACC_AB_ROW_SAFE1); return R; }
    const double T = S.T[k];
    const double A_hwp = 2.0;
    switch (type) {
    case EEPACC_AB_ROW_S: R.as = 1.0; R.lb = 0.0; R.ub = C.s_goal; break;                          // :256-279
    case EEPACC_AB_ROW_V: R.av = 1.0; R.lb = 0.0; R.ub = C.v_max; break;
    case EEPACC_AB_ROW_XI_V: R.slack = 0; R.sc = 1.0; R.lb = 0.0; break;
    case EEPACC_AB_ROW_XI_H: R.slack = 1; R.sc = 1.0; R.lb = 0.0; break;
    case EEPACC_AB_ROW_XI_S: R.slack = 2; R.sc = 1.0; R.lb = 0.0; break;
    case EEPACC_AB_ROW_XI_F: R.slack = 3; R.sc = 1.0; R.lb = 0.0; break;
    case EEPACC_AB_ROW_BLOCKED: R.de = 1.0; R.ga = -1.0; R.lb = 0.0; R.ub = 0.0; break;             // :283-289
    case EEPACC_AB_ROW_A_MAX: R.ga = 1.0; R.slack = 3; R.sc = -1.0; R.ub = S.a_max[k]; break;       // :292-299
    case EEPACC_AB_ROW_A_MIN: R.ga = 1.0; R.slack = 3; R.sc = 1.0; R.lb = S.a_min[k]; break;
    case EEPACC_AB_ROW_J_MAX:                                                                       // :302-322
        R.ga = 1.0; R.slack = 3; R.sc = -1.0;
        if (k > 0) { R.de = -1.0; R.ub = T * S.j_max[k]; } else R.ub = T * S.j_max[k] + a_minus1;
        break;
    case EEPACC_AB_ROW_J_MIN:
        R.ga = 1.0; R.slack = 3; R.sc = 1.0;
        if (k > 0) { R.de = -1.0; R.lb = T * S.j_min[k]; } else R.lb = T * S.j_min[k] + a_minus1;
        break;
    case EEPACC_AB_ROW_V_LIM: R.av = 1.0; R.slack = 3; R.sc = -1.0; R.ub = S.v_lim[k]; break;       // ORIG :307-329
    case EEPACC_AB_ROW_V_CURV: R.av = 1.0; R.slack = 3; R.sc = -1.0; R.ub = S.v_curv[k]; break;
    case EEPACC_AB_ROW_V_STOP: R.av = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.v_stop[k]; break;
    case EEPACC_AB_ROW_V_TL: R.av = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.v_TL[k]; break;
    case EEPACC_AB_ROW_V_INC: R.av = 1.0; R.slack = 0; R.sc = 1.0; R.lb = fmin(S.v_lim[k], S.v_curv[k]); break;   // :349-352
    case EEPACC_AB_ROW_SAFE1: R.as = 1.0; R.slack = 2; R.sc = -1.0; R.ub = S.stv[k] - C.h_min; break;            // :355-362
    case EEPACC_AB_ROW_SAFE2: R.as = 1.0; R.av = C.tau_min; R.slack = 2; R.sc = -1.0; R.ub = S.stv[k]; break;
    default: R.as = 1.0; R.av = S.chw[k]; R.slack = 1; R.sc = -1.0; R.ub = S.stv[k] - A_hwp; break;              // :365-371
    }
    return R;
}

__global__ void __launch_bounds__(BT) EEPACC_AB_BUILD_KERNEL(const DevCfg* __restrict__ cfg, int nC, const double* __restrict__ s,
                                                 const double* __restrict__ v, const double* __restrict__ a_prev,
                                                 const double* __restrict__ t0, const double* __restrict__ s_tv,
                                                 const double* __restrict__ v_tv, const double* __restrict__ a_tv_prev,
                                                 double* __restrict__ H, double* __restrict__ g, double* __restrict__ A,
                                                 double* __restrict__ lba, double* __restrict__ uba EEPACC_AB_BUILD_MORE_PARAMS) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ Stages S;
#ifdef EEPACC_AB_BUILD_CLASSES
    // the index is uniform over the workgroup, so the settings stay scalar loads; N and Tvec, and with them the LDS geometry,
    // are every class's alike, the row count and ab_route_rows the class's own (class handles have no move blocking)
    const DevCfg& C = cfg[class_of[blockIdx.x]];
    const int n_own = (C.ab_route_rows ? 18 : 14) * C.N + 2;
#else
    const DevCfg& C = *cfg;
    const int n_own = nC;
#endif
    const int N = C.N, nV = 5 * N, tid = threadIdx.x;
    const size_t b = blockIdx.x;
    const int ld = N | 1;
    double* Ss = reinterpret_cast<double*>(smem);           // [N+1][ld]
    unsigned short* rows = qp_build_rows(Ss, N, 1);         // [nC]
    const double s_0 = s[b], v_0 = v[b], a_minus1 = a_prev[b], t_0 = t0[b];

    // ---- estimators, bounds and the sparse-form objective per stage (A2, A3, CreateQP_AB.m:150-187)
    if (tid <= N) {
        const int k = tid;
        double se, ve, st, vt;
        const double* predp = C.pred + b * 128;
        ego_estimate(C, s_0, v_0, a_minus1, k, [&](int idx, double& ps, double& pv) { ps = predp[idx]; pv = predp[64 + idx]; },
                     se, ve);
        estimate_traj(C, C.TVestSetting, C.tConstACC_tar, s_tv[b], v_tv[b], a_tv_prev[b], k, st, vt);
        EEPACC_AB_BUILD_SUPPLIED
        S.stv[k] = st;
        double hv = 0.0, tv = 0.0, ta = 0.0, T = 0.0, q = 0.0;
        if (k < N) {
            T = C.Tvec[k];
            route_bounds(C, se, ve, t_0, k, S.v_lim[k], S.v_curv[k], S.v_stop[k], S.v_TL[k], S.a_min[k], S.a_max[k],
                         S.j_min[k], S.j_max[k]);
            const double T_hwp = 2.0, G_hwp = -0.0246 * T_hwp + 0.010819;
            S.chw[k] = T_hwp + G_hwp * ve;
            double cv, ca;
            if (C.ab_fuel_term == 2) {
                // ICE map :154-159, gear ratio of the stage from its estimated speed (LUTgearshift.m:17-41)
                double tg = C.ice_gb[7];
#pragma unroll
                for (int g2 = 6; g2 >= 0; --g2) if (ve < C.ice_up[g2]) tg = C.ice_gb[g2];
                hv = 2.0 * C.ice_cq / tg; cv = C.ice_lv * tg; ca = C.ice_la / tg;
            } else {
                hv = 2.0 * C.cq; cv = C.glin_v; ca = C.glin_a;                  // :162-166 (all zero without a fuel term)
            }
            tv = hv * v_0 + cv;
            ta = ca;
            if (k == 0) ta -= 2.0 * C.w_j / T * a_minus1;                       // :173-176
            q = 2.0 * C.w_j / (T * T);
        }
        S.T[k] = T; S.hv[k] = hv; S.tv[k] = tv; S.ta[k] = ta; S.q[k] = q;
    }
    __syncthreads();

    // ---- position sensitivities and free response; suffix sums and the a-a diagonal; the row catalogue
#ifdef EEPACC_AB_BUILD_CLASSES
    fill_pad_rows(rows, n_own, nC, tid);
#endif
    if (tid <= N) {
        const int k = tid;
        S.ds[k] = di_position_row(S.T, Ss, ld, k, s_0, v_0);
        if (k < N) {
            double hd = 2.0 * C.w_a + S.q[k];                                   // :169-180
            if (k + 1 < N) hd += S.q[k + 1];
            S.hd[k] = hd;
            // first row of the stage: the rows of the stages before it
            int r = (C.ab_route_rows ? 18 : 14) * k;
            for (int j = 0; j < k; ++j) r += C.mb_mask[j] ? 1 : 0;
            fill_stage_rows(rows, r, k, EEPACC_AB_ROW_N,
                            [&](int type, int kk) { return ab_row_present(type, C.ab_route_rows, C.mb_mask[kk]); });
        } else {
            fill_terminal_rows(rows, n_own, N, EEPACC_AB_ROW_SAFE1, EEPACC_AB_ROW_SAFE2);
        }
    } else if (tid == 64) {
        double acc = 0.0;
        S.hsuf[N] = 0.0;
        for (int k = N - 1; k >= 0; --k) { acc += S.hv[k]; S.hsuf[k] = acc; }
    }
    __syncthreads();

    // ---- H
    write_H(H + b * (size_t)nV * nV, nV, tid, [&](int ra, int rb) {
        const int i = ra / 5, ci = ra - 5 * i, j = rb / 5, cj = rb - 5 * j;
        double h = 0.0;
        if (ci == 0 && cj == 0) {
            const int hi = i > j ? i : j, lo = i > j ? j : i;
            if (i == j) h = S.hd[i];
            else if (hi == lo + 1) h = -S.q[hi];
            h += S.T[i] * S.T[j] * S.hsuf[hi + 1];
        } else if (ra == rb && ci == 2) {
            h = 2.0 * C.w_h;                                                    // :185
        }
        return h;
    });
    // ---- g: Psi'(Hs d + cs), the sum over ascending stages (:183-187 for the slacks)
    for (int col = tid; col < nV; col += BT) {
        const int i = col / 5, c = col - 5 * i;
        double gv;
        if (c == 0) {
            gv = S.ta[i];
            const double Ti = S.T[i];
            for (int k = i + 1; k < N; ++k) gv += Ti * S.tv[k];
        } else {
            gv = c == 1 ? C.w_v : c == 2 ? 1e2 * C.w_h : c == 3 ? C.w_s : C.w_f;
        }
        g[b * (size_t)nV + col] = gv;
    }
    // ---- lba, uba, A
#ifdef EEPACC_AB_BUILD_CLASSES
    const auto decode = [&](int e) { return row_is_pad(e) ? di_row_blank(0, -1) : ab_row(C, S, row_stage(e), row_type(e), a_minus1); };
    write_bounds(lba + b * (size_t)nC, uba + b * (size_t)nC, rows, nC, tid,
                 [&](int e) { return row_is_pad(e) ? RowBounds{-INFINITY, INFINITY, 0.0} : di_bounds(decode(e), S.ds, v_0); });
#else
    const auto decode = [&](int e) { return ab_row(C, S, row_stage(e), row_type(e), a_minus1); };
    write_bounds(lba + b * (size_t)nC, uba + b * (size_t)nC, rows, nC, tid,
                 [&](int e) { return di_bounds(decode(e), S.ds, v_0); });
#endif
    write_A<1, 4>(A + b * (size_t)nV * nC, rows, N, nC, tid, decode,
                  [&](const Row& R, int k, int i, double* x) { x[0] = di_A_entry(R, Ss, ld, S.T, k, i); });
}

