// eepacc_fb_qp_kernel.inc -- the kernel that writes the condensed QP of an FBMPC step, with what it alone uses.  Included
// into an anonymous namespace by eepacc_fb_qp.hip (k_fb_qp: the estimators' horizon guesses) and by eepacc_fb_qp_est.hip
// (k_fb_qp_est: the guesses of the caller), with three macros:
//   EEPACC_FB_QP_KERNEL       the kernel's name
//   EEPACC_FB_QP_MORE_PARAMS  its parameters after the argument block (with the leading comma), empty in k_fb_qp
//   EEPACC_FB_QP_SUPPLIED     the statement that puts the caller's guesses of stage k in place of the estimates, empty there
// One kernel per translation unit, as eepacc_bl_qp_kernel.inc: k_fb_qp is to keep its code (profiles/fb_est_codegen.txt).
struct Stages {                      // per-stage quantities of the step, static LDS
    double v_est[kS], stv_est[kS];
    double v_lim[kS], v_curv[kS], v_stop[kS], v_TL[kS], a_min[kS], a_max[kS], j_min[kS], j_max[kS];
    double A22[kS], D2[kS];          // the model: v_{k+1} = A22_k v_k + T_k/(lambda m) (Fm + Fb)_k + D2_k
    double ds[kS], dv[kS];           // free response
    double Dblk[9 * kS], Oblk[9 * kS];   // sparse-form Hessian over (v, Fm, Fb)_k, row-major 3 x 3 (CreateQP_FB.m:181-208)
    double cs[3 * kS];               // its linear term
    double tmp[3 * kS];              // Hs d + cs
};

// LDS of a workgroup at the longest horizon with every stage blocked: the two sensitivity tables are 64512 B of it
constexpr size_t kLdsMax = sizeof(Stages) + qp_build_smem_bytes(kMaxN, 28 * kMaxN + 2, 2);
static_assert(kLdsMax == 19456 + 64512 + 3532 && kLdsMax <= 160 * 1024, "k_fb_qp: LDS budget of a workgroup (160 KB per CU)");

__global__ void __launch_bounds__(BT) EEPACC_FB_QP_KERNEL(fb_qp_args a EEPACC_FB_QP_MORE_PARAMS) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ Stages S;
    const DevCfg& C = *a.cfg;
    const int N = C.N, nV = 6 * N, nC = a.nC, tid = threadIdx.x;
    const size_t b = blockIdx.x, B = (size_t)a.B;
    const int ld = N | 1;
    double* Sv = reinterpret_cast<double*>(smem);           // [N+1][ld] dv_k / dF_i
    double* Ss = Sv + (size_t)(N + 1) * ld;                 // [N+1][ld] ds_k / dF_i
    unsigned short* rows = qp_build_rows(Sv, N, 2);         // [nC]
    const double s_0 = a.s[b], v_0 = a.v[b], a_minus1 = a.a_prev[b], t_0 = a.t0[b];
    const double lm = C.lambda * C.m, za = C.zeta_a;
    const double zeta_rg = C.m * C.g * (C.c_r * C.cos_theta0 + C.sin_theta0);

    // ---- estimators and bounds per stage (A2, A3); the row catalogue
    if (tid <= N) {
        const int k = tid;
        double se, ve, st, vt;
        ego_estimate(C, s_0, v_0, a_minus1, k, [&](int idx, double& ps, double& pv) {
            ps = a.sp.p ? a.sp.at(idx, b) : 0.0; pv = a.vp.p ? a.vp.at(idx, b) : 0.0;
        }, se, ve);
        estimate_traj(C, C.TVestSetting, C.tConstACC_tar, a.s_tv[b], a.v_tv[b], a.a_tv_prev[b], k, st, vt);
        EEPACC_FB_QP_SUPPLIED
        S.v_est[k] = ve; S.stv_est[k] = st;
        if (k < N) {
            route_bounds(C, se, ve, t_0, k, S.v_lim[k], S.v_curv[k], S.v_stop[k], S.v_TL[k], S.a_min[k], S.a_max[k],
                         S.j_min[k], S.j_max[k]);
            fill_stage_rows(rows, C.fb_row0[k], k, EEPACC_FB_ROW_N,
                            [&](int type, int kk) { return fb_row_present(type, C.mb_mask[kk]); });
        } else {
            fill_terminal_rows(rows, nC, N, EEPACC_FB_ROW_SAFE1, EEPACC_FB_ROW_SAFE2);
        }
    }
    __syncthreads();

    // ---- the model with the A(k)/D(k) index quirk (RunOpt_FBMPC.m:78-90, 247-259), as k_fb_build applies it; nothing of it
    // goes back to where it was read
    if (tid < N) {
        const int k = tid;
        double A22, D2;
        if (!C.FBuseTaylor) {
            const double vi = S.v_est[k];
            A22 = 1.0;
            D2 = C.Tvec[k] / lm * (-za * vi * vi - zeta_rg);
        } else if (a.k_step < 0) {
            A22 = a.A22.at(k, b); D2 = a.D2.at(k, b);
        } else {
            if (a.k_step == 0) {
                A22 = 1.0 - 2.0 * C.Tvec[k] * za * v_0 * v_0 / lm; D2 = C.Tvec[k] / lm * (za * v_0 * v_0);
            } else {
                A22 = a.A22.at(k, b); D2 = a.D2.at(k, b);
            }
            if (k == a.k_step) {
                const int i = N - 1;
                const double vi = S.v_est[i];
                A22 = 1.0 - 2.0 * C.Tvec[i] * za * vi / lm;
                D2 = C.Tvec[i] / lm * (za * vi * vi - zeta_rg);
            }
        }
        S.A22[k] = A22; S.D2[k] = D2;
        if (a.A22_used) a.A22_used[(size_t)k * B + b] = A22;
        if (a.D2_used) a.D2_used[(size_t)k * B + b] = D2;
    }
    __syncthreads();

    // ---- sensitivities of (s_k, v_k) to the force of stage i, and the free response d; the blocks of the sparse-form
    // Hessian on the second wave while the first runs the recursions
    if (tid < N) fb_sens_column(C, S, Sv, Ss, ld, tid, lm);
    else if (tid == N) fb_free_response(C, S, s_0, v_0);
    else if (tid >= 64 && tid <= 64 + N) fb_hessian_blocks(C, S, tid - 64, v_0, a_minus1, lm, za, zeta_rg);
    __syncthreads();
    if (tid < 3 * N) fb_tmp_entry(C, S, tid);
    __syncthreads();

    // ---- H, g
    const double h_xih = 2.0 * C.fb_w[4];
    write_H(a.H + b * (size_t)nV * nV, nV, tid, [&](int ra, int rb) { return fb_H_entry(S, Sv, ld, N, h_xih, ra, rb); });
    for (int col = tid; col < nV; col += BT) a.g[b * (size_t)nV + col] = fb_g_entry(C, S, Sv, ld, N, col);
    // ---- lba, uba, A
    const auto decode = [&](int e) { return fb_row_typed(C, S, row_stage(e), row_type(e), s_0, v_0, a_minus1); };
    write_bounds(a.lba + b * (size_t)nC, a.uba + b * (size_t)nC, rows, nC, tid, [&](int e) {
        const RowDesc R = decode(e);
        const int k = row_stage(e);
        return RowBounds{R.lb, R.ub, R.as * S.ds[k] + R.av * S.dv[k]};
    });
    // a row carries its rows of the two tables, so that the walk over the stages keeps two running LDS addresses
    struct RowAt : RowDesc { const double *Ssk, *Svk; };
    write_A<2, 4>(a.A + b * (size_t)nV * nC, rows, N, nC, tid,
                  [&](int e) {
                      RowAt R{decode(e)};
                      R.Ssk = Ss + (size_t)row_stage(e) * ld; R.Svk = Sv + (size_t)row_stage(e) * ld;
                      return R;
                  },
                  [&](const RowAt& R, int k, int i, double* x) { fb_A_entry(R, R.Ssk, R.Svk, k, i, x); });
}
