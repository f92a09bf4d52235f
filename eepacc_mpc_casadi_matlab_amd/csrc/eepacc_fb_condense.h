// eepacc_fb_condense.h -- the arithmetic that condenses the FBMPC QP (CreateQP_FB.m:181-215, TransformToDenseFormulation.m:
// 30-91), shared by the build kernel of the dense FBMPC path (k_fb_build, eepacc_fb.hip) and the kernel that writes the
// problem out as data (k_fb_qp, eepacc_fb_qp.hip).  No dense product with Psi is formed: with B_k = T_k/(lambda m) [0 0; 1 1]
// only the state rows of Psi are dense, the columns Sv[.,i], Ss[.,i] of the speed / position sensitivities to the force of
// stage i, and the sparse-form Hessian is block tridiagonal in (v, Fm, Fb)_k: diagonal blocks D_k, coupling blocks O_k
// between stages k-1 and k.
//
// SD: the per-stage data of the step in LDS, indexable members v_est, A22, D2, ds, dv, Dblk, Oblk (row-major 3 x 3 per
// stage), cs, tmp (3 per stage).  Sv, Ss: [N+1][ld].  Whether products are contracted into fused multiply-adds is the
// including unit's choice (k_fb_qp: off; k_fb_build: the compiler's default), so this header sets no pragma of its own.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_device.h"

namespace eepacc {

// lm = lambda m, za = zeta_a, zeta_rg = m g (c_r cos theta0 + sin theta0): the callers hold them at kernel scope (the model
// update uses them too) and pass them in, so that each is formed once per kernel, under that kernel's contraction.

// Column i of the sensitivities of (s_k, v_k) to the force of stage i
template <class SD>
__device__ inline void fb_sens_column(const DevCfg& C, const SD& S, double* Sv, double* Ss, int ld, int i, double lm) {
    const int N = C.N;
    double ss = 0.0, sv = 0.0;
    for (int k = 0; k <= N; ++k) {
        if (k == i + 1) { ss = 0.0; sv = C.Tvec[i] / lm; }
        else if (k > i + 1) { const double ns = ss + C.Tvec[k - 1] * sv; sv = S.A22[k - 1] * sv; ss = ns; }
        Ss[(size_t)k * ld + i] = ss; Sv[(size_t)k * ld + i] = sv;
    }
}

// The free response d: S.ds, S.dv
template <class SD>
__device__ inline void fb_free_response(const DevCfg& C, SD& S, double s_0, double v_0) {
    const int N = C.N;
    double ss = s_0, sv = v_0;
    S.ds[0] = ss; S.dv[0] = sv;
    for (int k = 1; k <= N; ++k) {
        const double ns = ss + C.Tvec[k - 1] * sv;
        sv = S.A22[k - 1] * sv + S.D2[k - 1];
        ss = ns;
        S.ds[k] = ss; S.dv[k] = sv;
    }
}

// Blocks D_k, O_k of the sparse-form Hessian over (v,Fm,Fb)_k and its linear term cs_k (CreateQP_FB.m:181-215), k = 0 .. N
// (zeros at k = N)
template <class SD>
__device__ inline void fb_hessian_blocks(const DevCfg& C, SD& S, int k, double v_0, double a_minus1, double lm, double za,
                                         double zeta_rg) {
    const int N = C.N;
    double D[9], O[9], cs[3];
#pragma unroll
    for (int e = 0; e < 9; ++e) { D[e] = 0.0; O[e] = 0.0; }
    cs[0] = cs[1] = cs[2] = 0.0;
    if (k < N) {
        const double w_P = C.fb_w[0], w_a = C.fb_w[1], w_j = C.fb_w[2];
        const double* bq = C.b_quadr;
        const double K = (30.0 / M_PI) * C.phi;
        const double ve = S.v_est[k];
        // power :181-184
        D[0] += w_P * 2.0 * K * K * bq[5]; D[1] += w_P * K * bq[4]; D[3] += w_P * K * bq[4]; D[4] += w_P * 2.0 * bq[3];
        cs[0] += w_P * K * bq[2]; cs[1] += w_P * bq[1];
        // acceleration :187-191
        const double fa = 2.0 * w_a / (lm * lm);
        D[0] += fa * (za * za * ve * ve + za * zeta_rg);
        D[1] += fa * (-za * ve); D[2] += fa * (-za * ve); D[3] += fa * (-za * ve); D[6] += fa * (-za * ve);
        D[4] += fa; D[5] += fa; D[7] += fa; D[8] += fa;
        cs[1] += w_a / (lm * lm) * (-2.0 * zeta_rg); cs[2] += w_a / (lm * lm) * (-2.0 * zeta_rg);
        // jerk :194-208
        const double Tp = C.Tvec[k];
        const double f = 2.0 * w_j / ((lm * Tp) * (lm * Tp));
        if (k == 0) {
            D[4] += f; D[5] += f; D[7] += f; D[8] += f;
            const double cc = 2.0 * w_j * (za * v_0 * v_0 + zeta_rg + lm * a_minus1) / ((lm * Tp) * (lm * Tp));
            cs[1] -= cc; cs[2] -= cc;
        } else {
            const double vk = ve, vp = S.v_est[k - 1];
            // lower-right block of the 6x6 coupling (current stage) and the coupling block O_k
            D[0] += f * (za * za * vp * vp);
            D[1] += f * (-za * vk); D[2] += f * (-za * vk); D[3] += f * (-za * vk); D[6] += f * (-za * vk);
            D[4] += f; D[5] += f; D[7] += f; D[8] += f;
            O[0] = f * (-za * za * vk * vp); O[1] = f * (za * vp); O[2] = f * (za * vp);
            O[3] = f * (za * vk); O[4] = -f; O[5] = -f;
            O[6] = f * (za * vk); O[7] = -f; O[8] = -f;
        }
        if (k + 1 < N) {
            // upper-left block of stage k+1's coupling lands on this stage
            const double Tn = C.Tvec[k + 1];
            const double fn = 2.0 * w_j / ((lm * Tn) * (lm * Tn));
            const double vk = S.v_est[k + 1], vp = ve;
            D[0] += fn * (za * za * vk * vk);
            D[1] += fn * (-za * vp); D[2] += fn * (-za * vp); D[3] += fn * (-za * vp); D[6] += fn * (-za * vp);
            D[4] += fn; D[5] += fn; D[7] += fn; D[8] += fn;
        }
    }
#pragma unroll
    for (int e = 0; e < 9; ++e) { S.Dblk[9 * k + e] = D[e]; S.Oblk[9 * k + e] = O[e]; }
#pragma unroll
    for (int e = 0; e < 3; ++e) S.cs[3 * k + e] = cs[e];
}

// Entry t = 3 k + c of tmp = Hs d + cs on the (v,Fm,Fb) rows, t < 3 N
template <class SD>
__device__ inline void fb_tmp_entry(const DevCfg& C, SD& S, int t) {
    const int N = C.N, k = t / 3, c = t - 3 * k;
    double x = S.Dblk[9 * k + 3 * c + 0] * S.dv[k] + S.cs[3 * k + c];
    if (k >= 1) x += S.Oblk[9 * k + 0 * 3 + c] * S.dv[k - 1];
    if (k + 1 < N) x += S.Oblk[9 * (k + 1) + 3 * c + 0] * S.dv[k + 1];
    S.tmp[3 * k + c] = x;
}

// Entry col of g = Psi'(Hs d + cs), the sum over ascending stages (:211-215 for the slacks).  N = C.N, which the caller holds
// in a register (here and in fb_H_entry: they run once per output entry)
template <class SD>
__device__ inline double fb_g_entry(const DevCfg& C, const SD& S, const double* Sv, int ld, int N, int col) {
    const int i = col / 6, c = col - 6 * i;
    double gv;
    if (c < 2) {
        gv = S.tmp[3 * i + 1 + c];
        for (int k = i + 1; k < N; ++k) gv += Sv[(size_t)k * ld + i] * S.tmp[3 * k];
    } else {
        gv = (c == 2) ? C.fb_w[3] : (c == 3) ? 1e2 * C.fb_w[4] : (c == 4) ? C.fb_w[5] : C.fb_w[6];
    }
    return gv;
}

// Entry (ra, rb) of H = Psi' Hs Psi.  h_xih = 2 fb_w[4], the diagonal entry of the headway slack (:211-215)
template <class SD>
__device__ inline double fb_H_entry(const SD& S, const double* Sv, int ld, int N, double h_xih, int ra, int rb) {
    const int i = ra / 6, ci = ra - 6 * i, j = rb / 6, cj = rb - 6 * j;
    double h = 0.0;
    if (ci < 2 && cj < 2) {
        const double* Svi = Sv + i;
        const double* Svj = Sv + j;
        const int k0 = (i > j ? i : j) + 1;
        for (int k = k0; k < N; ++k) h += S.Dblk[9 * k] * Svi[(size_t)k * ld] * Svj[(size_t)k * ld];
        // stages below k0 have a zero in one of the two columns, and so has the coupling of k0 - 1 with k0 - 2
        for (int k = k0 > 1 ? k0 : 1; k < N; ++k)
            h += S.Oblk[9 * k] * (Svi[(size_t)(k - 1) * ld] * Svj[(size_t)k * ld] +
                                  Svi[(size_t)k * ld] * Svj[(size_t)(k - 1) * ld]);
        // v-F cross terms
        h += Svi[(size_t)j * ld] * S.Dblk[9 * j + 1 + cj];
        if (j >= 1) h += Svi[(size_t)(j - 1) * ld] * S.Oblk[9 * j + 1 + cj];
        if (j + 1 < N) h += Svi[(size_t)(j + 1) * ld] * S.Oblk[9 * (j + 1) + 3 * (1 + cj)];
        h += Svj[(size_t)i * ld] * S.Dblk[9 * i + 1 + ci];
        if (i >= 1) h += Svj[(size_t)(i - 1) * ld] * S.Oblk[9 * i + 1 + ci];
        if (i + 1 < N) h += Svj[(size_t)(i + 1) * ld] * S.Oblk[9 * (i + 1) + 3 * (1 + ci)];
        // F-F
        if (i == j) h += S.Dblk[9 * i + 3 * (1 + ci) + 1 + cj];
        else if (j == i + 1) h += S.Oblk[9 * j + 3 * (1 + ci) + 1 + cj];
        else if (i == j + 1) h += S.Oblk[9 * i + 3 * (1 + cj) + 1 + ci];
    } else if (ra == rb && ci == 3) {
        h = h_xih;
    }
    return h;
}

// Coefficients of row R (of stage k, eepacc_fb_rows.h) on Fm_i, Fb_i.  Ssk, Svk: row k of the two tables
template <class RowT>
__device__ inline void fb_A_entry(const RowT& R, const double* Ssk, const double* Svk, int k, int i, double* x) {
    const double st = R.as * Ssk[i] + R.av * Svk[i];
    double cF0 = st, cF1 = st;
    if (i == k) { cF0 += R.aFm; cF1 += R.aFb; }
    if (i == k - 1) { cF0 += R.aFmp; cF1 += R.aFbp; }
    x[0] = cF0; x[1] = cF1;
}

}  // namespace eepacc
