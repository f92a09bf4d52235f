// eepacc_fb_qp.hip -- the condensed QP of one FBMPC step, written out as data: H, g, A, lba, uba in the layout the dense QP
// operator reads.  The structured FBMPC kernels (eepacc_fbs.hip) never form this problem; the build kernel of the dense
// path (k_fb_build, eepacc_fb.hip) forms it, but inside a pipeline that measures the plant and updates the carried model.
// This kernel is the boundary for callers who want the problem itself: it takes the step's inputs and the model A(k), D(k)
// as arguments and writes nothing but its outputs.
//
// Reference: ABO/RunOpt_FBMPC.m:204-264: estimators (EstimateVehicleTrajectory.m:55-88), bounds
// (EstimateRouteAndComfortBounds.m:63-171), objective and rows of ABO/Functions/MPCs/CreateQP_FB.m:158-489, the model of
// RunOpt_FBMPC.m:78-90, 247-259 and the condensing of TransformToDenseFormulation.m:30-91.  The arithmetic is k_fb_build's.
//
// No dense product with Psi is formed.  With B_k = T_k/(lambda m) [0 0; 1 1] only the state rows of Psi are dense: the
// columns Sv[.,i], Ss[.,i] of the speed / position sensitivities to the force of stage i.  The sparse-form Hessian is block
// tridiagonal in (v, Fm, Fb)_k (diagonal blocks D_k, coupling blocks O_k between stages k-1 and k), and a row touches s_k,
// v_k, the forces of stages k and k-1 and one slack.  Every output entry is assembled from these pieces, which are put into
// LDS once.  Products are not contracted into fused multiply-adds, so that an entry carries the roundings of its products.
//
// Dense variable order per stage (6): Fm, Fb, xi_v, xi_h, xi_s, xi_f.  Rows: eepacc_fb_rows.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "eepacc_fb_qp.h"

// also for the estimators of eepacc_stage.h and the rows of eepacc_fb_rows.h as this file compiles them
#pragma clang fp contract(off)
#include "eepacc_fb_rows.h"
#include "eepacc_stage.h"

namespace eepacc {
namespace {

constexpr int BT = 256;              // threads of a workgroup: four waves
constexpr int kS = kMaxN + 1;        // stage arrays: index N is the terminal stage

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
constexpr size_t kLdsMax = sizeof(Stages) + 2 * (size_t)(kMaxN + 1) * (kMaxN | 1) * sizeof(double) +
                           (size_t)(28 * kMaxN + 2) * sizeof(unsigned short);
static_assert(kLdsMax == 19456 + 64512 + 3532 &&kLdsMax <= 160 * 1024, "k_fb_qp: LDS budget of a workgroup (160 KB per CU)");

__global__ void __launch_bounds__(BT) k_fb_qp(fb_qp_args a) {
    extern __shared__ __align__(16) unsigned char smem[];
    __shared__ Stages S;
    const DevCfg& C = *a.cfg;
    const int N = C.N, nV = 6 * N, nC = a.nC, tid = threadIdx.x;
    const size_t b = blockIdx.x, B = (size_t)a.B;
    const int ld = N | 1;                                   // odd row stride: a column is read without bank conflicts
    double* Sv = reinterpret_cast<double*>(smem);           // [N+1][ld] dv_k / dF_i
    double* Ss = Sv + (size_t)(N + 1) * ld;                 // [N+1][ld] ds_k / dF_i
    unsigned short* rows = reinterpret_cast<unsigned short*>(Ss + (size_t)(N + 1) * ld);   // [nC]: stage | type << 8
    const double s_0 = a.s[b], v_0 = a.v[b], a_minus1 = a.a_prev[b], t_0 = a.t0[b];
    const double lm = C.lambda * C.m, za = C.zeta_a;
    const double zeta_rg = C.m * C.g * (C.c_r * C.cos_theta0 + C.sin_theta0);

    // ---- estimators and bounds per stage (A2, A3); the row catalogue
    if (tid <= N) {
        const int k = tid;
        double se, ve, st, vt;
        if (C.paramEstSetting == 2) {
            // EstimateVehicleTrajectory.m:81-88: [x_curr; prev(3:end); prev(end) + Ts v_prev(end)]; the handle carries
            // the previous step's predictions, which are read and not written here
            const int idx = k < N ? k + 1 : N;
            const double ps = a.sp.p ? a.sp.at(idx, b) : 0.0, pv = a.vp.p ? a.vp.at(idx, b) : 0.0;
            se = k == 0 ? s_0 : (k < N ? ps : ps + C.Tvec[N - 1] * pv);
            ve = k == 0 ? v_0 : pv;
        } else {
            estimate_traj(C, C.paramEstSetting, C.tConstACC_ego, s_0, v_0, a_minus1, k, se, ve);
        }
        estimate_traj(C, C.TVestSetting, C.tConstACC_tar, a.s_tv[b], a.v_tv[b], a.a_tv_prev[b], k, st, vt);
        S.v_est[k] = ve; S.stv_est[k] = st;
        if (k < N) {
            route_bounds(C, se, ve, t_0, k, S.v_lim[k], S.v_curv[k], S.v_stop[k], S.v_TL[k], S.a_min[k], S.a_max[k],
                         S.j_min[k], S.j_max[k]);
            int r = C.fb_row0[k];
            for (int type = 0; type < EEPACC_FB_ROW_N; ++type)
                if (fb_row_present(type, C.mb_mask[k])) rows[r++] = (unsigned short)(k | (type << 8));
        } else {
            rows[nC - 2] = (unsigned short)(N | (EEPACC_FB_ROW_SAFE1 << 8));
            rows[nC - 1] = (unsigned short)(N | (EEPACC_FB_ROW_SAFE2 << 8));
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

    // ---- sensitivities of (s_k, v_k) to the force of stage i, and the free response d
    if (tid < N) {
        const int i = tid;
        double ss = 0.0, sv = 0.0;
        for (int k = 0; k <= N; ++k) {
            if (k == i + 1) { ss = 0.0; sv = C.Tvec[i] / lm; }
            else if (k > i + 1) { const double ns = ss + C.Tvec[k - 1] * sv; sv = S.A22[k - 1] * sv; ss = ns; }
            Ss[(size_t)k * ld + i] = ss; Sv[(size_t)k * ld + i] = sv;
        }
    } else if (tid == N) {
        double ss = s_0, sv = v_0;
        S.ds[0] = ss; S.dv[0] = sv;
        for (int k = 1; k <= N; ++k) {
            const double ns = ss + C.Tvec[k - 1] * sv;
            sv = S.A22[k - 1] * sv + S.D2[k - 1];
            ss = ns;
            S.ds[k] = ss; S.dv[k] = sv;
        }
    } else if (tid >= 64 && tid <= 64 + N) {
        // ---- block-tridiagonal sparse-form Hessian over (v,Fm,Fb)_k and linear term (CreateQP_FB.m:181-215), on the
        // second wave while the first runs the recursions above
        const int k = tid - 64;
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
    __syncthreads();
    // tmp = Hs d + cs on the (v,Fm,Fb) rows
    if (tid < 3 * N) {
        const int k = tid / 3, c = tid - 3 * k;
        double t = S.Dblk[9 * k + 3 * c + 0] * S.dv[k] + S.cs[3 * k + c];
        if (k >= 1) t += S.Oblk[9 * k + 0 * 3 + c] * S.dv[k - 1];
        if (k + 1 < N) t += S.Oblk[9 * (k + 1) + 3 * c + 0] * S.dv[k + 1];
        S.tmp[3 * k + c] = t;
    }
    __syncthreads();

    // ---- H, row-major: consecutive lanes write consecutive entries; (ra, rb) advance without a division
    {
        double* Hd = a.H + b * (size_t)nV * nV;
        const int total = nV * nV, dra = BT / nV, drb = BT % nV;
        int ra = tid / nV, rb = tid % nV;
        for (int idx = tid; idx < total; idx += BT) {
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
                h = 2.0 * C.fb_w[4];                                            // :211-215
            }
            Hd[idx] = h;
            rb += drb; ra += dra;
            if (rb >= nV) { rb -= nV; ++ra; }
        }
    }
    // ---- g: Psi'(Hs d + cs), the sum over ascending stages (:211-215 for the slacks)
    for (int col = tid; col < nV; col += BT) {
        const int i = col / 6, c = col - 6 * i;
        double gv;
        if (c < 2) {
            gv = S.tmp[3 * i + 1 + c];
            for (int k = i + 1; k < N; ++k) gv += Sv[(size_t)k * ld + i] * S.tmp[3 * k];
        } else {
            gv = (c == 2) ? C.fb_w[3] : (c == 3) ? 1e2 * C.fb_w[4] : (c == 4) ? C.fb_w[5] : C.fb_w[6];
        }
        a.g[b * (size_t)nV + col] = gv;
    }
    // ---- lba, uba: the row's bounds less its value at the free response
    for (int r = tid; r < nC; r += BT) {
        const int e = rows[r], k = e & 0xff;
        const RowDesc R = fb_row_typed(C, S, k, e >> 8, s_0, v_0, a_minus1);
        const double shift = R.as * S.ds[k] + R.av * S.dv[k];
        a.lba[b * (size_t)nC + r] = R.lb - shift;
        a.uba[b * (size_t)nC + r] = R.ub - shift;
    }
    // ---- A, column-major nC x nV: a wave takes 64 consecutive rows (consecutive addresses of one column), decodes its row
    // once and walks the columns of its quarter of the stages, so the four waves share every block of rows evenly
    {
        double* Ad = a.A + b * (size_t)nV * nC;
        const int wave = tid >> 6, lane = tid & 63;
        const int i0 = wave * N / 4, i1 = (wave + 1) * N / 4;
        for (int r0 = 0; r0 < nC; r0 += 64) {
            const int r = r0 + lane;
            if (r >= nC) continue;
            const int e = rows[r], k = e & 0xff;
            const RowDesc R = fb_row_typed(C, S, k, e >> 8, s_0, v_0, a_minus1);
            const double* Ssk = Ss + (size_t)k * ld;
            const double* Svk = Sv + (size_t)k * ld;
            double* col = Ad + (size_t)(6 * i0) * nC + r;
            for (int i = i0; i < i1; ++i) {
                const double st = R.as * Ssk[i] + R.av * Svk[i];
                double cF0 = st, cF1 = st;
                if (i == k) { cF0 += R.aFm; cF1 += R.aFb; }
                if (i == k - 1) { cF0 += R.aFmp; cF1 += R.aFbp; }
                col[0] = cF0;
                col[nC] = cF1;
#pragma unroll
                for (int c = 0; c < 4; ++c) col[(size_t)(2 + c) * nC] = (i == k && c == R.slack) ? R.sc : 0.0;
                col += (size_t)6 * nC;
            }
        }
    }
}

}  // namespace

size_t fb_qp_smem_bytes(int N, int nC) {
    return sizeof(Stages) + 2 * (size_t)(N + 1) * (N | 1) * sizeof(double) + (size_t)nC * sizeof(unsigned short);
}

hipError_t launch_fb_qp(const fb_qp_args& a, int N, hipStream_t stream) {
    const size_t smem = fb_qp_smem_bytes(N, a.nC) - sizeof(Stages);
    if (fb_qp_smem_bytes(N, a.nC) > kLdsMax) return hipErrorInvalidValue;
    // The attribute belongs to the kernel, not to the handle: always the largest size, so that launches of handles with
    // different horizons on different host threads cannot lower it under one another.
    const hipError_t e = hipFuncSetAttribute((const void*)k_fb_qp, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)(kLdsMax - sizeof(Stages)));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_fb_qp, dim3(a.B), dim3(BT), smem, stream, a);
    return hipGetLastError();
}

}  // namespace eepacc
