// eepacc_ab_cols.h -- the columns of S = C He C' of the ABMPC working set at NS = 32, four per pass: the condensed
// double integrator of a horizon takes half a wave, so lanes 0-31 carry columns j, j+1 and lanes 32-63 columns j+2, j+3.
// Outside the variant namespaces of eepacc_ab_impl.inc (move blocking comes in through two callables) so that the test
// harness can call it.  Every entry of S is computed by the operations of the two-column loop, in their order: P comes
// out bit for bit the same.
#pragma once
#include "eepacc_schur.h"

namespace eepacc {

// normal_at() of eepacc_ab_impl.inc at stage j = l & 31, whose T_j and tau_{j+1} the caller hands to both halves
__device__ __forceinline__ double ab_normal_at_half(int j, int N, double T, double tau1, int kq, double al, double be,
                                                    double ga, double de, double tau_kq) {
    double c = 0.0;
    if (j < N) {
        if (j < kq) c = T * (be + al * (0.5 * T + tau_kq - tau1));
        if (j == kq) c += ga;
        if (j == kq - 1) c += de;
    }
    return c;
}

// hom_traj() per half, as inclusive sums: lane j holds vh_{j+1} and sh_{j+1} (stage 0 is zero; stage N = 32 of a horizon
// that fills the half is lane 31's, which an exclusive scan over 32 lanes has no room for)
__device__ __forceinline__ void ab_hom_traj_half(int j, int N, double T, double x, double& sh1, double& vh1) {
    const int lane = wv::lane_id();
    double xi = (j < N) ? x : 0.0;
    vh1 = wv::scan_incl_half(T * xi);
    double vh = wv::dpp_zero<0x138, 0xf>(vh1);
    vh = lane == 32 ? 0.0 : vh;
    double inc = (j < N) ? (T * vh + 0.5 * T * T * xi) : 0.0;
    sh1 = wv::scan_incl_half(inc);
}

// P (packed lower triangle) = C He C' for the m rows of M (w_k, e_al .. e_de).  T, tau1: T_j and tau_{j+1} of stage
// j = l & 31 in both halves.  reduce / expand: the move-blocking maps E' and E on a half (identity without blocking).
// Input vectors in yv | lam (lower half) and sv | rv (upper half), all free while the factor is rebuilt.
template <int NS, class Mem, class Reduce, class Expand>
__device__ __forceinline__ void ab_schur_columns4(Mem& M, const double* Hs, const double* tauv, int m, int N, int lane,
                                                  double T, double tau1, Reduce reduce, Expand expand) {
    static_assert(NS == 32, "two horizons per wave");
    const int hl = lane & (NS - 1), up = (lane >> 5) & 1;
    double* y0 = up ? M.sv : M.yv;
    double* y1 = up ? M.rv : M.lam;
    const int ki = lane < m ? M.w_k[lane] : 0;
    const int kim1 = ki > 0 ? ki - 1 : 0;
    const int kiu = ki < NS ? ki : NS - 1;          // (ega is zero at stage N)
    const double eal = lane < m ? M.e_al[lane] : 0.0, ebe = lane < m ? M.e_be[lane] : 0.0;
    const double ega = (lane < m && ki < N) ? M.e_ga[lane] : 0.0;
    const double ede = (lane < m && ki > 0 && ki <= N) ? M.e_de[lane] : 0.0;
    for (int j = 0; j < m; j += 4) {
        const int ja = min(j + 2 * up, m - 1), jb = min(j + 2 * up + 1, m - 1);
        const int kj0 = M.w_k[ja], kj1 = M.w_k[jb];
        const double c0 = reduce(ab_normal_at_half(hl, N, T, tau1, kj0, M.e_al[ja], M.e_be[ja], M.e_ga[ja], M.e_de[ja], tauv[kj0]));
        const double c1 = reduce(ab_normal_at_half(hl, N, T, tau1, kj1, M.e_al[jb], M.e_be[jb], M.e_ga[jb], M.e_de[jb], tauv[kj1]));
        y0[hl] = c0; y1[hl] = c1;
        WSYNC();
        double u0, u1;
        he_mul2<NS, false>(Hs, y0, y1, N, hl, u0, u1);
        u0 = expand(u0); u1 = expand(u1);
        WSYNC();
        double su0, vu0, su1, vu1;
        ab_hom_traj_half(hl, N, T, u0, su0, vu0);
        ab_hom_traj_half(hl, N, T, u1, su1, vu1);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            // row i picks the images at its stage from the half that carries the column (sh_k, vh_k: lane k - 1)
            const int sk = kiu + 32 * h, sk1 = kim1 + 32 * h;
            // (every lane takes part in every shuffle; the selects come afterwards)
            double s0 = __shfl(su0, sk1, 64), v0 = __shfl(vu0, sk1, 64), a0 = __shfl(u0, sk, 64);
            double s1 = __shfl(su1, sk1, 64), v1 = __shfl(vu1, sk1, 64), a1 = __shfl(u1, sk, 64);
            const double d0 = __shfl(u0, sk1, 64), d1 = __shfl(u1, sk1, 64);
            s0 = ki > 0 ? s0 : 0.0; v0 = ki > 0 ? v0 : 0.0; a0 = ki < N ? a0 : 0.0;
            s1 = ki > 0 ? s1 : 0.0; v1 = ki > 0 ? v1 : 0.0; a1 = ki < N ? a1 : 0.0;
            const double sx = eal * s0 + ebe * v0 + ega * a0 + ede * d0;
            const double sy = eal * s1 + ebe * v1 + ega * a1 + ede * d1;
            const int col = j + 2 * h;
            if (col < m && lane >= col && lane < m) M.P[pidx(lane, col)] = sx;
            if (col + 1 < m && lane >= col + 1 && lane < m) M.P[pidx(lane, col + 1)] = sy;
        }
    }
    WSYNC();
}

}  // namespace eepacc
