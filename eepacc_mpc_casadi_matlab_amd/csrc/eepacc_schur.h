// eepacc_schur.h -- working-set linear algebra shared by the ABMPC (eepacc_ab_impl.inc) and FBMPC (eepacc_fbs.hip)
// active-set kernels.  Both keep, per wavefront and in LDS, an explicit inverse He of the effective Hessian and an
// explicit packed inverse Schur block P = (C He C' + D)^-1 of the working set.  This header is where the two tables are
// maintained: products with He and its column update, the in-LDS inversion of a full Hessian, the bordered update, the
// downdate and the full inversion of P, and the multipliers that come out of P.  What is built into the tables (row
// catalogues, condensing, which terms are folded into He) stays with each solver.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_units.h"
#include "eepacc_wave.h"

namespace eepacc {

struct SolveStats { int status, iters, events, m; };

// What the last event of a solve did to the working set, for the solver's rebuild_and_factor:
// fast = 1: it appended the plain row (kq, tq) whose column sv = C u, rv = P sv and pivot zz = c'u - sv'rv are still in
// LDS -> bordered update of P (schur_insert);  fast = 2: it dropped the row at list position drop_pos -> rank-one
// downdate (schur_remove);  fast = 0 (or any inconsistency): full rebuild (schur_invert).
struct FastInfo { int fast, m_old, kq, tq, drop_pos; double zz; };

// the row a dual iteration is about to take into the working set
struct Incoming { int kq, qcode, tq, gq; bool is_bound; double al, be, ga, de, d; };

// ----------------------------------------------------------------------------------------------
// He: the per-wave inverse of the effective Hessian.  Full layout: NS x NS, zero padded, every load of a product has an
// immediate offset.  Packed layout (PACKED): lower triangle, entry (i,j), i >= j, at i(i+1)/2 + j.  Lane k reads (i,k)
// for i >= k and (k,i) for i < k; the triangular numbers are a permutation modulo 32, so both access patterns spread
// over the LDS banks.
__device__ __forceinline__ int he_tri(int i) { return i * (i + 1) / 2; }

// out_k = sum_i He[i][k] * yv[i]   (He symmetric, table in LDS, yv in LDS)
template <int NS, bool PACKED>
__device__ __forceinline__ double he_mul(const double* Hs, const double* yv, int N, int lane) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if constexpr (PACKED) {
        const int k = lane & (NS - 1), tk = he_tri(k);
#pragma unroll
        for (int i = 0; i < NS; i += 4) {
            a0 = fma(Hs[(i + 0) >= k ? he_tri(i + 0) + k : tk + (i + 0)], yv[i + 0], a0);
            a1 = fma(Hs[(i + 1) >= k ? he_tri(i + 1) + k : tk + (i + 1)], yv[i + 1], a1);
            a2 = fma(Hs[(i + 2) >= k ? he_tri(i + 2) + k : tk + (i + 2)], yv[i + 2], a2);
            a3 = fma(Hs[(i + 3) >= k ? he_tri(i + 3) + k : tk + (i + 3)], yv[i + 3], a3);
        }
    } else {
        const double* col = Hs + (lane & (NS - 1));
#pragma unroll
        for (int i = 0; i < NS; i += 4) {
            a0 = fma(col[(i + 0) * NS], yv[i + 0], a0);
            a1 = fma(col[(i + 1) * NS], yv[i + 1], a1);
            a2 = fma(col[(i + 2) * NS], yv[i + 2], a2);
            a3 = fma(col[(i + 3) * NS], yv[i + 3], a3);
        }
    }
    return lane < N ? (a0 + a1) + (a2 + a3) : 0.0;
}

// two products with one pass over the table
template <int NS, bool PACKED>
__device__ __forceinline__ void he_mul2(const double* Hs, const double* y0, const double* y1, int N, int lane,
                                        double& o0, double& o1) {
    double a0 = 0.0, a1 = 0.0, b0 = 0.0, b1 = 0.0;
    const int k = lane & (NS - 1), tk = he_tri(k);
    const double* col = Hs + k;
#pragma unroll
    for (int i = 0; i < NS; i += 2) {
        double h0, h1;
        if constexpr (PACKED) {
            h0 = Hs[(i + 0) >= k ? he_tri(i + 0) + k : tk + (i + 0)];
            h1 = Hs[(i + 1) >= k ? he_tri(i + 1) + k : tk + (i + 1)];
        } else { h0 = col[(i + 0) * NS]; h1 = col[(i + 1) * NS]; }
        a0 = fma(h0, y0[i + 0], a0); b0 = fma(h0, y1[i + 0], b0);
        a1 = fma(h1, y0[i + 1], a1); b1 = fma(h1, y1[i + 1], b1);
    }
    o0 = lane < N ? a0 + a1 : 0.0;
    o1 = lane < N ? b0 + b1 : 0.0;
}

// column `lane` (< NS) of  He -= yv yj'  (yv in LDS, yj = this lane's entry of the scaled second factor)
template <int NS, bool PACKED>
__device__ __forceinline__ void he_sub_outer(double* He, const double* yv, double yj, int lane) {
    if constexpr (PACKED) {
        // lane j owns column j of the lower triangle: entries (i, j), i >= j
        for (int i = lane; i < NS; ++i) {
            const int e = he_tri(i) + lane;
            He[e] = fma(-yv[i], yj, He[e]);
        }
    } else {
        double* col = He + lane;
#pragma unroll
        for (int i = 0; i < NS; i += 4) {
            const double h0 = col[(i + 0) * NS], h1 = col[(i + 1) * NS], h2 = col[(i + 2) * NS], h3 = col[(i + 3) * NS];
            const double y0 = yv[i], y1 = yv[i + 1], y2 = yv[i + 2], y3 = yv[i + 3];
            col[(i + 0) * NS] = fma(-y0, yj, h0); col[(i + 1) * NS] = fma(-y1, yj, h1);
            col[(i + 2) * NS] = fma(-y2, yj, h2); col[(i + 3) * NS] = fma(-y3, yj, h3);
        }
    }
}

// ---- full layout at NS = 32: a column takes half a wave, so the other half shares the work (the split he_invert_full
// uses: lane l works on rows [16 (l >> 5), +16) of column l & 31).  The functions above keep serving the packed layout,
// NS = 64 and the FBMPC kernels.

// He -= yv yj' with all 64 lanes; yj = the scaled second factor's entry l & 31, in both halves.  Every entry is the one
// fma of he_sub_outer: the table comes out bit for bit the same.
template <int NS>
__device__ __forceinline__ void he_sub_outer_halves(double* He, const double* yv, double yj, int lane) {
    static_assert(NS == 32, "two lanes per column");
    constexpr int RPL = NS / 2;
    const int r0 = (lane & NS) / 2;
    double* col = He + r0 * NS + (lane & (NS - 1));
    const double* y = yv + r0;
#pragma unroll
    for (int i = 0; i < RPL; i += 4) {
        const double h0 = col[(i + 0) * NS], h1 = col[(i + 1) * NS], h2 = col[(i + 2) * NS], h3 = col[(i + 3) * NS];
        const double y0 = y[i], y1 = y[i + 1], y2 = y[i + 2], y3 = y[i + 3];
        col[(i + 0) * NS] = fma(-y0, yj, h0); col[(i + 1) * NS] = fma(-y1, yj, h1);
        col[(i + 2) * NS] = fma(-y2, yj, h2); col[(i + 3) * NS] = fma(-y3, yj, h3);
    }
}

// out_k = sum_i He[i][k] yv[i] with the sum split over the halves: 16 terms per lane, then one cross-half add.  The
// order of summation differs from he_mul's (rounding-level differences).  Lanes >= N return exactly 0.
template <int NS>
__device__ __forceinline__ double he_mul_halves(const double* Hs, const double* yv, int N, int lane) {
    static_assert(NS == 32, "two lanes per column");
    constexpr int RPL = NS / 2;
    const int r0 = (lane & NS) / 2;
    const double* col = Hs + r0 * NS + (lane & (NS - 1));
    const double* y = yv + r0;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
#pragma unroll
    for (int i = 0; i < RPL; i += 4) {
        a0 = fma(col[(i + 0) * NS], y[i + 0], a0);
        a1 = fma(col[(i + 1) * NS], y[i + 1], a1);
        a2 = fma(col[(i + 2) * NS], y[i + 2], a2);
        a3 = fma(col[(i + 3) * NS], y[i + 3], a3);
    }
    const double s = wv::half_sum((a0 + a1) + (a2 + a3));
    return lane < N ? s : 0.0;
}

// In-place inverse of the positive definite N x N matrix in the full NS x NS table Hs by symmetric sweeps; afterwards
// Hs = -H^-1 (the caller negates).  colk: NS doubles of LDS scratch.  Returns non-zero on a non-positive pivot.
template <int NS>
__device__ __forceinline__ int he_invert_full(double* Hs, double* colk, int N, int lane) {
    // all 64 lanes work: lane l updates rows [r0, r0 + RPL) of column l % NS (NS = 32: two lanes per column)
    constexpr int HALVES = 64 / NS, RPL = NS / HALVES;
    // r0 = (l / NS) * RPL for l < 64, written with the bit of l that selects the half.  This function is optimised on its
    // own before it is inlined, without the range of a lane: the division then comes out as other instructions at NS = 32,
    // and with the range masked in (l & 63) the NS = 64 loop is peeled once more than inside its caller.  Either changes
    // the register spills of the kernels.
    const int jcol = lane & (NS - 1), r0 = (lane & NS) / HALVES;
    double* col = Hs + jcol;
    int bad = 0;
    for (int k = 0; k < N; ++k) {
        const double d = Hs[k * NS + k];
        if (!(d > 0.0)) { bad = 1; break; }
        const double inv = 1.0 / d;
        if (lane < NS) colk[lane] = (lane < N) ? Hs[k * NS + lane] : 0.0;
        WSYNC();
        const double hkj = colk[jcol];
        const double f = hkj * inv;
        const bool piv = jcol == k;
#pragma unroll
        for (int ii = 0; ii < RPL; ++ii) {
            const int i = r0 + ii;
            const double ck = colk[i], old = col[i * NS];
            const double upd = piv ? ck * inv : fma(-ck, f, old);
            col[i * NS] = (i == k) ? (piv ? -inv : f) : upd;
        }
        WSYNC();
    }
    return bad;
}

// ----------------------------------------------------------------------------------------------
// P: the inverse Schur block of the m working-set rows, packed lower triangle in LDS (pidx).  The triangle is spread
// over all 64 lanes (entry e = lane + 64 t; its row and column come from the small table rc = rc_table<MMAX>()), so an
// update costs m(m+1)/128 entry updates per lane instead of m.
//
// Contract: m <= 64.  A row's scratch entry (the pivot column colk, the pivot scale sv, a multiplier) is loaded by the
// lane of the same number, so everything below -- and the solvers' own `lane < m` loads around it -- handles one row per
// lane; at m = 65 or 66 rows 64 and 65 would never be loaded or sign-flipped.  A solver whose tables hold MMAX > 64 rows
// (MMAX = N + 2 at the long horizons, for the table sizes) still refuses a working set above schur_capacity<MMAX>().
template <int MMAX>
__host__ __device__ constexpr int schur_capacity() { return MMAX < 64 ? MMAX : 64; }

// Bordered update: a row joined the list at position p (m: new size).  rv = P sv of the old P, iz = 1 / pivot.
__device__ __forceinline__ void schur_insert(double* P, const double* rv, const unsigned short* rc, int m, int p,
                                             double iz, int lane) {
    const int nnz = m * (m + 1) / 2;
    // in place, highest entries first: an entry moves to a higher packed index, so a chunk never
    // overwrites what a later (lower) chunk still has to read
    for (int e0 = ((nnz - 1) >> 6) << 6; e0 >= 0; e0 -= 64) {
        const int e = e0 + lane;
        double v = 0.0;
        if (e < nnz) {
            const int code = rc[e], r = code >> 8, cc = code & 255;
            const int i = r < p ? r : r - 1, j = cc < p ? cc : cc - 1;
            if (r == p && cc == p) v = iz;
            else if (r == p) v = -rv[j] * iz;
            else if (cc == p) v = -rv[i] * iz;
            else v = P[pidx(i, j)] + rv[i] * rv[j] * iz;
        }
        WSYNC();
        if (e < nnz) P[e] = v;
        WSYNC();
    }
}

// Rank-one downdate: the row at position p left a list of m_old rows (m = m_old - 1: new size).  colk: m_old doubles
// of LDS scratch.
__device__ __forceinline__ void schur_remove(double* P, double* colk, const unsigned short* rc, int m_old, int m,
                                             int p, int lane) {
    if (lane < m_old) colk[lane] = P[pidx(lane, p)];
    WSYNC();
    const double ip = 1.0 / colk[p];
    const int nnz = m * (m + 1) / 2;
    // lowest entries first: an entry moves to a lower packed index
    for (int e0 = 0; e0 < nnz; e0 += 64) {
        const int e = e0 + lane;
        double v = 0.0;
        if (e < nnz) {
            const int code = rc[e], r = code >> 8, cc = code & 255;
            const int i = r < p ? r : r + 1, j = cc < p ? cc : cc + 1;
            v = P[pidx(i, j)] - colk[i] * colk[j] * ip;
        }
        WSYNC();
        if (e < nnz) P[e] = v;
        WSYNC();
    }
}

// Full rebuild: P holds S = C He C' + D on entry and S^-1 on return (in-place symmetric sweeps, then the sign flip).
// sv: m doubles (receives the original diagonal), colk: m doubles of LDS scratch.  Returns 0, or 1 + k when pivot k is
// not positive relative to its original diagonal (S numerically singular; P is then undefined).
__device__ __forceinline__ int schur_invert(double* P, double* sv, double* colk, const unsigned short* rc, int m,
                                            int lane) {
    // in-place inversion by symmetric sweeps: after sweeping every pivot P = -S^-1
    int singular = 0;
    if (lane < m) sv[lane] = fabs(P[pidx(lane, lane)]);     // original diagonal (pivot scale)
    WSYNC();
    const int nnz = m * (m + 1) / 2;
    for (int k = 0; k < m; ++k) {
        const double d = P[pidx(k, k)];
        if (!(d > 1e-12 * sv[k])) { singular = 1 + k; break; }
        const double inv = 1.0 / d;
        if (lane < m) colk[lane] = P[pidx(lane, k)];
        WSYNC();
#pragma unroll 2
        for (int e = lane; e < nnz; e += 64) {
            const int code = rc[e], r = code >> 8, cc = code & 255;
            const double c0 = colk[r];
            const double cl = colk[cc] * inv;
            double v0 = P[e] - c0 * cl;
            if (cc == k) v0 = c0 * inv;
            if (r == k) v0 = (cc == k) ? -inv : cl;
            P[e] = v0;
        }
        WSYNC();
    }
    if (singular) return singular;
    if (lane < m)
        for (int r = lane; r < m; ++r) P[pidx(r, lane)] = -P[pidx(r, lane)];
    WSYNC();
    return 0;
}

// ----------------------------------------------------------------------------------------------
// Multipliers.  Mem is the solver's per-wave LDS struct (P, the effective rows e_al / e_be / e_ga / e_de / e_d at stages
// w_k, and the vectors sv, lam, ub, sub, vub).

// C x for the working-set rows (x given through LDS images x / sx / vx): result for lane i < m
template <class Mem>
__device__ __forceinline__ double rows_dot_img(const Mem& M, int i, int N, const double* x, const double* sx,
                                               const double* vx) {
    const int ki = M.w_k[i];
    double s = M.e_al[i] * sx[ki] + M.e_be[i] * vx[ki];
    if (ki < N) s += M.e_ga[i] * x[ki];
    if (ki > 0) s += M.e_de[i] * x[ki - 1];
    return s;
}

// lam = -P (d + C h (+ nothing else)); h given through ub/sub/vub
template <class Mem>
__device__ __forceinline__ void solve_multipliers(Mem& M, int m, int lane, int N) {
    if (lane < m) M.sv[lane] = M.e_d[lane] + rows_dot_img(M, lane, N, M.ub, M.sub, M.vub);
    WSYNC();
    if (lane < m) {
        double acc = 0.0;
        for (int j = 0; j < m; ++j) acc = fma(M.P[pidx(lane, j)], M.sv[j], acc);
        M.lam[lane] = -acc;
    }
    WSYNC();
}

}  // namespace eepacc
