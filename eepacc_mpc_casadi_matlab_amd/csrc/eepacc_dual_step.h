// eepacc_dual_step.h -- the part of a dual active-set pass that the ABMPC (eepacc_ab_impl.inc) and FBMPC (eepacc_fbs.hip)
// solvers share, between the table maintenance of eepacc_schur.h and what is each controller's own (row catalogue,
// condensing, slack groups, the local variable w): the scatter of C' vec into the stage images, the value of a row at
// its stage, the step rates, the refinement loop of the primal point, the event codes of the ratio test and the ladder of the
// violation tolerance.  Mem is the solver's per-wave LDS struct (WaveMem / FMem); everything else is plain scalars, and
// what a solver does in the middle of a routine comes in as a lambda.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_schur.h"

namespace eepacc {

// ----------------------------------------------------------------------------------------------
// Stage images ws | wv | wa: weights on (s_k, v_k, a_k), k = 0..N, that the solver's adjoint() turns into a covector.

// += scale * (row al, be, ga, de at stage kq), by the one lane that calls it (a_N and a_{-1} do not exist)
template <class Mem>
__device__ __forceinline__ void scatter_row(Mem& M, int kq, int N, double scale, double al, double be, double ga, double de) {
    atomicAdd(&M.ws[kq], scale * al);
    atomicAdd(&M.wv[kq], scale * be);
    if (kq < N && ga != 0.0) atomicAdd(&M.wa[kq], scale * ga);
    if (kq > 0 && de != 0.0) atomicAdd(&M.wa[kq - 1], scale * de);
}

// += sign * C' vec for the m working-set rows, one row per lane
template <class Mem>
__device__ __forceinline__ void scatter_rows(Mem& M, int m, int N, int lane, const double* vec, double sign) {
    if (lane < m) {
        const int ki = M.w_k[lane];
        const double l = sign * vec[lane];
        atomicAdd(&M.ws[ki], l * M.e_al[lane]);
        atomicAdd(&M.wv[ki], l * M.e_be[lane]);
        if (ki < N && M.e_ga[lane] != 0.0) atomicAdd(&M.wa[ki], l * M.e_ga[lane]);
        if (ki > 0 && M.e_de[lane] != 0.0) atomicAdd(&M.wa[ki - 1], l * M.e_de[lane]);
    }
}

// value of the row q at its stage kq minus d, for a vector given through its LDS images a / s / v (d is subtracted where
// the solvers have always subtracted it, before the two input terms: the sum rounds as it did)
__device__ __forceinline__ double row_value(const Incoming& q, int kq, int N, const double* a, const double* s, const double* v,
                                            double d) {
    double x = q.al * s[kq] + q.be * v[kq] - d;
    if (kq < N) x += q.ga * a[kq];
    if (kq > 0) x += q.de * a[kq - 1];
    return x;
}

// ----------------------------------------------------------------------------------------------
// Rates of the working-set multipliers along the step of an incoming row whose u = He c_q lies in ub | sub | vub:
// sv = C u, rv = P sv; returns sv' rv.  For m > 0: the solvers keep `if (m > 0)` around the call (with the test inside the
// routine, four ABMPC kernels spill other scalar registers: profiles/dual_step_codegen.txt)
template <class Mem>
__device__ __forceinline__ double step_rates(Mem& M, int m, int N, int lane) {
    if (lane < m) M.sv[lane] = rows_dot_img(M, lane, N, M.ub, M.sub, M.vub);
    WSYNC();
    double r = 0.0, sr = 0.0;
    if (lane < m) {
        for (int j = 0; j < m; ++j) r = fma(M.P[pidx(lane, j)], M.sv[j], r);
        M.rv[lane] = r;
        sr = M.sv[lane] * r;
    }
    WSYNC();
    return wv::wave_sum(sr);
}

// Primal point + iterative refinement: the multipliers come out of the explicit inverse P, whose accuracy degrades with
// cond(S) (many active rows, stiff ORIG weights); the residual of the working-set equations  C a - D lam = d  is evaluated
// exactly from the images av | shv | vhv and fed back through P until it is at rounding level.  recompute() is the
// solver's primal point from M.lam (stationarity holds by its construction); it refreshes the three images.
// Returns the relative residual of the working-set rows before any correction: a measure of how good P still is.
template <class Mem, class Recompute>
__device__ __forceinline__ double refine_rounds(Mem& M, int m, int N, int lane, int max_rounds, double res_tol,
                                                Recompute recompute) {
    recompute();
    if (m == 0) return 0.0;
    double rel0 = 0.0;
    for (int round = 0; round < max_rounds; ++round) {
        double res = 0.0, rel = 0.0;
        if (lane < m) {
            res = rows_dot_img(M, lane, N, M.av, M.shv, M.vhv) - M.e_d[lane];
            rel = fabs(res) / (1.0 + fabs(M.e_d[lane]));
            M.sv[lane] = res;
        }
        int dummy = lane;
        wv::wave_argmax(rel, dummy);
        if (round == 0) rel0 = rel;
        if (!(rel > res_tol)) break;
        WSYNC();
        if (lane < m) {
            double acc = 0.0;
            for (int j = 0; j < m; ++j) acc = fma(M.P[pidx(lane, j)], M.sv[j], acc);
            M.lam[lane] += acc;
        }
        WSYNC();
        recompute();
    }
    return rel0;
}

// ----------------------------------------------------------------------------------------------
// Ratio test: what can end a step before the incoming row is satisfied
enum Ev : int { EV_NONE = 0, EV_DROP, EV_COMPL, EV_DROPH, EV_CAP, EV_CAPIN };

// Code of an event: what happens (Ev), at which lane, to which row type or group.  kNoEvent: a lane without a candidate.
struct EvCode {
    static constexpr int kNoEvent = 0x7fffffff;
    __device__ __forceinline__ static int pack(int kind, int lane, int t) { return (kind << 16) | (lane << 5) | t; }
    __device__ __forceinline__ static int kind(int ev) { return ev >> 16; }
    __device__ __forceinline__ static int lane(int ev) { return (ev >> 5) & 63; }
    __device__ __forceinline__ static int type(int ev) { return ev & 31; }
};

// Anti-cycling: rounding noise of the order of (largest multiplier) x eps can flip rows in and out at the tightest
// violation tolerance tol0 (seen with the ORIG weights, w_f = 1e7); it is relaxed decade by decade, never beyond
// 1000 tol0, if the iteration count shows that this is happening.
__device__ __forceinline__ double viol_tolerance(double tol0, int iters, int N) {
    const int relax_every = 3 * N + 30;
    return tol0 * (iters < relax_every ? 1.0 : (iters < 2 * relax_every ? 10.0 : (iters < 3 * relax_every ? 100.0 : 1000.0)));
}

}  // namespace eepacc
