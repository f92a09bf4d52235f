// eepacc_follow.hip -- k_follow_kpis: how every instance of a closed-loop run kept its distance to the lead (headway
// distance and time of ABO/Main.m:679-771 against the minimum-headway policy of :687) and what every term of the objective
// cost over the run (the last entries of cost_* of ABO/RunOpt_ABMPC.m:382-404 and ABO/RunOpt_FBMPC.m:373-397), reduced on the
// device from traj [n_steps][EEPACC_OUT_N][B] and the lead traces s_tv, v_tv [n_steps][B].  Field list and definitions:
// include/eepacc.h, eepacc_follow_kpis; report.follow_table is the same in numpy.
//
// Geometry: that of k_kpis (eepacc_kpis.hip).  A workgroup serves 64 consecutive instances, lane = instance, so every row
// read of a wave is one contiguous 512-byte line; its kKpiWaves waves take contiguous slices of the step axis and every
// thread reduces its slice serially.  There is no cut-off here, so a slice's record is plain: four minima, the first index
// of the smallest gap, one maximum, two counts and seven sums.  Wave 0 joins the records from LDS in slice order, without
// atomics.  The only thing that reaches over a slice boundary is a[k1], the jerk of a slice's last step, read from global
// memory.
//
// Exactness.  Contraction is off in this translation unit and the minima, the maximum and the index are kept by
// comparisons (`<`, `>`), never by an instruction that may pick either of two equal values: v tau_min, h / v and a * a are
// each rounded once, the first of equal gaps wins within a slice and, the join being in slice order with `<`, across
// slices.  Those fields and the counts equal the specification bit for bit; a sum differs from it by the order of addition.
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_power.h"
#include "eepacc_follow.h"
#include "../../include/eepacc.h"

#pragma clang fp contract(off)      // file scope: nothing in this translation unit is fused by the compiler's choice

namespace eepacc {

namespace {

// slots of a slice's record in LDS: doubles [slot][wave][lane], then ints [slot][wave][lane]
enum { Q_HMIN = 0, Q_THW, Q_MARGIN, Q_TTC, Q_XIMAX, Q_SUM };      // Q_SUM + i: the sum of cost term i (P, a, j, xi_v, xi_h, xi_s, xi_f)
enum { QI_INDEX = 0, QI_LEAD, QI_VIOL };
constexpr int kTerms = 7;
constexpr int kSlots = 64 * kKpiWaves;                            // records of a workgroup per slot
static_assert(Q_SUM + kTerms == kFollowRecDoubles && QI_VIOL + 1 == kFollowRecInts, "record layout");
static_assert(EEPACC_FKPI_COST_XI_F - EEPACC_FKPI_COST_P + 1 == kTerms && EEPACC_FKPI_COST_XI_F + 1 == EEPACC_FKPI_N, "include/eepacc.h lists the seven costs last");
static_assert(kFollowLdsBytes <= 160 * 1024, "a workgroup's records must fit the LDS of one CU");

}  // namespace

// Ls: kpi_slice_len(n); class_of: null on a handle without classes.
__global__ __launch_bounds__(64 * kKpiWaves) void k_follow_kpis(const FollowCfg* __restrict__ Fp, const int32_t* __restrict__ class_of,
                                                                int weights, int B, int n, int Ls, const double* __restrict__ traj,
                                                                const double* __restrict__ s_tv, const double* __restrict__ v_tv,
                                                                double* __restrict__ fkpi) {
    extern __shared__ __attribute__((aligned(16))) double rec[];
    int32_t* reci = reinterpret_cast<int32_t*>(rec + kFollowRecDoubles * kSlots);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b_own = blockIdx.x * 64 + lane;
    const int b = b_own < B ? b_own : B - 1;               // lanes past the batch redo the last instance and store nothing
    const FollowCfg& K = Fp[class_of ? class_of[b] : 0];
    const double* wt = K.w[weights];
    const double Ts = K.Ts, h_min = K.h_min, tau_min = K.tau_min;
    const bool with_P = wt[0] != 0.0;
    const size_t stride = (size_t)EEPACC_OUT_N * B;
    const double* ps = traj + (size_t)EEPACC_OUT_S * B + b;
    const double* pv = traj + (size_t)EEPACC_OUT_V * B + b;
    const double* pf = traj + (size_t)EEPACC_OUT_FM * B + b;
    const double* pa = traj + (size_t)EEPACC_OUT_A * B + b;
    const double* pxv = traj + (size_t)EEPACC_OUT_XI_V * B + b;
    const double* pxh = traj + (size_t)EEPACC_OUT_XI_H * B + b;
    const double* pxs = traj + (size_t)EEPACC_OUT_XI_S * B + b;
    const double* pxf = traj + (size_t)EEPACC_OUT_XI_F * B + b;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    const int k0 = w * Ls, k1 = (k0 + Ls < n) ? k0 + Ls : n;
    if (k0 < n) {
        double hmin = inf, thw = inf, margin = inf, ttc = inf, ximax = -inf;
        double sum[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        int index = -1, lead = 0, viol = 0;
        double a_k = pa[(size_t)k0 * stride];
        for (int k = k0; k < k1; ++k) {
            const double s_k = ps[(size_t)k * stride], v = pv[(size_t)k * stride];
            const double xv = pxv[(size_t)k * stride], xh = pxh[(size_t)k * stride];
            const double xs = pxs[(size_t)k * stride], xf = pxf[(size_t)k * stride];
            const double stv = s_tv[(size_t)k * B + b], vtv = v_tv[(size_t)k * B + b];
            if (xh > ximax) ximax = xh;
            if (stv < 1e6) {                               // a lead sample (Main.m:288); false for a NaN
                const double h = stv - s_k;
                ++lead;
                if (h < hmin) { hmin = h; index = k; }
                if (v > 0.0) {
                    const double t = h / v;
                    if (t < thw) thw = t;
                }
                const double vt = v * tau_min;
                const double m = h - (vt > h_min ? vt : h_min);
                if (m < margin) margin = m;
                viol += m < 0.0;
                const double dv = v - vtv;
                if (dv > 0.0) {
                    const double t = h / dv;
                    if (t < ttc) ttc = t;
                }
            }
            double a_n = 0.0;
            if (k + 1 < n) {                               // k = 1:N_sim of the reference: the last sample is in no cost
                a_n = pa[(size_t)(k + 1) * stride];
                const double j = (a_n - a_k) / Ts;
                if (with_P) {
                    const double p = power_surface(K.b5, pf[(size_t)k * stride], kRpmPerRadS * v * K.phi);
                    sum[0] += p * p;
                }
                sum[1] += a_k * a_k; sum[2] += j * j;
                sum[3] += xv; sum[4] += xh; sum[5] += xs; sum[6] += xf;
            }
            a_k = a_n;
        }
        const int o = w * 64 + lane;
        rec[Q_HMIN * kSlots + o] = hmin;
        rec[Q_THW * kSlots + o] = thw;
        rec[Q_MARGIN * kSlots + o] = margin;
        rec[Q_TTC * kSlots + o] = ttc;
        rec[Q_XIMAX * kSlots + o] = ximax;
#pragma unroll
        for (int i = 0; i < kTerms; ++i) rec[(Q_SUM + i) * kSlots + o] = sum[i];
        reci[QI_INDEX * kSlots + o] = index;
        reci[QI_LEAD * kSlots + o] = lead;
        reci[QI_VIOL * kSlots + o] = viol;
    }
    __syncthreads();
    if (w != 0 || b_own >= B) return;

    // join, in slice order; `<` keeps the earlier slice's index where two slices hold the same smallest gap
    const int nS = (n + Ls - 1) / Ls;
    double hmin = inf, thw = inf, margin = inf, ttc = inf, ximax = -inf;
    double sum[kTerms] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    int index = -1, lead = 0, viol = 0;
    for (int q = 0; q < nS; ++q) {
        const int o = q * 64 + lane;
        const double h = rec[Q_HMIN * kSlots + o], t = rec[Q_THW * kSlots + o], m = rec[Q_MARGIN * kSlots + o];
        const double c = rec[Q_TTC * kSlots + o], x = rec[Q_XIMAX * kSlots + o];
        if (h < hmin) { hmin = h; index = reci[QI_INDEX * kSlots + o]; }
        if (t < thw) thw = t;
        if (m < margin) margin = m;
        if (c < ttc) ttc = c;
        if (x > ximax) ximax = x;
        lead += reci[QI_LEAD * kSlots + o];
        viol += reci[QI_VIOL * kSlots + o];
#pragma unroll
        for (int i = 0; i < kTerms; ++i) sum[i] += rec[(Q_SUM + i) * kSlots + o];
    }
    double* out = fkpi + b;
    out[(size_t)EEPACC_FKPI_LEAD_SAMPLES * B] = (double)lead;
    out[(size_t)EEPACC_FKPI_H_MIN_M * B] = hmin;
    out[(size_t)EEPACC_FKPI_H_MIN_INDEX * B] = (double)index;
    out[(size_t)EEPACC_FKPI_THW_MIN_S * B] = thw;
    out[(size_t)EEPACC_FKPI_MARGIN_MIN_M * B] = margin;
    out[(size_t)EEPACC_FKPI_MARGIN_VIOL_STEPS * B] = (double)viol;
    out[(size_t)EEPACC_FKPI_TTC_MIN_S * B] = ttc;
    out[(size_t)EEPACC_FKPI_XI_H_MAX * B] = ximax;
    out[(size_t)EEPACC_FKPI_COST_P * B] = with_P ? wt[0] * sum[0] : 0.0;
#pragma unroll
    for (int i = 1; i < kTerms; ++i) out[(size_t)(EEPACC_FKPI_COST_P + i) * B] = wt[i] * sum[i];
}

hipError_t launch_follow_kpis(const FollowCfg* dF, const int32_t* class_of, int weights, int B, int n_steps, const double* traj,
                              const double* s_tv, const double* v_tv, double* fkpi, hipStream_t stream) {
    // 108 KiB: above the 64 KiB a kernel gets unasked; set per launch, since the attribute belongs to the current device
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(k_follow_kpis), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)kFollowLdsBytes);
    if (e != hipSuccess) return e;
    const int Ls = kpi_slice_len(n_steps);
    const dim3 grid((B + 63) / 64), block(64 * kKpiWaves);
    hipLaunchKernelGGL(k_follow_kpis, grid, block, kFollowLdsBytes, stream, dF, class_of, weights, B, n_steps, Ls, traj, s_tv, v_tv, fkpi);
    return hipGetLastError();
}

}  // namespace eepacc
