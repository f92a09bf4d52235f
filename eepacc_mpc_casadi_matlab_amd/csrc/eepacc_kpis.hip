// eepacc_kpis.hip -- k_kpis: the per-instance key figures of a closed-loop run (the report of ABO/Main.m:131-263 and the
// fuel economy of ABO/Custom_plots.m:73-107; field list and definitions: include/eepacc.h, eepacc_kpis) reduced on the device
// from traj [n_steps][EEPACC_OUT_N][B] and status [n_steps][B].  report.kpi_table is the same in numpy.
//
// Geometry.  The operator streams four of the twelve rows once and does a few dozen flops per sample: bandwidth and
// latency decide.  A workgroup serves 64 consecutive instances, lane = instance, so every row read of a wave is one
// contiguous 512-byte line; its kKpiWaves waves take contiguous slices of the step axis and every thread reduces its slice
// serially.  The slices are joined through LDS by wave 0, in slice order and without atomics: the result does not depend
// on timing, two runs agree bit for bit.
//
// The cut-off in one pass.  The comfort statistics and the figures "at the cut-off distance" depend on ind, the first
// i >= 1 with s[i-1] < cut < s[i] (n - 1 where there is none), which may lie in any slice.  Every slice therefore
// reduces "up to my own first crossing, or all of me" next to its full-range sums, treating i = n - 1 as a crossing, so
// that some slice always has one; the join merges the slices in order up to and including the first that saw one.  What
// reaches over a slice boundary is read from global memory (s[k0-1], a[k1]) or kept beside the sums (the energy at
// sample ind - 2 may end one or two samples before a slice starts: every slice also hands on its sum without its last
// sample).
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_device.h"
#include "eepacc_stage.h"
#include "eepacc_power.h"
#include "eepacc_kpis.h"
#include "../../include/eepacc.h"

namespace eepacc {

namespace {

// slots of a slice's record in LDS, [slot][wave][lane]
enum { Q_SUMP = 0, Q_SUMPX, Q_CUTP, Q_SUMFC, Q_SMAX, Q_AMAX, Q_AMIN, Q_ASQ, Q_JMAX, Q_JMIN, Q_JSQ, Q_INTS };
static_assert(Q_INTS + 1 == kKpiRecDoubles, "record layout");
static_assert(kKpiWaves == EEPACC_KPI_WAVES && kKpiMinSlice == EEPACC_KPI_MIN_SLICE, "include/eepacc.h states the geometry");

}  // namespace

// Ls: kpi_slice_len(n).  kClasses: Kp and cutp are the handle's class arrays and every instance reads its own class's.
template <bool kClasses>
__global__ __launch_bounds__(64 * kKpiWaves) void k_kpis(const KpiCfg* __restrict__ Kp, const int32_t* __restrict__ class_of,
                                                         const double* __restrict__ cutp, int B, int n, int Ls,
                                                         const double* __restrict__ traj, const int32_t* __restrict__ status,
                                                         double* __restrict__ kpi) {
#pragma clang fp contract(off)
    extern __shared__ double rec[];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b_own = blockIdx.x * 64 + lane;
    const int b = b_own < B ? b_own : B - 1;               // lanes past the batch redo the last instance and store nothing
    const int cls = kClasses ? class_of[b] : 0;
    const KpiCfg& K = Kp[cls];
    const double cut = cutp[cls];
    const double Ts = K.Ts;
    const size_t stride = (size_t)EEPACC_OUT_N * B;
    const double* ps = traj + (size_t)EEPACC_OUT_S * B + b;
    const double* pv = traj + (size_t)EEPACC_OUT_V * B + b;
    const double* pf = traj + (size_t)EEPACC_OUT_FM * B + b;
    const double* pa = traj + (size_t)EEPACC_OUT_A * B + b;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    const int k0 = w * Ls, k1 = (k0 + Ls < n) ? k0 + Ls : n;
    if (k0 < n) {
        double acc = 0.0, acc_m1 = 0.0;                    // sum of P over the samples [k0, k) and [k0, k-1)
        double cutP = 0.0, sumFC = 0.0, smax = -inf;
        double amax = -inf, amin = inf, asq = 0.0, jmax = -inf, jmin = inf, jsq = 0.0;
        int bad = 0, code = -1;                            // code: 2 * (index of the first crossing) + (a real one)
        double a_k = pa[(size_t)k0 * stride];
        double s_prev = k0 > 0 ? ps[(size_t)(k0 - 1) * stride] : 0.0;
        for (int k = k0; k < k1; ++k) {
            const double s_k = ps[(size_t)k * stride], v = pv[(size_t)k * stride], x = pf[(size_t)k * stride];
            const double a_n = (k + 1 < n) ? pa[(size_t)(k + 1) * stride] : 0.0;
            bad += status[(size_t)k * B + b] != 0;
            smax = fmax(smax, s_k);
            const double p = power_surface(K.b5, x, kRpmPerRadS * v * K.phi);
            if (k >= 1) {                                  // Custom_plots.m:81: the loop starts at the second sample
                const double TW = fmax(0.0, (K.lm * a_k + K.F0 + K.F2 * v * v) * K.R_w);
                sumFC += fmax(0.25, K.p00 + K.p10 * v + K.p01 * TW);
            }
            const bool real = k >= 1 && s_prev < cut && s_k > cut;
            if (code < 0 && (real || k == n - 1)) {
                code = 2 * k + (real ? 1 : 0);
                // sum of P up to sample max(k - 2, 0), as far as it lies in this slice
                cutP = k >= 2 ? acc_m1 : (k == 1 ? acc : p);
            }
            if (code < 0) {                                // k < ind: inside the comfort window
                const double j = (a_n - a_k) / Ts;
                amax = fmax(amax, a_k); amin = fmin(amin, a_k); asq += a_k * a_k;
                jmax = fmax(jmax, j); jmin = fmin(jmin, j); jsq += j * j;
            }
            acc_m1 = acc; acc += p;
            s_prev = s_k; a_k = a_n;
        }
        const int o = w * 64 + lane;
        rec[Q_SUMP * 64 * kKpiWaves + o] = acc;
        rec[Q_SUMPX * 64 * kKpiWaves + o] = acc_m1;        // without the slice's last sample
        rec[Q_CUTP * 64 * kKpiWaves + o] = cutP;
        rec[Q_SUMFC * 64 * kKpiWaves + o] = sumFC;
        rec[Q_SMAX * 64 * kKpiWaves + o] = smax;
        rec[Q_AMAX * 64 * kKpiWaves + o] = amax;
        rec[Q_AMIN * 64 * kKpiWaves + o] = amin;
        rec[Q_ASQ * 64 * kKpiWaves + o] = asq;
        rec[Q_JMAX * 64 * kKpiWaves + o] = jmax;
        rec[Q_JMIN * 64 * kKpiWaves + o] = jmin;
        rec[Q_JSQ * 64 * kKpiWaves + o] = jsq;
        rec[Q_INTS * 64 * kKpiWaves + o] = __hiloint2double(bad, code);
    }
    __syncthreads();
    if (w != 0) return;

    // join, in slice order
    const int nS = (n + Ls - 1) / Ls;
    double Eall = 0.0, Eprev = 0.0, pxPrev = 0.0, Ecut = 0.0, fuel = 0.0, smax = -inf;
    double amax = -inf, amin = inf, asq = 0.0, jmax = -inf, jmin = inf, jsq = 0.0;
    int bad = 0, ind = 0, reached = 0;
    bool done = false;
    for (int q = 0; q < nS; ++q) {
        const int o = q * 64 + lane;
        const double ints = rec[Q_INTS * 64 * kKpiWaves + o];
        const int code = __double2loint(ints);
        bad += __double2hiint(ints);
        fuel += rec[Q_SUMFC * 64 * kKpiWaves + o];
        smax = fmax(smax, rec[Q_SMAX * 64 * kKpiWaves + o]);
        if (!done) {
            amax = fmax(amax, rec[Q_AMAX * 64 * kKpiWaves + o]); amin = fmin(amin, rec[Q_AMIN * 64 * kKpiWaves + o]);
            asq += rec[Q_ASQ * 64 * kKpiWaves + o];
            jmax = fmax(jmax, rec[Q_JMAX * 64 * kKpiWaves + o]); jmin = fmin(jmin, rec[Q_JMIN * 64 * kKpiWaves + o]);
            jsq += rec[Q_JSQ * 64 * kKpiWaves + o];
            if (code >= 0) {
                ind = code >> 1; reached = code & 1;
                // sample ind - 2 is the last but one of the slice before when the crossing is a slice's first step
                const bool drop = q > 0 && ind == q * Ls;
                Ecut = (drop ? Eprev + pxPrev : Eall) + rec[Q_CUTP * 64 * kKpiWaves + o];
                done = true;
            }
        }
        Eprev = Eall;
        pxPrev = rec[Q_SUMPX * 64 * kKpiWaves + o];
        Eall += rec[Q_SUMP * 64 * kKpiWaves + o];
    }
    if (b_own >= B) return;
    const int k2 = ind >= 2 ? ind - 2 : 0;                 // the host code's index wraps for ind < 2; clamped here
    const double vlim = interp_pwa(cut, K.s_speedLim, K.v_speedLim, K.n_speedLim);
    if (n == 1) {                                          // ind = 0: the window is the one sample; no jerk
        const double a0 = pa[0];
        amax = a0; amin = a0; asq = a0 * a0; jmax = 0.0; jmin = 0.0; jsq = 0.0;
    }
    const double cnt = ind >= 1 ? (double)ind : 1.0;
    const double fuel_kg = fuel / 1000.0 * Ts;
    double* out = kpi + b;
    out[(size_t)EEPACC_KPI_BAD_EXITS * B] = (double)bad;
    out[(size_t)EEPACC_KPI_DISTANCE_M * B] = ps[(size_t)(n - 1) * stride];
    out[(size_t)EEPACC_KPI_ENERGY_J * B] = Ts * Eall;
    out[(size_t)EEPACC_KPI_CUTOFF_INDEX * B] = (double)ind;
    out[(size_t)EEPACC_KPI_REACHED * B] = (double)reached;
    out[(size_t)EEPACC_KPI_VLIM_ERR * B] = vlim - pv[(size_t)k2 * stride];
    out[(size_t)EEPACC_KPI_ENERGY_CUTOFF_J * B] = Ts * Ecut;
    out[(size_t)EEPACC_KPI_TIME_CUTOFF_S * B] = (double)ind * Ts;
    out[(size_t)EEPACC_KPI_A_MAX * B] = amax;
    out[(size_t)EEPACC_KPI_A_MIN * B] = amin;
    out[(size_t)EEPACC_KPI_A_RMS * B] = sqrt(asq / cnt);
    out[(size_t)EEPACC_KPI_J_MAX * B] = jmax;
    out[(size_t)EEPACC_KPI_J_MIN * B] = jmin;
    out[(size_t)EEPACC_KPI_J_RMS * B] = sqrt(jsq / cnt);
    out[(size_t)EEPACC_KPI_FUEL_KG * B] = fuel_kg;
    out[(size_t)EEPACC_KPI_FE_L_PER_100KM * B] = fuel_kg / 0.835 / (smax / 1000.0) * 100.0;
}

hipError_t launch_kpis(const KpiCfg* dK, const int32_t* class_of, const double* cut, int B, int n_steps, const double* traj,
                       const int32_t* status, double* kpi, hipStream_t stream) {
    constexpr size_t smem = (size_t)kKpiRecDoubles * kKpiWaves * 64 * sizeof(double);      // 96 KiB
    // above the 64 KiB a kernel gets unasked; set per launch, since the attribute belongs to the current device
    const void* fn = class_of ? reinterpret_cast<const void*>(k_kpis<true>) : reinterpret_cast<const void*>(k_kpis<false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
    if (e != hipSuccess) return e;
    const int Ls = kpi_slice_len(n_steps);
    const dim3 grid((B + 63) / 64), block(64 * kKpiWaves);
    if (class_of) hipLaunchKernelGGL(k_kpis<true>, grid, block, smem, stream, dK, class_of, cut, B, n_steps, Ls, traj, status, kpi);
    else hipLaunchKernelGGL(k_kpis<false>, grid, block, smem, stream, dK, class_of, cut, B, n_steps, Ls, traj, status, kpi);
    return hipGetLastError();
}

}  // namespace eepacc
