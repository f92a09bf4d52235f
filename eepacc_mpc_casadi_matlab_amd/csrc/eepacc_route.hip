// eepacc_route.hip -- k_route_kpis: whether every instance of a closed-loop run obeyed its route and the comfort envelope,
// reduced on the device from traj [n_steps][EEPACC_OUT_N][B]: the measured speed against the sign-posted limit, the curve
// speed, the stop-sign profile and the red-light cap (what ABO/Main.m:374-433 draws for one run), the stop lines and lights
// that were crossed and the phase the lights were in (:486-534), and the acceleration and jerk against the limits of
// EstimateRouteAndComfortBounds.m:154-189.  Field list, definitions and the deviations from the planner's own look-up:
// include/eepacc.h, eepacc_route_kpis; report.route_table and report.route_limits are the same in numpy.
//
// Geometry: that of k_kpis (eepacc_kpis.hip).  A workgroup serves 64 consecutive instances, lane = instance, so every row
// read of a wave is one contiguous 512-byte line; its kKpiWaves waves take contiguous slices of the step axis and every
// thread reduces its slice serially.  A slice's record is nine maxima, one minimum, two first indices and nine counts.
// Wave 0 joins the records from LDS in slice order, without atomics.  Three things reach over a slice boundary, all read from
// global memory: s[k0-1] and v[k0-1], for a line crossed on a slice's first step, and a[k1], for the jerk of its last step.
// A crossing between k-1 and k belongs to the slice that holds k, so none is counted twice or lost.
//
// Route tables: on a handle without classes every lane reads the one RouteCfg through a wave-uniform address, which the
// compiler turns into scalar loads (k_route_kpis<false>); on a class handle the lanes differ and read per lane (<true>).
//
// Exactness.  Every figure is a maximum, a minimum, a count or an index; there are no sums.  Contraction is off in this
// translation unit, maxima and the minimum are kept by comparisons (`>`, `<`) from -inf and +inf, never by an instruction
// that may pick either of two equal values or hand a NaN on: the first of equal values wins within a slice and, the join
// being in slice order, across slices; a NaN is never taken and never counted.  All fields, and `limits`, equal the
// specification bit for bit.
#include <hip/hip_runtime.h>
#include <math.h>
#include "eepacc_route.h"
#include "../../include/eepacc.h"

#pragma clang fp contract(off)      // file scope: nothing in this translation unit is fused by the compiler's choice

namespace eepacc {

namespace {

// slots of a slice's record in LDS: doubles [slot][wave][lane], then ints [slot][wave][lane]
enum { Q_VLIM = 0, Q_VCURV, Q_VSTOP, Q_VTL, Q_CROSSV, Q_AOVER, Q_AUNDER, Q_JOVER, Q_JUNDER, Q_VMIN };
enum { QI_INDEX = 0, QI_VIOL /* four */, QI_STOPS = QI_VIOL + 4, QI_LIGHTS, QI_RED, QI_REDPOSS, QI_REDFIRST, QI_COMFORT };
constexpr int kSlots = 64 * kKpiWaves;                            // records of a workgroup per slot
constexpr double kNoCap = 1e5;                                    // "no cap" of EstimateRouteAndComfortBounds.m:115,126
static_assert(Q_VMIN + 1 == kRouteRecDoubles && QI_COMFORT + 1 == kRouteRecInts, "record layout");
static_assert(EEPACC_RKPI_V_MIN + 1 == EEPACC_RKPI_N && EEPACC_RLIM_V_TL + 1 == EEPACC_RLIM_N && EEPACC_RLIM_N == 4, "include/eepacc.h");
static_assert(kRouteLdsBytes <= 160 * 1024, "a workgroup's records must fit the LDS of one CU");

// vals[j] on knots[j] <= s < knots[j+1]; vals[0] before the first knot and for a NaN, vals[n-1] from the last knot on
__device__ inline double held_table(double s, const double* knots, const double* vals, int n) {
    double y = vals[0];
    for (int j = 0; j < n; ++j)
        if (s >= knots[j]) y = vals[j];
    return y;
}

// MATLAB's mod(t - TL(2), TL(3) + TL(4)) < TL(3); a cycle of length 0 returns its argument (route_bounds, eepacc_stage.h)
__device__ inline bool is_red(const double* TL, double t) {
    const double x = t - TL[1], mm = TL[2] + TL[3];
    const double md = (mm == 0.0) ? x : x - floor(x / mm) * mm;
    return md < TL[2];
}

// the four caps at the position s and the time t, in the order EEPACC_RLIM_*
__device__ inline void route_caps(const RouteCfg& K, double s, double t, double cap[4]) {
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    cap[0] = held_table(s, K.s_speedLim, K.v_speedLim, K.n_speedLim);
    cap[1] = held_table(s, K.s_curv, K.vcurv_tab, K.n_curv);
    double v_stop = K.n_stop > 0 ? inf : kNoCap;
    for (int j = 0; j < K.n_stop; ++j) {
        const double x = fabs(K.stopLoc[j] - s) * K.stopRefVelSlope + K.stopVel;     // Main.m:375-385
        if (x < v_stop) v_stop = x;
    }
    cap[2] = v_stop;
    double v_TL = inf;
    for (int j = 0; j < K.n_TL; ++j) {
        const double* TL = &K.TLLoc[4 * j];
        if (!is_red(TL, t)) continue;
        const double d = TL[0] - s, ad = fabs(d);
        double x;                                                                    // EstimateRouteAndComfortBounds.m:133-139
        if (d < 0.0) x = ad * K.stopRefVelSlope + K.TLstopVel;
        else if (ad < K.TLStopRegionSize) x = K.TLstopVel;
        else x = fabs(d - K.stopVel) * K.stopRefVelSlope + K.TLstopVel;
        if (ad < K.stopRefDist && x < v_TL) v_TL = x;
    }
    cap[3] = (v_TL == inf) ? kNoCap : v_TL;
}

// EstimateRouteAndComfortBounds.m:154-172, and :173-189 on a handle of a baseline controller; a NaN takes the last branch
__device__ inline void comfort_envelope(const RouteCfg& K, double v, double& a_min, double& a_max, double& j_min, double& j_max) {
    if (K.bl_mode) {
        double a, j;
        if (v < 5.0) { a = K.bl_aLo; j = K.bl_jLo; }
        else if (v < 20.0) {
            a = (4.0 * K.bl_aLo - K.bl_aHi) / 3.0 + (K.bl_aHi - K.bl_aLo) / 15.0 * v;
            j = (4.0 * K.bl_jLo - K.bl_jHi) / 3.0 + (K.bl_jHi - K.bl_jLo) / 15.0 * v;
        } else { a = K.bl_aHi; j = K.bl_jHi; }
        a_min = -a; a_max = a; j_min = -j; j_max = j;
        return;
    }
    if (v < 5.0) { a_min = -5.0; a_max = 4.0; j_min = -5.0; j_max = 5.0; }
    else if (v < 20.0) {
        a_min = -5.5 + v / 10.0; a_max = 14.0 / 3.0 - 2.0 * v / 15.0;
        j_min = -35.0 / 6.0 + v / 6.0; j_max = 35.0 / 6.0 - v / 6.0;
    } else { a_min = -3.5; a_max = 2.0; j_min = -2.5; j_max = 2.5; }
}

}  // namespace

// Ls: kpi_slice_len(n); Classes: class_of is the map of a class handle (otherwise it is not read and every lane takes Rp[0]).
template <bool Classes>
__global__ __launch_bounds__(64 * kKpiWaves) void k_route_kpis(const RouteCfg* __restrict__ Rp, const int32_t* __restrict__ class_of,
                                                               int B, int n, int Ls, double t_start, double v_tol, double a_tol,
                                                               double j_tol, const double* __restrict__ traj,
                                                               double* __restrict__ rkpi, double* __restrict__ limits) {
    extern __shared__ __attribute__((aligned(16))) double rec[];
    int32_t* reci = reinterpret_cast<int32_t*>(rec + kRouteRecDoubles * kSlots);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b_own = blockIdx.x * 64 + lane;
    const int b = b_own < B ? b_own : B - 1;               // lanes past the batch redo the last instance and store nothing
    const RouteCfg& K = Rp[Classes ? class_of[b] : 0];
    const double Ts = K.Ts;
    const size_t stride = (size_t)EEPACC_OUT_N * B;
    const double* ps = traj + (size_t)EEPACC_OUT_S * B + b;
    const double* pv = traj + (size_t)EEPACC_OUT_V * B + b;
    const double* pa = traj + (size_t)EEPACC_OUT_A * B + b;
    const double inf = __longlong_as_double(0x7ff0000000000000LL);

    const int k0 = w * Ls, k1 = (k0 + Ls < n) ? k0 + Ls : n;
    if (k0 < n) {
        double ex[4] = {-inf, -inf, -inf, -inf};
        double crossv = -inf, aover = -inf, aunder = -inf, jover = -inf, junder = -inf, vmin = inf;
        int index = -1, viol[4] = {0, 0, 0, 0};
        int stops = 0, lights = 0, red = 0, redposs = 0, redfirst = -1, comfort = 0;
        double s_prev = 0.0, v_prev = 0.0;
        if (k0 > 0) { s_prev = ps[(size_t)(k0 - 1) * stride]; v_prev = pv[(size_t)(k0 - 1) * stride]; }
        double a_k = pa[(size_t)k0 * stride];
        for (int k = k0; k < k1; ++k) {
            const double s_k = ps[(size_t)k * stride], v = pv[(size_t)k * stride];
            const double t = t_start + (double)k * Ts;
            double cap[4];
            route_caps(K, s_k, t, cap);
            if (limits && b_own < B) {
#pragma unroll
                for (int i = 0; i < 4; ++i) limits[((size_t)k * EEPACC_RLIM_N + i) * B + b] = cap[i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const double e = v - cap[i];
                const bool live = i < 3 || cap[3] < kNoCap;
                if (live && e > ex[i]) { ex[i] = e; if (i == 0) index = k; }
                viol[i] += live && e > v_tol;
            }
            if (v < vmin) vmin = v;
            if (k >= 1) {
                const double t_prev = t_start + (double)(k - 1) * Ts;
                const double slow = v < v_prev ? v : v_prev;
                for (int j = 0; j < K.n_stop; ++j) {
                    const double loc = K.stopLoc[j];
                    if (s_prev < loc && loc <= s_k) {
                        ++stops;
                        if (slow > crossv) crossv = slow;
                    }
                }
                for (int j = 0; j < K.n_TL; ++j) {
                    const double* TL = &K.TLLoc[4 * j];
                    if (s_prev < TL[0] && TL[0] <= s_k) {
                        const bool r0 = is_red(TL, t_prev), r1 = is_red(TL, t);
                        ++lights;
                        red += r0 && r1;
                        if (r0 || r1) {
                            ++redposs;
                            if (redfirst < 0) redfirst = k;
                        }
                    }
                }
            }
            double a_min, a_max, j_min, j_max;
            comfort_envelope(K, v, a_min, a_max, j_min, j_max);
            double eo = a_k - a_max, eu = a_min - a_k;
            if (eo > aover) aover = eo;
            if (eu > aunder) aunder = eu;
            bool bad = eo > a_tol || eu > a_tol;
            double a_n = 0.0;
            if (k + 1 < n) {
                a_n = pa[(size_t)(k + 1) * stride];
                const double j = (a_n - a_k) / Ts;
                eo = j - j_max; eu = j_min - j;
                if (eo > jover) jover = eo;
                if (eu > junder) junder = eu;
                bad = bad || eo > j_tol || eu > j_tol;
            }
            comfort += bad;
            a_k = a_n; s_prev = s_k; v_prev = v;
        }
        const int o = w * 64 + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            rec[(Q_VLIM + i) * kSlots + o] = ex[i];
            reci[(QI_VIOL + i) * kSlots + o] = viol[i];
        }
        rec[Q_CROSSV * kSlots + o] = crossv;
        rec[Q_AOVER * kSlots + o] = aover;
        rec[Q_AUNDER * kSlots + o] = aunder;
        rec[Q_JOVER * kSlots + o] = jover;
        rec[Q_JUNDER * kSlots + o] = junder;
        rec[Q_VMIN * kSlots + o] = vmin;
        reci[QI_INDEX * kSlots + o] = index;
        reci[QI_STOPS * kSlots + o] = stops;
        reci[QI_LIGHTS * kSlots + o] = lights;
        reci[QI_RED * kSlots + o] = red;
        reci[QI_REDPOSS * kSlots + o] = redposs;
        reci[QI_REDFIRST * kSlots + o] = redfirst;
        reci[QI_COMFORT * kSlots + o] = comfort;
    }
    __syncthreads();
    if (w != 0 || b_own >= B) return;

    // join, in slice order; `>` keeps the earlier slice's index where two slices hold the same largest excess
    const int nS = (n + Ls - 1) / Ls;
    double ex[4] = {-inf, -inf, -inf, -inf};
    double crossv = -inf, aover = -inf, aunder = -inf, jover = -inf, junder = -inf, vmin = inf;
    int index = -1, viol[4] = {0, 0, 0, 0};
    int stops = 0, lights = 0, red = 0, redposs = 0, redfirst = -1, comfort = 0;
    for (int q = 0; q < nS; ++q) {
        const int o = q * 64 + lane;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const double e = rec[(Q_VLIM + i) * kSlots + o];
            if (e > ex[i]) { ex[i] = e; if (i == 0) index = reci[QI_INDEX * kSlots + o]; }
            viol[i] += reci[(QI_VIOL + i) * kSlots + o];
        }
        const double c = rec[Q_CROSSV * kSlots + o], ao = rec[Q_AOVER * kSlots + o], au = rec[Q_AUNDER * kSlots + o];
        const double jo = rec[Q_JOVER * kSlots + o], ju = rec[Q_JUNDER * kSlots + o], vm = rec[Q_VMIN * kSlots + o];
        if (c > crossv) crossv = c;
        if (ao > aover) aover = ao;
        if (au > aunder) aunder = au;
        if (jo > jover) jover = jo;
        if (ju > junder) junder = ju;
        if (vm < vmin) vmin = vm;
        stops += reci[QI_STOPS * kSlots + o];
        lights += reci[QI_LIGHTS * kSlots + o];
        red += reci[QI_RED * kSlots + o];
        redposs += reci[QI_REDPOSS * kSlots + o];
        const int f = reci[QI_REDFIRST * kSlots + o];
        if (redfirst < 0) redfirst = f;
        comfort += reci[QI_COMFORT * kSlots + o];
    }
    double* out = rkpi + b;
    out[(size_t)EEPACC_RKPI_VLIM_EXCESS_MAX * B] = ex[0];
    out[(size_t)EEPACC_RKPI_VLIM_EXCESS_INDEX * B] = (double)index;
    out[(size_t)EEPACC_RKPI_VLIM_VIOL_STEPS * B] = (double)viol[0];
    out[(size_t)EEPACC_RKPI_VCURV_EXCESS_MAX * B] = ex[1];
    out[(size_t)EEPACC_RKPI_VCURV_VIOL_STEPS * B] = (double)viol[1];
    out[(size_t)EEPACC_RKPI_VSTOP_EXCESS_MAX * B] = ex[2];
    out[(size_t)EEPACC_RKPI_VSTOP_VIOL_STEPS * B] = (double)viol[2];
    out[(size_t)EEPACC_RKPI_VTL_EXCESS_MAX * B] = ex[3];
    out[(size_t)EEPACC_RKPI_VTL_VIOL_STEPS * B] = (double)viol[3];
    out[(size_t)EEPACC_RKPI_STOPS_PASSED * B] = (double)stops;
    out[(size_t)EEPACC_RKPI_STOP_CROSS_V_MAX * B] = crossv;
    out[(size_t)EEPACC_RKPI_TL_PASSED * B] = (double)lights;
    out[(size_t)EEPACC_RKPI_RED_CROSSINGS * B] = (double)red;
    out[(size_t)EEPACC_RKPI_RED_CROSSINGS_POSSIBLE * B] = (double)redposs;
    out[(size_t)EEPACC_RKPI_RED_CROSS_FIRST_INDEX * B] = (double)redfirst;
    out[(size_t)EEPACC_RKPI_A_OVER_MAX * B] = aover;
    out[(size_t)EEPACC_RKPI_A_UNDER_MAX * B] = aunder;
    out[(size_t)EEPACC_RKPI_J_OVER_MAX * B] = jover;
    out[(size_t)EEPACC_RKPI_J_UNDER_MAX * B] = junder;
    out[(size_t)EEPACC_RKPI_COMFORT_VIOL_STEPS * B] = (double)comfort;
    out[(size_t)EEPACC_RKPI_V_MIN * B] = vmin;
}

hipError_t launch_route_kpis(const RouteCfg* dR, const int32_t* class_of, int B, int n_steps, double t_start, double v_tol,
                             double a_tol, double j_tol, const double* traj, double* rkpi, double* limits, hipStream_t stream) {
    // 124 KiB: above the 64 KiB a kernel gets unasked; set per launch, since the attribute belongs to the current device
    const void* fn = class_of ? reinterpret_cast<const void*>(k_route_kpis<true>) : reinterpret_cast<const void*>(k_route_kpis<false>);
    const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kRouteLdsBytes);
    if (e != hipSuccess) return e;
    const int Ls = kpi_slice_len(n_steps);
    const dim3 grid((B + 63) / 64), block(64 * kKpiWaves);
    if (class_of)
        hipLaunchKernelGGL(k_route_kpis<true>, grid, block, kRouteLdsBytes, stream, dR, class_of, B, n_steps, Ls, t_start, v_tol, a_tol,
                           j_tol, traj, rkpi, limits);
    else
        hipLaunchKernelGGL(k_route_kpis<false>, grid, block, kRouteLdsBytes, stream, dR, class_of, B, n_steps, Ls, t_start, v_tol, a_tol,
                           j_tol, traj, rkpi, limits);
    return hipGetLastError();
}

}  // namespace eepacc
