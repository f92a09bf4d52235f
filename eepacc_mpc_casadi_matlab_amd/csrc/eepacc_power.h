// eepacc_power.h -- the fifth-order battery-power surface P(Fm, rpm) of ABO/RunOpt_ABMPC.m:343-349 as one device
// function (used by k_kpis, eepacc_kpis.hip), with its rounding written down: the monomials are plain products, and every
// term enters the sum through one fused multiply-add, acc = fma(c, m, acc) or, for a term c * m1 * m2, fma(c * m1, m2, acc),
// in the order of the reference's coefficient list.  That is the instruction stream the compiler makes of k_postprocess's
// expression (eepacc_kernels.hip; profiles/kpis_codegen.txt lists it), so the two kernels give the same P bit for bit, and
// report.power_surface states the same roundings in numpy.  Contraction is off here: nothing else is fused or left to the
// compiler's choice.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

namespace eepacc {

constexpr double kRpmPerRadS = 30.0 / 3.14159265358979323846;

// x = Fm [N], y = motor speed [rpm] = kRpmPerRadS * v * phi
__device__ __forceinline__ double power_surface(const double* __restrict__ bb, double x, double y) {
#pragma clang fp contract(off)
    const double x2 = x * x, x3 = x2 * x, x4 = x3 * x, x5 = x4 * x;
    const double y2 = y * y, y3 = y2 * y, y4 = y3 * y, y5 = y4 * y;
    double p = fma(bb[1], x, bb[0]);
    p = fma(bb[2], y, p);
    p = fma(bb[3], x2, p);
    p = fma(bb[4] * x, y, p);
    p = fma(bb[5], y2, p);
    p = fma(bb[6], x3, p);
    p = fma(bb[7] * x2, y, p);
    p = fma(bb[8] * x, y2, p);
    p = fma(bb[9], y3, p);
    p = fma(bb[10], x4, p);
    p = fma(bb[11] * x3, y, p);
    p = fma(bb[12] * x2, y2, p);
    p = fma(bb[13] * x, y3, p);
    p = fma(bb[14], y4, p);
    p = fma(bb[15], x5, p);
    p = fma(bb[16] * x4, y, p);
    p = fma(bb[17] * x3, y2, p);
    p = fma(bb[18] * x2, y3, p);
    p = fma(bb[19] * x, y4, p);
    p = fma(bb[20], y5, p);
    return p;
}

}  // namespace eepacc
