// halfwave_harness.hip -- test-only device harness for the functions that put both 32-lane halves of a wave to work at
// NS = 32: scan_excl_half (eepacc_wave.h), he_sub_outer_halves and he_mul_halves (eepacc_schur.h) and the four-column
// build of S = C He C' (eepacc_ab_cols.h).  The two-column loop that rebuild_and_factor ran before is kept here as the
// reference of the four-column build.
//
// Same conventions as linalg_harness.hip: one problem per wave, 1..4 waves per block, operands staged into LDS, scratch
// filled with NaN before the call, extern "C" entry points that take host pointers and return 0, 1 (bad argument) or
// 1000 + hipError_t.  Built into its own shared object by tests/halfwave_harness.py.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "eepacc_wave.h"
#include "eepacc_units.h"
#include "eepacc_schur.h"
#include "eepacc_ab_cols.h"

using namespace eepacc;
using namespace eepacc::wv;

namespace {

constexpr int NS = 32, MMAX = 34, PS = MMAX * (MMAX + 1) / 2;

__device__ __forceinline__ int problem_id() { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
__device__ __forceinline__ double poison() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---------------------------------------------------------------------------------------------- scan_excl_half
__global__ void k_scan_half(const double* x, double* out, int nprob) {
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    out[q * 64 + lane] = scan_excl_half(x[q * 64 + lane]);
}

// ---------------------------------------------------------------------------------------------- He
enum { HW_MUL, HW_SUB_OUTER, HW_SUB_OUTER_REF };

// Hin [nprob][NS * NS], y0 / y1 [nprob][NS], N [nprob]; o0 [nprob][64] (product), Hout [nprob][NS * NS] (update).
// HW_SUB_OUTER: y0 = yv, y1 = the scaled second factor, read from LDS at l & 31 as he_rank1 reads it.  HW_SUB_OUTER_REF:
// the one-lane-per-column he_sub_outer on the same operands.
template <int OP>
__global__ void k_he(const double* Hin, const double* y0, const double* y1, const int* N, double* o0, double* Hout,
                     int nprob) {
    extern __shared__ double smem[];
    constexpr int HS = NS * NS, WS = HS + 2 * NS;
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    double* Hs = smem + (threadIdx.x >> 6) * WS;
    double* ya = Hs + HS;
    double* yb = ya + NS;
    for (int e = lane; e < HS; e += 64) Hs[e] = Hin[(size_t)q * HS + e];
    if (lane < NS) { ya[lane] = y0[q * NS + lane]; yb[lane] = y1[q * NS + lane]; }
    WSYNC();
    if constexpr (OP == HW_MUL) {
        o0[q * 64 + lane] = he_mul_halves<NS>(Hs, ya, N[q], lane);
    } else {
        if constexpr (OP == HW_SUB_OUTER) he_sub_outer_halves<NS>(Hs, ya, yb[lane & (NS - 1)], lane);
        else if (lane < NS) he_sub_outer<NS, false>(Hs, ya, yb[lane], lane);
        WSYNC();
        for (int e = lane; e < HS; e += 64) Hout[(size_t)q * HS + e] = Hs[e];
    }
}

// ---------------------------------------------------------------------------------------------- columns of S
// the fields ab_schur_columns4 and the two-column loop name, laid out like the solver's per-wave struct
struct ColMem {
    double P[PS];
    double yv[NS];
    double e_al[MMAX], e_be[MMAX], e_ga[MMAX], e_de[MMAX];
    double lam[MMAX], sv[MMAX], rv[MMAX];
    double tauv[NS + 1];
    int w_k[MMAX];
};

// normal_at() and hom_traj() of eepacc_ab_impl.inc for a lane that holds T_j and tau_{j+1} of its own stage
__device__ __forceinline__ double ref_normal_at(int j, int N, double T, double tau1, int kq, double al, double be, double ga,
                                                double de, double tau_kq) {
    double c = 0.0;
    if (j < N) {
        if (j < kq) c = T * (be + al * (0.5 * T + tau_kq - tau1));
        if (j == kq) c += ga;
        if (j == kq - 1) c += de;
    }
    return c;
}
__device__ __forceinline__ void ref_hom_traj(int lane, int N, double T, double x, double& sh, double& vh) {
    double xi = (lane < N) ? x : 0.0;
    vh = scan_excl(T * xi);
    double inc = (lane < N) ? (T * vh + 0.5 * T * T * xi) : 0.0;
    sh = scan_excl(inc);
}

// the S-column loop of rebuild_and_factor as it was before the four-column build (no move blocking)
__device__ __forceinline__ void ref_columns2(ColMem& M, const double* Hs, int m, int N, int lane, double T, double tau1) {
    const double* tauv = M.tauv;
    const int ki = lane < m ? M.w_k[lane] : 0;
    const int kim1 = ki > 0 ? ki - 1 : 0;
    const double eal = lane < m ? M.e_al[lane] : 0.0, ebe = lane < m ? M.e_be[lane] : 0.0;
    const double ega = (lane < m && ki < N) ? M.e_ga[lane] : 0.0;
    const double ede = (lane < m && ki > 0 && ki <= N) ? M.e_de[lane] : 0.0;
    for (int j = 0; j < m; j += 2) {
        const bool two = j + 1 < m;
        const int j1 = two ? j + 1 : j;
        const int kj0 = M.w_k[j], kj1 = M.w_k[j1];
        const double c0 = ref_normal_at(lane, N, T, tau1, kj0, M.e_al[j], M.e_be[j], M.e_ga[j], M.e_de[j], tauv[kj0]);
        const double c1 = ref_normal_at(lane, N, T, tau1, kj1, M.e_al[j1], M.e_be[j1], M.e_ga[j1], M.e_de[j1], tauv[kj1]);
        if (lane < NS) { M.yv[lane] = c0; M.lam[lane] = c1; }
        WSYNC();
        double u0, u1;
        he_mul2<NS, false>(Hs, M.yv, M.lam, N, lane, u0, u1);
        WSYNC();
        double su0, vu0, su1, vu1;
        ref_hom_traj(lane, N, T, u0, su0, vu0);
        ref_hom_traj(lane, N, T, u1, su1, vu1);
        const double sx = eal * __shfl(su0, ki, 64) + ebe * __shfl(vu0, ki, 64) + ega * __shfl(u0, ki, 64) + ede * __shfl(u0, kim1, 64);
        const double sy = eal * __shfl(su1, ki, 64) + ebe * __shfl(vu1, ki, 64) + ega * __shfl(u1, ki, 64) + ede * __shfl(u1, kim1, 64);
        if (lane >= j && lane < m) M.P[pidx(lane, j)] = sx;
        if (two && lane >= j + 1 && lane < m) M.P[pidx(lane, j + 1)] = sy;
    }
    WSYNC();
}

// He [nprob][NS * NS], Tvec [nprob][NS], tau [nprob][NS + 1], rows [nprob][4][MMAX] (e_al | e_be | e_ga | e_de),
// w_k [nprob][MMAX], m / N [nprob]; P [nprob][PS].  FOUR = 0: the two-column reference loop, 1: ab_schur_columns4.
template <int FOUR>
__global__ void k_columns(const double* He, const double* Tvec, const double* tau, const double* rows, const int* w_k,
                          const int* m_in, const int* N_in, double* P, int nprob) {
    extern __shared__ double smem[];
    constexpr int HS = NS * NS;
    constexpr size_t WB = sizeof(ColMem) + sizeof(double) * HS;
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    unsigned char* base = reinterpret_cast<unsigned char*>(smem) + WB * (threadIdx.x >> 6);
    ColMem& M = *reinterpret_cast<ColMem*>(base);
    double* Hs = reinterpret_cast<double*>(base + sizeof(ColMem));
    const int m = m_in[q], N = N_in[q];
    for (int e = lane; e < HS; e += 64) Hs[e] = He[(size_t)q * HS + e];
    for (int e = lane; e < PS; e += 64) M.P[e] = poison();
    for (int e = lane; e < NS + 1; e += 64) M.tauv[e] = tau[q * (NS + 1) + e];
    if (lane < NS) M.yv[lane] = poison();
    for (int e = lane; e < MMAX; e += 64) {
        M.e_al[e] = rows[(q * 4 + 0) * MMAX + e]; M.e_be[e] = rows[(q * 4 + 1) * MMAX + e];
        M.e_ga[e] = rows[(q * 4 + 2) * MMAX + e]; M.e_de[e] = rows[(q * 4 + 3) * MMAX + e];
        M.w_k[e] = w_k[q * MMAX + e];
        M.lam[e] = poison(); M.sv[e] = poison(); M.rv[e] = poison();
    }
    WSYNC();
    // the lane's registers as ab_step sets them: T_j (zero beyond the horizon) and tau_{j+1}
    const int kk = lane <= N ? lane : N;
    const double T = lane < N ? Tvec[q * NS + lane] : 0.0;
    const double tau1 = M.tauv[kk + (lane < N ? 1 : 0)];
    if constexpr (FOUR) {
        ab_schur_columns4<NS>(M, Hs, M.tauv, m, N, lane, half_lo(T), half_lo(tau1), [](double x) { return x; },
                              [](double x) { return x; });
    } else {
        ref_columns2(M, Hs, m, N, lane, T, tau1);
    }
    for (int e = lane; e < PS; e += 64) P[(size_t)q * PS + e] = M.P[e];
}

// ---------------------------------------------------------------------------------------------- host side
#define CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return 1000 + (int)e_; } while (0)

struct Dev {                     // a device copy of a host array (zero filled without one)
    void* d = nullptr;
    size_t bytes;
    hipError_t err;
    Dev(const void* h, size_t n) : bytes(n) {
        err = hipMalloc(&d, n ? n : 1);
        if (err != hipSuccess) { d = nullptr; return; }
        err = h ? hipMemcpy(d, h, n, hipMemcpyHostToDevice) : hipMemset(d, 0, n);
    }
    ~Dev() { if (d) (void)hipFree(d); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    hipError_t get(void* h) const { return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost); }
    template <class T> T* as() const { return static_cast<T*>(d); }
};

bool bad_shape(int nprob, int wpb) { return nprob < 1 || nprob > 4096 || wpb < 1 || wpb > 4; }
int grid_of(int nprob, int wpb) { return (nprob + wpb - 1) / wpb; }

template <class K>
hipError_t allow_smem(K kernel, size_t bytes) {
    return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}
int finish() {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return 0;
}

template <int OP>
int run_he(const double* H, const double* y0, const double* y1, const int* N, double* o0, double* Hout, int nprob, int wpb) {
    constexpr int HS = NS * NS;
    Dev dH(H, sizeof(double) * HS * nprob), d0(y0, sizeof(double) * NS * nprob), d1(y1, sizeof(double) * NS * nprob);
    Dev dN(N, sizeof(int) * nprob), a(nullptr, sizeof(double) * 64 * nprob), dO(nullptr, sizeof(double) * HS * nprob);
    CK(dH.err); CK(d0.err); CK(d1.err); CK(dN.err); CK(a.err); CK(dO.err);
    const size_t smem = sizeof(double) * (HS + 2 * NS) * wpb;
    CK(allow_smem(k_he<OP>, smem));
    hipLaunchKernelGGL(k_he<OP>, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0, dH.as<double>(), d0.as<double>(),
                       d1.as<double>(), dN.as<int>(), a.as<double>(), dO.as<double>(), nprob);
    if (int rc = finish()) return rc;
    if (o0) CK(a.get(o0));
    if (Hout) CK(dO.get(Hout));
    return 0;
}

template <int FOUR>
int run_columns(const double* He, const double* Tvec, const double* tau, const double* rows, const int* w_k, const int* m,
                const int* N, double* P, int nprob, int wpb) {
    Dev dH(He, sizeof(double) * NS * NS * nprob), dT(Tvec, sizeof(double) * NS * nprob);
    Dev dt(tau, sizeof(double) * (NS + 1) * nprob), dr(rows, sizeof(double) * 4 * MMAX * nprob);
    Dev dw(w_k, sizeof(int) * MMAX * nprob), dm(m, sizeof(int) * nprob), dN(N, sizeof(int) * nprob);
    Dev dP(nullptr, sizeof(double) * PS * nprob);
    CK(dH.err); CK(dT.err); CK(dt.err); CK(dr.err); CK(dw.err); CK(dm.err); CK(dN.err); CK(dP.err);
    const size_t smem = (sizeof(ColMem) + sizeof(double) * NS * NS) * wpb;
    CK(allow_smem(k_columns<FOUR>, smem));
    hipLaunchKernelGGL(k_columns<FOUR>, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0, dH.as<double>(), dT.as<double>(),
                       dt.as<double>(), dr.as<double>(), dw.as<int>(), dm.as<int>(), dN.as<int>(), dP.as<double>(), nprob);
    if (int rc = finish()) return rc;
    CK(dP.get(P));
    return 0;
}

}  // namespace

extern "C" {

// x, out [nprob][64]
int hw_scan_excl_half(const double* x, double* out, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    Dev dx(x, sizeof(double) * 64 * nprob), dout(nullptr, sizeof(double) * 64 * nprob);
    CK(dx.err); CK(dout.err);
    hipLaunchKernelGGL(k_scan_half, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), 0, 0, dx.as<double>(), dout.as<double>(), nprob);
    if (int rc = finish()) return rc;
    CK(dout.get(out));
    return 0;
}

// op: 0 he_mul_halves (o0), 1 he_sub_outer_halves (Hout), 2 he_sub_outer (Hout); full layout, NS = 32; layouts as at k_he
int hw_he(int op, const double* H, const double* y0, const double* y1, const int* N, double* o0, double* Hout, int nprob,
          int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    for (int q = 0; q < nprob; ++q) if (N[q] < 0 || N[q] > NS) return 1;
    if (op == HW_MUL) return run_he<HW_MUL>(H, y0, y1, N, o0, Hout, nprob, wpb);
    if (op == HW_SUB_OUTER) return run_he<HW_SUB_OUTER>(H, y0, y1, N, o0, Hout, nprob, wpb);
    if (op == HW_SUB_OUTER_REF) return run_he<HW_SUB_OUTER_REF>(H, y0, y1, N, o0, Hout, nprob, wpb);
    return 1;
}

// four = 0: the two-column reference loop, 1: ab_schur_columns4; NS = 32, MMAX = 34; layouts as at k_columns
int hw_columns(int four, const double* He, const double* Tvec, const double* tau, const double* rows, const int* w_k,
               const int* m, const int* N, double* P, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    for (int q = 0; q < nprob; ++q) {            // every index the kernels use stays inside the tables
        if (N[q] < 1 || N[q] > NS || m[q] < 1 || m[q] > MMAX) return 1;
        for (int i = 0; i < m[q]; ++i) if (w_k[q * MMAX + i] < 0 || w_k[q * MMAX + i] > N[q]) return 1;
    }
    if (four == 0) return run_columns<0>(He, Tvec, tau, rows, w_k, m, N, P, nprob, wpb);
    if (four == 1) return run_columns<1>(He, Tvec, tau, rows, w_k, m, N, P, nprob, wpb);
    return 1;
}

}  // extern "C"
