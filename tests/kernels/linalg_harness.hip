// linalg_harness.hip -- test-only device harness for the shared headers of the active-set kernels:
// eepacc_wave.h (DPP scans, wave sums, arg-max), eepacc_units.h (pidx, rc_table, shift_codes), eepacc_schur.h
// (products with He, its column update and inversion, the bordered update, downdate and inversion of P, multipliers)
// and eepacc_dual_step.h (scatter into the stage images, row value, step rates, refinement rounds, event codes, tolerance).
//
// One small kernel per primitive: operands are staged from global memory into LDS, the header function is called the way
// the solvers call it, the result is copied back.  A block has 1..4 waves and every wave works on its own problem, so a
// launch also shows whether waves disturb each other and whether the per-workgroup rc_table is shared correctly.  LDS
// scratch is filled with NaN before a call: a primitive that reads scratch it has not written shows up in the result.
//
// The extern "C" entry points take host pointers, do their own allocation and copies and return 0 or a non-zero code
// (1: bad argument, 1000 + hipError_t: a HIP call failed).  This file is built into its own shared object
// (tests/linalg_harness.py), never into libeepacc.so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "eepacc_wave.h"
#include "eepacc_units.h"
#include "eepacc_schur.h"
#include "eepacc_dual_step.h"

using namespace eepacc;
using namespace eepacc::wv;

namespace {

__device__ __forceinline__ int problem_id() { return blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); }
__device__ __forceinline__ double poison() { return __longlong_as_double(0x7ff8000000000000ll); }

// ---------------------------------------------------------------------------------------------- eepacc_wave.h
enum { W_SCAN_INCL, W_SCAN_EXCL, W_WAVE_SUM, W_SCAN_PROD_EXCL, W_LANE_PREV, W_LANE_NEXT, W_WAVE_MAX, W_ARGMAX, W_ARGMIN,
       W_BCAST, W_BCAST_I, W_NUM };

template <int OP>
__global__ void k_wave(const double* x, const int* pi, const int* src, double* od, int* oi, int nprob) {
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    double v = x[q * 64 + lane];
    int p = pi[q * 64 + lane];
    if constexpr (OP == W_SCAN_INCL) v = scan_incl(v);
    if constexpr (OP == W_SCAN_EXCL) v = scan_excl(v);
    if constexpr (OP == W_WAVE_SUM) v = wave_sum(v);
    if constexpr (OP == W_SCAN_PROD_EXCL) v = scan_prod_excl(v);
    if constexpr (OP == W_LANE_PREV) v = lane_prev(v);
    if constexpr (OP == W_LANE_NEXT) v = lane_next(v);
    if constexpr (OP == W_WAVE_MAX) v = wave_max(v);
    if constexpr (OP == W_ARGMAX) wave_argmax(v, p);
    if constexpr (OP == W_ARGMIN) wave_argmin(v, p);
    if constexpr (OP == W_BCAST) v = bcast(v, src[q]);
    if constexpr (OP == W_BCAST_I) p = bcast_i(p, src[q]);
    od[q * 64 + lane] = v;
    oi[q * 64 + lane] = p;
}

// ---------------------------------------------------------------------------------------------- eepacc_units.h
__global__ void k_pidx(int n, int* out) {
    for (int e = threadIdx.x; e < n * n; e += blockDim.x) out[e] = pidx(e / n, e % n);
}

// every wave of every block copies the workgroup's table out
template <int MMAX>
__global__ void k_rc_table(unsigned short* out) {
    rc_table_init<MMAX>();
    const unsigned short* rc = rc_table<MMAX>();
    constexpr int PS = MMAX * (MMAX + 1) / 2;
    for (int e = lane_id(); e < PS; e += 64) out[(size_t)problem_id() * PS + e] = rc[e];
}

__global__ void k_shift_codes(const unsigned long long* code, const int* N, unsigned long long* out, int nprob) {
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    out[q * 64 + lane] = shift_codes(code[q * 64 + lane], N[q]);
}

// ---------------------------------------------------------------------------------------------- He
template <int NS, bool PACKED>
constexpr int he_size() { return PACKED ? NS * (NS + 1) / 2 : NS * NS; }

enum { HE_MUL, HE_MUL2, HE_SUB_OUTER };

// Hin [nprob][he_size], y0 / y1 [nprob][NS], N [nprob]; o0 / o1 [nprob][64] (products), Hout [nprob][he_size] (update).
// HE_SUB_OUTER: y0 = yv, y1[lane] = this lane's yj.
template <int NS, bool PACKED, int OP>
__global__ void k_he(const double* Hin, const double* y0, const double* y1, const int* N, double* o0, double* o1,
                     double* Hout, int nprob) {
    extern __shared__ double smem[];
    constexpr int HS = he_size<NS, PACKED>(), WS = HS + 2 * NS;
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    double* Hs = smem + (threadIdx.x >> 6) * WS;
    double* ya = Hs + HS;
    double* yb = ya + NS;
    for (int e = lane; e < HS; e += 64) Hs[e] = Hin[(size_t)q * HS + e];
    if (lane < NS) { ya[lane] = y0[q * NS + lane]; yb[lane] = y1[q * NS + lane]; }
    WSYNC();
    if constexpr (OP == HE_MUL) {
        o0[q * 64 + lane] = he_mul<NS, PACKED>(Hs, ya, N[q], lane);
    } else if constexpr (OP == HE_MUL2) {
        double a, b;
        he_mul2<NS, PACKED>(Hs, ya, yb, N[q], lane, a, b);
        o0[q * 64 + lane] = a;
        o1[q * 64 + lane] = b;
    } else {
        const double yj = lane < NS ? yb[lane] : 0.0;
        WSYNC();
        if (lane < NS) he_sub_outer<NS, PACKED>(Hs, ya, yj, lane);
        WSYNC();
        for (int e = lane; e < HS; e += 64) Hout[(size_t)q * HS + e] = Hs[e];
    }
}

// H [nprob][NS * NS] in place, ret [nprob][64] (every lane's return value)
template <int NS>
__global__ void k_he_invert(double* H, const int* N, int* ret, int nprob) {
    extern __shared__ double smem[];
    constexpr int HS = NS * NS, WS = HS + NS;
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    double* Hs = smem + (threadIdx.x >> 6) * WS;
    double* colk = Hs + HS;
    for (int e = lane; e < HS; e += 64) Hs[e] = H[(size_t)q * HS + e];
    if (lane < NS) colk[lane] = poison();
    WSYNC();
    ret[q * 64 + lane] = he_invert_full<NS>(Hs, colk, N[q], lane);
    WSYNC();
    for (int e = lane; e < HS; e += 64) H[(size_t)q * HS + e] = Hs[e];
}

// ---------------------------------------------------------------------------------------------- P
enum { S_INVERT, S_INSERT, S_REMOVE, S_CHAIN };
constexpr int kChainOps = 6;      // the longest run of updates solve_qp allows before it rebuilds

// P [nprob][PS] in place (PS = MMAX (MMAX + 1) / 2), m [nprob] (S_INSERT: new size, S_REMOVE: old size, S_CHAIN: start),
// ret [nprob][64].  S_INVERT: sv_out [nprob][MMAX] receives sv.  S_INSERT: vec [nprob][MMAX] = rv, pos [nprob], piv
// [nprob] = iz.  S_REMOVE: pos [nprob].  S_CHAIN: schur_invert, then kChainOps updates: kind [nprob][6] (1 insert, 2
// remove), pos [nprob][6], and for an insert vec [nprob][6][MMAX] = the column sv = C u of the new row against the
// current list and piv [nprob][6] = c'u; rv = P sv and the pivot zz = c'u - sv'rv are computed as solve_qp computes
// them.  m_out [nprob] receives the final size.
template <int MMAX, int OP>
__global__ void k_schur(double* P, const int* m_in, const int* kind, const int* pos, const double* vec, const double* piv,
                        int* ret, double* sv_out, int* m_out, int nprob) {
    extern __shared__ double smem[];
    constexpr int PS = MMAX * (MMAX + 1) / 2, WS = PS + 3 * MMAX;
    rc_table_init<MMAX>();
    const unsigned short* rc = rc_table<MMAX>();
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    double* Ps = smem + (threadIdx.x >> 6) * WS;
    double* sv = Ps + PS;
    double* colk = sv + MMAX;
    double* rv = colk + MMAX;
    for (int e = lane; e < PS; e += 64) Ps[e] = P[(size_t)q * PS + e];
    for (int e = lane; e < 3 * MMAX; e += 64) sv[e] = poison();
    WSYNC();
    int m = m_in[q], r = 0;
    if constexpr (OP == S_INVERT) {
        r = schur_invert(Ps, sv, colk, rc, m, lane);
        for (int e = lane; e < MMAX; e += 64) sv_out[q * MMAX + e] = sv[e];
    } else if constexpr (OP == S_INSERT) {
        for (int e = lane; e < MMAX; e += 64) rv[e] = vec[q * MMAX + e];
        WSYNC();
        schur_insert(Ps, rv, rc, m, pos[q], piv[q], lane);
    } else if constexpr (OP == S_REMOVE) {
        schur_remove(Ps, colk, rc, m, m - 1, pos[q], lane);
        m -= 1;
    } else {
        r = schur_invert(Ps, sv, colk, rc, m, lane);
        for (int s = 0; s < kChainOps && r == 0; ++s) {
            const int k = kind[q * kChainOps + s], p = pos[q * kChainOps + s];
            if (k == 1) {
                for (int e = lane; e < MMAX; e += 64) sv[e] = vec[((size_t)q * kChainOps + s) * MMAX + e];
                WSYNC();
                double sr = 0.0;
                if (lane < m) {
                    double a = 0.0;
                    for (int j = 0; j < m; ++j) a = fma(Ps[pidx(lane, j)], sv[j], a);
                    rv[lane] = a;
                    sr = sv[lane] * a;
                }
                WSYNC();
                sr = wave_sum(sr);
                const double zz = piv[q * kChainOps + s] - sr;
                m += 1;
                schur_insert(Ps, rv, rc, m, p, 1.0 / zz, lane);
            } else if (k == 2) {
                schur_remove(Ps, colk, rc, m, m - 1, p, lane);
                m -= 1;
            }
        }
    }
    WSYNC();
    ret[q * 64 + lane] = r;
    if (lane == 0) m_out[q] = m;
    for (int e = lane; e < PS; e += 64) P[(size_t)q * PS + e] = Ps[e];
}

// ---------------------------------------------------------------------------------------------- multipliers
// the fields solve_multipliers / rows_dot_img name, laid out like the solvers' per-wave structs
template <int MMAX, int NS>
struct MulMem {
    double P[MMAX * (MMAX + 1) / 2];
    double ub[NS + 1], sub[NS + 1], vub[NS + 1];
    double e_al[MMAX], e_be[MMAX], e_ga[MMAX], e_de[MMAX], e_d[MMAX];
    double lam[MMAX], sv[MMAX];
    int w_k[MMAX];
};

// P [nprob][PS], img [nprob][3][NS + 1] (ub | sub | vub), rows [nprob][5][MMAX] (e_al | e_be | e_ga | e_de | e_d),
// w_k [nprob][MMAX], m / N [nprob]; lam, sv [nprob][MMAX]
template <int MMAX, int NS>
__global__ void k_multipliers(const double* P, const double* img, const double* rows, const int* w_k, const int* m,
                              const int* N, double* lam, double* sv, int nprob) {
    extern __shared__ double smem[];
    using Mem = MulMem<MMAX, NS>;
    constexpr int PS = MMAX * (MMAX + 1) / 2;
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    Mem& M = *reinterpret_cast<Mem*>(reinterpret_cast<unsigned char*>(smem) + sizeof(Mem) * (threadIdx.x >> 6));
    for (int e = lane; e < PS; e += 64) M.P[e] = P[(size_t)q * PS + e];
    for (int e = lane; e < NS + 1; e += 64) {
        M.ub[e] = img[(q * 3 + 0) * (NS + 1) + e];
        M.sub[e] = img[(q * 3 + 1) * (NS + 1) + e];
        M.vub[e] = img[(q * 3 + 2) * (NS + 1) + e];
    }
    for (int e = lane; e < MMAX; e += 64) {
        M.e_al[e] = rows[(q * 5 + 0) * MMAX + e]; M.e_be[e] = rows[(q * 5 + 1) * MMAX + e];
        M.e_ga[e] = rows[(q * 5 + 2) * MMAX + e]; M.e_de[e] = rows[(q * 5 + 3) * MMAX + e];
        M.e_d[e] = rows[(q * 5 + 4) * MMAX + e];
        M.w_k[e] = w_k[q * MMAX + e];
        M.lam[e] = poison(); M.sv[e] = poison();
    }
    WSYNC();
    solve_multipliers(M, m[q], lane, N[q]);
    for (int e = lane; e < MMAX; e += 64) { lam[q * MMAX + e] = M.lam[e]; sv[q * MMAX + e] = M.sv[e]; }
}

// ---------------------------------------------------------------------------------------------- eepacc_dual_step.h
// the fields the routines of eepacc_dual_step.h name, laid out like the solvers' per-wave structs; map: the affine map
// lam -> (av, shv, vhv) of the harness's recompute (rows s0 | cs | v0 | cv | a0 | ca | cb, see D_REFINE)
template <int MMAX, int NS>
struct DualMem {
    double P[MMAX * (MMAX + 1) / 2];
    double av[NS], shv[NS + 1], vhv[NS + 1];
    double ub[NS + 1], sub[NS + 1], vub[NS + 1];
    double ws[NS + 1], wv[NS + 1], wa[NS + 1];
    double e_al[MMAX], e_be[MMAX], e_ga[MMAX], e_de[MMAX], e_d[MMAX];
    double lam[MMAX], sv[MMAX], rv[MMAX];
    double map[7][NS + 1];
    int w_k[MMAX];
};

enum { D_SCATTER_ROWS, D_SCATTER_ROW, D_ROW_VALUE, D_STEP_RATES, D_REFINE, D_NUM };
enum { IP_M, IP_N, IP_KQ, IP_X, IP_NUM };            // ipar: m, N, kq, (scatter_rows: 0 vec = lam, 1 vec = rv; refine: max_rounds)
enum { DP_SCALE, DP_AL, DP_BE, DP_GA, DP_DE, DP_D, DP_NUM };      // par: sign / scale / res_tol, then the row

// mem [nprob] DualMem in and out, par [nprob][DP_NUM], ipar [nprob][IP_NUM]; od, oi [nprob][64]: every lane's return
// value and (D_REFINE) the number of calls of recompute it saw.
// D_REFINE: one row per stage, w_k[i] = i; recompute is  shv_k = s0_k + cs_k lam_k,  vhv_k = v0_k + cv_k lam_k,
// av_k = a0_k + ca_k lam_k + cb_k lam_{k+1}  (lam_i = 0 for i >= m).
template <int MMAX, int NS, int OP>
__global__ void k_dual(DualMem<MMAX, NS>* mem, const double* par, const int* ipar, double* od, int* oi, int nprob) {
    extern __shared__ double smem[];
    using Mem = DualMem<MMAX, NS>;
    static_assert(sizeof(Mem) % sizeof(int) == 0, "copied as ints");
    constexpr int WORDS = sizeof(Mem) / sizeof(int);
    const int lane = lane_id(), q = problem_id();
    if (q >= nprob) return;
    Mem& M = *reinterpret_cast<Mem*>(reinterpret_cast<unsigned char*>(smem) + sizeof(Mem) * (threadIdx.x >> 6));
    for (int e = lane; e < WORDS; e += 64) reinterpret_cast<int*>(&M)[e] = reinterpret_cast<const int*>(mem + q)[e];
    WSYNC();
    const int m = ipar[q * IP_NUM + IP_M], N = ipar[q * IP_NUM + IP_N], kq = ipar[q * IP_NUM + IP_KQ], x = ipar[q * IP_NUM + IP_X];
    const double* p = par + q * DP_NUM;
    double r = 0.0;
    int calls = 0;
    if constexpr (OP == D_SCATTER_ROWS) {
        scatter_rows(M, m, N, lane, x ? M.rv : M.lam, p[DP_SCALE]);
    } else if constexpr (OP == D_SCATTER_ROW) {
        if (lane == 0) scatter_row(M, kq, N, p[DP_SCALE], p[DP_AL], p[DP_BE], p[DP_GA], p[DP_DE]);
    } else if constexpr (OP == D_ROW_VALUE) {
        const Incoming row{kq, 0, 0, 0, false, p[DP_AL], p[DP_BE], p[DP_GA], p[DP_DE], p[DP_D]};
        r = row_value(row, kq, N, M.av, M.shv, M.vhv, row.d);
    } else if constexpr (OP == D_STEP_RATES) {
        if (m > 0) r = step_rates(M, m, N, lane);       // as the solvers call it
    } else {
        r = refine_rounds(M, m, N, lane, x, p[DP_SCALE], [&] {
            ++calls;
            const double l0 = lane < m ? M.lam[lane] : 0.0, l1 = lane + 1 < m ? M.lam[lane + 1] : 0.0;
            WSYNC();
            if (lane <= N) { M.shv[lane] = M.map[0][lane] + M.map[1][lane] * l0; M.vhv[lane] = M.map[2][lane] + M.map[3][lane] * l0; }
            if (lane < N) M.av[lane] = M.map[4][lane] + M.map[5][lane] * l0 + M.map[6][lane] * l1;
            WSYNC();
        });
    }
    WSYNC();
    od[q * 64 + lane] = r;
    oi[q * 64 + lane] = calls;
    for (int e = lane; e < WORDS; e += 64) reinterpret_cast<int*>(mem + q)[e] = reinterpret_cast<const int*>(&M)[e];
}

// in [n][3]: EvCode::pack arguments (kind, lane, t), or viol_tolerance arguments (iters, N) with tol0 [n];
// out [n][4] = the code and its three parts; tol [n]
__global__ void k_event_code(const int* in, int* out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int ev = EvCode::pack(in[3 * i], in[3 * i + 1], in[3 * i + 2]);
    out[4 * i] = ev; out[4 * i + 1] = EvCode::kind(ev); out[4 * i + 2] = EvCode::lane(ev); out[4 * i + 3] = EvCode::type(ev);
}
__global__ void k_viol_tolerance(const double* tol0, const int* in, double* tol, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) tol[i] = viol_tolerance(tol0[i], in[3 * i], in[3 * i + 1]);
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
int run_wave(const Dev& x, const Dev& pi, const Dev& src, const Dev& od, const Dev& oi, int nprob, int wpb) {
    hipLaunchKernelGGL(k_wave<OP>, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), 0, 0, x.as<double>(), pi.as<int>(),
                       src.as<int>(), od.as<double>(), oi.as<int>(), nprob);
    return finish();
}

template <int NS, bool PACKED, int OP>
int run_he(const double* H, const double* y0, const double* y1, const int* N, double* o0, double* o1, double* Hout,
           int nprob, int wpb) {
    constexpr int HS = he_size<NS, PACKED>();
    Dev dH(H, sizeof(double) * HS * nprob), d0(y0, sizeof(double) * NS * nprob), d1(y1, sizeof(double) * NS * nprob);
    Dev dN(N, sizeof(int) * nprob), a(nullptr, sizeof(double) * 64 * nprob), b(nullptr, sizeof(double) * 64 * nprob);
    Dev dO(nullptr, sizeof(double) * HS * nprob);
    CK(dH.err); CK(d0.err); CK(d1.err); CK(dN.err); CK(a.err); CK(b.err); CK(dO.err);
    const size_t smem = sizeof(double) * (HS + 2 * NS) * wpb;
    CK(allow_smem(k_he<NS, PACKED, OP>, smem));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_he<NS, PACKED, OP>), dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0,
                       dH.as<double>(), d0.as<double>(), d1.as<double>(), dN.as<int>(), a.as<double>(), b.as<double>(),
                       dO.as<double>(), nprob);
    if (int rc = finish()) return rc;
    if (o0) CK(a.get(o0));
    if (o1) CK(b.get(o1));
    if (Hout) CK(dO.get(Hout));
    return 0;
}

template <int NS, bool PACKED>
int run_he_op(int op, const double* H, const double* y0, const double* y1, const int* N, double* o0, double* o1,
              double* Hout, int nprob, int wpb) {
    if (op == HE_MUL) return run_he<NS, PACKED, HE_MUL>(H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    if (op == HE_MUL2) return run_he<NS, PACKED, HE_MUL2>(H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    if (op == HE_SUB_OUTER) return run_he<NS, PACKED, HE_SUB_OUTER>(H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    return 1;
}

template <int NS>
int run_he_invert(double* H, const int* N, int* ret, int nprob, int wpb) {
    Dev dH(H, sizeof(double) * NS * NS * nprob), dN(N, sizeof(int) * nprob), dR(nullptr, sizeof(int) * 64 * nprob);
    CK(dH.err); CK(dN.err); CK(dR.err);
    const size_t smem = sizeof(double) * (NS * NS + NS) * wpb;
    CK(allow_smem(k_he_invert<NS>, smem));
    hipLaunchKernelGGL(k_he_invert<NS>, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0, dH.as<double>(), dN.as<int>(),
                       dR.as<int>(), nprob);
    if (int rc = finish()) return rc;
    CK(dH.get(H)); CK(dR.get(ret));
    return 0;
}

template <int MMAX, int OP>
int run_schur(double* P, const int* m, const int* kind, const int* pos, const double* vec, const double* piv, int* ret,
              double* sv, int* m_out, int nprob, int wpb) {
    constexpr int PS = MMAX * (MMAX + 1) / 2;
    const int per = OP == S_CHAIN ? kChainOps : 1;
    for (int q = 0; q < nprob; ++q) {                 // every index the kernel uses stays inside the tables
        const int lim = OP == S_REMOVE ? m[q] : (OP == S_INSERT ? m[q] : 0);
        if (m[q] < 1 || m[q] > schur_capacity<MMAX>()) return 1;      // the contract of eepacc_schur.h
        if ((OP == S_INSERT || OP == S_REMOVE) && (pos[q] < 0 || pos[q] >= lim)) return 1;
        if (OP == S_REMOVE && m[q] < 2) return 1;
        if (OP == S_CHAIN) {
            int mm = m[q];
            for (int s = 0; s < kChainOps; ++s) {
                const int k = kind[q * kChainOps + s], p = pos[q * kChainOps + s];
                if (k == 1) { if (mm + 1 > schur_capacity<MMAX>() || p < 0 || p > mm) return 1; ++mm; }
                else if (k == 2) { if (mm < 2 || p < 0 || p >= mm) return 1; --mm; }
                else if (k != 0) return 1;
            }
        }
    }
    Dev dP(P, sizeof(double) * PS * nprob), dm(m, sizeof(int) * nprob), dk(kind, sizeof(int) * per * nprob);
    Dev dp(pos, sizeof(int) * per * nprob), dv(vec, sizeof(double) * MMAX * per * nprob), dz(piv, sizeof(double) * per * nprob);
    Dev dR(nullptr, sizeof(int) * 64 * nprob), ds(nullptr, sizeof(double) * MMAX * nprob), dmo(nullptr, sizeof(int) * nprob);
    CK(dP.err); CK(dm.err); CK(dk.err); CK(dp.err); CK(dv.err); CK(dz.err); CK(dR.err); CK(ds.err); CK(dmo.err);
    const size_t smem = sizeof(double) * (PS + 3 * MMAX) * wpb;
    CK(allow_smem(k_schur<MMAX, OP>, smem));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_schur<MMAX, OP>), dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0,
                       dP.as<double>(), dm.as<int>(), dk.as<int>(), dp.as<int>(), dv.as<double>(), dz.as<double>(),
                       dR.as<int>(), ds.as<double>(), dmo.as<int>(), nprob);
    if (int rc = finish()) return rc;
    CK(dP.get(P)); CK(dR.get(ret));
    if (sv) CK(ds.get(sv));
    if (m_out) CK(dmo.get(m_out));
    return 0;
}

template <int MMAX>
int run_schur_op(int op, double* P, const int* m, const int* kind, const int* pos, const double* vec, const double* piv,
                 int* ret, double* sv, int* m_out, int nprob, int wpb) {
    if (op == S_INVERT) return run_schur<MMAX, S_INVERT>(P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    if (op == S_INSERT) return run_schur<MMAX, S_INSERT>(P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    if (op == S_REMOVE) return run_schur<MMAX, S_REMOVE>(P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    if (op == S_CHAIN) return run_schur<MMAX, S_CHAIN>(P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    return 1;
}

template <int MMAX, int NS>
int run_multipliers(const double* P, const double* img, const double* rows, const int* w_k, const int* m, const int* N,
                    double* lam, double* sv, int nprob, int wpb) {
    constexpr int PS = MMAX * (MMAX + 1) / 2;
    for (int q = 0; q < nprob; ++q) {
        if (m[q] < 1 || m[q] > schur_capacity<MMAX>() || N[q] < 1 || N[q] > NS) return 1;
        for (int i = 0; i < m[q]; ++i) if (w_k[q * MMAX + i] < 0 || w_k[q * MMAX + i] > N[q]) return 1;
    }
    Dev dP(P, sizeof(double) * PS * nprob), di(img, sizeof(double) * 3 * (NS + 1) * nprob);
    Dev dr(rows, sizeof(double) * 5 * MMAX * nprob), dw(w_k, sizeof(int) * MMAX * nprob), dm(m, sizeof(int) * nprob);
    Dev dN(N, sizeof(int) * nprob), dl(nullptr, sizeof(double) * MMAX * nprob), ds(nullptr, sizeof(double) * MMAX * nprob);
    CK(dP.err); CK(di.err); CK(dr.err); CK(dw.err); CK(dm.err); CK(dN.err); CK(dl.err); CK(ds.err);
    const size_t smem = sizeof(MulMem<MMAX, NS>) * wpb;
    CK(allow_smem(k_multipliers<MMAX, NS>, smem));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_multipliers<MMAX, NS>), dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0,
                       dP.as<double>(), di.as<double>(), dr.as<double>(), dw.as<int>(), dm.as<int>(), dN.as<int>(),
                       dl.as<double>(), ds.as<double>(), nprob);
    if (int rc = finish()) return rc;
    CK(dl.get(lam)); CK(ds.get(sv));
    return 0;
}

template <int MMAX, int NS, int OP>
int run_dual(void* mem, const double* par, const int* ipar, double* od, int* oi, int nprob, int wpb) {
    using Mem = DualMem<MMAX, NS>;
    const Mem* h = static_cast<const Mem*>(mem);
    for (int q = 0; q < nprob; ++q) {                 // every index the routines use stays inside the arrays
        const int m = ipar[q * IP_NUM + IP_M], N = ipar[q * IP_NUM + IP_N], kq = ipar[q * IP_NUM + IP_KQ], x = ipar[q * IP_NUM + IP_X];
        if (m < 0 || m > schur_capacity<MMAX>() || N < 1 || N > NS || kq < 0 || kq > N) return 1;
        for (int i = 0; i < m; ++i) if (h[q].w_k[i] < 0 || h[q].w_k[i] > N) return 1;
        if (OP == D_SCATTER_ROWS && x != 0 && x != 1) return 1;
        if (OP == D_REFINE) {
            if (x < 0 || x > 16 || m > N + 1) return 1;
            for (int i = 0; i < m; ++i) if (h[q].w_k[i] != i) return 1;
        }
    }
    Dev dM(mem, sizeof(Mem) * nprob), dp(par, sizeof(double) * DP_NUM * nprob), di(ipar, sizeof(int) * IP_NUM * nprob);
    Dev dod(nullptr, sizeof(double) * 64 * nprob), doi(nullptr, sizeof(int) * 64 * nprob);
    CK(dM.err); CK(dp.err); CK(di.err); CK(dod.err); CK(doi.err);
    const size_t smem = sizeof(Mem) * wpb;
    CK(allow_smem(k_dual<MMAX, NS, OP>, smem));
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_dual<MMAX, NS, OP>), dim3(grid_of(nprob, wpb)), dim3(64 * wpb), smem, 0,
                       dM.as<Mem>(), dp.as<double>(), di.as<int>(), dod.as<double>(), doi.as<int>(), nprob);
    if (int rc = finish()) return rc;
    CK(dM.get(mem)); CK(dod.get(od)); CK(doi.get(oi));
    return 0;
}

template <int MMAX, int NS>
int run_dual_op(int op, void* mem, const double* par, const int* ipar, double* od, int* oi, int nprob, int wpb) {
    if (op == D_SCATTER_ROWS) return run_dual<MMAX, NS, D_SCATTER_ROWS>(mem, par, ipar, od, oi, nprob, wpb);
    if (op == D_SCATTER_ROW) return run_dual<MMAX, NS, D_SCATTER_ROW>(mem, par, ipar, od, oi, nprob, wpb);
    if (op == D_ROW_VALUE) return run_dual<MMAX, NS, D_ROW_VALUE>(mem, par, ipar, od, oi, nprob, wpb);
    if (op == D_STEP_RATES) return run_dual<MMAX, NS, D_STEP_RATES>(mem, par, ipar, od, oi, nprob, wpb);
    if (op == D_REFINE) return run_dual<MMAX, NS, D_REFINE>(mem, par, ipar, od, oi, nprob, wpb);
    return 1;
}

}  // namespace

extern "C" {

// x, od [nprob][64] doubles; pi, oi [nprob][64] ints; src [nprob] (source lane of the broadcasts)
int lh_wave(int op, const double* x, const int* pi, const int* src, double* od, int* oi, int nprob, int wpb) {
    if (bad_shape(nprob, wpb) || op < 0 || op >= W_NUM) return 1;
    for (int q = 0; q < nprob; ++q) if (src[q] < 0 || src[q] > 63) return 1;
    Dev dx(x, sizeof(double) * 64 * nprob), dp(pi, sizeof(int) * 64 * nprob), ds(src, sizeof(int) * nprob);
    Dev dod(nullptr, sizeof(double) * 64 * nprob), doi(nullptr, sizeof(int) * 64 * nprob);
    CK(dx.err); CK(dp.err); CK(ds.err); CK(dod.err); CK(doi.err);
    int rc = 1;
    switch (op) {
    case W_SCAN_INCL: rc = run_wave<W_SCAN_INCL>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_SCAN_EXCL: rc = run_wave<W_SCAN_EXCL>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_WAVE_SUM: rc = run_wave<W_WAVE_SUM>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_SCAN_PROD_EXCL: rc = run_wave<W_SCAN_PROD_EXCL>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_LANE_PREV: rc = run_wave<W_LANE_PREV>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_LANE_NEXT: rc = run_wave<W_LANE_NEXT>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_WAVE_MAX: rc = run_wave<W_WAVE_MAX>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_ARGMAX: rc = run_wave<W_ARGMAX>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_ARGMIN: rc = run_wave<W_ARGMIN>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_BCAST: rc = run_wave<W_BCAST>(dx, dp, ds, dod, doi, nprob, wpb); break;
    case W_BCAST_I: rc = run_wave<W_BCAST_I>(dx, dp, ds, dod, doi, nprob, wpb); break;
    }
    if (rc) return rc;
    CK(dod.get(od)); CK(doi.get(oi));
    return 0;
}

// out [n][n] = pidx(i, j)
int lh_pidx(int n, int* out) {
    if (n < 1 || n > 256) return 1;
    Dev d(nullptr, sizeof(int) * n * n);
    CK(d.err);
    hipLaunchKernelGGL(k_pidx, dim3(1), dim3(256), 0, 0, n, d.as<int>());
    if (int rc = finish()) return rc;
    CK(d.get(out));
    return 0;
}

// out [nblocks * wpb][mmax (mmax + 1) / 2]: the table as every wave of every block sees it
int lh_rc_table(int mmax, unsigned short* out, int nblocks, int wpb) {
    if (bad_shape(nblocks, wpb)) return 1;
    if (mmax != 32 && mmax != 34 && mmax != 66) return 1;
    Dev d(nullptr, sizeof(unsigned short) * (mmax * (mmax + 1) / 2) * nblocks * wpb);
    CK(d.err);
    if (mmax == 32) hipLaunchKernelGGL(k_rc_table<32>, dim3(nblocks), dim3(64 * wpb), 0, 0, d.as<unsigned short>());
    if (mmax == 34) hipLaunchKernelGGL(k_rc_table<34>, dim3(nblocks), dim3(64 * wpb), 0, 0, d.as<unsigned short>());
    if (mmax == 66) hipLaunchKernelGGL(k_rc_table<66>, dim3(nblocks), dim3(64 * wpb), 0, 0, d.as<unsigned short>());
    if (int rc = finish()) return rc;
    CK(d.get(out));
    return 0;
}

// code, out [nprob][64]; N [nprob]
int lh_shift_codes(const unsigned long long* code, const int* N, unsigned long long* out, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    Dev dc(code, sizeof(unsigned long long) * 64 * nprob), dN(N, sizeof(int) * nprob);
    Dev dout(nullptr, sizeof(unsigned long long) * 64 * nprob);
    CK(dc.err); CK(dN.err); CK(dout.err);
    hipLaunchKernelGGL(k_shift_codes, dim3(grid_of(nprob, wpb)), dim3(64 * wpb), 0, 0, dc.as<unsigned long long>(),
                       dN.as<int>(), dout.as<unsigned long long>(), nprob);
    if (int rc = finish()) return rc;
    CK(dout.get(out));
    return 0;
}

// op: 0 he_mul (o0), 1 he_mul2 (o0, o1), 2 he_sub_outer (Hout); layouts as at k_he
int lh_he(int op, int ns, int packed, const double* H, const double* y0, const double* y1, const int* N, double* o0,
          double* o1, double* Hout, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    for (int q = 0; q < nprob; ++q) if (N[q] < 0 || N[q] > ns) return 1;
    if (ns == 32 && !packed) return run_he_op<32, false>(op, H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    if (ns == 32 && packed) return run_he_op<32, true>(op, H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    if (ns == 64 && !packed) return run_he_op<64, false>(op, H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    if (ns == 64 && packed) return run_he_op<64, true>(op, H, y0, y1, N, o0, o1, Hout, nprob, wpb);
    return 1;
}

// H [nprob][ns * ns] in place, ret [nprob][64]
int lh_he_invert(int ns, double* H, const int* N, int* ret, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    for (int q = 0; q < nprob; ++q) if (N[q] < 0 || N[q] > ns) return 1;
    if (ns == 32) return run_he_invert<32>(H, N, ret, nprob, wpb);
    if (ns == 64) return run_he_invert<64>(H, N, ret, nprob, wpb);
    return 1;
}

// op: 0 schur_invert, 1 schur_insert, 2 schur_remove, 3 update chain; layouts as at k_schur
int lh_schur(int op, int mmax, double* P, const int* m, const int* kind, const int* pos, const double* vec,
             const double* piv, int* ret, double* sv, int* m_out, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    if (mmax == 32) return run_schur_op<32>(op, P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    if (mmax == 34) return run_schur_op<34>(op, P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    if (mmax == 66) return run_schur_op<66>(op, P, m, kind, pos, vec, piv, ret, sv, m_out, nprob, wpb);
    return 1;
}

// (mmax, ns) in {(32, 32), (34, 32), (66, 64)}; layouts as at k_multipliers
int lh_multipliers(int mmax, int ns, const double* P, const double* img, const double* rows, const int* w_k, const int* m,
                   const int* N, double* lam, double* sv, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    if (mmax == 32 && ns == 32) return run_multipliers<32, 32>(P, img, rows, w_k, m, N, lam, sv, nprob, wpb);
    if (mmax == 34 && ns == 32) return run_multipliers<34, 32>(P, img, rows, w_k, m, N, lam, sv, nprob, wpb);
    if (mmax == 66 && ns == 64) return run_multipliers<66, 64>(P, img, rows, w_k, m, N, lam, sv, nprob, wpb);
    return 1;
}

// sizeof(DualMem<mmax, ns>): the caller's record layout must agree
int lh_dual_mem_size(int mmax, int ns) {
    if (mmax == 32 && ns == 32) return (int)sizeof(DualMem<32, 32>);
    if (mmax == 34 && ns == 32) return (int)sizeof(DualMem<34, 32>);
    if (mmax == 66 && ns == 64) return (int)sizeof(DualMem<66, 64>);
    return -1;
}

// op: 0 scatter_rows, 1 scatter_row (lane 0), 2 row_value, 3 step_rates, 4 refine_rounds; layouts as at k_dual
int lh_dual(int op, int mmax, int ns, void* mem, const double* par, const int* ipar, double* od, int* oi, int nprob, int wpb) {
    if (bad_shape(nprob, wpb)) return 1;
    if (mmax == 32 && ns == 32) return run_dual_op<32, 32>(op, mem, par, ipar, od, oi, nprob, wpb);
    if (mmax == 34 && ns == 32) return run_dual_op<34, 32>(op, mem, par, ipar, od, oi, nprob, wpb);
    if (mmax == 66 && ns == 64) return run_dual_op<66, 64>(op, mem, par, ipar, od, oi, nprob, wpb);
    return 1;
}

// in [n][3], tol0 [n] -> code [n][4] (EvCode::pack of the three and its parts) and tol [n] (viol_tolerance(tol0, in0, in1))
int lh_step_scalars(const int* in, const double* tol0, int* code, double* tol, int n) {
    if (n < 1 || n > 4096) return 1;
    Dev di(in, sizeof(int) * 3 * n), dt0(tol0, sizeof(double) * n), dc(nullptr, sizeof(int) * 4 * n), dt(nullptr, sizeof(double) * n);
    CK(di.err); CK(dt0.err); CK(dc.err); CK(dt.err);
    hipLaunchKernelGGL(k_event_code, dim3((n + 63) / 64), dim3(64), 0, 0, di.as<int>(), dc.as<int>(), n);
    hipLaunchKernelGGL(k_viol_tolerance, dim3((n + 63) / 64), dim3(64), 0, 0, dt0.as<double>(), di.as<int>(), dt.as<double>(), n);
    if (int rc = finish()) return rc;
    CK(dc.get(code)); CK(dt.get(tol));
    return 0;
}

// rows the solvers accept in a working set of capacity mmax (their guard in rebuild_and_factor)
int lh_schur_capacity(int mmax) {
    if (mmax == 32) return schur_capacity<32>();
    if (mmax == 34) return schur_capacity<34>();
    if (mmax == 66) return schur_capacity<66>();
    return -1;
}

}  // extern "C"
