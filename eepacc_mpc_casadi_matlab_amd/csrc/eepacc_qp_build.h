// eepacc_qp_build.h -- the skeleton of a kernel that writes the condensed QP of one MPC step out as data (H, g, A, lba, uba
// in the layout the dense QP operator reads): k_ab_build (eepacc_ab_build.hip), k_fb_qp (eepacc_fb_qp.hip) and k_bl_qp
// (eepacc_bl_qp.hip).  One workgroup of BT threads per instance; stage quantities go into LDS once; the dynamic LDS holds the
// sensitivity tables [N+1][N|1] and the row list.  What is here is what the three kernels do alike: the ego estimate (and the
// guesses a caller supplies in its place, which k_ab_build_est and k_bl_qp_est take), the row
// list, the walks over H, the bounds and A, and for the two double-integrator controllers (AB, BL) the row type, the position
// sensitivities and the entry of A.  The entry formulas differ per controller and stay in the units, which hand them to the
// writers as lambdas; everything inlines.
//
// Products are not contracted into fused multiply-adds, here and in whatever a unit includes or defines after this header
// (the estimators of eepacc_stage.h among them), so that an entry has the roundings of the reference's products.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#pragma clang fp contract(off)
#include "eepacc_device.h"
#include "eepacc_stage.h"

namespace eepacc {

constexpr int BT = 256;              // threads of a workgroup: four waves
constexpr int kS = kMaxN + 1;        // stage arrays: index N is the terminal stage

// ---- the row list: one entry per row of A, stage | type << 8
__device__ inline unsigned short row_code(int k, int type) { return (unsigned short)(k | (type << 8)); }
__device__ inline int row_stage(int e) { return e & 0xff; }
__device__ inline int row_type(int e) { return e >> 8; }

// Dynamic LDS of a workgroup: n_tables sensitivity tables [N+1][N|1] (the odd row stride lets a column be read without bank
// conflicts), then the row list [nC].
constexpr size_t qp_build_smem_bytes(int N, int nC, int n_tables) {
    return (size_t)n_tables * (N + 1) * (N | 1) * sizeof(double) + (size_t)nC * sizeof(unsigned short);
}
__device__ inline unsigned short* qp_build_rows(double* tables, int N, int n_tables) {
    return reinterpret_cast<unsigned short*>(tables + (size_t)n_tables * (N + 1) * (N | 1));
}

// The rows of stage k, from its first row r on: the present types in ascending order
template <class Present>
__device__ inline void fill_stage_rows(unsigned short* rows, int r, int k, int n_types, Present present) {
    for (int type = 0; type < n_types; ++type)
        if (present(type, k)) rows[r++] = row_code(k, type);
}
__device__ inline void fill_terminal_rows(unsigned short* rows, int nC, int N, int safe1, int safe2) {
    rows[nC - 2] = row_code(N, safe1);
    rows[nC - 1] = row_code(N, safe2);
}

// Padding (k_ab_build_cls): where the instances of a launch differ in their row count, the arrays have the leading row
// dimension nC of the largest and an instance with n_own rows carries nC - n_own padding rows behind its own.  They are
// entries of the row list like any other, of a type no controller has, so the walks over the bounds and A write them on their
// way: a blank row (every coefficient 0.0, no slack) with the bounds below, which no finite x violates.
constexpr int kRowPad = 0xff;
__device__ inline bool row_is_pad(int e) { return row_type(e) == kRowPad; }
__device__ inline void fill_pad_rows(unsigned short* rows, int n_own, int nC, int tid) {
    for (int r = n_own + tid; r < nC; r += BT) rows[r] = row_code(0, kRowPad);
}

// Ego estimate of stage k.  pred(idx, ps, pv) supplies the previous step's predictions of stage idx for paramEstSetting 2.
template <class Pred>
__device__ inline void ego_estimate(const DevCfg& C, double s_0, double v_0, double a_minus1, int k, Pred pred,
                                    double& se, double& ve) {
    const int N = C.N;
    if (C.paramEstSetting == 2) {
        // EstimateVehicleTrajectory.m:81-88: [x_curr; prev(3:end); prev(end) + Ts v_prev(end)]; the handle carries
        // the previous step's predictions, which are read and not written here
        const int idx = k < N ? k + 1 : N;
        double ps, pv;
        pred(idx, ps, pv);
        se = k == 0 ? s_0 : (k < N ? ps : ps + C.Tvec[N - 1] * pv);
        ve = k == 0 ? v_0 : pv;
    } else {
        estimate_traj(C, C.paramEstSetting, C.tConstACC_ego, s_0, v_0, a_minus1, k, se, ve);
    }
}

// Horizon guesses of stage k that the caller supplies instead ([N+1][B] each, as EstimateVehicleTrajectory returns them;
// s_est and v_est both or neither; a null array keeps the estimate).  Row N of s_tv_est is not read: no row uses it.
__device__ inline void supplied_estimates(int k, int N, size_t B, size_t b, const double* s_est, const double* v_est,
                                          const double* s_tv_est, double& se, double& ve, double& st) {
    if (s_est) { se = s_est[(size_t)k * B + b]; ve = v_est[(size_t)k * B + b]; }
    if (s_tv_est && k < N) st = s_tv_est[(size_t)k * B + b];
}

// ---- H, row-major: consecutive lanes write consecutive entries; (ra, rb) advance without a division.  entry(ra, rb) -> double
template <class Entry>
__device__ inline void write_H(double* Hd, int nV, int tid, Entry entry) {
    const int total = nV * nV, dra = BT / nV, drb = BT % nV;
    int ra = tid / nV, rb = tid % nV;
    for (int idx = tid; idx < total; idx += BT) {
        Hd[idx] = entry(ra, rb);
        rb += drb; ra += dra;
        if (rb >= nV) { rb -= nV; ++ra; }
    }
}

// ---- lba, uba: the row's bounds less its value at the free response.  bounds(e) -> RowBounds of row-list entry e
struct RowBounds { double lb, ub, shift; };
template <class Bounds>
__device__ inline void write_bounds(double* lba, double* uba, const unsigned short* rows, int nC, int tid, Bounds bounds) {
    for (int r = tid; r < nC; r += BT) {
        const RowBounds Bd = bounds((int)rows[r]);
        lba[r] = Bd.lb - Bd.shift;
        uba[r] = Bd.ub - Bd.shift;
    }
}

// ---- A, column-major nC x nV: a wave takes 64 consecutive rows (consecutive addresses of one column), decodes its row once
// and walks the columns of its quarter of the stages, so the four waves share every block of rows evenly.  A stage has NX
// controls and then NXI slacks.  decode(e) -> a row with members slack (0 .. NXI-1, -1 none) and sc; vars(R, k, i, x) puts the
// row's coefficients on the controls of stage i into x[NX]; the slack columns are one-hot in the row's own stage.
template <int NX, int NXI, class Decode, class Vars>
__device__ inline void write_A(double* Ad, const unsigned short* rows, int N, int nC, int tid, Decode decode, Vars vars) {
    const int wave = tid >> 6, lane = tid & 63;
    const int i0 = wave * N / 4, i1 = (wave + 1) * N / 4;
    for (int r0 = 0; r0 < nC; r0 += 64) {
        const int r = r0 + lane;
        if (r >= nC) continue;
        const int e = rows[r], k = row_stage(e);
        const auto R = decode(e);
        double* col = Ad + (size_t)((NX + NXI) * i0) * nC + r;
        for (int i = i0; i < i1; ++i) {
            double x[NX];
            vars(R, k, i, x);
#pragma unroll
            for (int c = 0; c < NX; ++c) col[(size_t)c * nC] = x[c];
#pragma unroll
            for (int c = 0; c < NXI; ++c) col[(size_t)(NX + c) * nC] = (i == k && c == R.slack) ? R.sc : 0.0;
            col += (size_t)(NX + NXI) * nC;
        }
    }
}

// ---- the double-integrator controllers (AB, BL): A_k = [1 T_k; 0 1], B_k = [T_k^2/2; T_k] on the acceleration only,
//   v_k = v_0 + sum_{i<k} T_i a_i,   s_k = d_s[k] + sum_{i<k} Ss[k][i] a_i,   Ss[k][i] = T_i^2/2 + T_i (T_{k-1} + .. + T_{i+1})

struct Row {                         // one row: as s_k + av v_k + ga a_k + de a_{k-1} + sc xi_slack in [lb, ub]
    int k, slack;                    // slack: index among the stage's slacks, -1 none
    double as, av, ga, de, sc, lb, ub;
};

__device__ inline Row di_row_blank(int k, int slack) {
    Row R;
    R.k = k; R.slack = slack;
    R.as = R.av = R.ga = R.de = R.sc = 0.0;
    R.lb = -INFINITY; R.ub = INFINITY;
    return R;
}

// The two terminal rows (CreateQP_AB.m:376-387, CreateQP_BL.m:306-314) on a blank row; stv: the lead's estimated position
__device__ inline void di_row_terminal(Row& R, const DevCfg& C, const double* stv, bool safe1) {
    const int N = C.N;
    R.as = 1.0;
    if (safe1) R.ub = stv[N - 1] - C.h_min;
    else { R.av = C.tau_min; R.ub = stv[N - 1]; }
}

// Row k of Ss; returns the free response d_s[k].  T: the stage durations in LDS
__device__ inline double di_position_row(const double* T, double* Ss, int ld, int k, double s_0, double v_0) {
    double R = 0.0;                                         // T_{k-1} + .. + T_{i+1}, summed downwards as the reference does
    for (int i = k - 1; i >= 0; --i) {
        const double Ti = T[i];
        Ss[(size_t)k * ld + i] = 0.5 * Ti * Ti + R * Ti;
        R += Ti;
    }
    return k == 0 ? s_0 : s_0 + R * v_0;
}

__device__ inline RowBounds di_bounds(const Row& R, const double* ds, double v_0) {
    return RowBounds{R.lb, R.ub, R.as * ds[R.k] + R.av * v_0};
}

// Coefficient of row R (of stage k) on a_i
__device__ inline double di_A_entry(const Row& R, const double* Ss, int ld, const double* T, int k, int i) {
    double va = 0.0;
    if (i < k) { va = R.as * Ss[(size_t)k * ld + i]; va += R.av * T[i]; }
    if (i == k) va = R.ga;
    if (i == k - 1) va += R.de;
    return va;
}

}  // namespace eepacc
