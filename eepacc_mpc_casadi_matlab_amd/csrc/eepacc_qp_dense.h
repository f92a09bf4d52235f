// Internal interface of the batched dense QP kernel (eepacc_qp_dense.hip).
#ifndef EEPACC_QP_DENSE_H
#define EEPACC_QP_DENSE_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

struct eepacc_qp_args {
    int B, nV, nC;
    const double *H, *g, *A, *lba, *uba, *lbx, *ubx, *x0;   // device, instance-major
    double *x, *cost;
    int32_t *status, *iters;
    int* counter;          // device int, zeroed before the launch (work distribution)
    int* rho_k;            // [B] in/out hint: exponent k of the regularisation found last time (may be NULL)
    double* ws;            // grid * ws_stride doubles
    size_t ws_stride;
    double rho_rel;        // <= 0: 1e-7
    int max_prox;          // <= 0: 8
    // read and written by the dual instantiation only (eepacc_qp_dense_launch_dual); each may be NULL
    const int8_t *ws0_a = nullptr, *ws0_x = nullptr;   // [B][nC], [B][nV] warm start: -1 lower side, +1 upper side, else none
    double *lam_a = nullptr, *lam_x = nullptr;         // [B][nC], [B][nV] multipliers, CasADi's sign
    int8_t *ws_a = nullptr, *ws_x = nullptr;           // [B][nC], [B][nV] final working set, coded like ws0
};

size_t eepacc_qp_dense_ws_doubles(int nV);
size_t eepacc_qp_dense_lds_bytes(int nV, int nC);
hipError_t eepacc_qp_dense_launch(const eepacc_qp_args& a, int grid, hipStream_t stream);
// the instantiation with multipliers, working set and warm start (same workspace, same LDS)
hipError_t eepacc_qp_dense_launch_dual(const eepacc_qp_args& a, int grid, hipStream_t stream);

// k_qp_kkt: nR linear solves per instance with the KKT matrix of a given working set (eepacc_qp_kkt_solve_batched).
// Workspace, LDS and work distribution are those of the solver.
struct eepacc_qp_kkt_args {
    int B, nV, nC, nR;
    const double *H, *A;                 // as eepacc_qp_args
    const int8_t *ws_a, *ws_x;           // [B][nC], [B][nV]: +-1 held, anything else not; each may be NULL
    const double *r_p, *r_a, *r_x;       // [B][nR][nV], [B][nR][nC], [B][nR][nV]; r_a, r_x may be NULL (zeros)
    double *p, *q_a, *q_x;               // same shapes; q_a, q_x may be NULL
    int32_t* status;                     // [B] 0 solved, 1 singular or more than nV held (outputs NaN); may be NULL
    int* counter;
    double* ws;
    size_t ws_stride;
};
hipError_t eepacc_qp_kkt_launch(const eepacc_qp_kkt_args& a, int grid, hipStream_t stream);

#endif
