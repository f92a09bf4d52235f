// stage_harness.hip -- test-only device harness for the per-stage device functions of csrc/eepacc_stage.h: the trajectory
// estimator (modes 0 and 1), the route / comfort bounds, the PWA interpolation and the RK4 plant.
//
// One kernel per function, one thread per problem, flat arrays of per-problem inputs and outputs; the DevCfg is the byte
// image the settings translation produced on the host (tests/cfg_harness.py), copied to the device unchanged.  Outputs are
// filled with NaN before a launch: a problem the kernel did not write shows up in the result.
//
// The extern "C" entry points take host pointers, do their own allocation and copies and return 0 or a non-zero code
// (1: bad argument, 1000 + hipError_t: a HIP call failed).  This file is built into its own shared object
// (tests/stage_harness.py), never into libeepacc.so.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "eepacc_device.h"
#include "eepacc_stage.h"

using namespace eepacc;

namespace {

constexpr int kBlock = 64;
constexpr int kMaxProblems = 8192;

__global__ void k_estimate(const DevCfg* cfg, int n, const int* mode, const double* tConstACC, const double* s0,
                           const double* v0, const double* a0, const int* lane, double* s_est, double* v_est) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double s, v;
    estimate_traj(*cfg, mode[q], tConstACC[q], s0[q], v0[q], a0[q], lane[q], s, v);
    s_est[q] = s;
    v_est[q] = v;
}

// out [8][n]: v_lim, v_curv, v_stop, v_TL, a_min, a_max, j_min, j_max
__global__ void k_route_bounds(const DevCfg* cfg, int n, const double* s_est, const double* v_est, const double* t0,
                               const int* i, double* out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double o[8];
    route_bounds(*cfg, s_est[q], v_est[q], t0[q], i[q], o[0], o[1], o[2], o[3], o[4], o[5], o[6], o[7]);
    for (int k = 0; k < 8; ++k) out[(size_t)k * n + q] = o[k];
}

__global__ void k_interp_pwa(int n, const double* d, const double* doms, const double* vals, int nk, double* out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    out[q] = interp_pwa(d[q], doms, vals, nk);
}

__global__ void k_plant(const DevCfg* cfg, int n, const double* s, const double* v, const double* u, double* s1, double* v1) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= n) return;
    double a, b;
    plant_rk4(*cfg, s[q], v[q], u[q], a, b);
    s1[q] = a;
    v1[q] = b;
}

// ---------------------------------------------------------------------------------------------- host side
#define CK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return 1000 + (int)e_; } while (0)

struct Dev {                     // a device copy of a host array (NaN bytes without one)
    void* d = nullptr;
    size_t bytes;
    hipError_t err;
    Dev(const void* h, size_t n) : bytes(n) {
        err = hipMalloc(&d, n ? n : 1);
        if (err != hipSuccess) { d = nullptr; return; }
        err = h ? hipMemcpy(d, h, n, hipMemcpyHostToDevice) : hipMemset(d, 0xff, n);
    }
    ~Dev() { if (d) (void)hipFree(d); }
    Dev(const Dev&) = delete;
    Dev& operator=(const Dev&) = delete;
    hipError_t get(void* h) const { return hipMemcpy(h, d, bytes, hipMemcpyDeviceToHost); }
    template <class T> T* as() const { return static_cast<T*>(d); }
};

bool bad_count(int n) { return n < 1 || n > kMaxProblems; }
bool bad_cfg(const void* cfg, int cfg_bytes) { return !cfg || cfg_bytes != (int)sizeof(DevCfg); }
dim3 grid_of(int n) { return dim3((n + kBlock - 1) / kBlock); }
int finish() {
    CK(hipGetLastError());
    CK(hipDeviceSynchronize());
    return 0;
}

}  // namespace

extern "C" {

int sh_sizeof_devcfg() { return (int)sizeof(DevCfg); }

// mode, lane [n] ints (mode 0 or 1, lane >= 0); tConstACC, s0, v0, a0 [n]; s_est, v_est [n] out
int sh_estimate(const void* cfg, int cfg_bytes, const int* mode, const double* tConstACC, const double* s0,
                const double* v0, const double* a0, const int* lane, double* s_est, double* v_est, int n) {
    if (bad_cfg(cfg, cfg_bytes) || bad_count(n)) return 1;
    const int N = static_cast<const DevCfg*>(cfg)->N;
    if (N < 1 || N > kMaxN) return 1;
    for (int q = 0; q < n; ++q) if ((mode[q] != 0 && mode[q] != 1) || lane[q] < 0) return 1;
    const size_t db = sizeof(double) * n, ib = sizeof(int) * n;
    Dev dc(cfg, sizeof(DevCfg)), dm(mode, ib), dt(tConstACC, db), ds(s0, db), dv(v0, db), da(a0, db), dl(lane, ib);
    Dev os(nullptr, db), ov(nullptr, db);
    CK(dc.err); CK(dm.err); CK(dt.err); CK(ds.err); CK(dv.err); CK(da.err); CK(dl.err); CK(os.err); CK(ov.err);
    hipLaunchKernelGGL(k_estimate, grid_of(n), dim3(kBlock), 0, 0, dc.as<DevCfg>(), n, dm.as<int>(), dt.as<double>(),
                       ds.as<double>(), dv.as<double>(), da.as<double>(), dl.as<int>(), os.as<double>(), ov.as<double>());
    if (int rc = finish()) return rc;
    CK(os.get(s_est)); CK(ov.get(v_est));
    return 0;
}

// s_est, v_est, t0 [n]; i [n] the 0-based stage, 0 <= i < N (it indexes Tvec); out [8][n]
int sh_route_bounds(const void* cfg, int cfg_bytes, const double* s_est, const double* v_est, const double* t0,
                    const int* i, double* out, int n) {
    if (bad_cfg(cfg, cfg_bytes) || bad_count(n)) return 1;
    const DevCfg* C = static_cast<const DevCfg*>(cfg);
    if (C->N < 1 || C->N > kMaxN) return 1;
    if (C->n_speedLim < 0 || C->n_speedLim > kMaxKnots || C->n_curv < 0 || C->n_curv > kMaxKnots || C->n_stop < 0 ||
        C->n_stop > kMaxStops || C->n_TL < 0 || C->n_TL > kMaxTL)
        return 1;
    for (int q = 0; q < n; ++q) if (i[q] < 0 || i[q] >= C->N) return 1;
    const size_t db = sizeof(double) * n;
    Dev dc(cfg, sizeof(DevCfg)), ds(s_est, db), dv(v_est, db), dt(t0, db), di(i, sizeof(int) * n), o(nullptr, 8 * db);
    CK(dc.err); CK(ds.err); CK(dv.err); CK(dt.err); CK(di.err); CK(o.err);
    hipLaunchKernelGGL(k_route_bounds, grid_of(n), dim3(kBlock), 0, 0, dc.as<DevCfg>(), n, ds.as<double>(), dv.as<double>(),
                       dt.as<double>(), di.as<int>(), o.as<double>());
    if (int rc = finish()) return rc;
    CK(o.get(out));
    return 0;
}

// d, out [n]; doms, vals [nk], 1 <= nk <= kMaxKnots
int sh_interp_pwa(const double* d, const double* doms, const double* vals, int nk, double* out, int n) {
    if (bad_count(n) || nk < 1 || nk > kMaxKnots || !doms || !vals) return 1;
    const size_t db = sizeof(double) * n, kb = sizeof(double) * nk;
    Dev dd(d, db), dk(doms, kb), dv(vals, kb), o(nullptr, db);
    CK(dd.err); CK(dk.err); CK(dv.err); CK(o.err);
    hipLaunchKernelGGL(k_interp_pwa, grid_of(n), dim3(kBlock), 0, 0, n, dd.as<double>(), dk.as<double>(), dv.as<double>(), nk,
                       o.as<double>());
    if (int rc = finish()) return rc;
    CK(o.get(out));
    return 0;
}

// s, v, u [n] (u the total force Fm + Fb); s1, v1 [n] out
int sh_plant(const void* cfg, int cfg_bytes, const double* s, const double* v, const double* u, double* s1, double* v1, int n) {
    if (bad_cfg(cfg, cfg_bytes) || bad_count(n)) return 1;
    const DevCfg* C = static_cast<const DevCfg*>(cfg);
    if (C->N_integratePlant < 1 || C->N_integratePlant > 1000 || C->n_slope < 1 || C->n_slope > kMaxKnots) return 1;
    const size_t db = sizeof(double) * n;
    Dev dc(cfg, sizeof(DevCfg)), ds(s, db), dv(v, db), du(u, db), o0(nullptr, db), o1(nullptr, db);
    CK(dc.err); CK(ds.err); CK(dv.err); CK(du.err); CK(o0.err); CK(o1.err);
    hipLaunchKernelGGL(k_plant, grid_of(n), dim3(kBlock), 0, 0, dc.as<DevCfg>(), n, ds.as<double>(), dv.as<double>(),
                       du.as<double>(), o0.as<double>(), o1.as<double>());
    if (int rc = finish()) return rc;
    CK(o0.get(s1)); CK(o1.get(v1));
    return 0;
}

}  // extern "C"
