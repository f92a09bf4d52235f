// eepacc_units.h -- closed-loop plumbing shared by the ABMPC (k_run_abmpc, eepacc_ab_impl.inc) and FBMPC (k_fbs_run,
// eepacc_fbs.hip) kernels: the work-unit scheduler with its inter-wave hand-off, the carried loop state, the measurement
// at the head of an MPC step, the output row, the working-set shift and the packed-triangle index table; on the host,
// the prologue of a closed-loop launch.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "eepacc_device.h"
#include "eepacc_stage.h"
#include "eepacc_wave.h"
#include "../../include/eepacc.h"

namespace eepacc {

struct StepOut { double out[EEPACC_OUT_N]; int status, iters; };

// index of entry (i, j) of a packed symmetric matrix (lower triangle, row-major)
__device__ __forceinline__ int pidx(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// row/column of entry e of a packed lower triangle (e = r(r+1)/2 + c), one table per workgroup
template <int MMAX>
__device__ __forceinline__ unsigned short* rc_table() {
    __shared__ unsigned short tab[MMAX * (MMAX + 1) / 2];
    return tab;
}
template <int MMAX>
__device__ __forceinline__ void rc_table_init() {      // every thread of the workgroup, before any returns
    unsigned short* tab = rc_table<MMAX>();
    for (int e = threadIdx.x; e < MMAX * (MMAX + 1) / 2; e += blockDim.x) {
        int r = (int)((sqrtf(8.0f * (float)e + 1.0f) - 1.0f) * 0.5f);
        while (r * (r + 1) / 2 > e) --r;
        while ((r + 1) * (r + 2) / 2 <= e) ++r;
        tab[e] = (unsigned short)((r << 8) | (e - r * (r + 1) / 2));
    }
    __syncthreads();
}

// receding-horizon shift of the working set: stage k takes stage k+1's codes, the last stage and the terminal rows
// keep theirs
__device__ __forceinline__ unsigned long long shift_codes(unsigned long long code, int N) {
    const int lane = wv::lane_id();
    unsigned lo = (unsigned)code, hi = (unsigned)(code >> 32);
    unsigned nlo = __shfl_down(lo, 1, 64), nhi = __shfl_down(hi, 1, 64);
    unsigned long long nxt = ((unsigned long long)nhi << 32) | nlo;
    if (lane < N - 1) return nxt;
    return code;
}

// output row of instance b in a field-major [rows][B] array: lane f stores field f in row row0 + f
__device__ __forceinline__ void write_out(double* out, size_t row0, int B, int b, const StepOut& so, int lane) {
    if (lane < EEPACC_OUT_N) {
        double val = 0.0;
#pragma unroll
        for (int f = 0; f < EEPACC_OUT_N; ++f) if (f == lane) val = so.out[f];
        out[(row0 + lane) * B + b] = val;
    }
}

// Loop state of an instance between MPC steps; it travels between work units (and launches) as carry[6][B]:
// s, v, Fm, Fb of the previous step, the previous measured lead speed, t_0.
struct Carry {
    double s = 0.0, v = 0.0, Fm = 0.0, Fb = 0.0, v_tv = 0.0, t0 = 0.0;

    __device__ __forceinline__ void load(const double* c, int B, int b) {
        s = c[0 * (size_t)B + b]; v = c[1 * (size_t)B + b];
        Fm = c[2 * (size_t)B + b]; Fb = c[3 * (size_t)B + b];
        v_tv = c[4 * (size_t)B + b]; t0 = c[5 * (size_t)B + b];
    }
    __device__ __forceinline__ void store(double* c, int B, int b) const {
        c[0 * (size_t)B + b] = s; c[1 * (size_t)B + b] = v;
        c[2 * (size_t)B + b] = Fm; c[3 * (size_t)B + b] = Fb;
        c[4 * (size_t)B + b] = v_tv; c[5 * (size_t)B + b] = t0;
    }
    // the step's applied forces become the state of the next step (RunOpt_ABMPC.m:329)
    __device__ __forceinline__ void advance(const StepOut& so, double Ts) {
        s = so.out[EEPACC_OUT_S]; v = so.out[EEPACC_OUT_V];
        Fm = so.out[EEPACC_OUT_FM]; Fb = so.out[EEPACC_OUT_FB];
        t0 += Ts;
    }
};

// Measurement at the head of MPC step k = k_start + kk (RunOpt_ABMPC.m:159-191, RunOpt_FBMPC.m:165-200): step 0 reads
// the initial state, a later step integrates the plant over the previous one and differences the measured lead speed.
// Fills the fields of the step input both controllers have.
template <class StepIn>
__device__ __forceinline__ void measure(const DevCfg& C, double Ts, int k, int kk, int B, int b, const double* s0,
                                        const double* v0, const double* a_m1, const double* s_tv, const double* v_tv,
                                        Carry& cs, StepIn& in) {
    if (k == 0) {                                        // RunOpt_ABMPC.m:159-172
        in.s = s0[b]; in.v = v0[b]; in.a_prev = a_m1[b];
        in.s_tv = s_tv[b]; in.v_tv = 0.0; in.a_tv_prev = 0.0;
        cs.v_tv = 0.0;
    } else {                                             // :173-191
        double sm, vm;
        plant_rk4(C, cs.s, cs.v, cs.Fm + cs.Fb, sm, vm);
        in.s = sm; in.v = vm;
        in.a_prev = (vm - cs.v) / Ts;
        in.s_tv = s_tv[(size_t)kk * B + b];
        const double v_tv_prev = cs.v_tv;
        cs.v_tv = v_tv[(size_t)kk * B + b];
        in.v_tv = cs.v_tv;
        in.a_tv_prev = (cs.v_tv - v_tv_prev) / Ts;
    }
    in.t0 = cs.t0;
}

// The same without a lead vehicle (RunOpt_TVMPC.m:134-154): the target-vehicle MPC follows nobody, its kernels get no traces.
template <class StepIn>
__device__ __forceinline__ void measure_no_lead(const DevCfg& C, double Ts, int k, int b, const double* s0,
                                                const double* v0, const double* a_m1, Carry& cs, StepIn& in) {
    if (k == 0) {                                        // RunOpt_TVMPC.m:134-137
        in.s = s0[b]; in.v = v0[b]; in.a_prev = a_m1[b];
    } else {                                             // :143-153
        double sm, vm;
        plant_rk4(C, cs.s, cs.v, cs.Fm + cs.Fb, sm, vm);
        in.s = sm; in.v = vm;
        in.a_prev = (vm - cs.v) / Ts;
    }
    in.s_tv = 0.0; in.v_tv = 0.0; in.a_tv_prev = 0.0;
    in.t0 = cs.t0;
}

// Instances take very different numbers of working-set changes (per-instance run times spread 0.75x..1.7x around the
// mean), so the simulation is cut into work units (instance, chunk of chunk_steps MPC steps) handed out through a
// device-wide counter in chunk-major order.  The loop state of an instance travels between units through HBM: the
// producer wave publishes done[b] = chunk+1 behind an agent-scope release, the consumer polls done[b] relaxed and then
// takes one agent-scope acquire (cdna_hip_programming.md, Guideline 16).  A unit is only handed out after its
// predecessor has been picked by a running wave, so the wait is bounded.
//
// body(b, kk0, kk1) runs MPC steps kk0 .. kk1-1 of instance b, stores the loop state it carries and returns its
// working-set changes, which are added to iters_total[b] (microseconds of the unit instead with EEPACC_DEBUG_TIMING).
template <class Body>
__device__ __forceinline__ void run_units(int B, int n_steps, int chunk_steps, int* work_counter, int* done,
                                          int* err_word, int spin_limit, int32_t* status, int32_t* iters_total,
                                          Body&& body) {
    const int lane = wv::lane_id();
    const int n_chunks = (n_steps + chunk_steps - 1) / chunk_steps;
    const int n_units = n_chunks * B;
    for (int fetch = 0; fetch <= n_units; ++fetch) {
        int u = 0;
        if (lane == 0) u = atomicAdd(work_counter, 1);
        u = __builtin_amdgcn_readfirstlane(u);
        if (u >= n_units || u < 0) break;
        const int chunk = u / B, b = u - chunk * B;
        const int kk0 = chunk * chunk_steps;
        const int kk1 = (kk0 + chunk_steps < n_steps) ? kk0 + chunk_steps : n_steps;
        bool failed = false;
        if (chunk > 0) {
            int spins = 0;
            while (__hip_atomic_load(&done[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < chunk) {
                __builtin_amdgcn_s_sleep(32);
                if (++spins > spin_limit) { failed = true; break; }   // never expected; keeps every wave finite
                // an earlier time-out of this launch: do not wait the full limit again behind it
                if ((spins & 63) == 0 && __hip_atomic_load(err_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) break;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        // A predecessor that was never published (or any earlier failure of this launch) must not be continued
        // from stale state: the unit's steps get status 3, the sticky error word of the handle is set (the host
        // turns it into EEPACC_EDEVICE, eepacc_synchronize) and the unit is still published so that its
        // successors terminate.
        if (failed || __hip_atomic_load(err_word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
            if (lane == 0) {
                if (failed) atomicOr(err_word, 1);
                for (int kk = kk0; kk < kk1; ++kk) status[(size_t)kk * B + b] = 3;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                __hip_atomic_fetch_max(&done[b], chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            continue;
        }
#ifdef EEPACC_DEBUG_TIMING
        const long long t_begin = wall_clock64();
#endif
        [[maybe_unused]] const int it_total = body(b, kk0, kk1);
        if (lane == 0) {
#ifdef EEPACC_DEBUG_TIMING
            if (iters_total) atomicAdd(&iters_total[b], (int)((wall_clock64() - t_begin) / 100));   // microseconds
#else
            if (iters_total) atomicAdd(&iters_total[b], it_total);
#endif
        }
        // publish the unit: all of this wave's stores, then release, then the flag
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (lane == 0) {
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __hip_atomic_fetch_max(&done[b], chunk + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Host prologue of a closed-loop launch: resets the hand-off state (work counter, done flags, iters_total) on the
// stream and sizes the grid to one block per `wpb` work units, at most `max_grid` (one chip-filling wave of blocks).
// spin_limit bounds the inter-unit wait; the debug hook EEPACC_DEBUG_SPIN_LIMIT lowers it to exercise the failure path.
struct UnitsLaunch { int grid, spin_limit; };
inline hipError_t begin_units(int* work_counter, int* done, int32_t* iters_total, int B, int n_steps, int chunk_steps,
                              int wpb, int max_grid, hipStream_t stream, UnitsLaunch& ul) {
    hipError_t e = hipMemsetAsync(work_counter, 0, sizeof(int), stream);
    if (e != hipSuccess) return e;
    e = hipMemsetAsync(done, 0, sizeof(int) * (size_t)B, stream);
    if (e != hipSuccess) return e;
    if (iters_total) {
        e = hipMemsetAsync(iters_total, 0, sizeof(int32_t) * (size_t)B, stream);
        if (e != hipSuccess) return e;
    }
    const int n_units = ((n_steps + chunk_steps - 1) / chunk_steps) * B;
    const int need = (n_units + wpb - 1) / wpb;
    ul.grid = max_grid > need ? need : max_grid;
    ul.spin_limit = 1 << 26;
    if (const char* ev = getenv("EEPACC_DEBUG_SPIN_LIMIT")) ul.spin_limit = atoi(ev);
    return hipSuccess;
}

}  // namespace eepacc
