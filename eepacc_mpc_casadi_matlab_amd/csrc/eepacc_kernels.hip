// eepacc_kernels.hip -- hand-written HIP (gfx950) kernels of the batched ABMPC step.
//
// One QP instance per 64-lane wavefront: horizon stage k lives on lane k (terminal stage on
// lane N), the small inverse-KKT block of the working set and all per-stage vectors are staged
// in LDS.  The horizon condensing is never materialised: every constraint row of the reference
// QP (ABO/Functions/MPCs/CreateQP_AB.m:256-387) is  al*s_k + be*v_k + ga*a_k + de*a_{k-1} - xi <= b
// and the condensed double integrator (ABO/RunOpt_ABMPC.m:74-82 +
// ABO/Functions/MPCs/TransformToDenseFormulation.m:46-68) turns into wave-level prefix /
// suffix scans.  The slack columns are eliminated exactly (capped-multiplier groups, compliant
// row for the quadratic slack); the dense active-set solve is a dual (Goldfarb-Idnani type)
// method on the N x N acceleration block.  DESIGN.md has the derivation.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>
#include "eepacc_device.h"
#include "eepacc_stage.h"
#include "eepacc_units.h"
#include "eepacc_schur.h"
#include "eepacc_dual_step.h"
#include "eepacc_ab_cols.h"
#include "eepacc_ab.h"
#include "../../include/eepacc.h"

// The variants of eepacc_ab_impl.inc, each compiled into its own namespace so that the default path carries no register or
// instruction cost for the others: X(AbVariant, namespace, EEPACC_IMPL_MB, _BL, _TV, _ICE, _CLS, _EST, ...).  A new variant is a line here,
// its AbVariant (eepacc_ab.h) and its #include below.
//   blc    baseline controller (RunOpt_BLMPC): the same kernels with CreateQP_BL's row grouping
//   tvc    target-vehicle MPC (RunOpt_TVMPC): the baseline variant with CreateQP_TV's row catalogue (no vehicle-following
//          rows, 0.8 of the speed-limit and curve caps, low-speed comfort limits) and no lead inputs
//   ice*   ICE-map fuel term (CreateQP_AB.m:154-159): step-varying Hessian, built and inverted in LDS every step; icemb
//          folds the Hessian into E'HE before the inversion.  Two namespaces: compiled into one, the blocking code costs
//          the small ICE kernel 18 % of its throughput at N = 30 even where the handle has no Mb.
//   cls    settings classes (eepacc_create_classes): the plain kernels with the DevCfg bound per instance, through the
//          class map that its kernels alone take as one more argument
//   blcls  the baseline controller with settings classes (eepacc_create_classes_bl, bl_mode = 1 in every class): blc with the
//          DevCfg bound per instance as in cls
//   tvcls  the target-vehicle MPC with settings classes (eepacc_create_classes_bl, bl_mode = 2 in every class): tvc likewise
//   est    horizon guesses from the caller (eepacc_ab_step_est, eepacc_run_abmpc_preview): the plain kernels with the three
//          supplied arrays (step) or the preview tables (closed loop) as further arguments of its kernels alone; no handle
//          has this variant, its two entry points run a plain handle
//   blest  the same for the baseline controller (eepacc_bl_step_est, eepacc_run_blmpc_preview): blc with est's further
//          arguments; no handle has this variant either, its entry points run a bl_mode = 1 handle
//   clsest, blclsest  cls and blcls with est's further arguments behind the class map (eepacc_classes_step_est,
//          eepacc_run_classes_preview): no handle has these variants, the two entry points run a handle of
//          eepacc_create_classes through clsest and one of eepacc_create_classes_bl with bl_mode = 1 through blclsest
//          
#define EEPACC_AB_VARIANTS(X, ...)                                                     \
    X(Plain, nomb, false, false, false, false, false, false, __VA_ARGS__)              \
    X(MoveBlocking, withmb, true, false, false, false, false, false, __VA_ARGS__)      \
    X(Baseline, blc, false, true, false, false, false, false, __VA_ARGS__)             \
    X(Ice, ice, false, false, false, true, false, false, __VA_ARGS__)                  \
    X(IceMoveBlocking, icemb, true, false, false, true, false, false, __VA_ARGS__)     \
    X(TargetVehicle, tvc, false, true, true, false, false, false, __VA_ARGS__)         \
    X(Classes, cls, false, false, false, false, true, false, __VA_ARGS__)              \
    X(ClassesBL, blcls, false, true, false, false, true, false, __VA_ARGS__)           \
    X(ClassesTV, tvcls, false, true, true, false, true, false, __VA_ARGS__)            \
    X(Est, est, false, false, false, false, false, true, __VA_ARGS__)                  \
    X(BlEst, blest, false, true, false, false, false, true, __VA_ARGS__)               \
    X(ClassesEst, clsest, false, false, false, false, true, true, __VA_ARGS__)         \
    X(ClassesBlEst, blclsest, false, true, false, false, true, true, __VA_ARGS__)

// an instantiation reads its switches from the list by the name of its namespace
namespace eepacc { namespace ab_switch {
#define EEPACC_AB_SWITCHES(E, NSP, MB_, BL_, TV_, ICE_, CLS_, EST_, ...) struct NSP { static constexpr bool MB = MB_, BL = BL_, TV = TV_, ICE = ICE_, CLS = CLS_, EST = EST_; };
EEPACC_AB_VARIANTS(EEPACC_AB_SWITCHES)
} }
#define EEPACC_IMPL_MB ab_switch::EEPACC_IMPL_NS::MB
#define EEPACC_IMPL_BL ab_switch::EEPACC_IMPL_NS::BL
#define EEPACC_IMPL_TV ab_switch::EEPACC_IMPL_NS::TV
#define EEPACC_IMPL_ICE ab_switch::EEPACC_IMPL_NS::ICE
#define EEPACC_IMPL_CLS ab_switch::EEPACC_IMPL_NS::CLS
#define EEPACC_IMPL_EST ab_switch::EEPACC_IMPL_NS::EST
#define EEPACC_IMPL_NS nomb
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS withmb
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS blc
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS ice
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS icemb
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS tvc
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS cls
#define EEPACC_IMPL_CLASS_MAP       // the preprocessor's copy of the list's CLS switch (eepacc_ab_impl.inc checks that they agree)
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS blcls
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS tvcls
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS clsest
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS blclsest
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_CLASS_MAP
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS est
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS
#define EEPACC_IMPL_NS blest
#include "eepacc_ab_impl.inc"
#undef EEPACC_IMPL_NS

// ----------------------------------------------------------------------------------------------
// host-side launchers used by eepacc_capi.cpp
namespace eepacc {

// working-set tables: rigid rows are linearly independent, so m <= N (+ terminal rows) and the tables hold N + 2 rows.
// The capacity the solvers accept is schur_capacity<MMAX>() = min(MMAX, 64): the working-set linear algebra handles one
// row per lane (eepacc_schur.h), so at N = 63 a working set of 65 rows is refused as an overflow, like one above MMAX.
constexpr int kMMaxSmall = 34, kNSSmall = 32;     // N <= 32: 8 waves / CU (4 per block, 2 blocks)
constexpr int kBlocksSmall = 2;
// N <= 63: 44.6 KB of LDS per wave (He packed 16.6 KB, P 17.7 KB), 3 waves per CU (round 2: a full He of 32 KB allowed 2).
// Trading working-set capacity for more does not work: with a capacity of 50 rigid rows the S2 workload at N = 60
// overflows the working set on 15 % of the steps (measured), so the tables stay at N + 2 (capacity 64, see above).
constexpr int kMMaxLarge = 66, kNSLarge = 64, kWpbLarge = 3;
constexpr int kChunkStepsDefault = nomb::kChunkStepsDefault;

#ifdef EEPACC_AB_TIMING
extern "C" int eepacc_debug_ab_prof(unsigned long long* out, int reset) {
    unsigned long long z[24] = {0};
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(nomb::g_ab_prof), sizeof(z)) != hipSuccess) return -1;
    if (reset && hipMemcpyToSymbol(HIP_SYMBOL(nomb::g_ab_prof), z, sizeof(z)) != hipSuccess) return -1;
    return 0;
}
#endif

size_t ab_smem_bytes(int N) {
    return N <= kNSSmall ? nomb::wave_bytes(sizeof(nomb::WaveMem<kMMaxSmall, kNSSmall>), kNSSmall) * 4
                         : nomb::wave_bytes(sizeof(nomb::WaveMem<kMMaxLarge, kNSLarge>), kNSLarge) * kWpbLarge;
}

// the kernel of the handle's variant, small or large horizon; a kernel with one parameter more than the launch has
// arguments is a class kernel (eepacc_ab_impl.inc, cfg_of) and gets the class map as its last.  The est and blest kernels
// have three more, the clsest and blclsest kernels four: no handle has those variants, and launch_est below gives them
// theirs (est for a plain handle, blest for one of the baseline controller, clsest and blclsest for the class handles of
// the two, with the class map in front of est's arguments).
template <class... P, class... A>
static void launch_ab(void (*kernel)(P...), int grid, int block, size_t smem, hipStream_t stream, const int32_t* class_of, A... args) {
    if constexpr (sizeof...(P) == sizeof...(A) + 1) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), smem, stream, args..., class_of);
    else if constexpr (sizeof...(P) == sizeof...(A)) hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), smem, stream, args...);
}
template <class K, class... A>
static void launch_est(K kernel, int grid, int wpb, int N, hipStream_t stream, A... args) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(64 * wpb), ab_smem_bytes(N), stream, args...);
}
#define EEPACC_LAUNCH_CASE(E, NSP, MB, BL, TV, ICE, CLS, EST, KERNEL, MM, NSV, WPB, GRID, ...)                          \
    case AbVariant::E: launch_ab(NSP::KERNEL<MM, NSV, WPB>(), GRID, 64 * WPB, ab_smem_bytes(N), stream, class_of, __VA_ARGS__); break;
#define EEPACC_LAUNCH(KERNEL, MM, NSV, WPB, GRID, ...)                                                        \
    do { switch (variant) { EEPACC_AB_VARIANTS(EEPACC_LAUNCH_CASE, KERNEL, MM, NSV, WPB, GRID, __VA_ARGS__) } } while (0)

// MPC steps per work unit of the closed-loop kernels: 16 (EEPACC_CHUNK overrides), fewer when the launch is so short
// that the resident waves would otherwise get fewer than about eight units each (tail imbalance)
int pick_chunk_steps(int n_steps, int B, int resident_waves) {
    static int forced = -1;
    if (forced < 0) {
        const char* ev = getenv("EEPACC_CHUNK");
        forced = (ev && atoi(ev) > 0) ? atoi(ev) : 0;
    }
    if (forced > 0) return forced;
    long long per = ((long long)n_steps * B) / (8LL * (resident_waves > 0 ? resident_waves : 1));
    int c = per > kChunkStepsDefault ? kChunkStepsDefault : (int)per;
    return c < 2 ? 2 : c;
}

// per-wave scratch of the ICE variant (base inverse of the step): one NS x NS block for every wave a launch can have
// (the kernels index it by blockIdx.x * WPB + wave: k_ab_step has ceil(B / WPB) blocks, k_run_abmpc at most one
// chip-filling wave of blocks, see launch_run_abmpc)
size_t ab_hb_doubles(int N, int B, int num_cus) {
    const bool large = N > kNSSmall;
    const size_t wpb = large ? kWpbLarge : 4, ns = large ? kNSLarge : kNSSmall;
    const size_t step_waves = (size_t)((B + wpb - 1) / wpb) * wpb, run_waves = (size_t)num_cus * (large ? 1 : kBlocksSmall) * wpb;
    return (step_waves > run_waves ? step_waves : run_waves) * ns * ns;
}

hipError_t launch_ab_step(const DevCfg* dC, const int32_t* class_of, int N, AbVariant variant, int B, const double* s, const double* v,
                          const double* a_prev, const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                          unsigned long long* codes, double* out, double* s_pred, double* v_pred,
                          int32_t* status, int32_t* iters, hipStream_t stream, const AbSupplied* sup) {
    if (sup) {
        const bool bl = variant == AbVariant::Baseline || variant == AbVariant::ClassesBL;
#define EEPACC_EST_STEP(NSP, MM, NSV, WPB, ...) launch_est(NSP::step_kernel<MM, NSV, WPB>(), (B + WPB - 1) / WPB, WPB, N, stream, dC, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, codes, out, s_pred, v_pred, status, iters, __VA_ARGS__)
#define EEPACC_EST_STEP_SIZE(MM, NSV, WPB)                                                                                  \
        do {                                                                                                                 \
            if (class_of) { if (bl) EEPACC_EST_STEP(blclsest, MM, NSV, WPB, class_of, sup->s_est, sup->v_est, sup->s_tv_est); \
                            else EEPACC_EST_STEP(clsest, MM, NSV, WPB, class_of, sup->s_est, sup->v_est, sup->s_tv_est); }    \
            else if (bl) EEPACC_EST_STEP(blest, MM, NSV, WPB, sup->s_est, sup->v_est, sup->s_tv_est);                        \
            else EEPACC_EST_STEP(est, MM, NSV, WPB, sup->s_est, sup->v_est, sup->s_tv_est);                                  \
        } while (0)
        if (N > kNSSmall) EEPACC_EST_STEP_SIZE(kMMaxLarge, kNSLarge, kWpbLarge);
        else EEPACC_EST_STEP_SIZE(kMMaxSmall, kNSSmall, 4);
#undef EEPACC_EST_STEP_SIZE
#undef EEPACC_EST_STEP
        return hipGetLastError();
    }
    if (N > kNSSmall) EEPACC_LAUNCH(step_kernel, kMMaxLarge, kNSLarge, kWpbLarge, (B + kWpbLarge - 1) / kWpbLarge, dC, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, codes, out, s_pred, v_pred, status, iters);
    else EEPACC_LAUNCH(step_kernel, kMMaxSmall, kNSSmall, 4, (B + 3) / 4, dC, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, codes, out, s_pred, v_pred, status, iters);
    return hipGetLastError();
}

hipError_t launch_run_abmpc(const DevCfg* dC, const int32_t* class_of, int N, AbVariant variant, int B, int k_start, int n_steps,
                            const double* s0, const double* v0, const double* a_m1, const double* s_tv, const double* v_tv,
                            double* carry, unsigned long long* codes, double* traj,
                            int32_t* status, int32_t* iters_total, int* work_counter, int* done, int* err_word, int num_cus,
                            hipStream_t stream, const AbPreview* pv) {
    const bool large = N > kNSSmall;
    const int kChunkSteps = pick_chunk_steps(n_steps, B, num_cus * (large ? kWpbLarge : 4 * kBlocksSmall));
    // one chip-filling wave of blocks: LDS admits 8 (small) / 3 (large) waves per CU
    UnitsLaunch ul;
    hipError_t e = begin_units(work_counter, done, iters_total, B, n_steps, kChunkSteps, large ? kWpbLarge : 4,
                               num_cus * (large ? 1 : kBlocksSmall), stream, ul);
    if (e != hipSuccess) return e;
    if (pv) {
        const bool bl = variant == AbVariant::Baseline || variant == AbVariant::ClassesBL;
#define EEPACC_EST_RUN(NSP, MM, NSV, WPB, ...) launch_est(NSP::run_kernel<MM, NSV, WPB>(), ul.grid, WPB, N, stream, dC, B, k_start, n_steps, s0, v0, a_m1, s_tv, v_tv, carry, codes, traj, status, iters_total, work_counter, done, kChunkSteps, err_word, ul.spin_limit, __VA_ARGS__)
#define EEPACC_EST_RUN_SIZE(MM, NSV, WPB)                                                                       \
        do {                                                                                                     \
            if (class_of) { if (bl) EEPACC_EST_RUN(blclsest, MM, NSV, WPB, class_of, pv->idx, pv->frac, pv->n_lead); \
                            else EEPACC_EST_RUN(clsest, MM, NSV, WPB, class_of, pv->idx, pv->frac, pv->n_lead); }    \
            else if (bl) EEPACC_EST_RUN(blest, MM, NSV, WPB, pv->idx, pv->frac, pv->n_lead);                     \
            else EEPACC_EST_RUN(est, MM, NSV, WPB, pv->idx, pv->frac, pv->n_lead);                               \
        } while (0)
        if (large) EEPACC_EST_RUN_SIZE(kMMaxLarge, kNSLarge, kWpbLarge);
        else EEPACC_EST_RUN_SIZE(kMMaxSmall, kNSSmall, 4);
#undef EEPACC_EST_RUN_SIZE
#undef EEPACC_EST_RUN
        return hipGetLastError();
    }
    if (large)
        EEPACC_LAUNCH(run_kernel, kMMaxLarge, kNSLarge, kWpbLarge, ul.grid, dC, B, k_start, n_steps, s0, v0, a_m1, s_tv, v_tv, carry, codes, traj, status, iters_total, work_counter, done, kChunkSteps, err_word, ul.spin_limit);
    else
        EEPACC_LAUNCH(run_kernel, kMMaxSmall, kNSSmall, 4, ul.grid, dC, B, k_start, n_steps, s0, v0, a_m1, s_tv, v_tv, carry, codes, traj, status, iters_total, work_counter, done, kChunkSteps, err_word, ul.spin_limit);
    return hipGetLastError();
}

// A10: post-processing (ABO/RunOpt_ABMPC.m:343-349), one thread per instance, sequential in time.  kClasses: Cp is the
// class array of the handle and every instance reads the vehicle and the power fit of its own class.
template <bool kClasses>
__global__ void k_postprocess(const DevCfg* __restrict__ Cp, int B, int n_steps, const double* __restrict__ traj,
                              double* __restrict__ rpm, double* __restrict__ Tm, double* __restrict__ P,
                              double* __restrict__ E, const int32_t* __restrict__ class_of) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const DevCfg& C = kClasses ? Cp[class_of[b]] : *Cp;
    const double Ts = C.Tvec[0];
    double acc = 0.0;
    const double kr = (30.0 / 3.14159265358979323846);
    for (int k = 0; k < n_steps; ++k) {
        const double v = traj[((size_t)k * EEPACC_OUT_N + EEPACC_OUT_V) * B + b];
        const double x = traj[((size_t)k * EEPACC_OUT_N + EEPACC_OUT_FM) * B + b];
        const double y = kr * v * C.phi;
        const double sg = (x > 0.0) ? 1.0 : ((x < 0.0) ? -1.0 : 0.0);
        const double tm = x / C.phi / pow(C.eta_TF, sg);
        const double* bb = C.b5;
        const double x2 = x * x, x3 = x2 * x, x4 = x3 * x, x5 = x4 * x;
        const double y2 = y * y, y3 = y2 * y, y4 = y3 * y, y5 = y4 * y;
        const double p = bb[0] + bb[1] * x + bb[2] * y + bb[3] * x2 + bb[4] * x * y + bb[5] * y2 + bb[6] * x3 +
                         bb[7] * x2 * y + bb[8] * x * y2 + bb[9] * y3 + bb[10] * x4 + bb[11] * x3 * y +
                         bb[12] * x2 * y2 + bb[13] * x * y3 + bb[14] * y4 + bb[15] * x5 + bb[16] * x4 * y +
                         bb[17] * x3 * y2 + bb[18] * x2 * y3 + bb[19] * x * y4 + bb[20] * y5;
        acc += p;
        const size_t o = (size_t)k * B + b;
        rpm[o] = y; Tm[o] = tm; P[o] = p; E[o] = Ts * acc;
    }
}

hipError_t launch_postprocess(const DevCfg* dC, const int32_t* class_of, int B, int n_steps, const double* traj, double* rpm,
                              double* Tm, double* P, double* E, hipStream_t stream) {
    if (class_of) hipLaunchKernelGGL(k_postprocess<true>, dim3((B + 127) / 128), dim3(128), 0, stream, dC, B, n_steps, traj, rpm, Tm, P, E, class_of);
    else hipLaunchKernelGGL(k_postprocess<false>, dim3((B + 127) / 128), dim3(128), 0, stream, dC, B, n_steps, traj, rpm, Tm, P, E, class_of);
    return hipGetLastError();
}

// 160 KB of LDS per CU minus the kernel's static index table (one ushort per packed entry of P)
template <int MM, class K>
static hipError_t raise_smem(hipError_t e, K* kernel) {
    const int dyn = 160 * 1024 - ((MM * (MM + 1) / 2 * 2 + 255) & ~255);
    return e != hipSuccess ? e : hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, dyn);
}
#define EEPACC_RAISE_SMEM(E, NSP, MB, BL, TV, ICE, CLS, EST, MM, NSV, WPB) \
    e = raise_smem<MM>(e, NSP::step_kernel<MM, NSV, WPB>()); e = raise_smem<MM>(e, NSP::run_kernel<MM, NSV, WPB>());
hipError_t set_max_smem() {
    hipError_t e = hipSuccess;
    EEPACC_AB_VARIANTS(EEPACC_RAISE_SMEM, kMMaxSmall, kNSSmall, 4)
    EEPACC_AB_VARIANTS(EEPACC_RAISE_SMEM, kMMaxLarge, kNSLarge, kWpbLarge)
    return e;
}

}  // namespace eepacc
