// eepacc_capi.cpp -- C-ABI of libeepacc (include/eepacc.h): handle management, argument checks, kernel launches.  The
// translation of the reference settings (validation, one-time host precomputation) is eepacc_cfg.cpp.  Compiled with hipcc.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <string>
#include <vector>
#include <memory>
#include "eepacc_device.h"
#include "eepacc_cfg.h"
#include "eepacc_ab.h"
#include "eepacc_ab_build.h"
#include "eepacc_bl_qp.h"
#include "eepacc_qp_dense.h"
#include "eepacc_fb.h"
#include "eepacc_fb_qp.h"
#include "eepacc_fb_rows.h"
#include "eepacc_fbs.h"
#include "eepacc_kpis.h"
#include "eepacc_follow.h"
#include "eepacc_route.h"
#include "../../include/eepacc.h"

using eepacc::DevCfg;
using eepacc::KpiCfg;
using eepacc::FollowCfg;
using eepacc::RouteCfg;

static thread_local std::string g_err;
static int fail(int code, const std::string& msg) { g_err = msg; return code; }
namespace eepacc { int set_error(int code, const std::string& msg) { return fail(code, msg); } }   // other translation units (eepacc_cfg.cpp, eepacc_nlp.hip)
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(EEPACC_EDEVICE, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

// Device memory owned by a handle or by a host-pointer wrapper: move-only, freed with its owner.
template <class T> struct DevMem {
    T* p = nullptr;
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p(o.p) { o.p = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { release(); p = o.p; o.p = nullptr; } return *this; }
    ~DevMem() { release(); }
    void release() { if (p) (void)hipFree(p); p = nullptr; }
    hipError_t alloc(size_t n) { release(); return hipMalloc(&p, n * sizeof(T)); }
    hipError_t alloc_zero(size_t n) { const hipError_t e = alloc(n); return e != hipSuccess ? e : hipMemset(p, 0, n * sizeof(T)); }
    operator T*() const { return p; }
};

// dense FBMPC path (eepacc_fb.hip + the dense QP operator): buffers for B instances, allocated on first use
struct FbDense {
    int B = 0, chunk = 0;
    int steps_B = 0;                                       // B of the steps that wrote A22, D2, sp, vp: their stride (<= B)
    DevMem<double> H, g, A, lba, uba;                      // [chunk]
    DevMem<double> x, x0, cost, meas, carry, A22, D2;      // [B]
    DevMem<double> sp, vp;                                 // [N+1][B] predictions of the last step
    DevMem<int32_t> qpstat;
    DevMem<int> rhok;                                      // [B] regularisation exponent found at the previous step
};

struct eepacc_handle {
    int device = 0;
    int max_batch = 0;
    DevCfg cfg;
    DevMem<DevCfg> d_cfg;
    DevMem<double> d_Hinv;
    DevMem<double> d_hb;                     // ICE variant: per-wave base inverse of the step
    DevMem<double> d_pred;                   // [max_batch][2][64] previous predictions (paramEstSetting 2)
    DevMem<unsigned long long> d_codes;      // [max_batch][64]
    DevMem<int32_t> d_iters;                 // [max_batch]
    DevMem<double> d_carry;                  // [6][B] closed-loop carry (see Carry, eepacc_units.h)
    DevMem<int> d_counter;                   // work counter of the closed-loop kernel
    DevMem<int> d_done;                      // [max_batch] chunks finished per instance
    DevMem<int> d_err;                       // sticky device error word (bit 0: a closed-loop hand-off timed out)
    int num_cus = 256;
    // Resume bookkeeping.  ABMPC / TVMPC resume on k_done / carry_B.  FBMPC resumes on fb_k_done and compares B with last_B,
    // which every step and closed-loop entry point writes, the ABMPC ones included: an ABMPC call between two FBMPC launches
    // changes what the FBMPC resume check sees.
    int last_B = 0;
    int k_done = 0;                          // closed-loop steps already run since the last reset
    int carry_B = 0;
    DevMem<double> d_qp_ws;                  // workspace of the dense QP operator
    size_t qp_ws_doubles = 0;
    DevMem<int> d_qp_counter;
    int fb_k_done = 0;
    bool fb_by_step = false;                 // the FB step counter was advanced by eepacc_fb_step (no closed-loop carry to resume from)
    FbDense fb;
    // structured FBMPC path (eepacc_fbs.hip): per-instance state, closed-loop carry, base-inverse scratch
    bool fbs = false;                        // settings are covered by the structured solver
    DevMem<double> fbs_state, fbs_carry, fbs_hb;
    // The same on a handle of eepacc_create_classes (eepacc_fbs_cls.hip: eepacc_classes_fb_step, eepacc_run_classes_fbmpc), where
    // every class is covered and the horizon fits: fbs stays false there, since eepacc_fb_step / eepacc_run_fbmpc refuse class handles
    bool fbs_cls = false;
    std::vector<const char*> fb_unsup;       // [n_classes] eepacc::fbs_unsupported_field of every class (bl_mode = 0 classes only)
    // Settings classes (eepacc_create_classes): d_cfg holds DevCfg[n_classes], d_Hinv one N x N block per class and cfg is
    // class 0, whose N and Tvec every class shares.  n_classes = 0 marks a handle of eepacc_create.
    int n_classes = 0;
    DevMem<int32_t> d_class_of;              // [max_batch] class of every instance
    int classes_B = 0;                       // B of the last eepacc_set_classes (0: none yet)
    std::vector<eepacc::QpRowsCfg> qp_rows;  // [n_classes] what the row catalogue of eepacc_classes_build_qp reads of every class
    // key figures (eepacc_kpis): what they read of every class, and the cut-off distances of the call in flight
    DevMem<KpiCfg> d_kpi;                    // [max(n_classes, 1)]
    DevMem<double> d_kpi_cut;                // [max(n_classes, 1)]
    DevMem<FollowCfg> d_follow;              // [max(n_classes, 1)] what eepacc_follow_kpis reads of every class
    DevMem<RouteCfg> d_route;                // [max(n_classes, 1)] what eepacc_route_kpis reads of every class
    // eepacc_run_abmpc_preview: where stage k looks into the lead trace (eepacc::preview_tables), made at the first call
    DevMem<int32_t> d_pv_idx;                // [N]
    DevMem<double> d_pv_frac;                // [N]
    // a class handle's kernels follow from the controller its classes share (eepacc_create_classes: ABMPC, _classes_bl: bl_mode 1 or 2)
    eepacc::AbVariant variant() const {
        if (!n_classes) return eepacc::ab_variant(cfg);
        return cfg.bl_mode == 0 ? eepacc::AbVariant::Classes : cfg.bl_mode == 2 ? eepacc::AbVariant::ClassesTV : eepacc::AbVariant::ClassesBL;
    }
    const int32_t* class_map() const { return n_classes ? d_class_of.p : nullptr; }
};

extern "C" const char* eepacc_last_error(void) { return g_err.c_str(); }
extern "C" int eepacc_version(void) { return EEPACC_VERSION; }
extern "C" int eepacc_sizeof_settings(void) { return (int)sizeof(eepacc_settings); }
extern "C" int eepacc_sizeof_vehicle(void) { return (int)sizeof(eepacc_vehicle); }

// The settings as the kernels read them: eepacc::build_cfg (eepacc_cfg.cpp, host only), then the one refusal that needs the
// kernels' own LDS layout.
static int build_cfg_fit(const eepacc_settings* S, const eepacc_vehicle* V, DevCfg& C, std::vector<double>& Hinv) {
    if (const int rc = eepacc::build_cfg(S, V, C, Hinv)) return rc;
    if (eepacc::ab_smem_bytes(C.N) > 157 * 1024)
        return fail(EEPACC_ENOTSUP, "N_hor too large for the LDS layout of this build");
    return EEPACC_OK;
}
using eepacc::build_kpi_cfg;
using eepacc::build_follow_cfg;
using eepacc::build_route_cfg;

// The device side of a handle.  Cs: one validated DevCfg per class with its inverse Hessian in Hinv (N x N each, class after
// class); classes: the handle of eepacc_create_classes, which keeps a class map and runs AbVariant::Classes, also with one class.
static int create_on_device(eepacc_handle** out, std::vector<DevCfg>& Cs, const std::vector<double>& Hinv,
                            const std::vector<KpiCfg>& Ks, const std::vector<FollowCfg>& Fs, const std::vector<RouteCfg>& Rs,
                            bool classes, int device, int max_batch) {
    DevCfg& C = Cs[0];
    int ndev = 0;
    HIPCHK(hipGetDeviceCount(&ndev));
    if (ndev < 1) return fail(EEPACC_EDEVICE, "no HIP device: libeepacc has no CPU path");
    if (device < 0 || device >= ndev) return fail(EEPACC_EINVAL, "device ordinal out of range");
    HIPCHK(hipSetDevice(device));
    // the handle owns its device memory: everything allocated so far is freed if any later step fails
    std::unique_ptr<eepacc_handle> h(new eepacc_handle());
    h->device = device; h->max_batch = max_batch;
    const size_t nB = (size_t)max_batch;
    HIPCHK(h->d_Hinv.alloc(Hinv.size()));
    HIPCHK(hipMemcpy(h->d_Hinv, Hinv.data(), Hinv.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h->d_pred.alloc_zero(nB * 128));
    for (size_t k = 0; k < Cs.size(); ++k) {                // pred is indexed by instance: one buffer for all classes
        Cs[k].Hinv = h->d_Hinv + k * (size_t)C.N * C.N;
        Cs[k].pred = h->d_pred;
    }
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device));
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (C.ab_fuel_term == 2 && !C.bl_mode) {
        HIPCHK(h->d_hb.alloc(eepacc::ab_hb_doubles(C.N, max_batch, h->num_cus)));
        C.hb = h->d_hb;
    }
    h->cfg = C;
    HIPCHK(h->d_cfg.alloc(Cs.size()));
    HIPCHK(hipMemcpy(h->d_cfg, Cs.data(), Cs.size() * sizeof(DevCfg), hipMemcpyHostToDevice));
    HIPCHK(h->d_kpi.alloc(Ks.size()));
    HIPCHK(hipMemcpy(h->d_kpi, Ks.data(), Ks.size() * sizeof(KpiCfg), hipMemcpyHostToDevice));
    HIPCHK(h->d_kpi_cut.alloc_zero(Ks.size()));
    HIPCHK(h->d_follow.alloc(Fs.size()));
    HIPCHK(hipMemcpy(h->d_follow, Fs.data(), Fs.size() * sizeof(FollowCfg), hipMemcpyHostToDevice));
    HIPCHK(h->d_route.alloc(Rs.size()));
    HIPCHK(hipMemcpy(h->d_route, Rs.data(), Rs.size() * sizeof(RouteCfg), hipMemcpyHostToDevice));
    if (classes) {
        h->n_classes = (int)Cs.size();
        for (const DevCfg& Ck : Cs) h->qp_rows.push_back(eepacc::qp_rows_cfg(Ck));
        HIPCHK(h->d_class_of.alloc_zero(nB));
    }
    HIPCHK(h->d_codes.alloc_zero(nB * 64));
    HIPCHK(h->d_iters.alloc_zero(nB));
    HIPCHK(h->d_carry.alloc_zero(nB * 6));
    HIPCHK(h->d_counter.alloc(1));
    HIPCHK(h->d_done.alloc(nB));
    HIPCHK(h->d_err.alloc_zero(1));
    HIPCHK(h->d_qp_counter.alloc(1));
    HIPCHK(eepacc::set_max_smem());
    // FBMPC: structured kernels unless the settings need the dense path (or EEPACC_FB_DENSE=1 asks for it)
    h->fbs = !classes && eepacc::fbs_supported(C) && eepacc::fbs_smem_bytes(C.N) <= 160 * 1024 - 4608;
    if (const char* e = getenv("EEPACC_FB_DENSE")) if (atoi(e) != 0) h->fbs = false;
    if (classes && C.bl_mode == 0) {
        h->fbs_cls = eepacc::fbs_smem_bytes(C.N) <= eepacc::kFbsLdsBudget;
        for (const DevCfg& Ck : Cs) {
            h->fb_unsup.push_back(eepacc::fbs_unsupported_field(Ck));
            if (h->fb_unsup.back()) h->fbs_cls = false;
        }
    }
    if (h->fbs || h->fbs_cls) {
        HIPCHK(eepacc::fbs_set_max_smem());
        HIPCHK(h->fbs_state.alloc_zero(nB * eepacc::kFbsStateDoubles));
        HIPCHK(h->fbs_carry.alloc_zero(nB * 6));
        HIPCHK(h->fbs_hb.alloc(eepacc::fbs_hb_doubles(C.N, max_batch, h->num_cus)));
    }
    *out = h.release();
    return EEPACC_OK;
}

extern "C" int eepacc_create(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                             int device, int max_batch) {
    if (!out || !S || !V || max_batch < 1) return fail(EEPACC_EINVAL, "eepacc_create: bad arguments");
    *out = nullptr;
    std::vector<DevCfg> Cs(1);
    std::vector<double> Hinv;
    int rc = build_cfg_fit(S, V, Cs[0], Hinv);
    if (rc != EEPACC_OK) return rc;
    return create_on_device(out, Cs, Hinv, {build_kpi_cfg(S, V)}, {build_follow_cfg(S, V)}, {build_route_cfg(S, V)}, false, device, max_batch);
}

// Every class is checked like the settings of eepacc_create, and against class 0 in what selects the kernel and the launch
// geometry, before the device is touched.  The two creation entries share this body: entry names the caller in the messages,
// baseline says which controllers its classes hold (false: ABMPC, bl_mode = 0 in every class; true: bl_mode = 1 in every class
// or 2 in every class).
static int create_classes_impl(const std::string& entry, bool baseline, eepacc_handle** out, const eepacc_settings* S,
                               const eepacc_vehicle* V, int n_classes, int device, int max_batch) {
    if (!out || !S || !V || max_batch < 1) return fail(EEPACC_EINVAL, entry + ": bad arguments");
    *out = nullptr;
    if (n_classes < 1 || n_classes > EEPACC_MAX_CLASSES)
        return fail(EEPACC_EINVAL, entry + ": n_classes must be in [1, " + std::to_string(EEPACC_MAX_CLASSES) + "]");
    const int N = S[0].N_hor;
    if (N < 2 || N > eepacc::kMaxN) return fail(EEPACC_EINVAL, entry + ": class 0: N_hor must be in [2, 63]");
    if (baseline && S[0].bl_mode != 1 && S[0].bl_mode != 2)
        return fail(EEPACC_EINVAL, entry + ": class 0: bl_mode = " + std::to_string(S[0].bl_mode) + " must be 1 (RunOpt_BLMPC) or 2 (RunOpt_TVMPC); eepacc_create_classes takes ABMPC classes (bl_mode = 0)");
    std::vector<DevCfg> Cs((size_t)n_classes);
    std::vector<double> Hinv, Hk;
    std::vector<KpiCfg> Ks;
    std::vector<FollowCfg> Fs;
    std::vector<RouteCfg> Rs;
    for (int k = 0; k < n_classes; ++k) {
        const std::string who = entry + ": class " + std::to_string(k) + ": ";
        if (S[k].N_hor != N)
            return fail(EEPACC_EINVAL, who + "N_hor = " + std::to_string(S[k].N_hor) + " differs from class 0 (" + std::to_string(N) + "); the classes of a handle share the horizon");
        if (baseline) {
            if (S[k].bl_mode != S[0].bl_mode)
                return fail(EEPACC_EINVAL, who + "bl_mode = " + std::to_string(S[k].bl_mode) + " differs from class 0 (" + std::to_string(S[0].bl_mode) + "); the classes of a handle share the controller");
        } else {
            if (S[k].bl_mode != 0) return fail(EEPACC_ENOTSUP, who + "bl_mode != 0: the baseline and target-vehicle controllers have no class variant here; eepacc_create_classes_bl takes their classes");
            if (S[k].ab_fuel_term == 2) return fail(EEPACC_ENOTSUP, who + "ab_fuel_term == 2: the ICE-map fuel term has no class variant");
            if (S[k].Mb)
                for (int j = 0; j < N; ++j)
                    if (S[k].Mb[j] != 0) return fail(EEPACC_ENOTSUP, who + "Mb[" + std::to_string(j) + "] != 0: move blocking has no class variant");
        }
        const int rc = build_cfg_fit(&S[k], &V[k], Cs[(size_t)k], Hk);
        if (rc != EEPACC_OK) return fail(rc, who + g_err);
        for (int j = 0; j < N; ++j)
            if (Cs[(size_t)k].Tvec[j] != Cs[0].Tvec[j])
                return fail(EEPACC_EINVAL, who + "Tvec[" + std::to_string(j) + "] differs from class 0; the classes of a handle share the time grid");
        Hinv.insert(Hinv.end(), Hk.begin(), Hk.end());
        Ks.push_back(build_kpi_cfg(&S[k], &V[k]));
        Fs.push_back(build_follow_cfg(&S[k], &V[k]));
        Rs.push_back(build_route_cfg(&S[k], &V[k]));
    }
    return create_on_device(out, Cs, Hinv, Ks, Fs, Rs, true, device, max_batch);
}

extern "C" int eepacc_create_classes(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                                     int n_classes, int device, int max_batch) {
    return create_classes_impl("eepacc_create_classes", false, out, S, V, n_classes, device, max_batch);
}
extern "C" int eepacc_create_classes_bl(eepacc_handle** out, const eepacc_settings* S, const eepacc_vehicle* V,
                                        int n_classes, int device, int max_batch) {
    return create_classes_impl("eepacc_create_classes_bl", true, out, S, V, n_classes, device, max_batch);
}

extern "C" int eepacc_num_classes(const eepacc_handle* h) { return h && h->n_classes ? h->n_classes : 1; }

extern "C" void eepacc_destroy(eepacc_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    delete h;
}

extern "C" int eepacc_reset(eepacc_handle* h) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipMemset(h->d_codes, 0, (size_t)h->max_batch * 64 * sizeof(unsigned long long)));
    HIPCHK(hipMemset(h->d_pred, 0, (size_t)h->max_batch * 128 * sizeof(double)));
    HIPCHK(hipMemset(h->d_err, 0, sizeof(int)));
    h->k_done = 0; h->carry_B = 0;
    h->fb_k_done = 0; h->fb_by_step = false;
    if (h->fbs_state) HIPCHK(hipMemset(h->fbs_state, 0, (size_t)h->max_batch * eepacc::kFbsStateDoubles * sizeof(double)));
    if (h->fb.x0) HIPCHK(hipMemset(h->fb.x0, 0, (size_t)h->fb.B * 6 * h->cfg.N * sizeof(double)));
    if (h->fb.sp) {
        HIPCHK(hipMemset(h->fb.sp, 0, (size_t)h->fb.B * (h->cfg.N + 1) * sizeof(double)));
        HIPCHK(hipMemset(h->fb.vp, 0, (size_t)h->fb.B * (h->cfg.N + 1) * sizeof(double)));
    }
    return EEPACC_OK;
}

extern "C" int eepacc_set_classes(eepacc_handle* h, int B, const int32_t* class_of_host) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    if (!h->n_classes) return fail(EEPACC_EINVAL, "eepacc_set_classes: this handle was not created by eepacc_create_classes");
    if (B < 1 || B > h->max_batch || !class_of_host) return fail(EEPACC_EINVAL, "eepacc_set_classes: B must be in [1, max_batch] and the map not NULL");
    for (int i = 0; i < B; ++i)
        if (class_of_host[i] < 0 || class_of_host[i] >= h->n_classes)
            return fail(EEPACC_EINVAL, "eepacc_set_classes: class_of[" + std::to_string(i) + "] = " + std::to_string(class_of_host[i]) +
                                       " is outside [0, " + std::to_string(h->n_classes) + ")");
    HIPCHK(hipSetDevice(h->device));
    // a launch in flight may still read the map, and the copy below does not wait for work on other streams
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->d_class_of, class_of_host, (size_t)B * sizeof(int32_t), hipMemcpyHostToDevice));
    h->classes_B = B;
    return eepacc_reset(h);
}

// A handle of eepacc_create_classes runs the ABMPC entry points only, one of eepacc_create_classes_bl those of its controller
// (BLMPC under both names, or TVMPC), and both only with the B their class map was set for.
// ab_classes_refused: the answer of a handle of eepacc_create_classes to an entry it does not run (every other handle passes);
// not_classes: the answer of any class handle, for the entries that no class handle runs (FBMPC, the dense QP operator).
static int ab_classes_refused(const eepacc_handle* h, const char* who) {
    if (h && h->n_classes && h->cfg.bl_mode == 0)
        return fail(EEPACC_ENOTSUP, std::string(who) + ": a handle of eepacc_create_classes runs ABMPC only (eepacc_ab_step, eepacc_run_abmpc, eepacc_run_abmpc_host)");
    return EEPACC_OK;
}
static int not_classes(const eepacc_handle* h, const char* who) {
    if (const int rc = ab_classes_refused(h, who)) return rc;
    if (h && h->n_classes)
        return fail(EEPACC_ENOTSUP, std::string(who) + ": a handle of eepacc_create_classes_bl runs the entry points of its controller only (" +
                                        (h->cfg.bl_mode == 2 ? "eepacc_tv_step, eepacc_run_tvmpc, eepacc_run_tvmpc_host)" : "eepacc_ab_step / eepacc_bl_step, eepacc_run_abmpc / eepacc_run_blmpc and their _host forms)"));
    return EEPACC_OK;
}
static int classes_ready(const eepacc_handle* h, const char* who, int B) {
    if (!h->n_classes || B == h->classes_B) return EEPACC_OK;
    if (!h->classes_B) return fail(EEPACC_EINVAL, std::string(who) + ": eepacc_set_classes has not been called on this handle");
    return fail(EEPACC_EINVAL, std::string(who) + ": B = " + std::to_string(B) + " differs from the B = " + std::to_string(h->classes_B) + " of the last eepacc_set_classes");
}

// The kind of a handle decides which entry points run it.  One created with bl_mode = 2 poses RunOpt_TVMPC's problem and takes
// no lead inputs: only eepacc_tv_step / eepacc_run_tvmpc* run it (need_tv), every other one refuses it (not_tv).  The
// eepacc_bl_* names are the ABMPC entry points for a handle that was created as the baseline controller (need_bl).
static int not_tv(const eepacc_handle* h, const char* who) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    if (h->cfg.bl_mode == 2)
        return fail(EEPACC_EINVAL, std::string(who) + ": this handle was created with bl_mode = 2 (RunOpt_TVMPC); use eepacc_tv_step / eepacc_run_tvmpc");
    return EEPACC_OK;
}
static int need_mode(const eepacc_handle* h, int bl_mode, const char* name) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    if (h->cfg.bl_mode != bl_mode)
        return fail(EEPACC_EINVAL, "this handle was not created with bl_mode = " + std::to_string(bl_mode) + " (" + name + ")");
    return EEPACC_OK;
}
// (a handle of eepacc_create_classes holds ABMPC classes: not served, as before; one of eepacc_create_classes_bl answers by its mode)
static int need_bl(const eepacc_handle* h) { const int rc = ab_classes_refused(h, "eepacc_bl_step / eepacc_run_blmpc"); return rc ? rc : need_mode(h, 1, "RunOpt_BLMPC"); }
static int need_tv(const eepacc_handle* h) { const int rc = ab_classes_refused(h, "eepacc_tv_step / eepacc_run_tvmpc"); return rc ? rc : need_mode(h, 2, "RunOpt_TVMPC"); }

// One step of the ABMPC kernels of the handle's variant.  A target-vehicle handle has no lead inputs: its kernels read none
// and the launcher gets null pointers.
static int ab_step_impl(eepacc_handle* h, const char* who, int B, const double* s, const double* v, const double* a_prev,
                        const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                        double* out, double* s_pred, double* v_pred, int32_t* status, void* stream,
                        const eepacc::AbSupplied* sup = nullptr) {
    const bool tv = h->cfg.bl_mode == 2;
    if (B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "B exceeds max_batch of the handle");
    if (B == 0) return EEPACC_OK;
    if (!s || !v || !a_prev || !t0 || (!tv && (!s_tv || !v_tv || !a_tv_prev)) || !out || !status)
        return fail(EEPACC_EINVAL, std::string(who) + ": NULL buffer");
    if (const int rc = classes_ready(h, who, B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    h->last_B = B;
    HIPCHK(eepacc::launch_ab_step(h->d_cfg, h->class_map(), h->cfg.N, h->variant(), B, s, v, a_prev, t0, tv ? nullptr : s_tv,
                                  tv ? nullptr : v_tv, tv ? nullptr : a_tv_prev, h->d_codes, out, s_pred, v_pred, status,
                                  h->d_iters, (hipStream_t)stream, sup));
    return EEPACC_OK;
}

// The closed loop of the same kernels; bad_sizes is the entry point's own wording of that refusal.
static int ab_run_impl(eepacc_handle* h, const char* who, const char* bad_sizes, int B, int n_steps, const double* s0,
                       const double* v0, const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                       int32_t* status, void* stream, const eepacc::AbPreview* pv = nullptr) {
    const bool tv = h->cfg.bl_mode == 2;
    if (B < 0 || B > h->max_batch || n_steps < 0) return fail(EEPACC_EINVAL, bad_sizes);
    if (B == 0 || n_steps == 0) return EEPACC_OK;
    if (!s0 || !v0 || !a_minus1 || (!tv && (!s_tv || !v_tv)) || !traj || !status)
        return fail(EEPACC_EINVAL, std::string(who) + ": NULL buffer");
    if (const int rc = classes_ready(h, who, B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    if (h->k_done > 0 && h->carry_B != B)
        return fail(EEPACC_EINVAL, std::string(who) + ": B changed while resuming; call eepacc_reset first");
    h->last_B = B;
    HIPCHK(eepacc::launch_run_abmpc(h->d_cfg, h->class_map(), h->cfg.N, h->variant(), B, h->k_done, n_steps, s0, v0, a_minus1,
                                    tv ? nullptr : s_tv, tv ? nullptr : v_tv, h->d_carry, h->d_codes, traj, status, h->d_iters,
                                    h->d_counter, h->d_done, h->d_err, h->num_cus, (hipStream_t)stream, pv));
    h->k_done += n_steps; h->carry_B = B;
    return EEPACC_OK;
}

// eepacc_bl_step / eepacc_run_blmpc report as the ABMPC entry points they stand for
extern "C" int eepacc_ab_step(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                              const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                              double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    const int rc = not_tv(h, "eepacc_ab_step");
    return rc != EEPACC_OK ? rc : ab_step_impl(h, "eepacc_ab_step", B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, stream);
}
extern "C" int eepacc_bl_step(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                              const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                              double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    const int rc = need_bl(h);
    return rc != EEPACC_OK ? rc : ab_step_impl(h, "eepacc_ab_step", B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, stream);
}
extern "C" int eepacc_tv_step(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                              const double* t0, double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    const int rc = need_tv(h);
    return rc != EEPACC_OK ? rc : ab_step_impl(h, "eepacc_tv_step", B, s, v, a_prev, t0, nullptr, nullptr, nullptr, out, s_pred, v_pred, status, stream);
}

extern "C" int eepacc_run_abmpc(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                int32_t* status, void* stream) {
    const int rc = not_tv(h, "eepacc_run_abmpc");
    return rc != EEPACC_OK ? rc : ab_run_impl(h, "eepacc_run_abmpc", "bad B / n_steps", B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream);
}
extern "C" int eepacc_run_blmpc(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                int32_t* status, void* stream) {
    const int rc = need_bl(h);
    return rc != EEPACC_OK ? rc : ab_run_impl(h, "eepacc_run_abmpc", "bad B / n_steps", B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream);
}
extern "C" int eepacc_run_tvmpc(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                const double* a_minus1, double* traj, int32_t* status, void* stream) {
    const int rc = need_tv(h);
    return rc != EEPACC_OK ? rc : ab_run_impl(h, "eepacc_run_tvmpc", "eepacc_run_tvmpc: bad B / n_steps", B, n_steps, s0, v0, a_minus1, nullptr, nullptr, traj, status, stream);
}

// ---- horizon guesses from the caller: eepacc_ab_step_est, eepacc_ab_build_qp_est, eepacc_run_abmpc_preview run a plain ABMPC
// handle (AbVariant::Plain) through the est kernels, eepacc_bl_step_est, eepacc_bl_build_qp_est, eepacc_run_blmpc_preview a
// handle of the baseline controller (bl_mode = 1, AbVariant::Baseline) through the blest kernels: on the handle's own state.
// bl: the entry belongs to the baseline controller.  With settings classes: est_classes_handle below.
static int est_handle(const eepacc_handle* h, const std::string& who, bool bl = false) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    if (h->n_classes) return fail(EEPACC_ENOTSUP, who + ": a handle of eepacc_create_classes / eepacc_create_classes_bl has no variant with supplied horizon guesses");
    const std::string mode = ": the handle was created with bl_mode = " + std::to_string(h->cfg.bl_mode);
    if (h->cfg.bl_mode == 2)
        return fail(EEPACC_ENOTSUP, who + mode + " (RunOpt_TVMPC); the target-vehicle controller has no lead and hands its bounds a zero speed estimate, so supplied horizon guesses are not built for it");
    if (bl) {
        if (h->cfg.bl_mode == 0)
            return fail(EEPACC_ENOTSUP, who + mode + "; eepacc_ab_step_est, eepacc_ab_build_qp_est and eepacc_run_abmpc_preview take the supplied horizon guesses of an ABMPC handle");
        return EEPACC_OK;       // (the baseline kernels have neither move blocking nor the ICE-map fuel term: ab_variant)
    }
    if (h->cfg.bl_mode == 1)
        return fail(EEPACC_ENOTSUP, who + mode + " (RunOpt_BLMPC); eepacc_bl_step_est, eepacc_bl_build_qp_est and eepacc_run_blmpc_preview take the supplied horizon guesses of the baseline controller");
    for (int k = 0; k < h->cfg.N; ++k)
        if (h->cfg.mb_mask[k]) return fail(EEPACC_ENOTSUP, who + ": Mb[" + std::to_string(k) + "] != 0: move blocking has no variant with supplied horizon guesses");
    if (h->cfg.ab_fuel_term == 2) return fail(EEPACC_ENOTSUP, who + ": ab_fuel_term == 2: the ICE-map fuel term has no variant with supplied horizon guesses");
    return EEPACC_OK;
}
// eepacc_classes_step_est, eepacc_run_classes_preview: the same for a handle with settings classes, which decides the
// controller itself (eepacc_create_classes: the clsest kernels, eepacc_create_classes_bl with bl_mode = 1: blclsest).  The
// six entries above keep refusing class handles; these two refuse every other handle.
static int est_classes_handle(const eepacc_handle* h, const std::string& who) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    if (!h->n_classes) {
        const char* plain = h->cfg.bl_mode == 1 ? "eepacc_bl_step_est / eepacc_run_blmpc_preview run a handle of the baseline controller"
                          : h->cfg.bl_mode == 2 ? "the target-vehicle controller has no entry with supplied horizon guesses"
                                                : "eepacc_ab_step_est / eepacc_run_abmpc_preview run a plain ABMPC handle";
        return fail(EEPACC_ENOTSUP, who + ": this handle has no settings classes (it was created by eepacc_create with bl_mode = " +
                                        std::to_string(h->cfg.bl_mode) + "); " + plain);
    }
    if (h->cfg.bl_mode == 2)
        return fail(EEPACC_ENOTSUP, who + ": the classes of this handle were created with bl_mode = 2 (RunOpt_TVMPC); the target-vehicle controller has no lead and hands its bounds a zero speed estimate, so supplied horizon guesses are not built for it");
    return EEPACC_OK;       // (class handles have neither move blocking nor the ICE-map fuel term: create_classes_impl)
}
enum class EstEntry { Ab, Bl, Classes };
static int est_entry_handle(EstEntry entry, const eepacc_handle* h, const std::string& who) {
    return entry == EstEntry::Classes ? est_classes_handle(h, who) : est_handle(h, who, entry == EstEntry::Bl);
}
static int est_pair(const std::string& who, const double* s_est, const double* v_est) {
    if (s_est && !v_est) return fail(EEPACC_EINVAL, who + ": s_est is given without v_est; the two are given together or both NULL");
    if (v_est && !s_est) return fail(EEPACC_EINVAL, who + ": v_est is given without s_est; the two are given together or both NULL");
    return EEPACC_OK;
}

static int step_est_impl(EstEntry entry, const std::string& who, eepacc_handle* h, int B, const double* s, const double* v,
                         const double* a_prev, const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                         const double* s_est, const double* v_est, const double* s_tv_est,
                         double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    if (const int rc = est_entry_handle(entry, h, who)) return rc;
    if (B < 0 || B > h->max_batch)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    if (const int rc = est_pair(who, s_est, v_est)) return rc;
    const eepacc::AbSupplied sup{s_est, v_est, s_tv_est};
    return ab_step_impl(h, who.c_str(), B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, stream, &sup);
}
extern "C" int eepacc_ab_step_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                  const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  const double* s_est, const double* v_est, const double* s_tv_est,
                                  double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    return step_est_impl(EstEntry::Ab, "eepacc_ab_step_est", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, s_est, v_est, s_tv_est, out, s_pred, v_pred, status, stream);
}
extern "C" int eepacc_bl_step_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                  const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  const double* s_est, const double* v_est, const double* s_tv_est,
                                  double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    return step_est_impl(EstEntry::Bl, "eepacc_bl_step_est", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, s_est, v_est, s_tv_est, out, s_pred, v_pred, status, stream);
}
extern "C" int eepacc_classes_step_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                       const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                       const double* s_est, const double* v_est, const double* s_tv_est,
                                       double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    return step_est_impl(EstEntry::Classes, "eepacc_classes_step_est", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, s_est, v_est, s_tv_est, out, s_pred, v_pred, status, stream);
}

// The preview tables of the handle (eepacc::preview_tables), made at the first preview launch of any controller
static int preview_tables_ready(eepacc_handle* h) {
    if (h->d_pv_idx) return EEPACC_OK;
    const int N = h->cfg.N;
    std::vector<int32_t> idx((size_t)N);
    std::vector<double> frac((size_t)N);
    eepacc::preview_tables(h->cfg.Tvec, N, idx.data(), frac.data());        // (class handle: class 0's Tvec, which every class shares)
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(h->d_pv_frac.alloc((size_t)N));
    HIPCHK(hipMemcpy(h->d_pv_frac, frac.data(), (size_t)N * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(h->d_pv_idx.alloc((size_t)N));
    HIPCHK(hipMemcpy(h->d_pv_idx, idx.data(), (size_t)N * sizeof(int32_t), hipMemcpyHostToDevice));
    return EEPACC_OK;
}

static int run_preview_impl(EstEntry entry, const std::string& who, eepacc_handle* h, int B, int n_steps, int n_lead, const double* s0,
                            const double* v0, const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                            int32_t* status, void* stream) {
    if (const int rc = est_entry_handle(entry, h, who)) return rc;
    if (B < 0 || B > h->max_batch || n_steps < 0)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " must be in [0, max_batch = " + std::to_string(h->max_batch) + "] and n_steps = " + std::to_string(n_steps) + " not negative");
    if (n_lead < n_steps)
        return fail(EEPACC_EINVAL, who + ": n_lead = " + std::to_string(n_lead) + " is below n_steps = " + std::to_string(n_steps) + "; the lead traces hold at least the rows of the launch's steps");
    if (B == 0 || n_steps == 0) return EEPACC_OK;
    if (const int rc = preview_tables_ready(h)) return rc;
    const eepacc::AbPreview pv{h->d_pv_idx, h->d_pv_frac, n_lead};
    return ab_run_impl(h, who.c_str(), (who + ": bad B / n_steps").c_str(), B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream, &pv);
}
extern "C" int eepacc_run_abmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead, const double* s0, const double* v0,
                                        const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                        int32_t* status, void* stream) {
    return run_preview_impl(EstEntry::Ab, "eepacc_run_abmpc_preview", h, B, n_steps, n_lead, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream);
}
extern "C" int eepacc_run_blmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead, const double* s0, const double* v0,
                                        const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                        int32_t* status, void* stream) {
    return run_preview_impl(EstEntry::Bl, "eepacc_run_blmpc_preview", h, B, n_steps, n_lead, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream);
}
extern "C" int eepacc_run_classes_preview(eepacc_handle* h, int B, int n_steps, int n_lead, const double* s0, const double* v0,
                                          const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                          int32_t* status, void* stream) {
    return run_preview_impl(EstEntry::Classes, "eepacc_run_classes_preview", h, B, n_steps, n_lead, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream);
}

// ---- the condensed QP of a step as data: eepacc_{ab,fb,bl}_qp_size, _qp_rows, _build_qp.  What the three families do alike is
// written once, over a descriptor of the family.
struct QpFamily {
    const char* stem;                       // name stem of the three entry points
    const char* on_classes;                 // refusal of a handle of eepacc_create_classes
    bool bl_handle;                         // the family of a handle with bl_mode != 0 (else: of one with bl_mode = 0)
    const char* on_mode;                    // refusal of a handle of the other kind, after "... bl_mode = <n>"
    int nV_stage;                           // variables per stage
    int (*nC)(const DevCfg&);
    int n_types, safe1, safe2;              // row types of a stage; the two terminal rows
    bool (*present)(const DevCfg&, int type, int k);
    bool (*terminal_rows)(const DevCfg&);   // has terminal rows; the lead buffers are required with them
};

static const QpFamily kQpAB = {
    "eepacc_ab", ": a handle of eepacc_create_classes has no single problem size (nC can differ per class)", false,
    "; only the ABMPC problem (CreateQP_AB) is built here, eepacc_bl_build_qp builds the problem of such a handle",
    5, eepacc::ab_qp_num_rows, EEPACC_AB_ROW_N, EEPACC_AB_ROW_SAFE1, EEPACC_AB_ROW_SAFE2,
    [](const DevCfg& C, int t, int k) { return eepacc::ab_row_present(t, C.ab_route_rows, C.mb_mask[k]); },
    [](const DevCfg&) { return true; }};
// Only a handle of eepacc_create with bl_mode = 1 or 2 has the BLMPC / TVMPC problem.  TVMPC has no lead vehicle: no terminal
// rows, and the three lead arrays are not read
static const QpFamily kQpBL = {
    "eepacc_bl", ": a handle of eepacc_create_classes has no baseline or target-vehicle problem (its classes are ABMPC settings)", true,
    "; eepacc_ab_build_qp / eepacc_fb_build_qp build its problems, only the BLMPC and TVMPC problems (CreateQP_BL, CreateQP_TV) are built here",
    2, eepacc::bl_qp_num_rows, EEPACC_BL_ROW_N, EEPACC_BL_ROW_SAFE1, EEPACC_BL_ROW_SAFE2,
    [](const DevCfg& C, int t, int) { return eepacc::bl_row_present(t, C.bl_mode); },
    [](const DevCfg& C) { return C.bl_mode != 2; }};
static const QpFamily kQpFB = {
    "eepacc_fb", ": a handle of eepacc_create_classes runs ABMPC only and has no FBMPC problem", false,
    "; only the FBMPC problem (CreateQP_FB) is built here, eepacc_bl_build_qp builds the problem of such a handle",
    6, eepacc::fb_qp_num_rows, EEPACC_FB_ROW_N, EEPACC_FB_ROW_SAFE1, EEPACC_FB_ROW_SAFE2,
    [](const DevCfg& C, int t, int k) { return eepacc::fb_row_present(t, C.mb_mask[k]); },
    [](const DevCfg&) { return true; }};

static int qp_handle(const QpFamily& F, const eepacc_handle* h, const std::string& who) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    if (h->n_classes && h->cfg.bl_mode != 0)
        return fail(EEPACC_ENOTSUP, who + ": a handle of eepacc_create_classes_bl has no single problem to build (its classes have settings of their own)");
    if (h->n_classes) return fail(EEPACC_ENOTSUP, who + F.on_classes);
    if ((h->cfg.bl_mode != 0) != F.bl_handle)
        return fail(EEPACC_ENOTSUP, who + ": the handle was created with bl_mode = " + std::to_string(h->cfg.bl_mode) + F.on_mode);
    return EEPACC_OK;
}

static int qp_size_impl(const QpFamily& F, const eepacc_handle* h, int* nV, int* nC) {
    const std::string who = std::string(F.stem) + "_qp_size";
    if (const int rc = qp_handle(F, h, who)) return rc;
    if (!nV) return fail(EEPACC_EINVAL, who + ": nV is NULL");
    if (!nC) return fail(EEPACC_EINVAL, who + ": nC is NULL");
    *nV = F.nV_stage * h->cfg.N;
    *nC = F.nC(h->cfg);
    return EEPACC_OK;
}

static int qp_rows_impl(const QpFamily& F, const eepacc_handle* h, int32_t* stage, int32_t* type) {
    const std::string who = std::string(F.stem) + "_qp_rows";
    if (const int rc = qp_handle(F, h, who)) return rc;
    if (!stage) return fail(EEPACC_EINVAL, who + ": stage is NULL");
    if (!type) return fail(EEPACC_EINVAL, who + ": type is NULL");
    const DevCfg& C = h->cfg;
    int r = 0;
    for (int k = 0; k < C.N; ++k)
        for (int t = 0; t < F.n_types; ++t)
            if (F.present(C, t, k)) { stage[r] = k; type[r] = t; ++r; }
    if (F.terminal_rows(C)) {
        stage[r] = C.N; type[r] = F.safe1; ++r;
        stage[r] = C.N; type[r] = F.safe2; ++r;
    }
    return EEPACC_OK;
}

// The arguments every _build_qp has, in the order of its parameter list
struct QpBufs { const double *s, *v, *a_prev, *t0, *s_tv, *v_tv, *a_tv_prev, *H, *g, *A, *lba, *uba; };

// Handle, B range, NULL buffers.  *launch: there is something to build (B > 0)
static int build_args_check(const QpFamily& F, const eepacc_handle* h, int B, const QpBufs& b, bool* launch, const char* entry = nullptr) {
    const std::string who = entry ? std::string(entry) : std::string(F.stem) + "_build_qp";      // (entry: eepacc_fb_build_qp_est)
    *launch = false;
    if (const int rc = qp_handle(F, h, who)) return rc;
    if (B < 0 || B > h->max_batch)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    const bool lead = F.terminal_rows(h->cfg);
    const struct { const void* p; const char* name; bool needed; } bufs[] = {
        {b.s, "s", true}, {b.v, "v", true}, {b.a_prev, "a_prev", true}, {b.t0, "t0", true}, {b.s_tv, "s_tv", lead},
        {b.v_tv, "v_tv", lead}, {b.a_tv_prev, "a_tv_prev", lead}, {b.H, "H", true}, {b.g, "g", true}, {b.A, "A", true},
        {b.lba, "lba", true}, {b.uba, "uba", true}};
    for (const auto& bf : bufs)
        if (bf.needed && !bf.p) return fail(EEPACC_EINVAL, who + ": " + bf.name + " is NULL");
    *launch = true;
    return EEPACC_OK;
}

extern "C" int eepacc_ab_qp_size(const eepacc_handle* h, int* nV, int* nC) { return qp_size_impl(kQpAB, h, nV, nC); }
extern "C" int eepacc_ab_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type) { return qp_rows_impl(kQpAB, h, stage, type); }

extern "C" int eepacc_ab_build_qp(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                  const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    bool launch;
    if (const int rc = build_args_check(kQpAB, h, B, {s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, H, g, A, lba, uba}, &launch)) return rc;
    if (!launch) return EEPACC_OK;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(eepacc::launch_ab_build(h->d_cfg, h->cfg.N, eepacc::ab_qp_num_rows(h->cfg), B, s, v, a_prev, t0, s_tv, v_tv,
                                   a_tv_prev, H, g, A, lba, uba, (hipStream_t)stream));
    return EEPACC_OK;
}

static int build_qp_est_impl(bool bl, const std::string& who, eepacc_handle* h, int B, const double* s, const double* v,
                             const double* a_prev, const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                             const double* s_est, const double* v_est, const double* s_tv_est,
                             double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    if (const int rc = est_handle(h, who, bl)) return rc;
    if (B < 0 || B > h->max_batch)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    const struct { const void* p; const char* name; } bufs[] = {
        {s, "s"}, {v, "v"}, {a_prev, "a_prev"}, {t0, "t0"}, {s_tv, "s_tv"}, {v_tv, "v_tv"}, {a_tv_prev, "a_tv_prev"},
        {H, "H"}, {g, "g"}, {A, "A"}, {lba, "lba"}, {uba, "uba"}};
    for (const auto& bf : bufs)
        if (!bf.p) return fail(EEPACC_EINVAL, who + ": " + bf.name + " is NULL");
    if (const int rc = est_pair(who, s_est, v_est)) return rc;
    const eepacc::AbSupplied sup{s_est, v_est, s_tv_est};
    HIPCHK(hipSetDevice(h->device));
    if (bl)
        HIPCHK(eepacc::launch_bl_qp_est(h->d_cfg, h->cfg.N, eepacc::bl_qp_num_rows(h->cfg), B, s, v, a_prev, t0, s_tv, v_tv,
                                        a_tv_prev, H, g, A, lba, uba, (hipStream_t)stream, sup));
    else
        HIPCHK(eepacc::launch_ab_build(h->d_cfg, h->cfg.N, eepacc::ab_qp_num_rows(h->cfg), B, s, v, a_prev, t0, s_tv, v_tv,
                                       a_tv_prev, H, g, A, lba, uba, (hipStream_t)stream, &sup));
    return EEPACC_OK;
}
extern "C" int eepacc_ab_build_qp_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                      const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                      const double* s_est, const double* v_est, const double* s_tv_est,
                                      double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    return build_qp_est_impl(false, "eepacc_ab_build_qp_est", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, s_est, v_est, s_tv_est, H, g, A, lba, uba, stream);
}
extern "C" int eepacc_bl_build_qp_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                      const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                      const double* s_est, const double* v_est, const double* s_tv_est,
                                      double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    return build_qp_est_impl(true, "eepacc_bl_build_qp_est", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, s_est, v_est, s_tv_est, H, g, A, lba, uba, stream);
}

extern "C" int eepacc_bl_qp_size(const eepacc_handle* h, int* nV, int* nC) { return qp_size_impl(kQpBL, h, nV, nC); }
extern "C" int eepacc_bl_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type) { return qp_rows_impl(kQpBL, h, stage, type); }

extern "C" int eepacc_bl_build_qp(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                  const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    bool launch;
    if (const int rc = build_args_check(kQpBL, h, B, {s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, H, g, A, lba, uba}, &launch)) return rc;
    if (!launch) return EEPACC_OK;
    const bool tv = h->cfg.bl_mode == 2;                   // no lead vehicle: the three lead arrays are not read
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(eepacc::launch_bl_qp(h->d_cfg, h->cfg.N, eepacc::bl_qp_num_rows(h->cfg), B, s, v, a_prev, t0, tv ? nullptr : s_tv,
                                tv ? nullptr : v_tv, tv ? nullptr : a_tv_prev, H, g, A, lba, uba, (hipStream_t)stream));
    return EEPACC_OK;
}

// ---- the same on a handle with settings classes: eepacc_classes_qp_size, _qp_rows, _build_qp serve class handles only, of
// either creation entry; the nine entries above keep refusing them.  The catalogue (per-class rows, padding up to the largest
// class) is eepacc_cfg.cpp's.
static int classes_qp_handle(const eepacc_handle* h, const std::string& who) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    if (!h->n_classes) {
        const char* plain = h->cfg.bl_mode ? "eepacc_bl_qp_size, eepacc_bl_qp_rows and eepacc_bl_build_qp / eepacc_bl_build_qp_est build the problem of such a handle"
                                           : "eepacc_ab_qp_size, eepacc_ab_qp_rows and eepacc_ab_build_qp / eepacc_ab_build_qp_est build the problem of such a handle";
        return fail(EEPACC_ENOTSUP, who + ": this handle has no settings classes (it was created by eepacc_create with bl_mode = " +
                                        std::to_string(h->cfg.bl_mode) + "); " + plain);
    }
    return EEPACC_OK;
}

extern "C" int eepacc_classes_qp_size(const eepacc_handle* h, int* nV, int* nC) {
    const std::string who = "eepacc_classes_qp_size";
    if (const int rc = classes_qp_handle(h, who)) return rc;
    if (!nV) return fail(EEPACC_EINVAL, who + ": nV is NULL");
    if (!nC) return fail(EEPACC_EINVAL, who + ": nC is NULL");
    *nV = (h->cfg.bl_mode ? kQpBL.nV_stage : kQpAB.nV_stage) * h->cfg.N;
    *nC = eepacc::classes_qp_max_rows(h->qp_rows.data(), h->n_classes);
    return EEPACC_OK;
}

extern "C" int eepacc_classes_qp_rows(const eepacc_handle* h, int cls, int32_t* stage, int32_t* type) {
    const std::string who = "eepacc_classes_qp_rows";
    if (const int rc = classes_qp_handle(h, who)) return rc;
    if (!stage) return fail(EEPACC_EINVAL, who + ": stage is NULL");
    if (!type) return fail(EEPACC_EINVAL, who + ": type is NULL");
    return eepacc::classes_qp_rows(h->qp_rows.data(), h->n_classes, cls, stage, type);
}

extern "C" int eepacc_classes_build_qp(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                       const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                       const double* s_est, const double* v_est, const double* s_tv_est,
                                       double* H, double* g, double* A, double* lba, double* uba, void* stream) {
    const std::string who = "eepacc_classes_build_qp";
    if (const int rc = classes_qp_handle(h, who)) return rc;
    const bool tv = h->cfg.bl_mode == 2;                   // no lead vehicle: the three lead arrays are not read
    if (tv && (s_est || v_est || s_tv_est))
        return fail(EEPACC_ENOTSUP, who + ": the classes of this handle were created with bl_mode = 2 (RunOpt_TVMPC); the target-vehicle controller has no lead and hands its bounds a zero speed estimate, so supplied horizon guesses are not built for it");
    if (B < 0 || B > h->max_batch)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    const struct { const void* p; const char* name; bool needed; } bufs[] = {
        {s, "s", true}, {v, "v", true}, {a_prev, "a_prev", true}, {t0, "t0", true}, {s_tv, "s_tv", !tv}, {v_tv, "v_tv", !tv},
        {a_tv_prev, "a_tv_prev", !tv}, {H, "H", true}, {g, "g", true}, {A, "A", true}, {lba, "lba", true}, {uba, "uba", true}};
    for (const auto& bf : bufs)
        if (bf.needed && !bf.p) return fail(EEPACC_EINVAL, who + ": " + bf.name + " is NULL");
    if (const int rc = est_pair(who, s_est, v_est)) return rc;
    if (const int rc = classes_ready(h, who.c_str(), B)) return rc;
    const eepacc::AbSupplied sup{s_est, v_est, s_tv_est};
    const int nC = eepacc::classes_qp_max_rows(h->qp_rows.data(), h->n_classes);
    HIPCHK(hipSetDevice(h->device));
    if (h->cfg.bl_mode)
        HIPCHK(eepacc::launch_bl_qp_cls(h->d_cfg, h->d_class_of, h->cfg.N, nC, B, s, v, a_prev, t0, tv ? nullptr : s_tv,
                                        tv ? nullptr : v_tv, tv ? nullptr : a_tv_prev, H, g, A, lba, uba, (hipStream_t)stream, sup));
    else
        HIPCHK(eepacc::launch_ab_build_cls(h->d_cfg, h->d_class_of, h->cfg.N, nC, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev,
                                           H, g, A, lba, uba, (hipStream_t)stream, sup));
    return EEPACC_OK;
}

extern "C" int eepacc_postprocess(eepacc_handle* h, int B, int n_steps, const double* traj, double* rpm,
                                  double* Tm, double* P, double* E, void* stream) {
    if (!h || !traj || !rpm || !Tm || !P || !E) return fail(EEPACC_EINVAL, "eepacc_postprocess: NULL argument");
    if (B < 1 || n_steps < 1) return EEPACC_OK;
    if (const int rc = classes_ready(h, "eepacc_postprocess", B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(eepacc::launch_postprocess(h->d_cfg, h->class_map(), B, n_steps, traj, rpm, Tm, P, E, (hipStream_t)stream));
    return EEPACC_OK;
}

// Key figures of a closed-loop trajectory (ABO/Main.m:131-263, ABO/Custom_plots.m:73-107), per instance, on the device.
// Reads the trajectory and the handle's KpiCfg table only: no carried state, so it may follow a launch of any controller.
extern "C" int eepacc_kpis(eepacc_handle* h, int B, int n_steps, const double* traj, const int32_t* status,
                           const double* cutoff_dist_host, double* kpi, void* stream) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    if (B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "eepacc_kpis: B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (n_steps < 1) return fail(EEPACC_EINVAL, "eepacc_kpis: n_steps = " + std::to_string(n_steps) + " must be at least 1");
    if (!traj) return fail(EEPACC_EINVAL, "eepacc_kpis: traj is NULL");
    if (!status) return fail(EEPACC_EINVAL, "eepacc_kpis: status is NULL");
    if (!cutoff_dist_host) return fail(EEPACC_EINVAL, "eepacc_kpis: cutoff_dist_host is NULL");
    if (!kpi) return fail(EEPACC_EINVAL, "eepacc_kpis: kpi is NULL");
    const int nc = h->n_classes ? h->n_classes : 1;
    for (int k = 0; k < nc; ++k)
        if (!isfinite(cutoff_dist_host[k]))
            return fail(EEPACC_EINVAL, "eepacc_kpis: cutoff_dist_host[" + std::to_string(k) + "] is not finite");
    if (B == 0) return EEPACC_OK;
    if (const int rc = classes_ready(h, "eepacc_kpis", B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    // stream ordered behind an earlier call's kernel; the host array may be reused when this returns (pageable source)
    HIPCHK(hipMemcpyAsync(h->d_kpi_cut, cutoff_dist_host, (size_t)nc * sizeof(double), hipMemcpyHostToDevice, (hipStream_t)stream));
    HIPCHK(eepacc::launch_kpis(h->d_kpi, h->class_map(), h->d_kpi_cut, B, n_steps, traj, status, kpi, (hipStream_t)stream));
    return EEPACC_OK;
}

// Vehicle-following and cost key figures (ABO/Main.m:679-771, RunOpt_ABMPC.m:382-404, RunOpt_FBMPC.m:373-397), per instance, on
// the device.  Reads the trajectory, the lead traces and the handle's FollowCfg table only: no carried state.  What does not
// need the handle is checked first.
extern "C" int eepacc_follow_kpis(eepacc_handle* h, int B, int n_steps, int weights, const double* traj, const int32_t* status,
                                  const double* s_tv, const double* v_tv, double* fkpi, void* stream) {
    if (weights != EEPACC_FKPI_W_AB && weights != EEPACC_FKPI_W_FB && weights != EEPACC_FKPI_W_NONE)
        return fail(EEPACC_EINVAL, "eepacc_follow_kpis: weights = " + std::to_string(weights) + " is none of EEPACC_FKPI_W_AB, _W_FB, _W_NONE");
    if (n_steps < 1) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: n_steps = " + std::to_string(n_steps) + " must be at least 1");
    if (!traj) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: traj is NULL");
    if (!status) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: status is NULL");
    if (!s_tv) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: s_tv is NULL");
    if (!v_tv) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: v_tv is NULL");
    if (!fkpi) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: fkpi is NULL");
    if (!h) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: NULL handle");
    if (B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "eepacc_follow_kpis: B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    if (const int rc = classes_ready(h, "eepacc_follow_kpis", B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(eepacc::launch_follow_kpis(h->d_follow, h->class_map(), weights, B, n_steps, traj, s_tv, v_tv, fkpi, (hipStream_t)stream));
    return EEPACC_OK;
}

// Route-compliance key figures (ABO/Main.m:374-433, :486-534, EstimateRouteAndComfortBounds.m:154-189), per instance, on the
// device.  Reads the trajectory and the handle's RouteCfg table only: no carried state.  What does not need the handle is
// checked first.
extern "C" int eepacc_route_kpis(eepacc_handle* h, int B, int n_steps, double t_start, const double* tol_host,
                                 const double* traj, const int32_t* status, double* rkpi, double* limits, void* stream) {
    if (n_steps < 1) return fail(EEPACC_EINVAL, "eepacc_route_kpis: n_steps = " + std::to_string(n_steps) + " must be at least 1");
    if (!isfinite(t_start)) return fail(EEPACC_EINVAL, "eepacc_route_kpis: t_start is not finite");
    if (!tol_host) return fail(EEPACC_EINVAL, "eepacc_route_kpis: tol_host is NULL");
    static const char* const tol_name[3] = {"v_tol", "a_tol", "j_tol"};
    for (int i = 0; i < 3; ++i)
        if (!isfinite(tol_host[i]) || tol_host[i] < 0.0)
            return fail(EEPACC_EINVAL, std::string("eepacc_route_kpis: tol_host[") + std::to_string(i) + "] (" + tol_name[i] + ") must be finite and not negative");
    if (!traj) return fail(EEPACC_EINVAL, "eepacc_route_kpis: traj is NULL");
    if (!status) return fail(EEPACC_EINVAL, "eepacc_route_kpis: status is NULL");
    if (!rkpi) return fail(EEPACC_EINVAL, "eepacc_route_kpis: rkpi is NULL");
    if (!h) return fail(EEPACC_EINVAL, "eepacc_route_kpis: NULL handle");
    if (B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "eepacc_route_kpis: B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    if (const int rc = classes_ready(h, "eepacc_route_kpis", B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(eepacc::launch_route_kpis(h->d_route, h->class_map(), B, n_steps, t_start, tol_host[0], tol_host[1], tol_host[2], traj, rkpi,
                                     limits, (hipStream_t)stream));
    return EEPACC_OK;
}

extern "C" int eepacc_last_iterations(eepacc_handle* h, int B, int32_t* iters_host) {
    if (!h || !iters_host || B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "eepacc_last_iterations: bad arguments");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(iters_host, h->d_iters, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost));
    return EEPACC_OK;
}

extern "C" int eepacc_synchronize(eepacc_handle* h, void* stream) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    HIPCHK(hipSetDevice(h->device));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    int err = 0;
    HIPCHK(hipMemcpy(&err, h->d_err, sizeof(int), hipMemcpyDeviceToHost));
    if (err != 0)
        return fail(EEPACC_EDEVICE, "closed-loop kernel: a work unit waited for its predecessor beyond the spin limit; "
                                    "the affected steps carry status 3 and the results of this launch are invalid");
    return EEPACC_OK;
}

#ifndef EEPACC_BUILD_FLAGS
#define EEPACC_BUILD_FLAGS ""
#endif
extern "C" const char* eepacc_build_flags(void) { return EEPACC_BUILD_FLAGS; }

// B3 -- dense QP operator (ABO/RunOpt_ABMPC.m:252)
// persistent workgroups of the dense QP kernel per compute unit (EEPACC_QP_WGS_PER_CU overrides)
static int qp_grid(const eepacc_handle* h, int B) {
    int per_cu = 2;
    if (const char* e = getenv("EEPACC_QP_WGS_PER_CU")) { int v = atoi(e); if (v >= 1 && v <= 8) per_cu = v; }
    const int g = per_cu * h->num_cus;
    return B < g ? B : g;
}

static int qp_workspace(eepacc_handle* h, int grid, int nV) {
    size_t need = (size_t)grid * eepacc_qp_dense_ws_doubles(nV);
    if (need > h->qp_ws_doubles) {
        if (h->d_qp_ws) HIPCHK(hipDeviceSynchronize());
        h->qp_ws_doubles = 0;
        if (h->d_qp_ws.alloc(need) != hipSuccess) return fail(EEPACC_ENOMEM, "dense QP workspace allocation failed");
        h->qp_ws_doubles = need;
    }
    return EEPACC_OK;
}

// What the operator's entry points do before they fill their argument struct, in this order: the handle, the sizes (nR: 1
// where the entry point has none), B = 0, the limits, the entry point's own buffers (missing: one of them is NULL), the LDS
// fit; then device, grid and workspace.  *grid stays 0 where there is nothing to launch (B = 0, or a refusal).
static int qp_begin(eepacc_handle* h, const char* name, int B, int nV, int nC, int nR, bool missing, int* grid) {
    const std::string who = std::string(name) + ": ";
    *grid = 0;
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    if (const int rc = not_classes(h, name)) return rc;
    if (B < 0 || nV < 1 || nC < 0 || nR < 1) return fail(EEPACC_EINVAL, who + "bad sizes");
    if (B == 0) return EEPACC_OK;
    if (nV > EEPACC_QP_MAX_NV || nC > EEPACC_QP_MAX_NC)
        return fail(EEPACC_EINVAL, who + "nV/nC above EEPACC_QP_MAX_NV/NC");
    if (missing) return fail(EEPACC_EINVAL, who + "NULL buffer");
    if (eepacc_qp_dense_lds_bytes(nV, nC) > 160 * 1024) return fail(EEPACC_EINVAL, who + "problem does not fit LDS");
    HIPCHK(hipSetDevice(h->device));
    const int g = qp_grid(h, B);
    if (const int rc = qp_workspace(h, g, nV)) return rc;
    *grid = g;
    return EEPACC_OK;
}

// The tail of the preamble, which fb_one_step shares: workspace and work counter into the argument struct (a.nV set), the
// counter zeroed on the stream of the launch.
template <class Args> static int qp_arm(eepacc_handle* h, Args& a, hipStream_t stream) {
    a.ws = h->d_qp_ws; a.ws_stride = eepacc_qp_dense_ws_doubles(a.nV); a.counter = h->d_qp_counter;
    HIPCHK(hipMemsetAsync(h->d_qp_counter, 0, sizeof(int), stream));
    return EEPACC_OK;
}

// both entry points of the operator; dual = nullptr: eepacc_qp_solve_batched
struct QpDual {
    const int8_t *ws0_a, *ws0_x;
    double *lam_a, *lam_x;
    int8_t *ws_a, *ws_x;
    int32_t* iters;
};

static int qp_solve(eepacc_handle* h, const char* name, int B, int nV, int nC, const double* H, const double* g,
                    const double* A, const double* lba, const double* uba, const double* lbx, const double* ubx,
                    const double* x0, double* x, double* cost, int32_t* status, const QpDual* dual, void* stream) {
    int grid;
    const int rc = qp_begin(h, name, B, nV, nC, 1, !H || !g || !x || (nC > 0 && !A), &grid);
    if (rc != EEPACC_OK || !grid) return rc;
    eepacc_qp_args a;
    a.B = B; a.nV = nV; a.nC = nC; a.H = H; a.g = g; a.A = A; a.lba = lba; a.uba = uba; a.lbx = lbx; a.ubx = ubx;
    a.x0 = x0; a.x = x; a.cost = cost; a.status = status; a.iters = (B <= h->max_batch) ? h->d_iters : nullptr;
    a.rho_rel = 0.0; a.max_prox = 0; a.rho_k = nullptr;
    if (dual) {
        a.ws0_a = dual->ws0_a; a.ws0_x = dual->ws0_x; a.lam_a = dual->lam_a; a.lam_x = dual->lam_x;
        a.ws_a = dual->ws_a; a.ws_x = dual->ws_x; a.iters = dual->iters;
    }
    if (const int rc2 = qp_arm(h, a, (hipStream_t)stream)) return rc2;
    HIPCHK(dual ? eepacc_qp_dense_launch_dual(a, grid, (hipStream_t)stream) : eepacc_qp_dense_launch(a, grid, (hipStream_t)stream));
    return EEPACC_OK;
}

extern "C" int eepacc_qp_solve_batched(eepacc_handle* h, int B, int nV, int nC, const double* H, const double* g,
                                       const double* A, const double* lba, const double* uba, const double* lbx,
                                       const double* ubx, const double* x0, double* x, double* cost,
                                       int32_t* status, void* stream) {
    return qp_solve(h, "eepacc_qp_solve_batched", B, nV, nC, H, g, A, lba, uba, lbx, ubx, x0, x, cost, status, nullptr, stream);
}

extern "C" int eepacc_qp_solve_batched_dual(eepacc_handle* h, int B, int nV, int nC, const double* H, const double* g,
                                            const double* A, const double* lba, const double* uba, const double* lbx,
                                            const double* ubx, const double* x0, const int8_t* ws0_a, const int8_t* ws0_x,
                                            double* x, double* cost, int32_t* status, double* lam_a, double* lam_x,
                                            int8_t* ws_a, int8_t* ws_x, int32_t* iters, void* stream) {
    const QpDual d = {ws0_a, ws0_x, lam_a, lam_x, ws_a, ws_x, iters};
    return qp_solve(h, "eepacc_qp_solve_batched_dual", B, nV, nC, H, g, A, lba, uba, lbx, ubx, x0, x, cost, status, &d, stream);
}

extern "C" int eepacc_qp_kkt_solve_batched(eepacc_handle* h, int B, int nV, int nC, int nR, const double* H, const double* A,
                                           const int8_t* ws_a, const int8_t* ws_x, const double* r_p, const double* r_a,
                                           const double* r_x, double* p, double* q_a, double* q_x, int32_t* status,
                                           void* stream) {
    int grid;
    const int rc = qp_begin(h, "eepacc_qp_kkt_solve_batched", B, nV, nC, nR, !H || !r_p || !p || (nC > 0 && !A), &grid);
    if (rc != EEPACC_OK || !grid) return rc;
    eepacc_qp_kkt_args a;
    a.B = B; a.nV = nV; a.nC = nC; a.nR = nR; a.H = H; a.A = A; a.ws_a = nC > 0 ? ws_a : nullptr; a.ws_x = ws_x;
    a.r_p = r_p; a.r_a = nC > 0 ? r_a : nullptr; a.r_x = r_x; a.p = p; a.q_a = nC > 0 ? q_a : nullptr; a.q_x = q_x;
    a.status = status;
    if (const int rc2 = qp_arm(h, a, (hipStream_t)stream)) return rc2;
    HIPCHK(eepacc_qp_kkt_launch(a, grid, (hipStream_t)stream));
    return EEPACC_OK;
}

// FBMPC (ABO/RunOpt_FBMPC.m:161-331): build kernel -> dense QP operator -> extraction, per step.
static int fb_prepare(eepacc_handle* h, int B) {
    const int N = h->cfg.N;
    const size_t nV = 6 * (size_t)N, nC = (size_t)eepacc::fb_qp_num_rows(h->cfg);
    if (nV > EEPACC_QP_MAX_NV || nC > EEPACC_QP_MAX_NC || eepacc_qp_dense_lds_bytes((int)nV, (int)nC) > 160 * 1024)
        return fail(EEPACC_ENOTSUP, "FBMPC: horizon too long for the dense QP operator");
    if (B <= h->fb.B) return EEPACC_OK;
    HIPCHK(hipDeviceSynchronize());
    FbDense& f = h->fb;
    f = FbDense();
    // the dense QP data is held for a chunk of instances at a time (about 16 GB at most)
    const size_t per = (nV * nV + nC * nV + nV + 2 * nC) * sizeof(double);
    size_t chunk = (size_t)16e9 / per;
    if (chunk < 1) chunk = 1;
    if (chunk > (size_t)B) chunk = (size_t)B;
    const size_t nB = (size_t)B;
    hipError_t e = hipSuccess;
    auto get = [&e](auto& m, size_t n) { if (e == hipSuccess) e = m.alloc(n); };
    get(f.H, chunk * nV * nV); get(f.g, chunk * nV); get(f.A, chunk * nC * nV); get(f.lba, chunk * nC); get(f.uba, chunk * nC);
    get(f.x, nB * nV); get(f.x0, nB * nV); get(f.cost, nB); get(f.meas, 5 * nB); get(f.carry, 5 * nB);
    get(f.A22, nB * N); get(f.D2, nB * N); get(f.sp, nB * (N + 1)); get(f.vp, nB * (N + 1));
    get(f.qpstat, nB); get(f.rhok, nB);
    if (e != hipSuccess) { f = FbDense(); return fail(EEPACC_ENOMEM, "FBMPC: device allocation failed"); }
    HIPCHK(hipMemset(h->fb.x0, 0, nB * nV * sizeof(double)));
    HIPCHK(hipMemset(h->fb.rhok, 0, nB * sizeof(int)));
    HIPCHK(hipMemset(h->fb.A22, 0, nB * N * sizeof(double)));
    HIPCHK(hipMemset(h->fb.D2, 0, nB * N * sizeof(double)));
    HIPCHK(hipMemset(h->fb.sp, 0, nB * (N + 1) * sizeof(double)));
    HIPCHK(hipMemset(h->fb.vp, 0, nB * (N + 1) * sizeof(double)));
    h->fb.B = B; h->fb.chunk = (int)chunk;
    h->fb_k_done = 0; h->fb_by_step = false;
    return EEPACC_OK;
}

// one FBMPC step for B instances; in[] as eepacc_fb_args documents for the mode
static int fb_one_step(eepacc_handle* h, int B, int mode, const double* s, const double* v, const double* a_prev,
                       const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                       double* out, double* s_pred, double* v_pred, int32_t* status, hipStream_t stream) {
    const int N = h->cfg.N, nV = 6 * N, nC = eepacc::fb_qp_num_rows(h->cfg);
    for (int b0 = 0; b0 < B; b0 += h->fb.chunk) {
        const int nb = (B - b0 < h->fb.chunk) ? B - b0 : h->fb.chunk;
        eepacc::eepacc_fb_args a;
        a.cfg = h->d_cfg; a.B = B; a.k_step = h->fb_k_done; a.b0 = b0; a.nb = nb; a.mode = mode;
        a.s = s; a.v = v; a.a_prev = a_prev; a.t0 = t0; a.s_tv = s_tv; a.v_tv = v_tv; a.a_tv_prev = a_tv_prev;
        a.carry = h->fb.carry; a.A22 = h->fb.A22; a.D2 = h->fb.D2;
        a.sp_prev = h->fb.sp; a.vp_prev = h->fb.vp;
        a.H = h->fb.H; a.g = h->fb.g; a.A = h->fb.A; a.lba = h->fb.lba; a.uba = h->fb.uba; a.meas = h->fb.meas;
        HIPCHK(eepacc::launch_fb_build(a, N, stream));
        int grid = qp_grid(h, nb);
        int rc = qp_workspace(h, grid, nV);
        if (rc != EEPACC_OK) return rc;
        eepacc_qp_args q;
        q.B = nb; q.nV = nV; q.nC = nC; q.H = h->fb.H; q.g = h->fb.g; q.A = h->fb.A; q.lba = h->fb.lba; q.uba = h->fb.uba;
        q.lbx = nullptr; q.ubx = nullptr;
        q.x0 = h->fb.x0 + (size_t)b0 * nV; q.x = h->fb.x + (size_t)b0 * nV; q.cost = h->fb.cost + b0;
        q.status = h->fb.qpstat + b0; q.iters = (B <= h->max_batch) ? h->d_iters + b0 : nullptr;
        q.rho_rel = 0.0; q.max_prox = 0; q.rho_k = h->fb.rhok + b0;
        rc = qp_arm(h, q, stream);
        if (rc != EEPACC_OK) return rc;
        HIPCHK(eepacc_qp_dense_launch(q, grid, stream));
    }
    eepacc::eepacc_fb_apply_args p;
    p.cfg = h->d_cfg; p.B = B; p.x = h->fb.x; p.cost = h->fb.cost; p.qp_status = h->fb.qpstat; p.meas = h->fb.meas;
    p.A22 = h->fb.A22; p.D2 = h->fb.D2; p.out = out; p.s_pred = s_pred; p.v_pred = v_pred; p.status = status;
    p.carry = mode == 1 ? h->fb.carry : nullptr;
    const bool keep_pred = h->cfg.paramEstSetting == 2;
    if (keep_pred) { p.s_pred = h->fb.sp; p.v_pred = h->fb.vp; }      // stride B: fb_sp/fb_vp hold [N+1][B]
    HIPCHK(eepacc::launch_fb_apply(p, stream));
    if (keep_pred && s_pred && v_pred) {
        HIPCHK(hipMemcpyAsync(s_pred, h->fb.sp, (size_t)B * (N + 1) * sizeof(double), hipMemcpyDeviceToDevice, stream));
        HIPCHK(hipMemcpyAsync(v_pred, h->fb.vp, (size_t)B * (N + 1) * sizeof(double), hipMemcpyDeviceToDevice, stream));
    }
    // the solution is the proximal centre / initial guess of the next step
    HIPCHK(hipMemcpyAsync(h->fb.x0, h->fb.x, (size_t)B * nV * sizeof(double), hipMemcpyDeviceToDevice, stream));
    h->fb_k_done += 1;
    h->last_B = B;
    h->fb.steps_B = B;
    return EEPACC_OK;
}

// One step of a structured handle: eepacc_fb_step (sup == NULL) and eepacc_fb_step_est, on the same handle state
static int fbs_step_launch(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev, const double* t0,
                           const double* s_tv, const double* v_tv, const double* a_tv_prev, double* out, double* s_pred,
                           double* v_pred, int32_t* status, void* stream, const eepacc::AbSupplied* sup) {
    eepacc::fbs_step_args a;
    a.cfg = h->d_cfg; a.B = B; a.k_step = h->fb_k_done;
    a.s = s; a.v = v; a.a_prev = a_prev; a.t0 = t0; a.s_tv = s_tv; a.v_tv = v_tv; a.a_tv_prev = a_tv_prev;
    a.state = h->fbs_state; a.hb = h->fbs_hb; a.out = out; a.s_pred = s_pred; a.v_pred = v_pred;
    a.status = status; a.iters = h->d_iters;
    if (sup) HIPCHK(eepacc::launch_fbs_step_est(a, h->cfg.N, (hipStream_t)stream, sup->s_est, sup->v_est, sup->s_tv_est));
    else HIPCHK(eepacc::launch_fbs_step(a, h->cfg.N, (hipStream_t)stream));
    h->fb_k_done += 1; h->last_B = B; h->fb_by_step = true;
    return EEPACC_OK;
}

extern "C" int eepacc_fb_step(eepacc_handle* h, int B, const double* s, const double* v, const double* v_prev,
                              const double* a_prev, const double* Fm_prev, const double* Fb_prev, const double* t0,
                              const double* s_tv, const double* v_tv, const double* a_tv_prev,
                              double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    (void)v_prev; (void)Fm_prev; (void)Fb_prev;   // accepted and unused, as in CreateQP_FB.m:1 (inputs v_minus1, Fm_minus1, Fb_minus1)
    if (const int rc = not_classes(h, "eepacc_fb_step")) return rc;      // (any class handle, a target-vehicle one included: not supported)
    if (const int rc = not_tv(h, "eepacc_fb_step")) return rc;
    if (B < 0 || B > h->max_batch) return fail(EEPACC_EINVAL, "B exceeds max_batch of the handle");
    if (B == 0) return EEPACC_OK;
    if (!s || !v || !a_prev || !t0 || !s_tv || !v_tv || !a_tv_prev || !out || !status)
        return fail(EEPACC_EINVAL, "eepacc_fb_step: NULL buffer");
    HIPCHK(hipSetDevice(h->device));
    if (h->fbs)
        return fbs_step_launch(h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, stream, nullptr);
    int rc = fb_prepare(h, B);
    if (rc != EEPACC_OK) return rc;
    h->fb_by_step = true;              // after fb_prepare: its first (re)allocation clears the flag
    return fb_one_step(h, B, 0, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, (hipStream_t)stream);
}

// The condensed QP of an FBMPC step as data (eepacc_fb_qp.hip): kQpFB above.  After the checks every family has, the model
// and the carried state of the handle.
extern "C" int eepacc_fb_qp_size(const eepacc_handle* h, int* nV, int* nC) { return qp_size_impl(kQpFB, h, nV, nC); }
extern "C" int eepacc_fb_qp_rows(const eepacc_handle* h, int32_t* stage, int32_t* type) { return qp_rows_impl(kQpFB, h, stage, type); }

// eepacc_fb_build_qp (sup == NULL) and eepacc_fb_build_qp_est: the same checks, carried state and launch arguments
static int fb_build_impl(const std::string& who, eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                         const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                         const double* A22, const double* D2, double* H, double* g, double* A, double* lba,
                         double* uba, double* A22_used, double* D2_used, void* stream, const eepacc::AbSupplied* sup) {
    bool launch;
    if (const int rc = build_args_check(kQpFB, h, B, {s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, H, g, A, lba, uba}, &launch, who.c_str())) return rc;
    if (!launch) return EEPACC_OK;
    if (sup) { if (const int rc = est_pair(who, sup->s_est, sup->v_est)) return rc; }
    if (!A22 != !D2)
        return fail(EEPACC_EINVAL, who + ": " + (A22 ? "D2" : "A22") + " is NULL while " + (A22 ? "A22" : "D2") + " is given; pass both or neither");
    const DevCfg& C = h->cfg;
    if (A22 && !C.FBuseTaylor)
        return fail(EEPACC_EINVAL, who + ": A22 and D2 are given, but with FBuseTaylor = 0 no model is carried (A22 = 1, D2 from the step's estimate); pass NULL");
    const int N = C.N;
    eepacc::fb_qp_args a;
    a.cfg = h->d_cfg; a.B = B; a.nC = eepacc::fb_qp_num_rows(C);
    a.s = s; a.v = v; a.a_prev = a_prev; a.t0 = t0; a.s_tv = s_tv; a.v_tv = v_tv; a.a_tv_prev = a_tv_prev;
    a.H = H; a.g = g; a.A = A; a.lba = lba; a.uba = uba; a.A22_used = A22_used; a.D2_used = D2_used;
    a.A22 = a.D2 = a.sp = a.vp = eepacc::FbCarried{nullptr, 0, 0};
    // What the handle carries from its FBMPC steps: instance-major in fbs_state on a structured handle, [.][B of the steps]
    // in h->fb on a dense-path handle.  Before the first step (and after a reset) nothing is carried: the model is
    // initialised in the kernel and the predictions are zero.
    const bool carried_model = !A22 && C.FBuseTaylor && h->fb_k_done > 0;
    const bool carried_pred = C.paramEstSetting == 2 && h->fb_k_done > 0;
    // The stride of the dense path's arrays is the B of the FBMPC steps that wrote them (fb.steps_B <= fb.B, what they are
    // allocated for); h->last_B will not do, since the ABMPC entry points write it too.
    if (!h->fbs && (carried_model || carried_pred) && (B != h->fb.steps_B || B > h->fb.B))
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " differs from the B = " + std::to_string(h->fb.steps_B) +
                                   " of the FBMPC steps whose carried state this handle holds");
    const size_t ks = eepacc::kFbsStateDoubles, lB = (size_t)h->fb.steps_B;
    if (A22) {
        a.k_step = -1;
        a.A22 = eepacc::FbCarried{A22, (size_t)B, 1}; a.D2 = eepacc::FbCarried{D2, (size_t)B, 1};
    } else {
        a.k_step = h->fb_k_done;
        if (carried_model && h->fbs) {
            a.A22 = eepacc::FbCarried{h->fbs_state + 64, 1, ks}; a.D2 = eepacc::FbCarried{h->fbs_state + 128, 1, ks};
        } else if (carried_model) {
            a.A22 = eepacc::FbCarried{h->fb.A22, lB, 1}; a.D2 = eepacc::FbCarried{h->fb.D2, lB, 1};
        }
    }
    if (carried_pred && h->fbs) {
        a.sp = eepacc::FbCarried{h->fbs_state + 192, 1, ks}; a.vp = eepacc::FbCarried{h->fbs_state + 256, 1, ks};
    } else if (carried_pred) {
        a.sp = eepacc::FbCarried{h->fb.sp, lB, 1}; a.vp = eepacc::FbCarried{h->fb.vp, lB, 1};
    }
    HIPCHK(hipSetDevice(h->device));
    if (sup) HIPCHK(eepacc::launch_fb_qp_est(a, N, (hipStream_t)stream, sup->s_est, sup->v_est, sup->s_tv_est));
    else HIPCHK(eepacc::launch_fb_qp(a, N, (hipStream_t)stream));
    return EEPACC_OK;
}

extern "C" int eepacc_fb_build_qp(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                  const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  const double* A22, const double* D2, double* H, double* g, double* A, double* lba,
                                  double* uba, double* A22_used, double* D2_used, void* stream) {
    return fb_build_impl("eepacc_fb_build_qp", h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, A22, D2, H, g, A, lba, uba, A22_used, D2_used,
                         stream, nullptr);
}

// ---- FBMPC with horizon guesses from the caller: eepacc_fb_step_est, eepacc_fb_build_qp_est, eepacc_run_fbmpc_preview.  The
// refusals of a handle are eepacc::fb_est_refusal (eepacc_cfg.cpp); the step and the preview loop run the kernels of
// eepacc_fbs_est.hip on the state of eepacc_fb_step / eepacc_run_fbmpc.
static int fb_est_handle(const eepacc_handle* h, const std::string& who, bool needs_structured) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    return eepacc::fb_est_refusal(who, h->n_classes, h->cfg, h->fbs, needs_structured);
}

extern "C" int eepacc_fb_step_est(eepacc_handle* h, int B, const double* s, const double* v, const double* v_prev,
                                  const double* a_prev, const double* Fm_prev, const double* Fb_prev, const double* t0,
                                  const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                  const double* s_est, const double* v_est, const double* s_tv_est,
                                  double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    (void)v_prev; (void)Fm_prev; (void)Fb_prev;   // accepted and unused, as in eepacc_fb_step
    const std::string who = "eepacc_fb_step_est";
    if (const int rc = fb_est_handle(h, who, true)) return rc;
    if (B < 0 || B > h->max_batch)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " is outside [0, max_batch = " + std::to_string(h->max_batch) + "]");
    if (B == 0) return EEPACC_OK;
    const struct { const void* p; const char* name; } bufs[] = {{s, "s"}, {v, "v"}, {a_prev, "a_prev"}, {t0, "t0"}, {s_tv, "s_tv"},
        {v_tv, "v_tv"}, {a_tv_prev, "a_tv_prev"}, {out, "out"}, {status, "status"}};
    for (const auto& bf : bufs)
        if (!bf.p) return fail(EEPACC_EINVAL, who + ": " + bf.name + " is NULL");
    if (const int rc = est_pair(who, s_est, v_est)) return rc;
    HIPCHK(hipSetDevice(h->device));
    const eepacc::AbSupplied sup{s_est, v_est, s_tv_est};
    return fbs_step_launch(h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, out, s_pred, v_pred, status, stream, &sup);
}

extern "C" int eepacc_fb_build_qp_est(eepacc_handle* h, int B, const double* s, const double* v, const double* a_prev,
                                      const double* t0, const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                      const double* s_est, const double* v_est, const double* s_tv_est,
                                      const double* A22, const double* D2, double* H, double* g, double* A, double* lba,
                                      double* uba, double* A22_used, double* D2_used, void* stream) {
    const std::string who = "eepacc_fb_build_qp_est";
    if (const int rc = fb_est_handle(h, who, false)) return rc;
    const eepacc::AbSupplied sup{s_est, v_est, s_tv_est};
    return fb_build_impl(who, h, B, s, v, a_prev, t0, s_tv, v_tv, a_tv_prev, A22, D2, H, g, A, lba, uba, A22_used, D2_used, stream, &sup);
}

// The launch of eepacc_run_fbmpc (pv == NULL) and of eepacc_run_fbmpc_preview after their own checks of the handle and of B,
// n_steps: buffers, the resume rules and, on a structured handle, the closed-loop kernel
static int fb_run_impl(const std::string& who, eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                       const double* a_minus1, const double* s_tv, const double* v_tv,
                       double* traj, int32_t* status, void* stream, const eepacc::AbPreview* pv) {
    if (!s0 || !v0 || !a_minus1 || !s_tv || !v_tv || !traj || !status)
        return fail(EEPACC_EINVAL, who + ": NULL buffer");
    HIPCHK(hipSetDevice(h->device));
    if (h->fb_k_done > 0 && B != h->last_B)
        return fail(EEPACC_EINVAL, who + ": B changed while resuming; call eepacc_reset first");
    if (h->fb_k_done > 0 && h->fb_by_step)
        return fail(EEPACC_EINVAL, who + " after eepacc_fb_step: the per-step operator keeps no closed-loop state to resume from; call eepacc_reset first");
    if (h->fbs) {
        // work-unit length: 16 MPC steps, shorter for short launches so that every resident wave still gets several units
        int chunk_steps = eepacc::pick_chunk_steps(n_steps, B, eepacc::fbs_run_chunking_waves(h->cfg.N, h->num_cus));
        eepacc::fbs_run_args a;
        a.cfg = h->d_cfg; a.B = B; a.k_start = h->fb_k_done; a.n_steps = n_steps;
        a.s0 = s0; a.v0 = v0; a.a_m1 = a_minus1; a.s_tv = s_tv; a.v_tv = v_tv;
        a.carry = h->fbs_carry; a.state = h->fbs_state; a.hb = h->fbs_hb; a.traj = traj; a.status = status;
        a.iters_total = h->d_iters; a.work_counter = h->d_counter; a.done = h->d_done; a.err_word = h->d_err;
        a.chunk_steps = chunk_steps;
        a.cold = 0;
        if (const char* ev = getenv("EEPACC_DEBUG_FBS_COLD")) a.cold = atoi(ev) != 0;
        if (pv) HIPCHK(eepacc::launch_fbs_run_preview(a, h->cfg.N, h->num_cus, (hipStream_t)stream, pv->idx, pv->frac, pv->n_lead));
        else HIPCHK(eepacc::launch_fbs_run(a, h->cfg.N, h->num_cus, (hipStream_t)stream));
        h->fb_k_done += n_steps; h->last_B = B;
        return EEPACC_OK;
    }
    int rc = fb_prepare(h, B);
    if (rc != EEPACC_OK) return rc;
    for (int kk = 0; kk < n_steps; ++kk) {
        rc = fb_one_step(h, B, 1, s0, v0, a_minus1, nullptr, s_tv + (size_t)kk * B, v_tv + (size_t)kk * B, nullptr,
                         traj + (size_t)kk * EEPACC_OUT_N * B, nullptr, nullptr, status + (size_t)kk * B,
                         (hipStream_t)stream);
        if (rc != EEPACC_OK) return rc;
    }
    return EEPACC_OK;
}

extern "C" int eepacc_run_fbmpc(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                const double* a_minus1, const double* s_tv, const double* v_tv,
                                double* traj, int32_t* status, void* stream) {
    if (const int rc = not_classes(h, "eepacc_run_fbmpc")) return rc;      // (any class handle, a target-vehicle one included: not supported)
    if (const int rc = not_tv(h, "eepacc_run_fbmpc")) return rc;
    if (B < 0 || B > h->max_batch || n_steps < 0) return fail(EEPACC_EINVAL, "eepacc_run_fbmpc: bad B / n_steps");
    if (B == 0 || n_steps == 0) return EEPACC_OK;
    return fb_run_impl("eepacc_run_fbmpc", h, B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream, nullptr);
}

// ---- FBMPC on a handle with settings classes: eepacc_classes_fb_step, eepacc_run_classes_fbmpc.  Every refusal is
// eepacc::classes_fb_refusal (eepacc_cfg.cpp); the kernels are those of eepacc_fbs_cls.hip, on FBMPC state of the handle's own
// (fbs_state, fbs_carry, fbs_hb, fb_k_done) beside the ABMPC state, as on a structured handle of eepacc_create.
static int classes_fb_call(const eepacc_handle* h, const std::string& who, int B, int n_steps, const char* null_buffer) {
    if (!h) return fail(EEPACC_EINVAL, who + ": NULL handle");
    const eepacc::ClassesFbCall c{h->n_classes, h->cfg.bl_mode, h->cfg.N, h->fb_unsup.data(), eepacc::fbs_smem_bytes(h->cfg.N),
                                  eepacc::kFbsLdsBudget, h->max_batch, h->classes_B, B, n_steps, null_buffer};
    return eepacc::classes_fb_refusal(who, c);
}
struct NamedBuf { const void* p; const char* name; };
template <size_t n>
static const char* first_null(const NamedBuf (&bufs)[n]) {
    for (const NamedBuf& bf : bufs) if (!bf.p) return bf.name;
    return nullptr;
}

extern "C" int eepacc_classes_fb_step(eepacc_handle* h, int B, const double* s, const double* v, const double* v_prev,
                                      const double* a_prev, const double* Fm_prev, const double* Fb_prev, const double* t0,
                                      const double* s_tv, const double* v_tv, const double* a_tv_prev,
                                      double* out, double* s_pred, double* v_pred, int32_t* status, void* stream) {
    (void)v_prev; (void)Fm_prev; (void)Fb_prev;   // accepted and unused, as in eepacc_fb_step
    const NamedBuf bufs[] = {{s, "s"}, {v, "v"}, {a_prev, "a_prev"}, {t0, "t0"}, {s_tv, "s_tv"}, {v_tv, "v_tv"},
                             {a_tv_prev, "a_tv_prev"}, {out, "out"}, {status, "status"}};
    if (const int rc = classes_fb_call(h, "eepacc_classes_fb_step", B, 1, first_null(bufs))) return rc;
    if (B == 0) return EEPACC_OK;
    HIPCHK(hipSetDevice(h->device));
    eepacc::fbs_step_args a;
    a.cfg = h->d_cfg; a.B = B; a.k_step = h->fb_k_done;
    a.s = s; a.v = v; a.a_prev = a_prev; a.t0 = t0; a.s_tv = s_tv; a.v_tv = v_tv; a.a_tv_prev = a_tv_prev;
    a.state = h->fbs_state; a.hb = h->fbs_hb; a.out = out; a.s_pred = s_pred; a.v_pred = v_pred;
    a.status = status; a.iters = h->d_iters;
    HIPCHK(eepacc::launch_fbs_step_cls(a, h->cfg.N, (hipStream_t)stream, h->d_class_of));
    h->fb_k_done += 1; h->last_B = B; h->fb_by_step = true;
    return EEPACC_OK;
}

extern "C" int eepacc_run_classes_fbmpc(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                        const double* a_minus1, const double* s_tv, const double* v_tv,
                                        double* traj, int32_t* status, void* stream) {
    const std::string who = "eepacc_run_classes_fbmpc";
    const NamedBuf bufs[] = {{s0, "s0"}, {v0, "v0"}, {a_minus1, "a_minus1"}, {s_tv, "s_tv"}, {v_tv, "v_tv"}, {traj, "traj"}, {status, "status"}};
    if (const int rc = classes_fb_call(h, who, B, n_steps, first_null(bufs))) return rc;
    if (B == 0 || n_steps == 0) return EEPACC_OK;
    HIPCHK(hipSetDevice(h->device));
    // (B is that of the class map, so it cannot change while resuming)
    if (h->fb_k_done > 0 && h->fb_by_step)
        return fail(EEPACC_EINVAL, who + " after eepacc_classes_fb_step: the per-step operator keeps no closed-loop state to resume from; call eepacc_reset first");
    eepacc::fbs_run_args a;
    a.cfg = h->d_cfg; a.B = B; a.k_start = h->fb_k_done; a.n_steps = n_steps;
    a.s0 = s0; a.v0 = v0; a.a_m1 = a_minus1; a.s_tv = s_tv; a.v_tv = v_tv;
    a.carry = h->fbs_carry; a.state = h->fbs_state; a.hb = h->fbs_hb; a.traj = traj; a.status = status;
    a.iters_total = h->d_iters; a.work_counter = h->d_counter; a.done = h->d_done; a.err_word = h->d_err;
    a.chunk_steps = eepacc::pick_chunk_steps(n_steps, B, eepacc::fbs_run_chunking_waves(h->cfg.N, h->num_cus));      // as eepacc_run_fbmpc
    a.cold = 0;
    HIPCHK(eepacc::launch_fbs_run_cls(a, h->cfg.N, h->num_cus, (hipStream_t)stream, h->d_class_of));
    h->fb_k_done += n_steps; h->last_B = B;
    return EEPACC_OK;
}

extern "C" int eepacc_run_fbmpc_preview(eepacc_handle* h, int B, int n_steps, int n_lead, const double* s0, const double* v0,
                                        const double* a_minus1, const double* s_tv, const double* v_tv, double* traj,
                                        int32_t* status, void* stream) {
    const std::string who = "eepacc_run_fbmpc_preview";
    if (const int rc = fb_est_handle(h, who, true)) return rc;
    if (B < 0 || B > h->max_batch || n_steps < 0)
        return fail(EEPACC_EINVAL, who + ": B = " + std::to_string(B) + " must be in [0, max_batch = " + std::to_string(h->max_batch) + "] and n_steps = " + std::to_string(n_steps) + " not negative");
    if (n_lead < n_steps)
        return fail(EEPACC_EINVAL, who + ": n_lead = " + std::to_string(n_lead) + " is below n_steps = " + std::to_string(n_steps) + "; the lead traces hold at least the rows of the launch's steps");
    if (B == 0 || n_steps == 0) return EEPACC_OK;
    if (const int rc = preview_tables_ready(h)) return rc;
    const eepacc::AbPreview pv{h->d_pv_idx, h->d_pv_frac, n_lead};
    return fb_run_impl(who, h, B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status, stream, &pv);
}

// Host-pointer wrappers (what the MEX gateways mex/RunOpt_*MPC.c call): copy in, reset, run, wait, copy out.  The device
// scratch is freed on every return path.  A target-vehicle run has no lead trace (s_tv, v_tv null).
enum class Ctl { AB, FB, TV };
static int run_host(eepacc_handle* h, Ctl ctl, int B, int n_steps, const double* s0, const double* v0,
                    const double* a_minus1, const double* s_tv, const double* v_tv, double* traj, int32_t* status) {
    if (!h) return fail(EEPACC_EINVAL, "NULL handle");
    const bool lead = ctl != Ctl::TV;
    if (B < 1 || B > h->max_batch || n_steps < 1) return fail(EEPACC_EINVAL, "bad B / n_steps");
    if (!s0 || !v0 || !a_minus1 || (lead && (!s_tv || !v_tv)) || !traj || !status) return fail(EEPACC_EINVAL, "NULL buffer");
    if (ctl == Ctl::FB) { if (const int rc = not_classes(h, "eepacc_run_fbmpc_host")) return rc; }
    if (const int rc = classes_ready(h, "eepacc_run_abmpc_host", B)) return rc;
    HIPCHK(hipSetDevice(h->device));
    DevMem<double> d_in, d_tv, d_traj;
    DevMem<int32_t> d_status;
    const size_t nB = (size_t)B, nT = (size_t)n_steps * B;
    HIPCHK(d_in.alloc(3 * nB));
    if (lead) HIPCHK(d_tv.alloc(2 * nT));
    HIPCHK(d_traj.alloc(nT * EEPACC_OUT_N));
    HIPCHK(d_status.alloc(nT));
    HIPCHK(hipMemcpy(d_in, s0, nB * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_in + nB, v0, nB * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_in + 2 * nB, a_minus1, nB * sizeof(double), hipMemcpyHostToDevice));
    if (lead) {
        HIPCHK(hipMemcpy(d_tv, s_tv, nT * sizeof(double), hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(d_tv + nT, v_tv, nT * sizeof(double), hipMemcpyHostToDevice));
    }
    int rc = eepacc_reset(h);
    if (rc != EEPACC_OK) return rc;
    rc = ctl == Ctl::TV ? eepacc_run_tvmpc(h, B, n_steps, d_in, d_in + nB, d_in + 2 * nB, d_traj, d_status, nullptr)
       : ctl == Ctl::FB ? eepacc_run_fbmpc(h, B, n_steps, d_in, d_in + nB, d_in + 2 * nB, d_tv, d_tv + nT, d_traj, d_status, nullptr)
                        : eepacc_run_abmpc(h, B, n_steps, d_in, d_in + nB, d_in + 2 * nB, d_tv, d_tv + nT, d_traj, d_status, nullptr);
    if (rc != EEPACC_OK) return rc;
    rc = eepacc_synchronize(h, nullptr);
    HIPCHK(hipMemcpy(traj, d_traj, nT * EEPACC_OUT_N * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(status, d_status, nT * sizeof(int32_t), hipMemcpyDeviceToHost));
    return rc;
}

extern "C" int eepacc_run_abmpc_host(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                     const double* a_minus1, const double* s_tv, const double* v_tv,
                                     double* traj, int32_t* status) {
    return run_host(h, Ctl::AB, B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status);
}
extern "C" int eepacc_run_blmpc_host(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                     const double* a_minus1, const double* s_tv, const double* v_tv,
                                     double* traj, int32_t* status) {
    const int rc = need_bl(h);
    return rc != EEPACC_OK ? rc : run_host(h, Ctl::AB, B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status);
}
extern "C" int eepacc_run_fbmpc_host(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                     const double* a_minus1, const double* s_tv, const double* v_tv,
                                     double* traj, int32_t* status) {
    return run_host(h, Ctl::FB, B, n_steps, s0, v0, a_minus1, s_tv, v_tv, traj, status);
}
extern "C" int eepacc_run_tvmpc_host(eepacc_handle* h, int B, int n_steps, const double* s0, const double* v0,
                                     const double* a_minus1, double* traj, int32_t* status) {
    const int rc = need_tv(h);
    return rc != EEPACC_OK ? rc : run_host(h, Ctl::TV, B, n_steps, s0, v0, a_minus1, nullptr, nullptr, traj, status);
}
