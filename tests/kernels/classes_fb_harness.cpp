// Host harness of the FBMPC entries of a handle with settings classes (tests/test_classes_fb_cpu.py): the refusal predicate
// eepacc::classes_fb_refusal and eepacc::fbs_unsupported_field of csrc/eepacc_cfg.cpp on the DevCfg that build_cfg makes of the
// PODs of include/eepacc.h.  Plain C++, no HIP, no device.  With -DCLASSES_FB_HARNESS_MAIN it is a program of its own that walks
// the causes once (for a run under -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

extern "C" {

const char* ch_last_error(void) { return g_msg.c_str(); }

// build_cfg of one class, then what the structured FBMPC solver lacks of it ("" where it runs the class).  Settings that
// build_cfg refuses return its code.
int ch_unsupported(const eepacc_settings* S, const eepacc_vehicle* V, const char** field) {
    g_msg.clear();
    eepacc::DevCfg C;
    std::vector<double> Hinv;
    const int rc = eepacc::build_cfg(S, V, C, Hinv);
    if (rc != EEPACC_OK) return rc;
    const char* f = eepacc::fbs_unsupported_field(C);
    *field = f ? f : "";
    return EEPACC_OK;
}

// The predicate for the entry `who` on a handle of n_classes classes (0: a handle of eepacc_create) built from S, V
// [max(n_classes, 1)], with the LDS need and budget, max_batch and classes_B given, for a call with B, n_steps and null_buffer.
int ch_refusal(const eepacc_settings* S, const eepacc_vehicle* V, int n_classes, const char* who, long smem_bytes, long smem_budget,
               int max_batch, int classes_B, int B, int n_steps, const char* null_buffer) {
    g_msg.clear();
    const int n = n_classes > 0 ? n_classes : 1;
    std::vector<eepacc::DevCfg> Cs((size_t)n);
    std::vector<const char*> unsup;
    std::vector<double> Hinv;
    for (int k = 0; k < n; ++k) {
        const int rc = eepacc::build_cfg(&S[k], &V[k], Cs[(size_t)k], Hinv);
        if (rc != EEPACC_OK) return rc;
        unsup.push_back(eepacc::fbs_unsupported_field(Cs[(size_t)k]));
    }
    const eepacc::ClassesFbCall c{n_classes, Cs[0].bl_mode, Cs[0].N, unsup.data(), (size_t)smem_bytes, (size_t)smem_budget,
                                  max_batch, classes_B, B, n_steps, (null_buffer && *null_buffer) ? null_buffer : nullptr};
    return eepacc::classes_fb_refusal(who, c);
}

}  // extern "C"

#ifdef CLASSES_FB_HARNESS_MAIN
int main() {
    eepacc::DevCfg C = {};
    C.N = 20; C.phi = 10.0;
    C.fb_w[0] = 1.0; C.fb_w[1] = 1.0; C.fb_w[4] = 1.0; C.b_quadr[4] = 0.004;
    int bad = 0;
    bad += eepacc::fbs_unsupported_field(C) != nullptr;
    const char* ok[3] = {nullptr, nullptr, nullptr};
    eepacc::ClassesFbCall c{3, 0, 20, ok, 150000, 159232, 8, 6, 6, 5, nullptr};
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_OK;
    c.B = 0; c.null_buffer = "s0";
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_OK;
    c.B = 6;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_EINVAL || g_msg.find("s0 is NULL") == std::string::npos;
    c.null_buffer = nullptr; c.B = 5;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_EINVAL || g_msg.find("differs") == std::string::npos;
    c.B = 9;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_EINVAL || g_msg.find("max_batch = 8") == std::string::npos;
    c.B = 6; c.classes_B = 0;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_EINVAL || g_msg.find("eepacc_set_classes") == std::string::npos;
    c.classes_B = 6; c.n_steps = -1;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_EINVAL;
    c.n_steps = 5; c.smem_bytes = 200000;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_ENOTSUP || g_msg.find("N_hor = 20") == std::string::npos;
    c.smem_bytes = 150000;
    C.b_quadr[3] = 2.5e-4;
    const char* last[3] = {nullptr, nullptr, eepacc::fbs_unsupported_field(C)};      // the last class of the array
    c.unsupported = last;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_ENOTSUP || g_msg.find("class 2: b_quadr(4)") == std::string::npos;
    C.b_quadr[3] = 0.0; C.mb_any = 1;
    bad += eepacc::fbs_unsupported_field(C) == nullptr;
    C.mb_any = 0; C.fb_w[4] = 0.0;
    bad += eepacc::fbs_unsupported_field(C) == nullptr;
    c.unsupported = ok; c.bl_mode = 2;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_ENOTSUP || g_msg.find("eepacc_create_classes_bl") == std::string::npos;
    c.bl_mode = 0; c.n_classes = 0; c.unsupported = nullptr;
    bad += eepacc::classes_fb_refusal("run", c) != EEPACC_ENOTSUP || g_msg.find("eepacc_fb_step / eepacc_run_fbmpc") == std::string::npos;
    printf("classes_fb_harness: %d failed\n", bad);
    return bad;
}
#endif
