// Host harness of the FBMPC entries with supplied horizon guesses (tests/test_fb_est_cpu.py): the refusal predicate
// eepacc::fb_est_refusal of csrc/eepacc_cfg.cpp on the DevCfg that build_cfg makes of the PODs of include/eepacc.h, and the
// preview tables.  Plain C++, no HIP, no device.  With -DFB_EST_HARNESS_MAIN it is a program of its own that walks the
// causes once (for a run under -fsanitize=address,undefined).
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

extern "C" {

const char* fh_last_error(void) { return g_msg.c_str(); }

// build_cfg, then the predicate for the entry `who` on a handle with n_classes classes whose FBMPC steps are structured or not.
// Settings that build_cfg refuses return its code.
int fh_refusal(const eepacc_settings* S, const eepacc_vehicle* V, const char* who, int n_classes, int structured, int needs_structured) {
    g_msg.clear();
    eepacc::DevCfg C;
    std::vector<double> Hinv;
    const int rc = eepacc::build_cfg(S, V, C, Hinv);
    if (rc != EEPACC_OK) return rc;
    return eepacc::fb_est_refusal(who, n_classes, C, structured != 0, needs_structured != 0);
}

void fh_preview_tables(const double* Tvec, int N, int32_t* idx, double* frac) { eepacc::preview_tables(Tvec, N, idx, frac); }

}  // extern "C"

#ifdef FB_EST_HARNESS_MAIN
int main() {
    eepacc::DevCfg C = {};
    C.N = 20;
    int bad = 0;
    bad += eepacc::fb_est_refusal("step", 0, C, true, true) != EEPACC_OK;
    bad += eepacc::fb_est_refusal("step", 3, C, true, true) != EEPACC_ENOTSUP;
    bad += eepacc::fb_est_refusal("step", 0, C, false, true) != EEPACC_ENOTSUP;
    bad += eepacc::fb_est_refusal("build", 0, C, false, false) != EEPACC_OK;
    C.mb_any = 1; C.mb_mask[19] = 1;
    bad += eepacc::fb_est_refusal("step", 0, C, false, true) != EEPACC_ENOTSUP || g_msg.find("Mb[19]") == std::string::npos;
    C.bl_mode = 2;
    bad += eepacc::fb_est_refusal("build", 0, C, false, false) != EEPACC_ENOTSUP;
    double Tv[63]; int32_t idx[63]; double frac[63];
    for (int k = 0; k < 63; ++k) Tv[k] = 0.3 + 0.01 * k;
    eepacc::preview_tables(Tv, 63, idx, frac);
    bad += idx[0] != 0 || frac[0] != 0.0;
    printf("fb_est_harness: %d failed\n", bad);
    return bad;
}
#endif
