// Host harness of csrc/eepacc_cfg.cpp (tests/cfg_harness.py, tests/test_cfg_cpu.py): hands the settings translation the PODs
// of include/eepacc.h and returns the code, the message and the raw bytes it produced.  Plain C++, no HIP, no device.
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

using eepacc::DevCfg;
using eepacc::KpiCfg;
using eepacc::FollowCfg;

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

struct Field { const char* name; size_t offset, bytes; };
#define CH_FIELD(f) {#f, offsetof(DevCfg, f), sizeof(DevCfg::f)}
static const Field kFields[] = {
    CH_FIELD(N), CH_FIELD(const_T), CH_FIELD(const_slope), CH_FIELD(mb_any), CH_FIELD(max_iter), CH_FIELD(Tvec), CH_FIELD(tau),
    CH_FIELD(w_a), CH_FIELD(w_j), CH_FIELD(cq), CH_FIELD(bl_eps), CH_FIELD(bl_mode), CH_FIELD(Hinv), CH_FIELD(pred), CH_FIELD(hb),
    CH_FIELD(mb_lead), CH_FIELD(mb_end), CH_FIELD(mb_maxlen), CH_FIELD(fb_row0), CH_FIELD(mb_mask),
    CH_FIELD(N_integratePlant), CH_FIELD(n_TL)};

extern "C" {

const char* ch_last_error(void) { return g_msg.c_str(); }

void ch_sizes(int* devcfg, int* kpi, int* follow) {
    *devcfg = (int)sizeof(DevCfg); *kpi = (int)sizeof(KpiCfg); *follow = (int)sizeof(FollowCfg);
}

// where a field of DevCfg lies; -1: no such field in the table above
int ch_field(const char* name, int* offset, int* bytes) {
    for (const Field& f : kFields)
        if (!strcmp(f.name, name)) { *offset = (int)f.offset; *bytes = (int)f.bytes; return 0; }
    return -1;
}

// build_cfg and, where it accepts the settings, the two key-figure tables.  cfg [sizeof DevCfg] is written in either case;
// hinv has room for 63 x 63 doubles and takes N x N.
int ch_build(const eepacc_settings* S, const eepacc_vehicle* V, void* cfg, double* hinv, void* kpi, void* follow) {
    g_msg.clear();
    DevCfg C;
    std::vector<double> Hinv;
    const int rc = eepacc::build_cfg(S, V, C, Hinv);
    memcpy(cfg, &C, sizeof(C));
    if (rc != EEPACC_OK) return rc;
    memcpy(hinv, Hinv.data(), Hinv.size() * sizeof(double));
    const KpiCfg K = eepacc::build_kpi_cfg(S, V);
    const FollowCfg F = eepacc::build_follow_cfg(S, V);
    memcpy(kpi, &K, sizeof(K));
    memcpy(follow, &F, sizeof(F));
    return rc;
}

}  // extern "C"
