// Host harness of the RouteCfg translation of csrc/eepacc_cfg.cpp (tests/test_route_table_cpu.py): hands build_cfg and
// build_route_cfg the PODs of include/eepacc.h and returns the raw bytes of the table.  Plain C++, no HIP, no device.
#include <stddef.h>
#include <string.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

using eepacc::RouteCfg;

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

struct Field { const char* name; size_t offset, bytes; };
#define RH_FIELD(f) {#f, offsetof(RouteCfg, f), sizeof(RouteCfg::f)}
static const Field kFields[] = {
    RH_FIELD(Ts), RH_FIELD(n_speedLim), RH_FIELD(n_curv), RH_FIELD(n_stop), RH_FIELD(n_TL), RH_FIELD(bl_mode), RH_FIELD(pad),
    RH_FIELD(s_speedLim), RH_FIELD(v_speedLim), RH_FIELD(s_curv), RH_FIELD(vcurv_tab), RH_FIELD(stopLoc), RH_FIELD(TLLoc),
    RH_FIELD(stopRefDist), RH_FIELD(stopRefVelSlope), RH_FIELD(stopVel), RH_FIELD(TLstopVel), RH_FIELD(TLStopRegionSize),
    RH_FIELD(bl_aLo), RH_FIELD(bl_aHi), RH_FIELD(bl_jLo), RH_FIELD(bl_jHi)};

extern "C" {

const char* rh_last_error(void) { return g_msg.c_str(); }
int rh_sizeof(void) { return (int)sizeof(RouteCfg); }
int rh_num_fields(void) { return (int)(sizeof(kFields) / sizeof(kFields[0])); }

// field i of the table above: its name, where it lies and how long it is
const char* rh_field(int i, int* offset, int* bytes) {
    *offset = (int)kFields[i].offset; *bytes = (int)kFields[i].bytes;
    return kFields[i].name;
}

// build_cfg (the validation) and, where it accepts the settings, build_route_cfg into route [sizeof RouteCfg]
int rh_build(const eepacc_settings* S, const eepacc_vehicle* V, void* route) {
    g_msg.clear();
    eepacc::DevCfg C;
    std::vector<double> Hinv;
    const int rc = eepacc::build_cfg(S, V, C, Hinv);
    if (rc != EEPACC_OK) return rc;
    const RouteCfg R = eepacc::build_route_cfg(S, V);
    memcpy(route, &R, sizeof(R));
    return rc;
}

}  // extern "C"
