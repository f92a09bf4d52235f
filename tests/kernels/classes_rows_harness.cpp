// Host harness of the row catalogue of eepacc_classes_build_qp in csrc/eepacc_cfg.cpp (tests/test_classes_build_cpu.py), as
// cfg_harness.cpp is of the settings translation: hands the catalogue the three numbers it reads of every class and returns
// the code, the message and the arrays it filled.  Plain C++, no HIP, no device.
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

static std::vector<eepacc::QpRowsCfg> classes(int n, const int32_t* N, const int32_t* bl_mode, const int32_t* route_rows) {
    std::vector<eepacc::QpRowsCfg> c((size_t)n);
    for (int k = 0; k < n; ++k) c[(size_t)k] = eepacc::QpRowsCfg{N[k], bl_mode[k], route_rows[k]};
    return c;
}

extern "C" {

const char* cr_last_error(void) { return g_msg.c_str(); }

// rows of class cls alone, and nC of the handle
int cr_num_rows(int n, const int32_t* N, const int32_t* bl_mode, const int32_t* route_rows, int cls) {
    return eepacc::classes_qp_num_rows(classes(n, N, bl_mode, route_rows)[(size_t)cls]);
}
int cr_max_rows(int n, const int32_t* N, const int32_t* bl_mode, const int32_t* route_rows) {
    const auto c = classes(n, N, bl_mode, route_rows);
    return eepacc::classes_qp_max_rows(c.data(), n);
}

// stage, type [cr_max_rows]
int cr_rows(int n, const int32_t* N, const int32_t* bl_mode, const int32_t* route_rows, int cls, int32_t* stage, int32_t* type) {
    g_msg.clear();
    const auto c = classes(n, N, bl_mode, route_rows);
    return eepacc::classes_qp_rows(c.data(), n, cls, stage, type);
}

// what qp_rows_cfg takes of a DevCfg
void cr_of_devcfg(int N, int bl_mode, int route_rows, int32_t* out3) {
    eepacc::DevCfg C{};
    C.N = N; C.bl_mode = bl_mode; C.ab_route_rows = route_rows;
    const eepacc::QpRowsCfg q = eepacc::qp_rows_cfg(C);
    out3[0] = q.N; out3[1] = q.bl_mode; out3[2] = q.ab_route_rows;
}

}  // extern "C"
