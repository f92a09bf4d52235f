// Stand-alone host program for a sanitizer build (tests/test_classes_build_cpu.py), as cfg_sanitize_main.cpp: calls the row
// catalogue of eepacc_classes_build_qp (csrc/eepacc_cfg.cpp) with the output arrays allocated at exactly nC of the handle, at
// the longest horizon and at the shortest, for every kind of class, so that a write past either end is caught.  Exit status 0:
// everything was as expected.
#include <stdio.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

static int g_failed = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "classes_rows_sanitize: %s (message: %s)\n", what, g_msg.c_str()); g_failed = 1; }
}

static void check(const std::vector<eepacc::QpRowsCfg>& c, const char* what) {
    const int n = (int)c.size(), nC = eepacc::classes_qp_max_rows(c.data(), n);
    for (int cls = 0; cls < n; ++cls) {
        std::vector<int32_t> stage((size_t)nC, 77), type((size_t)nC, 77);      // exactly nC: nothing to spare
        expect(eepacc::classes_qp_rows(c.data(), n, cls, stage.data(), type.data()) == EEPACC_OK, what);
        const int own = eepacc::classes_qp_num_rows(c[(size_t)cls]);
        expect(own <= nC, "a class has more rows than the handle");
        for (int r = 0; r < nC; ++r) {
            const bool pad = r >= own;
            expect(pad ? (stage[(size_t)r] == -1 && type[(size_t)r] == -1)
                       : (stage[(size_t)r] >= 0 && stage[(size_t)r] <= c[(size_t)cls].N && type[(size_t)r] >= 0), what);
        }
    }
    int32_t none = 0;
    g_msg.clear();
    expect(eepacc::classes_qp_rows(c.data(), n, n, &none, &none) == EEPACC_EINVAL && none == 0 && !g_msg.empty(), "cls = n_classes was not refused");
    expect(eepacc::classes_qp_rows(c.data(), n, -1, &none, &none) == EEPACC_EINVAL && none == 0, "cls = -1 was not refused");
}

int main() {
    const int Ns[] = {2, eepacc::kMaxN};
    for (int N : Ns) {
        check({{N, 0, 0}, {N, 0, 1}, {N, 0, 0}}, "ABMPC classes with and without route rows");
        check({{N, 0, 0}}, "one ABMPC class");
        check({{N, 0, 1}}, "one ABMPC class with route rows");
        check({{N, 1, 0}, {N, 1, 1}}, "baseline classes");
        check({{N, 2, 0}, {N, 2, 0}, {N, 2, 1}}, "target-vehicle classes");
    }
    expect(eepacc::classes_qp_max_rows(nullptr, 0) == 0, "no classes");
    return g_failed;
}
