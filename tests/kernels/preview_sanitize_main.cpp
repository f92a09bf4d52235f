// Stand-alone host program: eepacc::preview_tables (eepacc_cfg.cpp) at the edges of its arrays, built with
// -fsanitize=address,undefined and run as a program of its own (tests/test_ab_est_cpu.py).  The output arrays are heap
// blocks of exactly N entries, so a write past stage N - 1 is caught.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

namespace eepacc { int set_error(int code, const std::string&) { return code; } }

static int check(const std::vector<double>& T, const std::vector<int32_t>& want_idx, const std::vector<double>& want_frac) {
    const int N = (int)T.size();
    std::vector<int32_t> idx((size_t)N, -1);
    std::vector<double> frac((size_t)N, -1.0);
    eepacc::preview_tables(T.data(), N, idx.data(), frac.data());
    for (int k = 0; k < N; ++k) {
        if (!(frac[k] >= 0.0 && frac[k] < 1.0) || idx[k] < 0) { printf("stage %d: idx %d frac %g\n", k, idx[k], frac[k]); return 1; }
        if (!want_idx.empty() && (idx[k] != want_idx[k] || frac[k] != want_frac[k])) {
            printf("stage %d: idx %d frac %.17g, expected %d, %.17g\n", k, idx[k], frac[k], want_idx[k], want_frac[k]);
            return 1;
        }
    }
    return 0;
}

int main() {
    int bad = 0;
    bad |= check({0.5, 0.75, 0.5, 1.0}, {0, 1, 2, 3}, {0.0, 0.0, 0.5, 0.5});
    bad |= check({0.3, 0.6, 0.9, 0.3, 0.6}, {0, 1, 3, 6, 7}, {0.0, 0.0, 0.0, 0.0, 0.0});      // the snap rule
    bad |= check({0.5, 0.5}, {0, 1}, {0.0, 0.0});                                               // N = 2
    std::vector<double> geo(63), uni(63, 0.3);
    for (int k = 0; k < 63; ++k) geo[k] = 0.5 * pow(3.0, k / 62.0);
    bad |= check(geo, {}, {});                                                                  // N = 63, fractional indices
    std::vector<int32_t> iu(63); for (int k = 0; k < 63; ++k) iu[k] = k;
    bad |= check(uni, iu, std::vector<double>(63, 0.0));
    if (!bad) printf("preview_tables: ok\n");
    return bad;
}
