// Stand-alone host program for a sanitizer build (tests/test_route_table_cpu.py): calls build_route_cfg of
// csrc/eepacc_cfg.cpp with every route table at the limit of the fixed arrays of RouteCfg and with none at all, every input
// array allocated at exactly the length the settings name, so that a read or write past either end is caught.  Exit status
// 0: everything was as expected.
#include <math.h>
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

static int g_failed = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "route_cfg_sanitize: %s\n", what); g_failed = 1; }
}

int main() {
    const int K = eepacc::kMaxKnots, nStop = eepacc::kMaxStops, nTL = eepacc::kMaxTL;
    std::vector<double> Tvec(2, 0.3), s_tab(K), v_tab(K), curv(K), stop(nStop), TL(4 * nTL);
    for (int i = 0; i < K; ++i) { s_tab[i] = 50.0 * i; v_tab[i] = 10.0 + 0.1 * i; curv[i] = i % 3 ? 1e-3 * (i + 1) : 0.0; }
    for (int i = 0; i < nStop; ++i) stop[i] = 120.0 * (i + 1);
    for (int i = 0; i < 4 * nTL; ++i) TL[i] = 10.0 * (i + 1);

    eepacc_settings S;
    memset(&S, 0, sizeof(S));
    S.N_hor = 2; S.Tvec = Tvec.data();
    S.n_speedLim = K; S.s_speedLim = s_tab.data(); S.v_speedLim = v_tab.data();
    S.n_curv = K; S.s_curv = s_tab.data(); S.curvature = curv.data();
    S.n_stop = nStop; S.stopLoc = stop.data();
    S.n_TL = nTL; S.TLLoc = TL.data();
    S.stopRefDist = 100.0; S.stopRefVelSlope = 1.0; S.stopVel = 0.2; S.TLstopVel = -1.0; S.TLStopRegionSize = 2.0;
    S.alpha_TTL = 3.34;
    S.bl_mode = 1; S.BL_a_LimLowVel = 3.0; S.BL_a_LimHighVel = 2.0; S.BL_j_LimLowVel = 3.0; S.BL_j_LimHighVel = 1.5;
    eepacc_vehicle V;
    memset(&V, 0, sizeof(V));

    eepacc::RouteCfg R = eepacc::build_route_cfg(&S, &V);
    expect(R.Ts == 0.3 && R.n_speedLim == K && R.n_curv == K && R.n_stop == nStop && R.n_TL == nTL && R.bl_mode == 1, "sizes");
    expect(R.s_speedLim[K - 1] == s_tab[K - 1] && R.v_speedLim[K - 1] == v_tab[K - 1] && R.s_curv[K - 1] == s_tab[K - 1], "last knots");
    expect(R.vcurv_tab[K - 1] == 3.34 * pow(fabs(curv[K - 1]), -1.0 / 3.0) && isinf(R.vcurv_tab[0]) && R.vcurv_tab[0] > 0, "curve speeds");
    expect(R.stopLoc[nStop - 1] == stop[nStop - 1] && R.TLLoc[4 * nTL - 1] == TL[4 * nTL - 1], "last stop and light");
    expect(R.stopRefDist == 100.0 && R.stopRefVelSlope == 1.0 && R.stopVel == 0.2 && R.TLstopVel == -1.0 && R.TLStopRegionSize == 2.0, "constants");
    expect(R.bl_aLo == 3.0 && R.bl_aHi == 2.0 && R.bl_jLo == 3.0 && R.bl_jHi == 1.5, "baseline limits");

    // a route with no feature: one-knot tables, no stops, no lights, and null pointers where the counts are zero
    S.n_speedLim = 1; S.n_curv = 1; S.n_stop = 0; S.stopLoc = nullptr; S.n_TL = 0; S.TLLoc = nullptr; S.bl_mode = 0;
    std::vector<double> one_s(1, 0.0), one_v(1, 13.5), one_c(1, 1e-6);
    S.s_speedLim = one_s.data(); S.v_speedLim = one_v.data(); S.s_curv = one_s.data(); S.curvature = one_c.data();
    R = eepacc::build_route_cfg(&S, &V);
    expect(R.n_stop == 0 && R.n_TL == 0 && R.v_speedLim[0] == 13.5 && R.v_speedLim[1] == 0.0 && R.stopLoc[0] == 0.0 && R.TLLoc[0] == 0.0, "empty route");
    return g_failed;
}
