// Stand-alone host program for a sanitizer build (tests/test_cfg_cpu.py): calls the settings translation of
// csrc/eepacc_cfg.cpp at the edges of the fixed arrays of DevCfg, every input array allocated at exactly the length the
// settings name, so that a read or write past either end is caught.  Exit status 0: everything was as expected.
#include <stdio.h>
#include <string.h>
#include <string>
#include <vector>
#include "eepacc_cfg.h"

static std::string g_msg;
namespace eepacc { int set_error(int code, const std::string& msg) { g_msg = msg; return code; } }

static int g_failed = 0;
static void expect(bool ok, const char* what) {
    if (!ok) { fprintf(stderr, "cfg_sanitize: %s (message: %s)\n", what, g_msg.c_str()); g_failed = 1; }
}

int main() {
    const int N = eepacc::kMaxN, K = eepacc::kMaxKnots, nStop = eepacc::kMaxStops, nTL = eepacc::kMaxTL;
    std::vector<double> Tvec(N), s_tab(K), v_tab(K), curv(K), slope(K), stop(nStop), TL(4 * nTL);
    std::vector<int32_t> Mb(N, 1);
    Mb[0] = 0;                                              // one block over the whole horizon
    for (int k = 0; k < N; ++k) Tvec[k] = 0.25 + 0.01 * k;
    for (int i = 0; i < K; ++i) { s_tab[i] = 50.0 * i; v_tab[i] = 10.0 + 0.1 * i; curv[i] = 1e-3 * (i + 1); slope[i] = 1e-3 * (i % 5); }
    for (int i = 0; i < nStop; ++i) stop[i] = 120.0 * (i + 1);
    for (int i = 0; i < 4 * nTL; ++i) TL[i] = 10.0 * (i + 1);

    eepacc_settings S;
    memset(&S, 0, sizeof(S));
    S.N_hor = N; S.Tvec = Tvec.data(); S.Mb = Mb.data();
    for (int i = 0; i < 7; ++i) { S.W_AB[i] = 1.0 + i; S.W_FB[i] = 2.0 + i; }
    S.ab_fuel_term = 2;                                     // ICE map
    S.tau_min = 0.5; S.h_min = 2.0; S.s_goal = 1e9;
    S.paramEstSetting = 2; S.TVestSetting = 1; S.tConstACC_ego = 3.0; S.tConstACC_tar = 5.0;
    S.N_integratePlant = 10; S.solverToUse = 1; S.FBuseTaylor = 1;
    for (int i = 0; i < 6; ++i) S.b_quadr[i] = 0.1 * (i + 1);
    for (int i = 0; i < 21; ++i) S.b_fifthOrder[i] = 0.01 * (i + 1);
    S.n_speedLim = K; S.s_speedLim = s_tab.data(); S.v_speedLim = v_tab.data();
    S.n_curv = K; S.s_curv = s_tab.data(); S.curvature = curv.data();
    S.n_slope = K; S.s_slope = s_tab.data(); S.slope = slope.data();
    S.n_stop = nStop; S.stopLoc = stop.data();
    S.n_TL = nTL; S.TLLoc = TL.data();
    S.stopRefDist = 100.0; S.stopRefVelSlope = 1.0; S.stopVel = 0.2; S.TLstopVel = -1.0; S.TLStopRegionSize = 2.0;
    S.alpha_TTL = 3.34;

    eepacc_vehicle V;
    memset(&V, 0, sizeof(V));
    V.m = 2620.0; V.lambda = 1.05; V.g = 9.81; V.R_w = 0.361; V.phi = 26.8; V.F0 = 275.0; V.F2 = 1.3;
    V.p00 = -1.178; V.p10 = 0.1154; V.p01 = 0.001764; V.k00 = -2.134; V.k10 = 0.01164; V.k01 = 0.01041;
    V.tau_fd = 3.615; V.eta_drive = 0.88; V.v_max = 41.0;
    for (int i = 0; i < 7; ++i) V.upSpd[i] = 4.0 * (i + 1);
    for (int i = 0; i < 8; ++i) V.tau_gb[i] = 4.7 - 0.5 * i;

    eepacc::DevCfg C;
    std::vector<double> Hinv;
    expect(eepacc::build_cfg(&S, &V, C, Hinv) == EEPACC_OK, "the settings at the limits were refused");
    expect(Hinv.size() == (size_t)N * N, "Hinv is not N x N");
    expect(C.mb_maxlen == N && C.mb_end[0] == N - 1 && C.mb_lead[N - 1] == 0 && C.mb_lead[N] == N, "block maps of one block over the horizon");
    expect(C.fb_row0[N] == 26 * N + 2 * (N - 1), "FBMPC row layout");
    expect(C.s_slope[K - 1] == s_tab[K - 1] && C.stopLoc[nStop - 1] == stop[nStop - 1] && C.TLLoc[4 * nTL - 1] == TL[4 * nTL - 1], "last table entries");
    const eepacc::KpiCfg Kc = eepacc::build_kpi_cfg(&S, &V);
    const eepacc::FollowCfg Fc = eepacc::build_follow_cfg(&S, &V);
    expect(Kc.n_speedLim == K && Kc.v_speedLim[K - 1] == v_tab[K - 1], "KpiCfg speed-limit table");
    expect(Fc.w[EEPACC_FKPI_W_FB][6] == S.W_FB[6] && Fc.w[EEPACC_FKPI_W_AB][6] == S.W_AB[4], "FollowCfg weights");

    // one entry above each limit: refused before any table is read
    int32_t* const sizes[] = {&S.n_speedLim, &S.n_curv, &S.n_slope, &S.n_stop, &S.n_TL};
    for (int32_t* n : sizes) {
        const int32_t keep = *n;
        *n = keep + 1;
        g_msg.clear();
        expect(eepacc::build_cfg(&S, &V, C, Hinv) == EEPACC_EINVAL && g_msg == "route table sizes out of range", "a table above its limit was not refused");
        *n = keep;
    }
    return g_failed;
}
