"""Plain-Python restatement of what every MPC step of the reference does before and after its QP, written from the .m files
(ABO/ = ACCMPC-ABO_CasADi/; the files of MATLAB_CasADi/ are the same), line numbers in the comments:

  EstimateVehicleTrajectory.m:55-80      estimate_trajectory       (paramEstSetting 0 and 1)
  EstimateRouteAndComfortBounds.m:89-207 route_and_comfort_bounds  (MPCtype 0, 1, 2), bounds_at_stage for one stage
  InterpPWA.m:14-27                      interp_pwa
  RunPlantModel.m:27-44                  plant_rk4                 (numpy fp64, or mpmath at 50 digits)

It is the reference of tests/test_gpu_stage.py, which calls the device functions of csrc/eepacc_stage.h one at a time.  It
takes the reference's OPTsettings as a dict and shares nothing with the device code, the settings translation or the C
oracle: loops, comparisons and the order of the arithmetic are the reference's.  Scalars are Python floats (IEEE double),
so a sum or product rounds exactly as MATLAB's does.

Not restated: the gear lookup (:63-66) and the slope_est loop (:72-86) of EstimateRouteAndComfortBounds.m, and the estimator
branch that reuses the previous solution (:81-88)."""
import math

import numpy as np

MP_DIGITS = 50


def _vec(a):
    return [float(x) for x in np.asarray(a, dtype=np.float64).ravel()]


# ---------------------------------------------------------------------------------------------- InterpPWA.m
def interp_pwa(d, doms, vals):
    """InterpPWA.m:14-27.  On a one-knot table with d on the knot the reference leaves val unset (the loop of :20 is empty);
    this returns None there."""
    doms = doms if isinstance(doms, list) else _vec(doms)
    vals = vals if isinstance(vals, list) else _vec(vals)
    if d < doms[0]:                                                   # :14
        return vals[0]
    if d > doms[-1]:                                                  # :16
        return vals[-1]
    for i in range(len(doms) - 1):                                    # :20
        if d >= doms[i] and d <= doms[i + 1]:                         # :21
            f_interp = (d - doms[i]) / (doms[i + 1] - doms[i])        # :22
            return vals[i] + f_interp * (vals[i + 1] - vals[i])       # :23
    return None


# ---------------------------------------------------------------------------------------------- EstimateVehicleTrajectory.m
def estimate_trajectory(OPT, estSetting, s_curr, v_curr, a_curr):
    """EstimateVehicleTrajectory.m:20-80 -> s_est [N_hor + 1], v_est [N_hor + 1].  estSetting 0 (ego) and 1 (target) step
    with Tvec; 2 (TVMPC) and 3 (BLMPC) with their own constant Ts."""
    if estSetting == 2:                                               # :20-24
        mode, Ts, N = int(OPT["TV_trajEstSett"]), float(OPT["TV_Ts"]), int(OPT["TV_N_hor"])
    elif estSetting == 3:                                             # :25-29
        mode, Ts, N = int(OPT["BL_trajEstSett"]), float(OPT["BL_Ts"]), int(OPT["BL_N_hor"])
    else:                                                             # :30-39
        N, Tvec = int(OPT["N_hor"]), _vec(OPT["Tvec"])
        mode = int(OPT["paramEstSetting"] if estSetting == 0 else OPT["TVestSetting"])
    tConstACC = float(OPT["tConstACC_tar"] if estSetting == 1 else OPT["tConstACC_ego"])      # :42-46
    s_curr, v_curr, a_curr = float(s_curr), float(v_curr), float(a_curr)
    s_est, v_est = [0.0] * (N + 1), [0.0] * (N + 1)                   # :49-50
    if mode == 0:                                                     # :55-64
        s_est[0] = s_curr
        for i in range(2, N + 2):                                     # i as in the reference, 1-based
            if estSetting < 2:
                Ts = Tvec[i - 2]                                      # Tvec(i-1)
            s_est[i - 1] = s_est[i - 2] + Ts * v_curr
        v_est = [v_curr] * (N + 1)
    elif mode == 1:                                                   # :65-80
        s_est[0], v_est[0] = s_curr, v_curr
        for i in range(2, N + 2):
            if estSetting < 2:
                Ts = Tvec[i - 2]
            if i <= tConstACC / Ts and v_est[i - 2] + Ts * a_curr > 0:             # :73
                v_est[i - 1] = v_est[i - 2] + Ts * a_curr
            else:
                v_est[i - 1] = v_est[i - 2]
            s_est[i - 1] = s_est[i - 2] + Ts * v_est[i - 2]           # :78
    else:
        raise NotImplementedError("paramEstSetting 2 (:81-88) is not restated here")
    return np.array(s_est), np.array(v_est)


# ---------------------------------------------------------------------------------------------- EstimateRouteAndComfortBounds.m
def matlab_mod(x, m):
    """MATLAB's mod: mod(x, 0) = x, otherwise x - floor(x / m) * m, which has the sign of m"""
    return x if m == 0 else x - math.floor(x / m) * m


def _comfort(MPCtype, OPT, v):
    """:155-207 for one stage -> a_min, a_max, j_min, j_max"""
    if MPCtype == 0:                                                  # :155-172 ISO limits
        if v < 5:
            return -5.0, 4.0, -5.0, 5.0
        if v < 20:
            return -5.5 + v / 10, 14 / 3 - 2 * v / 15, -35 / 6 + v / 6, 35 / 6 - v / 6
        return -3.5, 2.0, -2.5, 2.5
    p = "BL" if MPCtype == 1 else "TV"                                # :173-189 and :190-207 differ in the prefix only
    aLo, aHi = float(OPT[p + "_a_LimLowVel"]), float(OPT[p + "_a_LimHighVel"])
    jLo, jHi = float(OPT[p + "_j_LimLowVel"]), float(OPT[p + "_j_LimHighVel"])
    if v < 5:
        return -aLo, aLo, -jLo, jLo
    if v < 20:
        a = (4 * aLo - aHi) / 3 + (aHi - aLo) / 15 * v
        j = (4 * jLo - jHi) / 3 + (jHi - jLo) / 15 * v
        return -a, a, -j, j
    return -aHi, aHi, -jHi, jHi


def _tables(OPT):
    TL = np.asarray(OPT.get("TLLoc", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4)
    return dict(s_speedLim=_vec(OPT["s_speedLim"]), v_speedLim=_vec(OPT["v_speedLim"]), s_curv=_vec(OPT["s_curv"]),
                curvature=_vec(OPT["curvature"]), stopLoc=_vec(OPT.get("stopLoc", [])), TLLoc=[_vec(r) for r in TL],
                **{k: float(OPT[k]) for k in ("stopRefDist", "stopRefVelSlope", "stopVel", "TLstopVel", "TLStopRegionSize",
                                              "alpha_TTL")})


def bounds_at_stage(OPT, MPCtype, s, v, t_0, i, Tvec_i, T=None):
    """The bodies of the loops over the horizon of EstimateRouteAndComfortBounds.m:89-207 for the reference's 1-based stage i
    with s = s_est(i), v = v_est(i), Tvec_i = Tvec(i) -> dict of the eight bounds."""
    T = _tables(OPT) if T is None else T
    s, v, t_0 = float(s), float(v), float(t_0)
    s_sl, v_sl, s_cv, curv = T["s_speedLim"], T["v_speedLim"], T["s_curv"], T["curvature"]
    v_lim = 0.0                                                       # :89
    for j in range(1, len(s_sl) + 1):                                 # :91, j 1-based
        if j == len(s_sl):
            v_lim = s_sl[-1]                                          # :93 (s_speedLim, sic)
        elif s >= s_sl[j - 1] and s < s_sl[j]:                        # :94
            v_lim = v_sl[j - 1]
            break
    v_curv = 0.0                                                      # :102
    for j in range(1, len(s_cv) + 1):                                 # :104
        if j == len(s_cv):
            v_curv = T["alpha_TTL"] * abs(curv[-1]) ** (-1 / 3)       # :106
        elif s > s_cv[j - 1] and s < s_cv[j]:                         # :107
            v_curv = T["alpha_TTL"] * abs(curv[j - 1]) ** (-1 / 3)    # :108
            break
    v_stop = 1e5                                                      # :115
    for loc in T["stopLoc"]:                                          # :117
        dist = abs(loc - s)
        if dist < T["stopRefDist"]:                                   # :119
            v_stop = dist * T["stopRefVelSlope"] + T["stopVel"]
    v_TL = 1e5                                                        # :126
    for TL in T["TLLoc"]:                                             # :129
        if matlab_mod(t_0 + i * Tvec_i - TL[1], TL[2] + TL[3]) < TL[2]:            # :130 red
            d = TL[0] - s                                             # :131
            if abs(d) < T["stopRefDist"]:
                if d < 0:                                             # :133 behind the light
                    v_TL = abs(d) * T["stopRefVelSlope"] + T["TLstopVel"]
                elif abs(d) < T["TLStopRegionSize"]:                  # :135 close in front of it
                    v_TL = T["TLstopVel"]
                else:                                                 # :137 far in front of it
                    v_TL = abs(d - T["stopVel"]) * T["stopRefVelSlope"] + T["TLstopVel"]
    a_min, a_max, j_min, j_max = _comfort(MPCtype, OPT, v)
    return dict(v_lim=v_lim, v_curv=v_curv, v_stop=v_stop, v_TL=v_TL, a_min=a_min, a_max=a_max, j_min=j_min, j_max=j_max)


def route_and_comfort_bounds(OPT, s_est, v_est, t_0, MPCtype, N_hor=None):
    """EstimateRouteAndComfortBounds.m:89-207 -> dict of arrays [N_hor]: v_lim, v_curv, v_stop, v_TL, a_min, a_max, j_min,
    j_max.  N_hor defaults to what the caller of each MPCtype passes (N_hor, BL_N_hor, TV_N_hor)."""
    if N_hor is None:
        N_hor = int(OPT[("N_hor", "BL_N_hor", "TV_N_hor")[MPCtype]])
    Tvec = _vec(OPT["Tvec"])
    if len(Tvec) < N_hor:                                             # :55-58
        Tvec = [Tvec[0]] * N_hor
    T = _tables(OPT)
    rows = [bounds_at_stage(OPT, MPCtype, s_est[i - 1], v_est[i - 1], t_0, i, Tvec[i - 1], T) for i in range(1, N_hor + 1)]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


# ---------------------------------------------------------------------------------------------- RunPlantModel.m
def plant_rk4(OPT, V, s, v, u, mp=False):
    """RunPlantModel.m:15-44 with u the total force (:20) -> s_measured, v_measured.  The same scheme either in fp64 or, with
    mp = True, in mpmath at MP_DIGITS digits (the inputs and settings are the same doubles, taken exactly; the results are
    mpf).  The reference is the scheme, M steps of RK4, not the differential equation."""
    if mp:
        import mpmath
        with mpmath.workdps(MP_DIGITS):
            return _plant(OPT, V, s, v, u, mpmath.mpf, mpmath.sin, mpmath.cos)
    return _plant(OPT, V, s, v, u, float, math.sin, math.cos)


def _plant(OPT, V, s, v, u, num, sin, cos):
    s_slope, slope = [num(x) for x in _vec(OPT["s_slope"])], [num(x) for x in _vec(OPT["slope"])]        # :15-16
    M = int(OPT["N_integratePlant"])                                  # :17
    Ts = num(float(np.asarray(OPT["Tvec"]).ravel()[0]))               # :18
    lam, m, g, zeta_a, c_r = (num(float(V[k])) for k in ("lambda", "m", "g", "zeta_a", "c_r"))
    u_k = num(float(u))
    DT = Ts / M                                                       # :21
    x = (num(float(s)), num(float(v)))                                # :22

    def f_NL(x):                                                      # :41-44
        theta = interp_pwa(x[0], s_slope, slope)
        return (x[1], 1 / lam / m * (u_k - zeta_a * x[1] * x[1] - c_r * m * g * cos(theta) - m * g * sin(theta)))

    def axpy(a, k):                                                   # x_k + a * k
        return (x[0] + a * k[0], x[1] + a * k[1])

    for _ in range(M):                                                # :27-33
        k1 = f_NL(x)
        k2 = f_NL(axpy(DT / 2, k1))
        k3 = f_NL(axpy(DT / 2, k2))
        k4 = f_NL(axpy(DT, k3))
        x = (x[0] + DT / 6 * (k1[0] + 2 * k2[0] + 2 * k3[0] + k4[0]), x[1] + DT / 6 * (k1[1] + 2 * k2[1] + 2 * k3[1] + k4[1]))
    return x                                                          # :36-37
