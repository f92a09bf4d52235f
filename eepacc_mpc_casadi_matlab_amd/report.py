"""Key figures of a closed-loop run: the numbers ABO/Main.m:131-263 prints for one controller.

``kpi_report(optSol, OPTsettings)`` takes the struct returned by ``RunOpt_ABMPC`` / ``RunOpt_FBMPC``
(or a saved solution with the same fields) and returns them as a dict; ``format_report`` renders the
text block of Main.m for one controller.  ``kpi_table`` is the same for a batch, as a table: the specification of the
device operator eepacc_kpis (``Engine.kpis``); ``table_to_reports`` and ``summarise_table`` read such a table.
``follow_table`` is the specification of eepacc_follow_kpis (``Engine.follow_kpis``): the vehicle-following figures of
Main.m:679-771 and the final cost_* of RunOpt_ABMPC.m:382-404 / RunOpt_FBMPC.m:373-397, per instance.
``route_table`` and ``route_limits`` are the specification of eepacc_route_kpis (``Engine.route_kpis``): whether an
instance obeyed its route -- speed limits, curve speeds, stop signs, traffic lights (what Main.m:374-433 and :486-534 draw
for one run) -- and the comfort envelope, per instance.
Host-side numpy only.
"""
from __future__ import annotations

import math
from typing import Any, Dict

import numpy as np


def InterpPWA(d: float, doms, vals) -> float:
    """ABO/Functions/PWA_function_manipulation/InterpPWA.m:14-27."""
    doms = np.asarray(doms, dtype=np.float64); vals = np.asarray(vals, dtype=np.float64)
    if d < doms[0]:
        return float(vals[0])
    if d > doms[-1]:
        return float(vals[-1])
    for i in range(doms.size - 1):
        if doms[i] <= d <= doms[i + 1]:
            return float(vals[i] + (d - doms[i]) / (doms[i + 1] - doms[i]) * (vals[i + 1] - vals[i]))
    return float(vals[-1])


def _rms(x) -> float:
    x = np.asarray(x, dtype=np.float64)
    return float(np.sqrt(np.mean(x * x))) if x.size else 0.0


def kpi_report(sol: Dict[str, Any], OPT: Dict[str, Any]) -> Dict[str, float]:
    s = np.asarray(sol["s_opt"], dtype=np.float64).ravel()
    v = np.asarray(sol["v_opt"], dtype=np.float64).ravel()
    a = np.asarray(sol["a_opt"], dtype=np.float64).ravel()
    j = np.asarray(sol["j_opt"], dtype=np.float64).ravel()
    E = np.asarray(sol["E_opt"], dtype=np.float64).ravel()
    Ts = float(np.asarray(OPT["Tvec"]).ravel()[0])
    cut = float(OPT["cutOffDist"])
    # first sample pair that brackets the cut-off distance (1-based index as in Main.m:150-161)
    ind = 0
    for i in range(1, s.size):
        if s[i - 1] < cut and s[i] > cut:
            ind = i
            break
    if ind == 0:
        ind = s.size - 1
    vlim = InterpPWA(cut, OPT["s_speedLim"], OPT["v_speedLim"])                      # :133
    k = ind - 1                                                                     # MATLAB (ind-1), 1-based -> 0-based ind-2
    return {
        "bad_exit_messages": float(np.sum(np.asarray(sol["exitMessage"]))),           # :210
        "distance_km": s[-1] / 1e3,                                                  # :220
        "energy_kWh": E[-1] / 3.6e6,                                                 # :226
        "cutoff_index": float(ind),
        "speed_limit_error_at_cutoff": vlim - v[k - 1],                              # :232
        "energy_at_cutoff_kWh": E[k - 1] / 3.6e6,                                    # :245
        "travel_time_at_cutoff_s": 0.1 * round(ind * Ts * 10),                       # :238
        "a_max": float(a[:ind].max()), "a_min": float(a[:ind].min()), "a_rms": _rms(a[:ind]),       # :257
        "j_max": float(j[:ind].max()), "j_min": float(j[:ind].min()), "j_rms": _rms(j[:ind]),       # :261
    }


def _two_sum(a, b):
    s = a + b
    t = s - a
    return s, (a - (s - t)) + (b - t)


def _split(x):
    t = 134217729.0 * x                      # 2^27 + 1 (Veltkamp): x = hi + lo with 26-bit halves
    hi = t - (t - x)
    return hi, x - hi


def _fma(a, b, c):
    """The correctly rounded a * b + c of a fused multiply-add, for float64 arrays, in numpy: the exact product as a pair
    (Dekker / Veltkamp), the exact sum of c and its high part, the two low parts added with rounding to odd, one final
    rounding (Boldo and Melquiond, "Emulation of a FMA and correctly rounded sums", IEEE Trans. Computers 57, 2008).
    Exact away from overflow and from underflow of the product's low part, where the power surface stays."""
    a, b, c = [np.ascontiguousarray(x) for x in np.broadcast_arrays(*[np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in (a, b, c)])]
    (ah, al), (bh, bl) = _split(a), _split(b)
    uh = a * b
    ul = ((ah * bh - uh) + ah * bl + al * bh) + al * bl
    th, tl = _two_sum(c, uh)
    v, e = _two_sum(tl, ul)
    # to odd: an inexact sum whose last bit is even moves one step towards the part that was rounded off
    to_odd = (e != 0.0) & ((v.view(np.int64) & 1) == 0)
    v = np.where(to_odd, np.nextafter(v, np.where(e > 0.0, np.inf, -np.inf)), v)
    return th + v


def power_surface(b5, Fm, rpm):
    """The fifth-order battery-power surface of ABO/RunOpt_ABMPC.m:343-349 with the roundings of the device function of the
    same name (csrc/eepacc_power.h), which are those of eepacc_postprocess: plain products for the monomials, and every
    term added by one fused multiply-add, fma(c, m, acc) or fma(c * m1, m2, acc), in the order of the coefficient list."""
    bb = np.asarray(b5, dtype=np.float64).ravel()
    x = np.asarray(Fm, dtype=np.float64); y = np.asarray(rpm, dtype=np.float64)
    x2 = x * x; x3 = x2 * x; x4 = x3 * x; x5 = x4 * x
    y2 = y * y; y3 = y2 * y; y4 = y3 * y; y5 = y4 * y
    p = _fma(bb[1], x, bb[0])
    for c, m in ((bb[2], y), (bb[3], x2), (bb[4] * x, y), (bb[5], y2), (bb[6], x3), (bb[7] * x2, y), (bb[8] * x, y2),
                 (bb[9], y3), (bb[10], x4), (bb[11] * x3, y), (bb[12] * x2, y2), (bb[13] * x, y3), (bb[14], y4),
                 (bb[15], x5), (bb[16] * x4, y), (bb[17] * x3, y2), (bb[18] * x2, y3), (bb[19] * x, y4), (bb[20], y5)):
        p = _fma(c, m, p)
    return p


def kpi_table(s, v, Fm, a, status, Ts, cut, s_speedLim, v_speedLim, b5, phi, V) -> np.ndarray:
    """The key figures of kpi_report and fuel_economy for a batch, as a table [KPI_N, B] (rows: _abi.KPI_FIELDS) in raw SI
    units without rounding: the specification of eepacc_kpis (include/eepacc.h) in executable form, numpy on the host.

    s, v, Fm, a, status: [n, B] rows of a closed-loop trajectory; Ts = Tvec[0]; cut: cutOffDist, a scalar or [B]; the
    speed-limit table, the power fit b5, phi and the vehicle V are those of the instances' settings class (one class
    per call).  With P = power_surface(b5, Fm, 30/pi v phi) and E = Ts cumsum(P):

        bad_exits        count of status != 0                                            Main.m:210
        distance_m       s[n-1]                                                          :220
        energy_J         E[n-1]                                                          :226
        cutoff_index     ind: the first i >= 1 with s[i-1] < cut < s[i], else n-1        :150-161
        reached          1.0 where such an i exists, else 0.0
        vlim_err         InterpPWA(cut, s_speedLim, v_speedLim) - v[ind-2]               :133,232
        energy_cutoff_J  E[ind-2]                                                        :245
        time_cutoff_s    ind Ts                                                          :238
        a_max a_min a_rms   of a[0:ind]                                                  :257
        j_max j_min j_rms   of j[0:ind], j = diff(a) / Ts (n-1 entries)                  :261
        fuel_kg          last value of FC_tot of fuel_economy (first sample zero)        Custom_plots.m:81-90
        FE_L_per_100km   fuel_kg / 0.835 / (max(s) / 1000) * 100                         :100-107

    Two conventions where kpi_report is undefined: for ind < 2 the sample index ind-2 is taken as 0 (kpi_report's
    negative index wraps to the last sample); for n = 1 (ind = 0) the jerk figures are 0 and the acceleration figures
    are those of a[0]."""
    from ._abi import KPI, KPI_N
    s, v, Fm, a = [np.asarray(x, dtype=np.float64) for x in (s, v, Fm, a)]
    n, B = s.shape
    Ts = float(Ts)
    cut = np.broadcast_to(np.asarray(cut, dtype=np.float64).reshape(-1), (B,))
    cols = np.arange(B)
    cross = (s[:-1] < cut) & (s[1:] > cut)                                           # row i-1: the pair (i-1, i)
    reached = cross.any(axis=0)
    ind = np.where(reached, cross.argmax(axis=0) + 1, n - 1) if n > 1 else np.zeros(B, dtype=np.int64)
    k2 = np.maximum(ind - 2, 0)
    P = power_surface(b5, Fm, 30.0 / np.pi * v * phi)
    E = Ts * np.cumsum(P, axis=0)
    vlim = np.array([InterpPWA(float(c), s_speedLim, v_speedLim) for c in cut])
    k = np.arange(n)[:, None]
    in_a = k < np.maximum(ind, 1)[None, :]
    cnt = np.maximum(ind, 1).astype(np.float64)
    T = np.zeros((KPI_N, B))
    T[KPI["bad_exits"]] = (np.asarray(status) != 0).sum(axis=0)
    T[KPI["distance_m"]] = s[-1]
    T[KPI["energy_J"]] = E[-1]
    T[KPI["cutoff_index"]] = ind
    T[KPI["reached"]] = reached
    T[KPI["vlim_err"]] = vlim - v[k2, cols]
    T[KPI["energy_cutoff_J"]] = E[k2, cols]
    T[KPI["time_cutoff_s"]] = ind * Ts
    T[KPI["a_max"]] = np.where(in_a, a, -np.inf).max(axis=0)
    T[KPI["a_min"]] = np.where(in_a, a, np.inf).min(axis=0)
    T[KPI["a_rms"]] = np.sqrt(np.where(in_a, a * a, 0.0).sum(axis=0) / cnt)
    if n > 1:
        j = np.diff(a, axis=0) / Ts
        in_j = k[:-1] < ind[None, :]
        T[KPI["j_max"]] = np.where(in_j, j, -np.inf).max(axis=0)
        T[KPI["j_min"]] = np.where(in_j, j, np.inf).min(axis=0)
        T[KPI["j_rms"]] = np.sqrt(np.where(in_j, j * j, 0.0).sum(axis=0) / cnt)
    TW = np.maximum(0.0, (V["lambda"] * V["m"] * a + V["F0"] + V["F2"] * v * v) * V["R_w"])
    FC = np.maximum(0.25, V["p00"] + V["p10"] * v + V["p01"] * TW)
    FC[0] = 0.0
    T[KPI["fuel_kg"]] = np.cumsum(FC / 1000.0 * Ts, axis=0)[-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        T[KPI["FE_L_per_100km"]] = T[KPI["fuel_kg"]] / 0.835 / (s.max(axis=0) / 1000.0) * 100.0
    return T


def table_to_reports(table) -> list:
    """The dicts of kpi_report, one per column of a table of kpi_table / Engine.kpis: km and kWh, the 0.1 s rounding of
    the travel time (Main.m:238), plus reached, fuel_kg and FE_L_per_100km.  format_report renders each."""
    from ._abi import KPI
    T = np.asarray(table.cpu() if hasattr(table, "cpu") else table, dtype=np.float64)
    out = []
    for i in range(T.shape[1]):
        c = {name: float(T[row, i]) for name, row in KPI.items()}
        out.append({
            "bad_exit_messages": c["bad_exits"], "distance_km": c["distance_m"] / 1e3, "energy_kWh": c["energy_J"] / 3.6e6,
            "cutoff_index": c["cutoff_index"], "speed_limit_error_at_cutoff": c["vlim_err"],
            "energy_at_cutoff_kWh": c["energy_cutoff_J"] / 3.6e6,
            "travel_time_at_cutoff_s": 0.1 * round(c["time_cutoff_s"] * 10),
            "a_max": c["a_max"], "a_min": c["a_min"], "a_rms": c["a_rms"],
            "j_max": c["j_max"], "j_min": c["j_min"], "j_rms": c["j_rms"],
            "reached": c["reached"], "fuel_kg": c["fuel_kg"], "FE_L_per_100km": c["FE_L_per_100km"]})
    return out


def follow_weights(OPT: Dict[str, Any], weights: str = "ab") -> np.ndarray:
    """The seven weights [w_P, w_a, w_j, w_v, w_h, w_s, w_f] of follow_table's cost fields, as eepacc_follow_kpis selects
    them: "ab": W(1..5) of OPTsettings.W_AB with w_f = W(5) and w_P = 0 (RunOpt_ABMPC.m:383-388 -- in the ABO tree W(1) is
    w_FC, and the reference's cost_a uses it all the same); "fb": W_FB(1..7) (RunOpt_FBMPC.m:373-379); "none": ones, w_P = 0."""
    if weights == "ab":
        W = np.asarray(OPT["W_AB"], dtype=np.float64).ravel()
        return np.array([0.0, W[0], W[1], W[2], W[3], W[4], W[4]])
    if weights == "fb":
        return np.asarray(OPT["W_FB"], dtype=np.float64).ravel()[:7].copy()
    if weights == "none":
        return np.array([0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    raise ValueError("weights must be 'ab', 'fb' or 'none', got %r" % (weights,))


def follow_table(s, v, Fm, a, xi_v, xi_h, xi_s, xi_f, s_tv, v_tv, Ts, h_min, tau_min, W, b5, phi) -> np.ndarray:
    """The vehicle-following and cost key figures of a batch, as a table [FKPI_N, B] (rows: _abi.FKPI_FIELDS) in raw SI
    units: the specification of eepacc_follow_kpis (include/eepacc.h) in executable form, numpy on the host, serial over the
    steps with the operator's order of operations.

    s .. xi_f: [n, B] rows of a closed-loop trajectory; s_tv, v_tv: [n, B] the lead traces it was run on (TVlength
    subtracted, Main.m:88); Ts = Tvec[0]; h_min, tau_min: scalars or [B]; W: the seven weights [w_P, w_a, w_j, w_v, w_h,
    w_s, w_f] (follow_weights), [7] or [7, B]; b5, phi: the power fit and driveline of cost_P (one class per call).  With
    the gap h_k = s_tv[k] - s[k], the jerk j_k = (a[k+1] - a[k]) / Ts and a lead sample a k with s_tv[k] < 1e6 (Main.m:288):

        lead_samples       number of lead samples
        h_min_m            min h_k over the lead samples; +inf if none                               Main.m:692-739
        h_min_index        the first k that attains it; -1 if none
        thw_min_s          min h_k / v_k over the lead samples with v_k > 0; +inf if none            :752-764
        margin_min_m       min (h_k - max(h_min, v_k tau_min)) over the lead samples; +inf if none   :687
        margin_viol_steps  number of lead samples with that margin < 0
        ttc_min_s          min h_k / (v_k - v_tv[k]) over the lead samples that close in; +inf if none (not in the reference)
        xi_h_max           max xi_h[k] over all steps
        cost_P             w_P sum_{k<=n-2} P_k^2, P = power_surface(b5, Fm, 30/pi v phi); 0 where w_P = 0   RunOpt_FBMPC.m:383
        cost_a cost_j      w_a sum_{k<=n-2} a_k^2, w_j sum_{k<=n-2} j_k^2                            RunOpt_ABMPC.m:392-393
        cost_xi_v .. _f    w sum_{k<=n-2} xi[k]                                                      :394-397

    The minima, the maximum and the index are kept by `<` and `>` alone, so the first of equal gaps wins and a NaN is
    never taken; the sums are added in the order of k (the device adds slice by slice: they differ by rounding)."""
    from ._abi import FKPI, FKPI_N
    s, v, Fm, a, xi_v, xi_h, xi_s, xi_f, s_tv, v_tv = [np.asarray(x, dtype=np.float64) for x in (s, v, Fm, a, xi_v, xi_h, xi_s, xi_f, s_tv, v_tv)]
    n, B = s.shape
    Ts = float(Ts)
    h_min = np.broadcast_to(np.asarray(h_min, dtype=np.float64).reshape(-1), (B,))
    tau_min = np.broadcast_to(np.asarray(tau_min, dtype=np.float64).reshape(-1), (B,))
    W = np.broadcast_to(np.asarray(W, dtype=np.float64).reshape(7, -1), (7, B))
    hmin, thw, margin, ttc = [np.full(B, np.inf) for _ in range(4)]
    ximax = np.full(B, -np.inf)
    index = np.full(B, -1.0)
    lead, viol = np.zeros(B), np.zeros(B)
    sums = np.zeros((7, B))
    P = power_surface(b5, Fm, 30.0 / np.pi * v * phi) if (W[0] != 0.0).any() else np.zeros((n, B))
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for k in range(n):
            ximax = np.where(xi_h[k] > ximax, xi_h[k], ximax)
            is_lead = s_tv[k] < 1e6
            h = s_tv[k] - s[k]
            lead += is_lead
            take = is_lead & (h < hmin)
            hmin = np.where(take, h, hmin); index = np.where(take, float(k), index)
            t = h / v[k]
            thw = np.where(is_lead & (v[k] > 0.0) & (t < thw), t, thw)
            vt = v[k] * tau_min
            m = h - np.where(vt > h_min, vt, h_min)
            margin = np.where(is_lead & (m < margin), m, margin)
            viol += is_lead & (m < 0.0)
            dv = v[k] - v_tv[k]
            c = h / dv
            ttc = np.where(is_lead & (dv > 0.0) & (c < ttc), c, ttc)
            if k + 1 < n:                                      # k = 1:N_sim of the reference, N_sim = n - 1
                j = (a[k + 1] - a[k]) / Ts
                sums += np.stack([P[k] * P[k], a[k] * a[k], j * j, xi_v[k], xi_h[k], xi_s[k], xi_f[k]])
    T = np.zeros((FKPI_N, B))
    T[FKPI["lead_samples"]] = lead
    T[FKPI["h_min_m"]] = hmin
    T[FKPI["h_min_index"]] = index
    T[FKPI["thw_min_s"]] = thw
    T[FKPI["margin_min_m"]] = margin
    T[FKPI["margin_viol_steps"]] = viol
    T[FKPI["ttc_min_s"]] = ttc
    T[FKPI["xi_h_max"]] = ximax
    cost = W * sums
    cost[0] = np.where(W[0] != 0.0, cost[0], 0.0)
    T[FKPI["cost_P"]:FKPI["cost_xi_f"] + 1] = cost
    return T


def _route_tables(OPT: Dict[str, Any]) -> Dict[str, Any]:
    """What eepacc_route_kpis reads of a settings class (RouteCfg, csrc/eepacc_route_cfg.h), from OPTsettings: the route
    tables as Python floats, the curve speeds alpha_TTL |curvature|^(-1/3) through the C library's pow, as the settings
    translation computes them (inf where the curvature is 0)."""
    vec = lambda x: [float(y) for y in np.asarray(x, dtype=np.float64).ravel()]
    alpha = float(OPT["alpha_TTL"])
    TL = np.asarray(OPT.get("TLLoc", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4)
    return dict(s_speedLim=vec(OPT["s_speedLim"]), v_speedLim=vec(OPT["v_speedLim"]), s_curv=vec(OPT["s_curv"]),
                vcurv_tab=[alpha * (math.pow(abs(c), -1.0 / 3.0) if c != 0.0 else math.inf) for c in vec(OPT["curvature"])],
                stopLoc=vec(OPT.get("stopLoc", [])), TLLoc=[vec(r) for r in TL],
                **{k: float(OPT[k]) for k in ("stopRefDist", "stopRefVelSlope", "stopVel", "TLstopVel", "TLStopRegionSize")})


def _held_table(s, knots, vals):
    """vals[j] on knots[j] <= s < knots[j+1], vals[0] before the first knot (and for a NaN), vals[-1] from the last on"""
    out = np.full(s.shape, vals[0])
    for x, y in zip(knots, vals):
        out = np.where(s >= x, y, out)
    return out


def _is_red(t, TL):
    """MATLAB's mod(t - TL(2), TL(3) + TL(4)) < TL(3); a cycle of length 0 returns its argument"""
    x = t - TL[1]
    mm = TL[2] + TL[3]
    return (x if mm == 0.0 else x - math.floor(x / mm) * mm) < TL[2]


def _route_limits(s, t, R):
    """The four caps [4, B] of one sample: positions s [B] at the time t"""
    v_lim = _held_table(s, R["s_speedLim"], R["v_speedLim"])
    v_curv = _held_table(s, R["s_curv"], R["vcurv_tab"])
    v_stop = np.full(s.shape, np.inf if R["stopLoc"] else 1e5)
    for loc in R["stopLoc"]:
        x = np.abs(loc - s) * R["stopRefVelSlope"] + R["stopVel"]
        v_stop = np.where(x < v_stop, x, v_stop)
    v_TL = np.full(s.shape, np.inf)
    for TL in R["TLLoc"]:
        if not _is_red(t, TL):
            continue
        d = TL[0] - s
        ad = np.abs(d)
        x = np.where(d < 0.0, ad * R["stopRefVelSlope"] + R["TLstopVel"],                                  # :133 behind the light
                     np.where(ad < R["TLStopRegionSize"], R["TLstopVel"],                                  # :135 close in front
                              np.abs(d - R["stopVel"]) * R["stopRefVelSlope"] + R["TLstopVel"]))           # :137 far in front
        v_TL = np.where((ad < R["stopRefDist"]) & (x < v_TL), x, v_TL)
    v_TL = np.where(v_TL == np.inf, 1e5, v_TL)
    return np.stack([v_lim, v_curv, v_stop, v_TL])


def _comfort_envelope(v, OPT, bl_mode):
    """a_min, a_max, j_min, j_max [B] at the speeds v: EstimateRouteAndComfortBounds.m:154-172, or :173-189 with the
    baseline limits of OPT (BL_*_Lim*) where bl_mode != 0.  A NaN speed takes the last branch."""
    lo, mid = v < 5.0, v < 20.0
    pick = lambda a, b, c: np.where(lo, a, np.where(mid, b, c))
    if bl_mode:
        aLo, aHi, jLo, jHi = [float(OPT[k]) for k in ("BL_a_LimLowVel", "BL_a_LimHighVel", "BL_j_LimLowVel", "BL_j_LimHighVel")]
        a = pick(aLo, (4.0 * aLo - aHi) / 3.0 + (aHi - aLo) / 15.0 * v, aHi)
        j = pick(jLo, (4.0 * jLo - jHi) / 3.0 + (jHi - jLo) / 15.0 * v, jHi)
        return -a, a, -j, j
    return (pick(-5.0, -5.5 + v / 10.0, -3.5), pick(4.0, 14.0 / 3.0 - 2.0 * v / 15.0, 2.0),
            pick(-5.0, -35.0 / 6.0 + v / 6.0, -2.5), pick(5.0, 35.0 / 6.0 - v / 6.0, 2.5))


def route_limits(s, Ts, t_start, OPT) -> np.ndarray:
    """The per-sample output `limits` of eepacc_route_kpis, [n, RLIM_N, B] (rows: _abi.RLIM_FIELDS; [n, RLIM_N] for one
    instance given as s [n]): the sign-posted speed limit, the curve speed, the stop-sign profile of ABO/Main.m:375-385 and
    the red-light cap at every sample, at the positions s [n, B] and the times t_k = t_start + k Ts.  Definitions:
    include/eepacc.h, eepacc_route_kpis; every product, sum and quotient is rounded once, as on the device."""
    s = np.asarray(s, dtype=np.float64)
    one = s.ndim == 1
    s = s.reshape(s.shape[0], -1)
    R = _route_tables(OPT)
    Ts, t_start = float(Ts), float(t_start)
    L = np.stack([_route_limits(s[k], t_start + k * Ts, R) for k in range(s.shape[0])])
    return L[:, :, 0] if one else L


def route_table(s, v, a, Ts, t_start, tol, OPT, bl_mode=0) -> np.ndarray:
    """The route-compliance key figures of a batch, as a table [RKPI_N, B] (rows: _abi.RKPI_FIELDS; [RKPI_N] for one
    instance given as vectors [n]) in raw SI units: the specification of eepacc_route_kpis (include/eepacc.h) in executable
    form, numpy on the host, serial over the steps.

    s, v, a: [n, B] rows of a closed-loop trajectory; Ts = Tvec[0]; t_start: the time of row 0; tol = (v_tol, a_tol,
    j_tol); OPT: the settings of the instances' class (one class per call); bl_mode: that of the handle (the comfort
    envelope of the baseline controllers where it is not 0).  With the caps v_lim, v_curv, v_stop, v_TL of route_limits at
    every sample, the comfort envelope a_min .. j_max at v_k and the jerk j_k = (a[k+1] - a[k]) / Ts for k <= n-2:

        vlim_excess_max  vlim_excess_index  vlim_viol_steps   max (v_k - v_lim_k); the first k that attains it (-1 if no
                                                              sample is taken); the number of k with v_k - v_lim_k > v_tol
        vcurv_excess_max vcurv_viol_steps                     the same against v_curv
        vstop_excess_max vstop_viol_steps                     the same against v_stop
        vtl_excess_max   vtl_viol_steps                       the same against v_TL over the samples with v_TL < 1e5
        stops_passed     stop_cross_v_max                     pairs (k >= 1, stop j) with s[k-1] < stopLoc_j <= s[k]; the
                                                              largest min(v[k-1], v[k]) over them
        tl_passed  red_crossings  red_crossings_possible      such pairs with a light; those with it red at t_{k-1} and t_k;
        red_cross_first_index                                 those with it red at either; the first k of the latter, else -1
        a_over_max a_under_max j_over_max j_under_max         max (a_k - a_max), max (a_min - a_k), the same for the jerk
        comfort_viol_steps                                    k with an acceleration excess > a_tol or a jerk excess > j_tol
        v_min                                                 min v_k

    Maxima and the minimum are kept by `>` and `<` from -inf and +inf, so the first of equal values wins and a NaN is
    never taken and never counted; there are no sums: the device's table equals this one bit for bit."""
    from ._abi import RKPI, RKPI_N
    s, v, a = [np.asarray(x, dtype=np.float64) for x in (s, v, a)]
    one = s.ndim == 1
    s, v, a = [x.reshape(x.shape[0], -1) for x in (s, v, a)]
    n, B = s.shape
    Ts, t_start = float(Ts), float(t_start)
    v_tol, a_tol, j_tol = [float(x) for x in tol]
    R = _route_tables(OPT)
    NINF = -np.inf
    ex = np.full((4, B), NINF)                                        # excess maxima against v_lim, v_curv, v_stop, v_TL
    viol = np.zeros((4, B))
    index = np.full(B, -1.0)
    stops, lights, red, red_poss, comfort = [np.zeros(B) for _ in range(5)]
    red_first = np.full(B, -1.0)
    cross_v, a_over, a_under, j_over, j_under = [np.full(B, NINF) for _ in range(5)]
    v_min = np.full(B, np.inf)
    with np.errstate(invalid="ignore", over="ignore"):
        for k in range(n):
            t = t_start + k * Ts
            caps = _route_limits(s[k], t, R)
            for i in range(4):
                e = v[k] - caps[i]
                live = caps[i] < 1e5 if i == 3 else np.ones(B, dtype=bool)
                take = live & (e > ex[i])
                if i == 0:
                    index = np.where(take, float(k), index)
                ex[i] = np.where(take, e, ex[i])
                viol[i] += live & (e > v_tol)
            v_min = np.where(v[k] < v_min, v[k], v_min)
            if k >= 1:
                t_prev = t_start + (k - 1) * Ts
                slow = np.where(v[k] < v[k - 1], v[k], v[k - 1])
                for loc in R["stopLoc"]:
                    c = (s[k - 1] < loc) & (loc <= s[k])
                    stops += c
                    cross_v = np.where(c & (slow > cross_v), slow, cross_v)
                for TL in R["TLLoc"]:
                    c = (s[k - 1] < TL[0]) & (TL[0] <= s[k])
                    r0, r1 = _is_red(t_prev, TL), _is_red(t, TL)
                    lights += c
                    red += c & (r0 and r1)
                    red_poss += c & (r0 or r1)
                    red_first = np.where(c & (r0 or r1) & (red_first < 0.0), float(k), red_first)
            a_min, a_max, j_min, j_max = _comfort_envelope(v[k], OPT, bl_mode)
            eo, eu = a[k] - a_max, a_min - a[k]
            a_over = np.where(eo > a_over, eo, a_over)
            a_under = np.where(eu > a_under, eu, a_under)
            bad = (eo > a_tol) | (eu > a_tol)
            if k + 1 < n:
                j = (a[k + 1] - a[k]) / Ts
                eo, eu = j - j_max, j_min - j
                j_over = np.where(eo > j_over, eo, j_over)
                j_under = np.where(eu > j_under, eu, j_under)
                bad = bad | (eo > j_tol) | (eu > j_tol)
            comfort += bad
    T = np.zeros((RKPI_N, B))
    for i, name in enumerate(("vlim", "vcurv", "vstop", "vtl")):
        T[RKPI[name + "_excess_max"]] = ex[i]
        T[RKPI[name + "_viol_steps"]] = viol[i]
    T[RKPI["vlim_excess_index"]] = index
    T[RKPI["stops_passed"]] = stops
    T[RKPI["stop_cross_v_max"]] = cross_v
    T[RKPI["tl_passed"]] = lights
    T[RKPI["red_crossings"]] = red
    T[RKPI["red_crossings_possible"]] = red_poss
    T[RKPI["red_cross_first_index"]] = red_first
    T[RKPI["a_over_max"]] = a_over
    T[RKPI["a_under_max"]] = a_under
    T[RKPI["j_over_max"]] = j_over
    T[RKPI["j_under_max"]] = j_under
    T[RKPI["comfort_viol_steps"]] = comfort
    T[RKPI["v_min"]] = v_min
    return T[:, 0] if one else T


def summarise_table(table, class_of) -> Dict[str, np.ndarray]:
    """Per-class mean, minimum and maximum of every row of a table: {"classes": the class ids that occur, ascending [K],
    "count" [K], "mean" / "min" / "max" [K, rows]} (rows of the three in the table's order: _abi.KPI_FIELDS for a table
    of kpi_table / Engine.kpis, _abi.FKPI_FIELDS for one of follow_table / Engine.follow_kpis, _abi.RKPI_FIELDS for one of
    route_table / Engine.route_kpis).

    A table of follow_table holds +inf where an instance has no sample to take a minimum over (no lead, never closing).
    Such entries are kept as they are: the class's "max", and its "mean", are then +inf (never NaN: the fields that can
    be infinite are +inf only), and "min" is taken over the class's other instances.  Read "lead_samples" beside them.

    A table of route_table holds -inf where an instance has nothing to take a maximum over (no stop line crossed, no
    sample under a red light, one sample and so no jerk), and NaN nowhere.  Within one field the infinite entries all
    have the same sign, so a class's "mean" is -inf there (never NaN) and its "min" too; "max" is taken over the class's
    other instances.  Read "stops_passed", "vtl_viol_steps" and the indices (-1: none) beside them."""
    T = np.asarray(table.cpu() if hasattr(table, "cpu") else table, dtype=np.float64)
    class_of = np.asarray(class_of).reshape(-1)
    if class_of.size != T.shape[1]:
        raise ValueError(f"class_of needs one entry per column of the table ({T.shape[1]}), got {class_of.size}")
    classes = np.unique(class_of)
    cols = [T[:, class_of == c] for c in classes]
    return {"classes": classes, "count": np.array([x.shape[1] for x in cols]),
            "mean": np.array([x.mean(axis=1) for x in cols]), "min": np.array([x.min(axis=1) for x in cols]),
            "max": np.array([x.max(axis=1) for x in cols])}


def format_report(name: str, k: Dict[str, float], OPT: Dict[str, Any]) -> str:
    cut = float(OPT["cutOffDist"]) / 1e3
    return "\n".join([
        f"=== RESULTS of UC{OPT.get('useCaseNum', 0)} ===", "",
        "Feasibility:", f"   {name}: {k['bad_exit_messages']:g} bad exit messages", "",
        "Distance traveled:", f"   {name}: {k['distance_km']:.5g} km", "",
        "Energy consumption:", f"   {name}: {k['energy_kWh']:.5g} kWh", "",
        f"Error relative to the speed limit at {cut:g} km:", f"   {name}: {k['speed_limit_error_at_cutoff']:.5g} m/s", "",
        f"Energy consumption at {cut:g} km:", f"   {name}: {k['energy_at_cutoff_kWh']:.5g} kWh", "",
        f"Travel time at {cut:g} km:", f"   {name}: {k['travel_time_at_cutoff_s']:g} s", "",
        f"Comfort metrics at {cut:g} km:",
        f"   {name}: max. a = {k['a_max']:.5g}m/s2, min. a = {k['a_min']:.5g}m/s2, rms. a = {k['a_rms']:.5g}m/s2",
        f"   {name}: max. j = {k['j_max']:.5g}m/s3, min. j = {k['j_min']:.5g}m/s3, rms. j = {k['j_rms']:.5g}m/s3", ""])


def fuel_economy(sol: Dict[str, Any], V: Dict[str, float], Ts: float = 0.5) -> Dict[str, Any]:
    """Fuel consumption of a closed-loop run with the linear fuel map of the ABO tree (ABO/Custom_plots.m:73-107):
    wheel torque TW = max(0, (lambda m a + F0 + F2 v^2) R_w), fuel flow FC = max(0.25, p00 + p10 v + p01 TW) [g/s],
    cumulative fuel [kg] with the sample time Ts (0.5 s in the reference) and fuel economy [L/100 km] at a density of
    0.835 kg/L.  sol: struct with a_opt, v_opt, s_opt (RunOpt_ABMPC / a saved solution)."""
    a = np.asarray(sol["a_opt"], dtype=np.float64).ravel()
    v = np.asarray(sol["v_opt"], dtype=np.float64).ravel()
    s = np.asarray(sol["s_opt"], dtype=np.float64).ravel()
    TW = np.maximum(0.0, (V["lambda"] * V["m"] * a + V["F0"] + V["F2"] * v * v) * V["R_w"])
    FC = np.maximum(0.25, V["p00"] + V["p10"] * v + V["p01"] * TW)
    TW[0] = 0.0; FC[0] = 0.0                        # the loop starts at i = 2 (:81): the first sample stays zero
    FC_tot = np.cumsum(FC / 1000.0 * Ts)
    return {"TW_opt": TW, "FC": FC, "FC_tot_kg": FC_tot,
            "FE_L_per_100km": float(np.max(FC_tot / 0.835) / np.max(s / 1000.0) * 100.0)}


def fuel_economy_of_speed_trace(V_2Hz, V: Dict[str, float], Ts: float = 0.5) -> float:
    """The same figure for a vehicle that drives the lead trace itself (ABO/Custom_plots.m:113-155, `FE_lead`;
    the gear-dependent quantities of that block do not enter the fuel map)."""
    v = np.asarray(V_2Hz, dtype=np.float64).ravel().copy()
    v = np.concatenate([v, [0.0]]) if v.size == 870 else v              # V_TO(871,1) = 0 (:117)
    a = np.concatenate([[0.0], np.diff(v) / Ts])
    s = np.concatenate([[0.0], np.cumsum(v[1:] * Ts)])
    return fuel_economy({"a_opt": a, "v_opt": v, "s_opt": s}, V, Ts)["FE_L_per_100km"]
