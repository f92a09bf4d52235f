"""report.route_table / report.route_limits -- the route-compliance key figures of a batch, the executable specification of
eepacc_route_kpis -- on the CPU: hand values, a plain-Python loop over the samples, tests/stage_ref.py (the restatement of
EstimateRouteAndComfortBounds.m) wherever the table's definitions and the planner's coincide, the non-vacuity of the
closed-loop case of tests/test_gpu_route_kpis_loop.py, the settings translation into RouteCfg, the enum mirror and the
argument checks that need no device.

Every figure is a maximum, a minimum, a count or an index of values that are each rounded once: everything here is compared
with == / np.array_equal, there are no tolerances."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

import stage_ref
from conftest import ROOT
from eepacc_mpc_casadi_matlab_amd import build as eb
from eepacc_mpc_casadi_matlab_amd import report
from eepacc_mpc_casadi_matlab_amd._abi import (OUT, RKPI, RKPI_FIELDS, RKPI_N, RLIM, RLIM_FIELDS, RLIM_N, ROUTE_KPIS_ARGTYPES,
                                               SettingsHolder, SettingsPOD, Vehicle, make_vehicle)

HERE = os.path.dirname(os.path.abspath(__file__))
INF = np.inf
UC = 12                                  # GetUseCase.m: two stops, two lights, speed-limit steps, curves
CONSTS = dict(stopRefDist=100.0, stopRefVelSlope=1.0, stopVel=0.2, TLstopVel=-1.0, TLStopRegionSize=2.0, alpha_TTL=3.34)


def route(**kw):
    """A small route with every feature: limits 20 | 30 | 10 from 100 and 200 m, a curve between 50 and 60 m, stops at 150 and
    400 m, a light at 300 m (offset 2 s, red 10 s, green 5 s) and one at 305 m that is always red (green time 0)."""
    R = dict(s_speedLim=[0.0, 100.0, 200.0], v_speedLim=[20.0, 30.0, 10.0], s_curv=[0.0, 50.0, 60.0], curvature=[1e-6, 1.0 / 8.0, 1e-6],
             stopLoc=[150.0, 400.0], TLLoc=[[300.0, 2.0, 10.0, 5.0], [305.0, 0.0, 1.0, 0.0]], **CONSTS)
    R.update(kw)
    return R


def bare_route():
    return route(s_speedLim=[0.0], v_speedLim=[15.0], s_curv=[0.0], curvature=[0.0], stopLoc=[], TLLoc=np.zeros((0, 4)))


def use_case(case=UC, tree="ORIG"):
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, default_opt
    o = default_opt(); o["useCaseNum"] = case
    return Settings(o, tree=tree, N_hor=20), SetVehicleParameters(tree)


def table(s, v, a, OPT, Ts=0.5, t_start=0.0, tol=(0.0, 0.0, 0.0), bl_mode=0):
    T = report.route_table(s, v, a, Ts, t_start, tol, OPT, bl_mode)
    return {k: T[i] for k, i in RKPI.items()}


# ------------------------------------------------------------------------------------------------ hand values
def test_limits_by_hand():
    R = route()
    up, dn = lambda x: np.nextafter(x, INF), lambda x: np.nextafter(x, -INF)
    s = np.array([-5.0, 0.0, dn(100.0), 100.0, up(100.0), 150.0, dn(200.0), 200.0, 1e6, dn(50.0), 50.0, dn(60.0), 60.0])
    L = report.route_limits(s, 0.5, 0.0, R)
    assert L.shape == (s.size, RLIM_N)
    assert list(L[:9, RLIM["v_lim"]]) == [20.0, 20.0, 20.0, 30.0, 30.0, 30.0, 30.0, 10.0, 10.0]
    flat, curve = 3.34 * math.pow(1e-6, -1.0 / 3.0), 3.34 * math.pow(0.125, -1.0 / 3.0)
    assert list(L[9:, RLIM["v_curv"]]) == [flat, curve, curve, flat] and L[0, RLIM["v_curv"]] == flat
    # stop profile: the nearer stop wins, also beyond stopRefDist; exactly on the line it is stopVel
    assert list(L[[0, 5, 8], RLIM["v_stop"]]) == [155.0 * 1.0 + 0.2, 0.2, (1e6 - 400.0) * 1.0 + 0.2]
    # one instance [n] and a batch [n, B] agree
    assert np.array_equal(report.route_limits(np.stack([s, s[::-1]], axis=1), 0.5, 0.0, R)[:, :, 0], L)
    B = report.route_limits(s, 0.5, 0.0, bare_route())
    assert (B[:, RLIM["v_lim"]] == 15.0).all() and (B[:, RLIM["v_curv"]] == INF).all()
    assert (B[:, RLIM["v_stop"]] == 1e5).all() and (B[:, RLIM["v_tl"]] == 1e5).all()


def test_light_phases_and_cap_by_hand():
    R = route(TLLoc=[[300.0, 2.0, 10.0, 5.0]])
    cap = lambda s, t: report.route_limits(np.array([s]), 1.0, t, R)[0, RLIM["v_tl"]]
    # phase: red on [2, 12) + 15 i; before the offset the argument of mod is negative: mod(-1, 15) = 14 -> green, mod(-4, 15) = 11 -> green,
    # mod(-6, 15) = 9 -> red
    assert [cap(299.0, t) < 1e5 for t in (2.0, 11.5, 12.0, 16.5, 17.0, 1.0, -2.0, -4.0)] == [True, True, False, False, True, False, False, True]
    # three branches (:133-139) at a red time, and the two edges: exactly stopRefDist away is out of range, exactly
    # TLStopRegionSize in front is the far branch
    assert cap(310.0, 2.0) == 10.0 * 1.0 - 1.0 and cap(299.0, 2.0) == -1.0 and cap(250.0, 2.0) == abs(50.0 - 0.2) * 1.0 - 1.0
    assert cap(200.0, 2.0) == 1e5 and cap(400.0, 2.0) == 1e5 and cap(np.nextafter(200.0, INF), 2.0) < 1e5
    assert cap(298.0, 2.0) == abs(2.0 - 0.2) * 1.0 - 1.0 and cap(np.nextafter(298.0, INF), 2.0) == -1.0 and cap(300.0, 2.0) == -1.0
    # a cycle of length 0 returns its argument: red time 0 is never red after the offset; red time 3, green -3: red while t - offset < 3
    Z = route(TLLoc=[[300.0, 2.0, 0.0, 0.0]])
    assert report.route_limits(np.array([299.0]), 1.0, 5.0, Z)[0, RLIM["v_tl"]] == 1e5
    Z = route(TLLoc=[[300.0, 2.0, 3.0, -3.0]])
    assert [report.route_limits(np.array([299.0]), 1.0, t, Z)[0, RLIM["v_tl"]] < 1e5 for t in (4.5, 5.0, 100.0, -7.0)] == [True, False, False, True]
    # of two red lights in range the lower cap counts
    two = route(TLLoc=[[300.0, 0.0, 1.0, 0.0], [340.0, 0.0, 1.0, 0.0]])
    assert report.route_limits(np.array([320.0]), 1.0, 0.0, two)[0, RLIM["v_tl"]] == abs(20.0 - 0.2) - 1.0       # not 20 - 1 behind the first


def test_table_by_hand():
    """Four samples, 1 s apart from t = 1: 140 -> 149 -> 301 -> 306 m: the stop at 150 and the light at 300 are crossed in the
    step to k = 2 (light 0 is red from t = 2 to 12: at t_1 = 2 and at t_2 = 3), the always-red light at 305 in the step to
    k = 3."""
    R = route()
    s, v, a = [140.0, 149.0, 301.0, 306.0], [9.0, 31.5, 12.0, 5.0], [0.0, 4.5, -6.0, 0.0]
    r = table(s, v, a, R, Ts=1.0, t_start=1.0, tol=(1.0, 0.25, 10.0))
    assert r["vlim_excess_max"] == 2.0 and r["vlim_excess_index"] == 2.0 and r["vlim_viol_steps"] == 2.0      # 31.5 - 30 = 1.5, 12 - 10 = 2
    assert r["vstop_excess_max"] == 31.5 - 1.2 and r["vstop_viol_steps"] == 1.0      # 9 - 10.2 < 0; 12 - 99.2 and 5 - 94.2 far below
    assert r["stops_passed"] == 1.0 and r["stop_cross_v_max"] == 12.0
    assert r["tl_passed"] == 2.0 and r["red_crossings"] == 2.0 and r["red_crossings_possible"] == 2.0 and r["red_cross_first_index"] == 2.0
    # k = 2 (s = 301, t = 3): light 0 is 1 m behind (cap 0), the always-red light 4 m ahead (far branch, 2.8); k = 3 (s = 306):
    # 5 and 0; at k = 0, 1 both lights are more than stopRefDist away
    assert r["vtl_excess_max"] == 12.0 and r["vtl_viol_steps"] == 2.0
    # a: 4.5 at v = 31.5 (a_max = 2), -6 at v = 12 (a_min = -5.5 + 1.2); j: 6 at v = 12 (j_max = 35/6 - 2)
    assert r["a_over_max"] == 2.5 and r["a_under_max"] == (-5.5 + 12.0 / 10.0) + 6.0 and r["v_min"] == 5.0
    assert r["comfort_viol_steps"] == 2.0 and r["j_over_max"] == 6.0 - (35.0 / 6.0 - 12.0 / 6.0)
    assert r["j_under_max"] == -2.5 + 10.5                                           # j = -10.5 at v = 31.5
    assert table(s[:1], v[:1], a[:1], R)["j_over_max"] == -INF and table(s[:1], v[:1], a[:1], R)["stops_passed"] == 0.0
    # first sample pair green then red: possible, not certain (light 0: green at t = 1, red at t = 2)
    g = table([299.0, 300.0], [1.0, 1.0], [0.0, 0.0], route(TLLoc=[[300.0, 2.0, 10.0, 5.0]]), Ts=1.0, t_start=1.0)
    assert (g["tl_passed"], g["red_crossings"], g["red_crossings_possible"], g["red_cross_first_index"]) == (1.0, 0.0, 1.0, 1.0)
    # `<` on the left, `<=` on the right of a crossing: from exactly on the line nothing is crossed, onto it is
    on = table([150.0, 151.0, 400.0, 400.0], [3.0, 2.0, 7.0, 8.0], [0.0] * 4, R)
    assert on["stops_passed"] == 1.0 and on["stop_cross_v_max"] == 2.0
    # a NaN is never taken and never counted; -0.0 is 0
    nan = table([1.0, 2.0, 3.0], [np.nan, -0.0, 0.0], [np.nan, 1.0, 1.0], R)
    assert nan["vlim_excess_max"] == -20.0 and nan["vlim_excess_index"] == 1.0 and nan["v_min"] == 0.0 and nan["comfort_viol_steps"] == 0.0
    assert nan["a_over_max"] == -3.0 and nan["j_over_max"] == -5.0
    allnan = table([np.nan] * 2, [np.nan] * 2, [np.nan] * 2, R)
    assert allnan["vlim_excess_max"] == -INF and allnan["vlim_excess_index"] == -1.0 and allnan["v_min"] == INF
    assert not np.isnan(report.route_table([np.nan] * 2, [np.nan] * 2, [np.nan] * 2, 0.5, 0.0, (0, 0, 0), R)).any()


# ------------------------------------------------------------------------------------------------ a loop over the samples
def loop_table(s, v, a, Ts, t_start, tol, OPT, bl_mode):
    """The definitions of include/eepacc.h, one instance, sample by sample in plain Python (floats round as the device's
    doubles do), written apart from report.py: lists and `if`, stage_ref.matlab_mod for the phase."""
    n = len(s)
    T = report._route_tables(OPT)
    NINF = -INF
    red = lambda TL, t: stage_ref.matlab_mod(t - TL[1], TL[2] + TL[3]) < TL[2]
    r = dict.fromkeys(RKPI_FIELDS, 0.0)
    for k in ("vlim", "vcurv", "vstop", "vtl"):
        r[k + "_excess_max"] = NINF
    r.update(vlim_excess_index=-1.0, stop_cross_v_max=NINF, red_cross_first_index=-1.0, a_over_max=NINF, a_under_max=NINF,
             j_over_max=NINF, j_under_max=NINF, v_min=INF)
    limits = []
    for k in range(n):
        t = t_start + k * Ts
        caps = {}
        for name, knots, vals in (("vlim", T["s_speedLim"], T["v_speedLim"]), ("vcurv", T["s_curv"], T["vcurv_tab"])):
            c = vals[0]
            for j in range(len(knots)):
                last = j == len(knots) - 1
                if (s[k] >= knots[j]) and (last or s[k] < knots[j + 1]):
                    c = vals[j]
            caps[name] = c
        c = [abs(loc - s[k]) * T["stopRefVelSlope"] + T["stopVel"] for loc in T["stopLoc"]]
        c = [x for x in c if x == x]
        caps["vstop"] = (min(c) if c else INF) if T["stopLoc"] else 1e5
        c = []
        for TL in T["TLLoc"]:
            d = TL[0] - s[k]
            if red(TL, t) and abs(d) < T["stopRefDist"]:
                c.append(abs(d) * T["stopRefVelSlope"] + T["TLstopVel"] if d < 0 else
                         (T["TLstopVel"] if abs(d) < T["TLStopRegionSize"] else abs(d - T["stopVel"]) * T["stopRefVelSlope"] + T["TLstopVel"]))
        caps["vtl"] = min(c) if c else 1e5
        limits.append([caps[x] for x in ("vlim", "vcurv", "vstop", "vtl")])
        for name, cap in caps.items():
            if name == "vtl" and not cap < 1e5:
                continue
            e = v[k] - cap
            if e > r[name + "_excess_max"]:
                r[name + "_excess_max"] = e
                if name == "vlim":
                    r["vlim_excess_index"] = float(k)
            r[name + "_viol_steps"] += e > tol[0]
        if v[k] < r["v_min"]:
            r["v_min"] = v[k]
        if k >= 1:
            for loc in T["stopLoc"]:
                if s[k - 1] < loc <= s[k]:
                    r["stops_passed"] += 1
                    m = v[k] if v[k] < v[k - 1] else v[k - 1]
                    if m > r["stop_cross_v_max"]:
                        r["stop_cross_v_max"] = m
            for TL in T["TLLoc"]:
                if s[k - 1] < TL[0] <= s[k]:
                    r0, r1 = red(TL, t_start + (k - 1) * Ts), red(TL, t)
                    r["tl_passed"] += 1
                    r["red_crossings"] += r0 and r1
                    if r0 or r1:
                        r["red_crossings_possible"] += 1
                        if r["red_cross_first_index"] < 0:
                            r["red_cross_first_index"] = float(k)
        a_min, a_max, j_min, j_max = stage_ref._comfort(1 if bl_mode else 0, OPT, v[k])
        bad = False
        for key, e, lim in (("a_over_max", a[k] - a_max, tol[1]), ("a_under_max", a_min - a[k], tol[1])):
            if e > r[key]:
                r[key] = e
            bad = bad or e > lim
        if k + 1 < n:
            j = (a[k + 1] - a[k]) / Ts
            for key, e in (("j_over_max", j - j_max), ("j_under_max", j_min - j)):
                if e > r[key]:
                    r[key] = e
                bad = bad or e > tol[2]
        r["comfort_viol_steps"] += bad
    return np.array([float(r[k]) for k in RKPI_FIELDS]), np.array(limits)


def random_drive(OPT, n, B, seed):
    """Trajectories that drive over the whole of OPT's route, with samples planted on knots, stop lines and lights."""
    rng = np.random.default_rng(seed)
    T = report._route_tables(OPT)
    marks = np.array(T["s_speedLim"] + T["s_curv"] + T["stopLoc"] + [TL[0] for TL in T["TLLoc"]])
    top = float(np.max(marks[marks < 5e4])) + 150.0
    s = np.sort(rng.uniform(-20.0, top, (n, B)), axis=0)
    for b in range(B):
        for k in rng.choice(n, size=min(n, 6), replace=False):
            m = marks[rng.integers(marks.size)]
            s[k, b] = (m, np.nextafter(m, INF), np.nextafter(m, -INF))[rng.integers(3)]
    s = np.sort(s, axis=0)
    v = rng.integers(-8, 280, (n, B)) / 8.0
    a = rng.integers(-48, 40, (n, B)) / 8.0
    v[rng.integers(n), :] = [5.0, 20.0][seed % 2]
    return s, v, a


@pytest.mark.parametrize("bl_mode", [0, 1])
@pytest.mark.parametrize("which", ["uc12", "uc5", "small", "bare"])
def test_against_the_loop_over_samples(which, bl_mode):
    OPT = {"uc12": lambda: use_case(12)[0], "uc5": lambda: use_case(5)[0],
           "small": lambda: dict(use_case(1)[0], **route()), "bare": lambda: dict(use_case(1)[0], **bare_route())}[which]()
    n, B = 41, 5
    s, v, a = random_drive(OPT, n, B, seed=len(which) + bl_mode)
    tol = (0.25, 0.125, 0.5)
    for Ts, t_start in ((0.5, 0.0), (0.3, 7.3 * 13)):
        got = report.route_table(s, v, a, Ts, t_start, tol, OPT, bl_mode)
        lim = report.route_limits(s, Ts, t_start, OPT)
        assert got.shape == (RKPI_N, B) and lim.shape == (n, RLIM_N, B) and not np.isnan(got).any()
        for b in range(B):
            want, wl = loop_table(list(s[:, b]), list(v[:, b]), list(a[:, b]), Ts, t_start, tol, OPT, bl_mode)
            assert np.array_equal(got[:, b], want), (b, dict(zip(RKPI_FIELDS, zip(got[:, b], want))))
            assert np.array_equal(lim[:, :, b], wl), b
    if which != "bare":
        assert got[RKPI["stops_passed"]].min() >= 1.0 or which == "uc5"
        assert got[RKPI["tl_passed"]].min() >= 1.0 and (lim[:, RLIM["v_tl"]] < 1e5).any()


@pytest.mark.parametrize("MPCtype", [0, 1])
def test_against_the_planner_where_the_definitions_coincide(MPCtype):
    """stage_ref.bounds_at_stage (EstimateRouteAndComfortBounds.m:89-207) at stage i = 0 of t_0 = t_k takes the phase at the
    sample's own time.  Use case 12: v_lim before the last knot, v_curv inside the open intervals before the last knot,
    v_stop within stopRefDist of exactly one stop, v_TL where at most one light is red and in range; the comfort envelope
    everywhere, at the breaks 5 and 20 too."""
    OPT, _ = use_case(12)
    rng = np.random.default_rng(3 + MPCtype)
    s = np.concatenate([rng.uniform(1.0, 1000.0, 400), [299.0, 300.0, 509.0, 510.0, 250.0, 450.0, 350.0, 448.0, 452.0]])
    t = np.concatenate([rng.integers(0, 400, 400) * 0.5, np.arange(9) * 2.5])
    v = np.concatenate([rng.uniform(0.0, 30.0, 400), [5.0, 20.0, np.nextafter(5.0, 0), np.nextafter(20.0, 0), 0.0, 4.0, 12.5, 19.0, 25.0]])
    S_sl, S_cv = [float(x) for x in OPT["s_speedLim"]], [float(x) for x in OPT["s_curv"]]
    stops, lights = [float(x) for x in OPT["stopLoc"]], np.asarray(OPT["TLLoc"], dtype=np.float64)
    seen = dict.fromkeys(("v_lim", "v_curv", "v_stop", "v_TL", "far_branch", "behind", "region"), 0)
    for sk, tk, vk in zip(s, t, v):
        L = report.route_limits(np.array([sk]), 0.5, tk, OPT)[0]
        ref = stage_ref.bounds_at_stage(OPT, MPCtype, sk, vk, tk, 0, 0.5)
        if S_sl[0] <= sk < S_sl[-1]:
            assert L[RLIM["v_lim"]] == ref["v_lim"]; seen["v_lim"] += 1
        if S_cv[0] < sk < S_cv[-1] and sk not in S_cv:
            assert L[RLIM["v_curv"]] == ref["v_curv"]; seen["v_curv"] += 1
        if sum(abs(x - sk) < OPT["stopRefDist"] for x in stops) == 1:
            assert L[RLIM["v_stop"]] == ref["v_stop"]; seen["v_stop"] += 1
        near = [TL for TL in lights if stage_ref.matlab_mod(tk - TL[1], TL[2] + TL[3]) < TL[2] and abs(TL[0] - sk) < OPT["stopRefDist"]]
        if len(near) <= 1:
            assert L[RLIM["v_tl"]] == ref["v_TL"]; seen["v_TL"] += len(near)
            for TL in near:
                d = TL[0] - sk
                seen["behind" if d < 0 else ("region" if abs(d) < OPT["TLStopRegionSize"] else "far_branch")] += 1
        env = report._comfort_envelope(np.array([vk]), OPT, MPCtype)
        assert [float(x[0]) for x in env] == [ref[k] for k in ("a_min", "a_max", "j_min", "j_max")], vk
    assert all(x > 0 for x in seen.values()), seen


# ------------------------------------------------------------------------------------------------ the closed-loop case is not idle
@pytest.fixture(scope="module")
def oracle_runs():
    """The oracle's closed loops of use case 12 (ORIG tree, N = 20, no lead, the use case's own 201 steps): what
    tests/test_gpu_route_kpis_loop.py runs on the device."""
    from oracle import Oracle
    OPT, V = use_case(12)
    n = int(round(OPT["t_sim"] / OPT["Tvec"][0])) + 1
    out = {}
    for kind in ("ab", "fb"):
        tr, st, _ = Oracle(OPT, V).run(kind, n, OPT["s_init"], OPT["v_init"], OPT["a_minus1"], np.full(n, INF), np.zeros(n))
        assert st.sum() == 0
        out[kind] = tr
    return OPT, n, out


def test_the_closed_loop_case_is_not_idle(oracle_runs):
    """On the oracle's ABMPC trajectory the table shows a stop passed, a light passed, samples with a finite v_TL and samples
    above the sign-posted limit at v_tol = 0 (the ORIG controller holds the limit with a soft row, and overshoots it by
    rounding-sized amounts); FBMPC, which keeps below the limit, shows the first three."""
    OPT, n, runs = oracle_runs
    assert n == 201
    for kind, tr in runs.items():
        s, v, a = tr[:, OUT["s"]], tr[:, OUT["v"]], tr[:, OUT["a"]]
        r = table(s, v, a, OPT)
        lim = report.route_limits(s, 0.5, 0.0, OPT)
        print(kind, r)
        assert r["stops_passed"] >= 1.0 and r["stop_cross_v_max"] > -INF
        assert r["tl_passed"] >= 1.0
        assert (lim[:, RLIM["v_tl"]] < 1e5).sum() >= 1 and r["vtl_excess_max"] > -INF
        if kind == "ab":
            assert r["vlim_viol_steps"] > 0.0 and r["vlim_excess_max"] > 0.0
        assert r["red_crossings"] == 0.0 and r["v_min"] >= 0.0 and r["vlim_excess_max"] < 0.1      # the controllers do obey the route
        assert np.array_equal(report.route_table(s, v, a, 0.5, 0.0, (0, 0, 0), OPT), report.route_table(s[:, None], v[:, None], a[:, None], 0.5, 0.0, (0, 0, 0), OPT)[:, 0])


def test_summarise_table_takes_the_table():
    """summarise_table reduces this table by class too; -inf (no stop crossed in an instance) stays -inf in min and mean, no NaN."""
    T = np.zeros((RKPI_N, 4))
    T[RKPI["stop_cross_v_max"]] = [0.25, -INF, 0.5, 0.75]
    T[RKPI["red_cross_first_index"]] = [-1.0, 3.0, -1.0, -1.0]
    S = report.summarise_table(T, [0, 0, 1, 1])
    assert S["mean"].shape == (2, RKPI_N) and not np.isnan(S["mean"]).any()
    c = RKPI["stop_cross_v_max"]
    assert np.array_equal(S["max"][:, c], [0.25, 0.75]) and np.array_equal(S["min"][:, c], [-INF, 0.5]) and np.array_equal(S["mean"][:, c], [-INF, 0.625])
    assert "-inf" in report.summarise_table.__doc__ and "route_table" in report.summarise_table.__doc__


# ------------------------------------------------------------------------------------------------ the mirror and the C-ABI
def test_enum_mirror_equals_the_header():
    hdr = open(os.path.join(ROOT, "include", "eepacc.h")).read()
    body = re.search(r"enum \{\s*EEPACC_RKPI_VLIM_EXCESS_MAX = 0,(.*?)\};", hdr, re.S).group(0)
    names = re.findall(r"^\s*(EEPACC_RKPI_[A-Z_]+)", body, re.M)
    assert names == ["EEPACC_RKPI_" + f.upper() for f in RKPI_FIELDS] + ["EEPACC_RKPI_N"] and RKPI_N == 21
    body = re.search(r"enum \{\s*EEPACC_RLIM_V_LIM = 0,(.*?)\};", hdr, re.S).group(0)
    names = re.findall(r"^\s*(EEPACC_RLIM_[A-Z_]+)", body, re.M)
    assert names == ["EEPACC_RLIM_" + f.upper() for f in RLIM_FIELDS] + ["EEPACC_RLIM_N"] and RLIM_N == 4
    proto = re.search(r"int\s+eepacc_route_kpis\((.*?)\);", hdr, re.S).group(1)
    assert len(proto.split(",")) == len(ROUTE_KPIS_ARGTYPES) == 10
    assert "seen by neither call" in hdr                                                 # the limit of chunked runs is stated


def test_argument_checks_that_need_no_device():
    """n_steps, t_start, the tolerances and the three required buffers are checked before the handle is looked at."""
    from eepacc_mpc_casadi_matlab_amd import engine
    lib = engine.load_library()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    tol = lambda *x: (C.c_double * 3)(*x)
    ok = dict(B=1, n_steps=1, t_start=0.0, tol=tol(0.0, 0.0, 0.0), traj=p, status=p, rkpi=p, limits=None)
    order = ("B", "n_steps", "t_start", "tol", "traj", "status", "rkpi", "limits")

    def call(**kw):
        rc = lib.eepacc_route_kpis(None, *[dict(ok, **kw)[k] for k in order], None)
        return rc, lib.eepacc_last_error().decode()
    for bad in (0, -2):
        rc, msg = call(n_steps=bad)
        assert rc == -1 and "eepacc_route_kpis: n_steps = %d" % bad in msg, msg
    for bad in (INF, -INF, np.nan):
        rc, msg = call(t_start=bad)
        assert rc == -1 and "eepacc_route_kpis: t_start" in msg, msg
    for i, name in enumerate(("v_tol", "a_tol", "j_tol")):
        for bad in (-1e-300, INF, np.nan):
            x = [0.0, 0.0, 0.0]; x[i] = bad
            rc, msg = call(tol=tol(*x))
            assert rc == -1 and "eepacc_route_kpis: tol_host[%d] (%s)" % (i, name) in msg, msg
    rc, msg = call(tol=None)
    assert rc == -1 and "eepacc_route_kpis: tol_host is NULL" in msg, msg
    for name in ("traj", "status", "rkpi"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "eepacc_route_kpis: %s is NULL" % name in msg, msg
    rc, msg = call()
    assert rc == -1 and "NULL handle" in msg, msg                                  # everything else is in order; limits may be NULL


# ------------------------------------------------------------------------------------------------ settings -> RouteCfg
GXX_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-fPIC"]
UNIT = os.path.join(eb.CSRC, "eepacc_cfg.cpp")


def gxx():
    return os.environ.get("CXX", "g++")


@pytest.fixture(scope="module")
def route_harness(tmp_path_factory):
    """tests/kernels/route_cfg_harness.cpp and csrc/eepacc_cfg.cpp, compiled with plain g++ and loaded with ctypes."""
    lib = str(tmp_path_factory.mktemp("route_cfg") / "libeepacc_route_cfg_harness.so")
    subprocess.run([gxx()] + GXX_FLAGS + ["-O2", "-shared", "-I", eb.CSRC, os.path.join(HERE, "kernels", "route_cfg_harness.cpp"), UNIT, "-o", lib],
                   check=True, timeout=300)
    L = C.CDLL(lib)
    L.rh_last_error.restype = C.c_char_p
    L.rh_field.restype = C.c_char_p
    L.rh_field.argtypes = [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.rh_build.argtypes = [C.POINTER(SettingsPOD), C.POINTER(Vehicle), C.c_void_p]
    return L


def build_route_cfg(L, OPT, V):
    """RouteCfg of OPT as {field: array}, and the bytes that belong to no field."""
    holder, veh = SettingsHolder(OPT), make_vehicle(V)
    raw = np.full(L.rh_sizeof(), 0xAB, dtype=np.uint8)
    rc = L.rh_build(C.byref(holder.pod), C.byref(veh), raw.ctypes.data)
    assert rc == 0, L.rh_last_error()
    covered = np.zeros(raw.size, dtype=bool)
    out = {}
    for i in range(L.rh_num_fields()):
        off, nbytes = C.c_int(), C.c_int()
        name = L.rh_field(i, C.byref(off), C.byref(nbytes)).decode()
        dtype = np.int32 if name.startswith("n_") or name in ("bl_mode", "pad") else np.float64
        out[name] = np.frombuffer(raw, dtype=dtype, count=nbytes.value // np.dtype(dtype).itemsize, offset=off.value).copy()
        covered[off.value:off.value + nbytes.value] = True
    return out, raw[~covered]


@pytest.mark.parametrize("which", ["uc12", "uc11", "bare", "bl", "tv"])
def test_settings_translation_into_routecfg(route_harness, which):
    """Every field of RouteCfg is what report._route_tables reads of the same settings (the curve speeds bit for bit: both go
    through the C library's pow), the unused tails of the fixed arrays and the padding are zero."""
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV
    OPT, V = use_case(11 if which == "uc11" else 12)
    if which == "bare":
        OPT = dict(OPT, **{k: np.asarray(x, dtype=np.float64) for k, x in bare_route().items() if k not in CONSTS})
    if which in ("bl", "tv"):
        OPT = (Settings_BL if which == "bl" else Settings_TV)(OPT)
    R, rest = build_route_cfg(route_harness, OPT, V)
    T = report._route_tables(OPT)
    assert (rest == 0).all() and R["pad"][0] == 0
    assert R["Ts"][0] == float(OPT["Tvec"][0]) and R["bl_mode"][0] == {"bl": 1, "tv": 2}.get(which, 0)
    for count, fields in (("n_speedLim", ("s_speedLim", "v_speedLim")), ("n_curv", ("s_curv", "vcurv_tab")), ("n_stop", ("stopLoc",))):
        n = len(T[fields[0]])
        assert R[count][0] == n
        for f in fields:
            assert np.array_equal(R[f][:n], np.array(T[f])) and (R[f][n:] == 0.0).all(), f
    nTL = len(T["TLLoc"])
    assert R["n_TL"][0] == nTL and np.array_equal(R["TLLoc"][:4 * nTL], np.array(T["TLLoc"]).reshape(-1)) and (R["TLLoc"][4 * nTL:] == 0.0).all()
    for k in ("stopRefDist", "stopRefVelSlope", "stopVel", "TLstopVel", "TLStopRegionSize"):
        assert R[k][0] == T[k]
    if which in ("bl", "tv"):
        assert [R[k][0] for k in ("bl_aLo", "bl_aHi", "bl_jLo", "bl_jHi")] == [float(OPT["BL_" + k]) for k in ("a_LimLowVel", "a_LimHighVel", "j_LimLowVel", "j_LimHighVel")]
        assert R["bl_aLo"][0] == (3.0 if which == "bl" else 1.0)
    if which == "uc11":
        assert R["n_curv"][0] == 34 and R["n_stop"][0] == 5          # the longest curve table of the use cases
    if which == "bare":
        assert R["vcurv_tab"][0] == INF and R["n_stop"][0] == 0 and R["n_TL"][0] == 0


def test_sanitized_host_program(tmp_path):
    """tests/kernels/route_cfg_sanitize_main.cpp calls build_route_cfg with every table at the limit of RouteCfg's fixed arrays
    and with an empty route, as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "route_cfg_sanitize")
    cmd = [gxx(), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",        # the runtimes in the program itself: nothing to order or preload
           "-I", eb.CSRC, os.path.join(HERE, "kernels", "route_cfg_sanitize_main.cpp"), UNIT, "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)
