"""The settings and edge-case tables of tests/test_gpu_stage.py, and for each table the count of problems on every branch
edge it is meant to cover (tests/test_stage_ref_cpu.py asserts on the reference alone that none of them is empty).

Inputs that decide a branch are exactly representable (dyadic times, distances and speeds, integer knots), so the branch is
taken by the comparison and not by a rounding; the neighbours of an edge are its nextafter values."""
import functools
import math

import numpy as np

import stage_ref
from eepacc_mpc_casadi_matlab_amd.settings import Settings, Settings_BL, Settings_TV, SetVehicleParameters

INF = math.inf


def near(x):
    """x and its two neighbours"""
    return [np.nextafter(x, -INF), float(x), np.nextafter(x, INF)]


@functools.lru_cache(maxsize=None)
def _settings(tree, N):
    return Settings(tree=tree, N_hor=N), SetVehicleParameters(tree)


def view(OPT, MPCtype):
    """What the controller of an MPCtype hands to the translation: OPT itself (0), Settings_BL (1), Settings_TV (2).  A
    variable Tvec is kept for the baseline controller (the reference's EstimateRouteAndComfortBounds reads OPTsettings.Tvec
    for every MPCtype); the target-vehicle MPC is built for a uniform step only."""
    if MPCtype == 0:
        return dict(OPT)
    if MPCtype == 1:
        return dict(Settings_BL(dict(OPT, BL_N_hor=OPT["N_hor"], BL_Ts=float(OPT["Tvec"][0]))), Tvec=np.array(OPT["Tvec"]))
    Ts = float(OPT["Tvec"][0])
    return Settings_TV(dict(OPT, TV_N_hor=OPT["N_hor"], TV_Ts=Ts, Tvec=Ts * np.ones(OPT["N_hor"])))


# ---------------------------------------------------------------------------------------------- route_bounds
DYADIC = dict(stopRefDist=64.0, stopRefVelSlope=0.75, stopVel=0.25, TLstopVel=-0.5, TLStopRegionSize=4.0)
FIVE_KNOTS = dict(s_speedLim=np.array([-1.0, 100.0, 250.0, 1000.0, 4096.0]), v_speedLim=np.array([16.5, 13.75, 25.0, 8.5, 30.0]),
                  s_curv=np.array([0.0, 128.0, 256.0, 512.0, 1024.0]), curvature=np.array([1e-5, 4e-4, -1e-6, 2.5e-3, 1e-4]))
TWO_KNOTS = dict(s_speedLim=np.array([0.0, 500.0]), v_speedLim=np.array([10.0, 20.0]),
                 s_curv=np.array([64.0, 320.0]), curvature=np.array([1e-3, 1e-5]))
ONE_KNOT = dict(s_speedLim=np.array([300.0]), v_speedLim=np.array([12.5]), s_curv=np.array([300.0]), curvature=np.array([1e-4]))
# [location, offset, red, green]: two lights 30 m apart with different cycles, and one whose cycle has length zero (the
# translation accepts it; mod(x, 0) = x, so it is red while t_0 + i Tvec(i) < 4)
LIGHTS = np.array([[400.0, 8.0, 16.0, 16.0], [430.0, 0.0, 12.0, 20.0], [900.0, 0.0, 4.0, -4.0]])
STOPS = np.array([200.0, 260.0, 700.0])
T_VARIABLE = lambda N: 0.25 * (1 + np.arange(N) % 4)

ROUTE_VARIANTS = {
    # name: (tree, N, overrides)
    "abo20_five_knots": ("ABO", 20, dict(FIVE_KNOTS, stopLoc=STOPS, TLLoc=LIGHTS)),
    "orig63_five_knots_dyadic_tvec": ("ORIG", 63, dict(FIVE_KNOTS, **DYADIC, stopLoc=STOPS, TLLoc=LIGHTS, Tvec=T_VARIABLE(63))),
    "abo2_two_knots_dyadic": ("ABO", 2, dict(TWO_KNOTS, **DYADIC, stopLoc=STOPS[:2], TLLoc=LIGHTS[:2])),
    "orig20_one_knot_plain": ("ORIG", 20, dict(ONE_KNOT, stopLoc=np.zeros(0), TLLoc=np.zeros((0, 4)))),
}
MPC_TYPES = (0, 1, 2)
V_COMFORT = [0.0, -1.0, -0.0] + near(5.0) + near(20.0) + [12.5, 7.3, 19.99, 40.0, 55.5]
X_LIGHT = [-32.0, -20.0, -7.5, -0.25, 0.0, 3.75, 4.0, 11.75, 12.0, 15.5, 16.0, 16.5, 31.5, 32.0, 39.75, 40.0, 48.0]


def route_opt(name, MPCtype):
    tree, N, over = ROUTE_VARIANTS[name]
    OPT, V = _settings(tree, N)
    return view(dict(OPT, **over), MPCtype), V


def route_case(name, MPCtype):
    """-> OPT (the view of the MPCtype), V, and the per-problem arrays s_est, v_est, t0, i (0-based stage)"""
    OPT, V = route_opt(name, MPCtype)
    N, Tvec = int(OPT["N_hor"]), np.asarray(OPT["Tvec"], dtype=np.float64)
    R, reg = float(OPT["stopRefDist"]), float(OPT["TLStopRegionSize"])
    stops = [float(x) for x in np.asarray(OPT["stopLoc"]).ravel()]
    lights = np.asarray(OPT["TLLoc"], dtype=np.float64).reshape(-1, 4)
    knots = sorted(set(float(x) for k in ("s_speedLim", "s_curv") for x in OPT[k]))
    route_s = [knots[0] - 10.0, knots[-1] + 10.0, -0.0]
    for a, b in zip(knots, knots[1:]):
        route_s += [0.5 * (a + b), a + (b - a) / 3]
    for k in knots:
        route_s += near(k)
    for L in stops:
        for off in (-R - 1.0, -R, -0.5 * R, 0.0, 1.0 / 3, R, R + 1.0):
            route_s += near(L + off) if off in (-R, 0.0, R) else [L + off]
    light_s = []
    for L in lights[:, 0]:
        for off in (-R, -reg, 0.0, reg, R):
            light_s += near(L + off)
        light_s += [L - 0.5 * R, L - 0.5 * reg, L + 0.5 * reg, L + 0.7 * R]
    s, v, t0, i = [], [], [], []

    def add(ss, tt, ii):
        s.append(ss); t0.append(tt); i.append(ii); v.append(V_COMFORT[len(v) % len(V_COMFORT)])

    # the tables and the stops do not look at the time: every point once, the stage walking through the horizon
    for q, ss in enumerate(route_s + light_s):
        add(ss, 0.5 * (q % 7), q % N)
    # the lights: every position near one, at every phase x = t_0 + i Tvec(i) - offset of that light, at three stages;
    # t_0 = x + offset - i Tvec(i) is exact in these numbers
    for j, TL in enumerate(lights):
        mine = [ss for ss in light_s if abs(ss - TL[0]) <= 1.5 * R]
        for a, x in enumerate(X_LIGHT):
            for st in sorted({0, (a + j) % N, N - 1}):
                for ss in mine[(a + st) % 2::2]:
                    add(ss, x + TL[1] - (st + 1) * Tvec[st], st)
    for k, vv in enumerate(V_COMFORT):                                # every comfort speed at least once, whatever the cycle above
        add(knots[0] + 0.5, 0.0, (N - 1 - k) % N)
        v[-1] = vv
    return OPT, V, np.array(s), np.array(v), np.array(t0), np.array(i, dtype=np.int32)


def route_reference(OPT, MPCtype, s, v, t0, i):
    """dict of the eight bounds, each [n], from stage_ref (stage i is the reference's i + 1)"""
    Tvec, T = np.asarray(OPT["Tvec"], dtype=np.float64), stage_ref._tables(OPT)
    rows = [stage_ref.bounds_at_stage(OPT, MPCtype, s[q], v[q], t0[q], int(i[q]) + 1, float(Tvec[i[q]]), T) for q in range(len(s))]
    return {k: np.array([r[k] for r in rows]) for k in rows[0]}


def route_edges(OPT, s, v, t0, i):
    """name -> number of problems on that edge, from the inputs and the settings alone"""
    Tvec = np.asarray(OPT["Tvec"], dtype=np.float64)
    R, reg = float(OPT["stopRefDist"]), float(OPT["TLStopRegionSize"])
    s_sl, s_cv = np.asarray(OPT["s_speedLim"], dtype=np.float64), np.asarray(OPT["s_curv"], dtype=np.float64)
    stops = np.asarray(OPT["stopLoc"], dtype=np.float64).ravel()
    lights = np.asarray(OPT["TLLoc"], dtype=np.float64).reshape(-1, 4)
    E = {}
    for nm, tab in (("speedLim", s_sl), ("curv", s_cv)):
        E[nm + ": on every knot"] = min(int(np.sum(s == k)) for k in tab)
        E[nm + ": just below every knot"] = min(int(np.sum(s == np.nextafter(k, -INF))) for k in tab)
        E[nm + ": just above every knot"] = min(int(np.sum(s == np.nextafter(k, INF))) for k in tab)
        E[nm + ": below the first knot"] = int(np.sum(s < tab[0]))
        E[nm + ": beyond the last knot"] = int(np.sum(s > tab[-1]))
        if tab.size > 2:
            E[nm + ": inside an inner segment"] = int(np.sum((s > tab[1]) & (s < tab[-2])))
    if stops.size:
        dist = np.abs(stops[None, :] - s[:, None])
        E["stop: distance == stopRefDist"] = int(np.sum(dist == R))
        E["stop: distance just below stopRefDist"] = int(np.sum((dist < R) & (dist > R - 1e-9)))
        E["stop: on the stop"] = int(np.sum(dist == 0.0))
        E["stop: past a stop, within range"] = int(np.sum(((s[:, None] - stops[None, :]) > 0) & (dist < R)))
        E["stop: out of range of all"] = int(np.sum((dist >= R).all(axis=1)))
        if stops.size > 1:
            E["stop: two within range"] = int(np.sum((dist < R).sum(axis=1) >= 2))
    if lights.shape[0]:
        x = t0[:, None] + (i[:, None] + 1) * Tvec[i][:, None] - lights[None, :, 1]
        md = np.array([[stage_ref.matlab_mod(float(xx), float(L[2] + L[3])) for xx, L in zip(row, lights)] for row in x])
        red = md < lights[None, :, 2]
        d = lights[None, :, 0] - s[:, None]
        inr = np.abs(d) < R
        act = red & inr                                               # a light that sets v_TL
        E["TL: md == TL[2] (just green), in range"] = int(np.sum((md == lights[None, :, 2]) & inr))
        E["TL: md just below TL[2], in range"] = int(np.sum((md == lights[None, :, 2] - 0.5) & inr) + np.sum((md == lights[None, :, 2] - 0.25) & inr))
        E["TL: cycle wraps (md == 0, x != 0), in range"] = int(np.sum((md == 0.0) & (x != 0.0) & inr))
        E["TL: x < 0 and red, in range"] = int(np.sum((x < 0) & red & inr))
        E["TL: x < 0 and green where x itself is below TL[2], in range"] = int(np.sum((x < 0) & ~red & inr))
        E["TL: red, d < 0"] = int(np.sum(act & (d < 0)))
        E["TL: red, d == 0"] = int(np.sum(act & (d == 0)))
        E["TL: red, 0 < d < region"] = int(np.sum(act & (d > 0) & (d < reg)))
        E["TL: red, d == region"] = int(np.sum(act & (d == reg)))
        E["TL: red, d == -region"] = int(np.sum(act & (d == -reg)))
        E["TL: red, d > region"] = int(np.sum(act & (d > reg)))
        E["TL: red, |d| == stopRefDist"] = int(np.sum(red & (np.abs(d) == R)))
        E["TL: red, |d| just below stopRefDist"] = int(np.sum(red & (np.abs(d) < R) & (np.abs(d) > R - 1e-9)))
        E["TL: green, in range"] = int(np.sum(~red & inr))
        E["TL: last stage of the horizon, red"] = int(np.sum(act[i == int(OPT["N_hor"]) - 1]))
        if lights.shape[0] > 1:
            E["TL: two red within range"] = int(np.sum(act.sum(axis=1) >= 2))
        zero = (lights[:, 2] + lights[:, 3]) == 0
        if zero.any():
            E["TL: cycle of length zero, red"] = int(np.sum(act[:, zero]))
            E["TL: cycle of length zero, green in range"] = int(np.sum((~red & inr)[:, zero]))
        if not np.all(Tvec == Tvec[0]):
            E["TL: stages with different Tvec"] = len(set(Tvec[i[act.any(axis=1)]])) - 1
    for nm, m in (("v == 0", v == 0), ("v < 0", v < 0), ("v == 5", v == 5), ("v just below 5", v == np.nextafter(5.0, 0)),
                  ("v just above 5", v == np.nextafter(5.0, INF)), ("v == 20", v == 20),
                  ("v just below 20", v == np.nextafter(20.0, 0)), ("v just above 20", v == np.nextafter(20.0, INF)),
                  ("5 < v < 20", (v > 6) & (v < 19)), ("v >= 40", v >= 40)):
        E["comfort: " + nm] = int(np.sum(m))
    return E


# ---------------------------------------------------------------------------------------------- estimate_traj
T_GEOMETRIC = lambda N: 0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1))                       # ABO/Settings.m:120-121
T_NON_MONOTONE = lambda N: np.array(([0.5, 0.5, 2.0, 0.25, 0.25, 1.0, 0.5, 0.125] * 8)[:N])   # tConstACC = 3: i = 4 fails, i = 5 holds

ESTIMATE_VARIANTS = {
    # name: (tree, N, overrides, exact): exact where every sum and product of the table is representable
    "abo20_uniform": ("ABO", 20, {}, True),
    "orig63_uniform": ("ORIG", 63, {}, True),
    "abo2_uniform": ("ABO", 2, {}, True),
    "orig20_non_monotone": ("ORIG", 20, dict(Tvec=T_NON_MONOTONE(20)), True),
    "abo63_non_monotone": ("ABO", 63, dict(Tvec=T_NON_MONOTONE(63)), True),
    "abo20_geometric": ("ABO", 20, dict(Tvec=T_GEOMETRIC(20)), False),
    "orig63_geometric": ("ORIG", 63, dict(Tvec=T_GEOMETRIC(63)), False),
}
# tConstACC with Ts = 0.5: 3 and 1 are whole multiples (6, 2), 0.75 < 2 Ts (no accelerated step), 2.75 / Ts = 5.5
T_CONST = [3.0, 1.0, 0.75, 2.75, 256.0]
# (s0, v0, a0): v0 + k Ts a0 == 0 exactly at k = 4 (Ts = 0.5) for the second, at k = 1 for the third
STATES_EXACT = [(1000.5, 12.25, 1.5), (0.0, 2.0, -1.0), (37.0, 0.5, -1.0), (4096.0, 0.0, 0.75), (250.0, 3.0, -8.0), (12.0, 0.0, 0.0),
                (640.0, 10.0, -0.5)]
STATES_ROUNDED = [(1000.3, 12.7, 1.1), (0.1, 2.3, -0.9), (8191.9, 33.3, -0.7), (123.456, 0.0, 0.3)]


def estimate_opt(name):
    tree, N, over, exact = ESTIMATE_VARIANTS[name]
    OPT, V = _settings(tree, N)
    return dict(OPT, **over), V, exact


def estimate_case(name):
    """-> OPT, V, exact, runs, problems.  runs: list of (estSetting, mode, tConstACC, s0, v0, a0), one call of the reference
    each; problems: arrays run [n] (index into runs) and lane [n], with every lane 0 .. N and three beyond N per run."""
    OPT, V, exact = estimate_opt(name)
    N = int(OPT["N_hor"])
    runs = []
    for a, tc in enumerate(T_CONST):
        for b, st in enumerate(STATES_EXACT + ([] if exact else STATES_ROUNDED)):
            for mode in (0, 1):
                if mode == 0 and a > 0 and b > 1:
                    continue                                          # mode 0 does not look at tConstACC or a0
                runs.append(((a + b) % 2, mode, tc) + st)
    lanes = list(range(N + 1)) + [N + 1, N + 5, 200]
    run = np.repeat(np.arange(len(runs)), len(lanes)).astype(np.int32)
    lane = np.tile(np.array(lanes, dtype=np.int32), len(runs))
    return OPT, V, exact, runs, run, lane


def estimate_run_opt(OPT, r):
    """The settings of one run: the estimator mode and tConstACC of the vehicle it is for, a decoy in the other vehicle's"""
    est, mode, tc = r[:3]
    o = dict(OPT, paramEstSetting=mode if est == 0 else 1 - mode, TVestSetting=mode if est == 1 else 1 - mode)
    o.update(tConstACC_ego=tc if est == 0 else tc + 1.25, tConstACC_tar=tc if est == 1 else tc + 1.25)
    return o


def estimate_reference(OPT, runs, run, lane):
    """s_est [n], v_est [n]: the reference's trajectory of each run, read at min(lane, N_hor)"""
    N = int(OPT["N_hor"])
    traj = [stage_ref.estimate_trajectory(estimate_run_opt(OPT, r), r[0], *r[3:]) for r in runs]
    k = np.minimum(lane, N)
    return np.array([traj[q][0][kk] for q, kk in zip(run, k)]), np.array([traj[q][1][kk] for q, kk in zip(run, k)])


def estimate_edges(OPT, runs, run, lane):
    N, Tvec = int(OPT["N_hor"]), np.asarray(OPT["Tvec"], dtype=np.float64)
    E = {k: 0 for k in ("mode 0", "mode 1", "ego", "target", "tConstACC / Ts a whole number within the horizon",
                        "tConstACC < 2 Ts: no accelerated step", "accelerated at every stage", "v + Ts a == 0 exactly at a stage",
                        "the clamp holds for two stages running", "a0 == 0", "constant-velocity tail of at least two stages")}
    E["lane == N"], E["lane > N"], E["lane == 0"] = int(np.sum(lane == N)), int(np.sum(lane > N)), int(np.sum(lane == 0))
    fails_then_holds = again = 0
    for est, mode, tc, s0, v0, a0 in runs:
        E["mode %d" % mode] += 1
        E["ego" if est == 0 else "target"] += 1
        if mode == 0:
            continue
        ok = [(i <= tc / Tvec[i - 2]) for i in range(2, N + 2)]       # :73, i 1-based
        ratio = tc / Tvec
        E["tConstACC / Ts a whole number within the horizon"] += int(any(r == math.floor(r) and 2 <= r <= N + 1 and r == i
                                                                         for i, r in zip(range(2, N + 2), ratio)))
        E["tConstACC < 2 Ts: no accelerated step"] += int(not any(ok) and a0 != 0)
        E["accelerated at every stage"] += int(all(ok) and a0 > 0)
        E["a0 == 0"] += int(a0 == 0)
        fails_then_holds += int(any(not a and b for a, b in zip(ok, ok[1:])))
        if ok and not ok[-1] and not ok[-2]:
            E["constant-velocity tail of at least two stages"] += 1
        v, held = v0, False
        for i in range(2, N + 2):
            Ts = Tvec[i - 2]
            if ok[i - 2]:
                if v + Ts * a0 == 0:
                    E["v + Ts a == 0 exactly at a stage"] += 1
                if v + Ts * a0 > 0:
                    v = v + Ts * a0
                    again += int(held and a0 < 0)
                    held = False
                else:
                    E["the clamp holds for two stages running"] += int(held)
                    held = True
    if not np.all(Tvec == Tvec[0]) and np.any(np.diff(Tvec) < 0):
        E["index condition fails and then holds again"] = fails_then_holds
        E["accelerates again after the clamp held"] = again
    return E


# ---------------------------------------------------------------------------------------------- interp_pwa
def _unfaithful(a, b):
    """a + 1.0 * (b - a) != b: InterpPWA.m:22-23 on the right end of a segment does not return the table value"""
    return a + (b - a) != b


INTERP_TABLES = {
    # the first knot is not 0; a flat segment (4 .. 8); segments that end in a value the interpolation formula misses
    "five_knots": ([1.0, 2.0, 4.0, 8.0, 16.0], [0.1, 0.7, -0.3, -0.3, 1e-3]),
    "two_knots": ([-3.0, 5.0], [0.7, -0.9]),
    "two_knots_flat": ([0.0, 0.5], [0.05, 0.05]),
    "one_knot": ([7.0], [0.125]),
}


def interp_case(name):
    """-> doms, vals, d [n], expected [n], tol [n] (0 where the result is a table value or the formula with f = 0 or 1)"""
    doms, vals = INTERP_TABLES[name]
    d = [doms[0] - 1.0, doms[0] - 1e9, doms[-1] + 1.0, doms[-1] + 1e9, -INF, INF]
    for k in doms:
        d += near(k)
    for a, b in zip(doms, doms[1:]):
        d += [0.5 * (a + b), a + (b - a) / 3, a + 0.7 * (b - a), a + (b - a) / 1024]
    d = np.array(d)
    exp, tol = np.zeros(d.size), np.zeros(d.size)
    for q, dd in enumerate(d):
        r = stage_ref.interp_pwa(float(dd), doms, vals)
        if r is None:
            # one knot, d on it: InterpPWA.m leaves val unset (an error in MATLAB); a one-knot table is a constant, and the
            # device returns its only value
            assert len(doms) == 1 and dd == doms[0]
            r = vals[0]
        exp[q] = r
        inside = [k for k in range(len(doms) - 1) if doms[k] < dd < doms[k + 1]]
        if inside:                                                    # 2 ulp of the larger neighbouring value
            tol[q] = 2 * np.spacing(max(abs(vals[inside[0]]), abs(vals[inside[0] + 1])))
    return doms, vals, d, exp, tol


def interp_edges(name):
    doms, vals, d, exp, tol = interp_case(name)
    E = {"below the first knot": int(np.sum(d < doms[0])), "above the last knot": int(np.sum(d > doms[-1])),
         "on every knot": min(int(np.sum(d == k)) for k in doms)}
    if len(doms) > 1:
        E["inside every segment"] = min(int(np.sum((d > a) & (d < b))) for a, b in zip(doms, doms[1:]))
        E["just below and above every knot"] = min(int(np.sum(d == np.nextafter(k, s))) for k in doms for s in (-INF, INF))
    if name == "five_knots":
        E["a flat segment"] = int(any(a == b for a, b in zip(vals, vals[1:])))
        E["first knot not 0"] = int(doms[0] != 0)
        E["last knot: the formula misses the table value"] = int(_unfaithful(vals[-2], vals[-1]))
        E["an inner knot: the formula misses the table value"] = int(any(_unfaithful(a, b) for a, b in zip(vals, vals[1:-1])))
    if name == "two_knots":
        E["last knot: the formula misses the table value"] = int(_unfaithful(vals[0], vals[1]))
    return E


# ---------------------------------------------------------------------------------------------- plant_rk4
SLOPED = dict(s_slope=np.array([0.0, 100.0, 200.0, 5000.0, 10000.0]), slope=np.arctan(np.array([0.0, 5.0, -3.0, 2.0, 0.0]) / 100))
PLANT_VARIANTS = {
    # name: (tree, overrides); the settings' own N_integratePlant is 10, their own slope table flat ([1 2] -> [0 0])
    "abo_sloped_m10": ("ABO", dict(SLOPED)),
    "orig_sloped_m1": ("ORIG", dict(SLOPED, N_integratePlant=1)),
    "abo_flat_m1": ("ABO", dict(N_integratePlant=1)),
    "orig_flat_m10": ("ORIG", {}),
}
PLANT_S = [0.0, 2.0 ** -20, 0.5, 95.5, 99.75, 199.99, 4999.0, 9996.5, 9999.5, 10004.0]
PLANT_V = [0.0, 0.3, 13.9, 20.0, 35.0]


def plant_opt(name):
    tree, over = PLANT_VARIANTS[name]
    OPT, V = _settings(tree, 20)
    return dict(OPT, **over), V


def plant_case(name):
    """-> OPT, V, s [n], v [n], u [n]: every position with every speed, the force walking from hard braking to full drive"""
    OPT, V = plant_opt(name)
    full = V["phi"] * V["T_m_max"] * V["eta_TF"]
    U = [-1e4, -3000.0, -250.5, 0.0, 1200.0, 0.5 * full, full]
    s, v, u = [], [], []
    for a, ss in enumerate(PLANT_S):
        for b, vv in enumerate(PLANT_V):
            s.append(ss); v.append(vv); u.append(U[(3 * a + b) % len(U)])
    for uu in (-1e4, -3000.0):                                        # standstill and braking: no clamp, the speed goes negative
        s.append(50.0); v.append(0.0); u.append(uu)
    return OPT, V, np.array(s), np.array(v), np.array(u)


def plant_distance(s1, v1, ref):
    """Largest distance of (s1 [n], v1 [n]) to the mpmath results ref [n] of (s, v) pairs, relative to max(1, |value|)"""
    import mpmath
    worst = 0.0
    with mpmath.workdps(stage_ref.MP_DIGITS):
        for a, b, (rs, rv) in zip(s1, v1, ref):
            worst = max(worst, float(abs(mpmath.mpf(float(a)) - rs) / max(1, abs(rs))), float(abs(mpmath.mpf(float(b)) - rv) / max(1, abs(rv))))
    return worst


@functools.lru_cache(maxsize=None)
def plant_references(name):
    """-> (fp64 s1, fp64 v1, list of mpmath (s1, v1)) of stage_ref.plant_rk4 on the case's inputs"""
    OPT, V, s, v, u = plant_case(name)
    f = [stage_ref.plant_rk4(OPT, V, a, b, c) for a, b, c in zip(s, v, u)]
    m = [stage_ref.plant_rk4(OPT, V, a, b, c, mp=True) for a, b, c in zip(s, v, u)]
    return np.array([x[0] for x in f]), np.array([x[1] for x in f]), m


def plant_edges(name):
    OPT, V, s, v, u = plant_case(name)
    M, DT = int(OPT["N_integratePlant"]), float(OPT["Tvec"][0]) / int(OPT["N_integratePlant"])
    knots = np.asarray(OPT["s_slope"], dtype=np.float64)
    _, v1, _ = plant_references(name)
    E = {"hard braking": int(np.sum(u == -1e4)), "full drive": int(np.sum(u == u.max())), "no force": int(np.sum(u == 0)),
         "standstill, braking: speed goes negative": int(np.sum((v == 0) & (u < 0) & (v1 < 0))),
         "s near 0": int(np.sum(s < 1)), "s near 1e4 m": int(np.sum(np.abs(s - 1e4) < 10))}
    if not np.all(np.asarray(OPT["slope"]) == np.asarray(OPT["slope"])[0]):
        # the four stages of the first RK step are at s, about s + DT/2 v (twice) and about s + DT v
        E["the stages of one RK step straddle a slope knot"] = int(sum(np.any((knots > a) & (knots < a + 0.9 * DT * b)) for a, b in zip(s, v)))
        E["beyond the last slope knot"] = int(np.sum(s > knots[-1]))
    return E
