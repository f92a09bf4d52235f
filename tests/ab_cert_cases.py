"""The case table of tests/test_ab_cert_cpu.py and tests/test_gpu_ab_cert.py: ABMPC step inputs (s, v, a_prev, t0, s_tv, v_tv,
a_tv_prev) written by hand so that rows of every type carry a multiplier at the optimum, per configuration (tree, horizon,
move blocking, time steps, fuel map), and the map from a row's position within a stage to its type.

Nothing of the product is used here beyond the settings; the CPU test proves on the oracle's dense problem and the KKT
certificate of tests/qp_cert.py that the table does what this docstring says."""
import functools

import numpy as np

from conftest import GOLDEN_AB_ICEMAP
from eepacc_mpc_casadi_matlab_amd._abi import AB_ROW_TYPES
from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, default_opt

INS = ("s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev")
MB20 = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1]
ICE = dict(W_AB=np.array(GOLDEN_AB_ICEMAP["W_AB"]), fuel_map=GOLDEN_AB_ICEMAP["fuel_map"])
SLACK_BOUNDS = ("xi_v", "xi_h", "xi_s", "xi_f")
ROUTE_TYPES = ("v_lim", "v_curv", "v_stop", "v_tl")
# the route of tests/test_gpu_ab_build.py::test_route_features_vs_oracle: every ORIG configuration drives on it
ROUTE = dict(slopes=np.array([[3.0, 40, 160], [-2.0, 300, 420]]),
             speedLimZones=np.array([[50.0, 0.0], [30.0, 150.0], [70.0, 400.0]]),
             curves=np.array([[-1 / 25.0, 90, 120], [1 / 60.0, 250, 300]]),
             stopLoc=np.array([200.0, 520.0]),
             TLLoc=np.array([[330.0, 5.0, 20.0, 25.0], [600.0, 0.0, 15.0, 15.0]]))


def _geometric(N):
    return 0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1))


def _configs():
    C = {}
    for tree in ("ABO", "ORIG"):
        t = tree.lower()
        for N in (2, 3, 20, 32, 33, 63):
            C["%s%d" % (t, N)] = (tree, N, {})
        C["%s20_mb" % t] = (tree, 20, dict(Mb=np.array(MB20)))
        C["%s24_tvec" % t] = (tree, 24, dict(Tvec=_geometric(24), paramEstSetting=0, TVestSetting=0))
    C["abo20_ice"] = ("ABO", 20, dict(ICE))
    C["abo33_ice"] = ("ABO", 33, dict(ICE))
    C["abo20_ice_mb"] = ("ABO", 20, dict(ICE, Mb=np.array(MB20)))
    return C


CONFIGS = _configs()                      # name -> (tree, N, overrides)
EDGE_HORIZONS = (2, 3, 32, 33, 63)


@functools.lru_cache(maxsize=None)
def settings(name):
    """-> OPT, V of a configuration"""
    tree, N, over = CONFIGS[name]
    o = default_opt()
    if tree == "ORIG":
        o.update(ROUTE)
    OPT = Settings(o, tree=tree, N_hor=N)
    OPT.update(over)
    return OPT, SetVehicleParameters(tree)


def row_map(tree, N, Mb=None):
    """(stage, type name) of every row of the dense problem from the position within a stage alone: the order of
    AB_ROW_TYPES, `blocked` only at a blocked stage, the four route caps only in the ORIG tree, two terminal rows."""
    stage, typ = [], []
    for k in range(N):
        for t in AB_ROW_TYPES:
            if t == "blocked" and (Mb is None or not Mb[k]):
                continue
            if t in ROUTE_TYPES and tree != "ORIG":
                continue
            stage.append(k); typ.append(t)
    stage += [N, N]; typ += ["safe1", "safe2"]
    return np.array(stage), np.array(typ)


def config_row_map(name):
    tree, N, over = CONFIGS[name]
    return row_map(tree, N, over.get("Mb"))


def catalogue(name):
    """The row types of a configuration, in the order of AB_ROW_TYPES"""
    present = set(config_row_map(name)[1])
    return [t for t in AB_ROW_TYPES if t in present]


#         name               s       v     a_prev  t0     gap     v_tv  a_tv_prev
STATES = [
    # hard braking: the lead close, slow and decelerating
    ("brake_hard",          60.0,  14.0,   0.0,   3.0,   22.0,    6.0,  -1.5),
    ("brake_closing",       30.0,  11.0,   0.5,   1.0,   16.0,    5.0,  -0.8),
    ("brake_late",         420.0,  16.0,  -1.0,  40.0,   30.0,    7.5,  -2.0),
    ("brake_slow_lead",    230.0,   8.0,   0.0,  12.0,    9.0,    2.5,  -0.5),
    ("brake_wall",         240.0,  10.0,   0.0,  14.0,   14.0,    0.5,  -1.0),
    ("brake_wall_fast",    430.0,  14.0,  -1.5,  20.0,   30.0,    1.0,  -2.0),
    ("brake_below_limit",   40.0,  10.0,  -7.0,   7.0,   10.0,    4.0,  -1.0),
    # free acceleration: standstill or low speed, free road, a_prev far below the wanted acceleration
    ("free_standstill",      5.0,   0.0,  -1.0,   0.0,    1e4,    0.0,   0.0),
    ("free_low_speed",      20.0,   3.0,  -2.0,   2.0,   70.0,    7.0,   0.0),
    ("free_after_brake",   450.0,   6.0,  -3.0,  50.0,   90.0,    9.0,   0.5),
    ("free_pulling_hard",    8.0,   1.0,   5.5,   0.5,    1e4,    0.0,   0.0),
    ("pull_above_limit",     3.0,   2.0,   7.0,   0.5,    1e4,    0.0,   0.0),
    ("pull_at_limit",        6.0,   2.0,   3.9,   1.0,   50.0,    8.0,   0.0),
    # jerk at stage 0: a_prev at a limit with the opposite demand
    ("jerk0_brake",         70.0,  13.0,   2.5,   5.0,   20.0,    6.0,  -1.0),
    ("jerk0_release",       15.0,   4.0,  -4.5,   1.5,   55.0,    7.5,   0.0),
    # speed bound: v at and just above 0, the lead inside the safe distance and pulling away
    ("v_zero",              12.0,   0.0,   0.0,   0.0,    1.5,    1.0,   1.0),
    ("v_small",            460.0,   0.25, -2.0,   8.0,    1.0,    1.5,   1.0),
    # route features of the ORIG trees: above a speed-limit step, before a curve, before a stop, before a red light
    ("route_limit_step",   135.0,  13.5,   0.0,   2.0,    1e4,    0.0,   0.0),
    ("route_curve",         80.0,  13.0,   0.5,   1.0,  150.0,   12.0,   0.0),
    ("route_stop",         185.0,   7.0,   0.0,   4.0,    1e4,    0.0,   0.0),
    ("route_light",        318.0,   8.0,   0.0,   6.0,   60.0,    9.0,   0.0),
    # headway violated so far that the xi_h row reaches its cap before it becomes tight
    ("headway_deep",       480.0,  15.0,   0.0,  60.0,   12.0,   15.0,   0.0),
    ("headway_cut_in",      50.0,  12.0,   1.0,   9.0,    7.0,   13.0,   0.5),
    ("cut_in_tight",       440.0,  10.0,   0.0,  11.0,    3.5,   13.0,   1.0),
    ("cut_in_inside",       25.0,   9.0,  -1.0,   2.5,    2.5,   12.0,   1.5),
]


# States left out of a configuration.  There the optimum is degenerate by read_certificate's scaled ratio, measured on the
# oracle's problem: mostly the ORIG tree cruising on its speed limit, where the cap, the travel incentive and the bound of
# xi_v are tight together over many stages.  The threshold used for leaving out was 3e-6, three times DEGENERATE_RATIO on
# purpose: the device builds the same problem with other rounding, and a case must not change sides there.  At N = 63 a few
# more stay out to keep the refinement of 315 x 1136 problems short.  This selection does not bring the ORIG tables under the
# issue's unscaled measure; tests/test_ab_cert_cpu.py says what holds instead and why.
LEFT_OUT = {
    "abo63": ("brake_hard", "brake_late", "brake_wall_fast", "jerk0_brake", "route_limit_step", "route_curve", "route_stop",
              "route_light", "free_low_speed", "brake_slow_lead", "headway_cut_in", "cut_in_inside"),
    "orig20": ("free_standstill", "free_low_speed", "free_after_brake", "jerk0_release", "route_stop", "route_light",
               "headway_deep"),
    "orig32": ("free_standstill", "route_curve", "route_stop"),
    "orig33": ("free_standstill", "route_stop"),
    "orig63": ("brake_hard", "brake_wall_fast", "free_standstill", "pull_at_limit", "route_stop", "headway_deep", "headway_cut_in",
               "cut_in_tight", "brake_slow_lead", "free_low_speed", "free_after_brake", "cut_in_inside", "v_zero"),
    "orig20_mb": ("brake_wall", "free_standstill", "free_low_speed", "free_after_brake", "jerk0_brake", "jerk0_release", "v_small",
                  "route_stop", "route_light", "headway_deep"),
    "orig24_tvec": ("free_standstill", "free_pulling_hard", "pull_above_limit", "route_curve", "route_stop", "route_light",
                    "headway_deep", "headway_cut_in"),
    "abo20_ice": ("brake_below_limit",),
    "abo33_ice": ("v_zero", "v_small"),
    "abo20_ice_mb": ("brake_hard", "brake_wall"),
}
MAX_INSTANCES = 32


@functools.lru_cache(maxsize=None)
def cases(name):
    """-> (names, columns): the instances of a configuration; columns maps each of INS to a read-only float64 array"""
    rows = [r for r in STATES if r[0] not in LEFT_OUT.get(name, ())]
    assert 0 < len(rows) <= MAX_INSTANCES
    names = [r[0] for r in rows]
    A = np.array([r[1:] for r in rows], dtype=np.float64)
    cols = dict(s=A[:, 0], v=A[:, 1], a_prev=A[:, 2], t0=A[:, 3], s_tv=A[:, 0] + A[:, 4], v_tv=A[:, 5], a_tv_prev=A[:, 6])
    cols = {n: np.ascontiguousarray(cols[n]) for n in INS}
    for a in cols.values():
        a.setflags(write=False)
    return names, cols


def take(cols, idx):
    """The instances idx of a table, as fresh contiguous arrays"""
    return {n: np.ascontiguousarray(cols[n][idx]) for n in INS}


# ------------------------------------------------------------------------------------------------ reading a certificate
SLACK_OF = dict(a_max="xi_f", a_min="xi_f", j_max="xi_f", j_min="xi_f", v_lim="xi_f", v_curv="xi_f", v_stop="xi_s", v_tl="xi_s",
                v_inc="xi_v", safe1="xi_s", safe2="xi_s", hwp="xi_h")
DEGENERATE_RATIO = 1e-6


def slack_weights(OPT):
    """The linear cost of the four slacks (CreateQP_AB.m:183-187): what caps the multipliers of the rows they soften."""
    W = np.asarray(OPT["W_AB"], dtype=np.float64)
    w_v, w_h, w_s, w_f = W[-4:]
    return dict(xi_v=w_v, xi_h=100.0 * w_h, xi_s=w_s, xi_f=w_f)


def read_certificate(c, stage, typ, N, OPT):
    """What the tests read from qp_cert.certificate() of a dense ABMPC problem (rows of A only, no variable bounds):
    rows   (row, stage, type, multiplier) of every row with a strictly positive multiplier,
    rigid  those of them that are no slack bound,
    held   the rigid ones whose slack sits on its bound with a multiplier of its own, and the rows that have no slack: the
           rows a working set has to hold, as opposed to a soft row whose slack pays for it,
    ratio  the smallest positive multiplier relative to its scale: the cost of the row's slack (a slack bound's own cost),
           which is the multiplier's cap, and for a row without a slack the largest multiplier of such rows."""
    w = slack_weights(OPT)
    rows = [(i, int(stage[i]), str(typ[i]), float(l)) for (kind, i, sgn), l in zip(c["active"], c["lam"]) if l > 0.0]
    assert all(kind == 0 for kind, _, _ in c["active"])
    on_bound = {(t, k) for _, k, t, _ in rows if t in SLACK_BOUNDS}
    rigid = [r for r in rows if r[2] not in SLACK_BOUNDS]
    held = [r for r in rigid if r[1] == N or r[2] not in SLACK_OF or (SLACK_OF[r[2]], r[1]) in on_bound]
    bare = max([l for _, k, t, l in rows if t not in SLACK_BOUNDS and (k == N or t not in SLACK_OF)], default=1.0)
    ratio = 1.0
    for _, k, t, l in rows:
        scale = w[t] if t in SLACK_BOUNDS else bare if (k == N or t not in SLACK_OF) else w[SLACK_OF[t]]
        ratio = min(ratio, l / scale)
    lam = [l for *_, l in rows]
    return dict(rows=rows, rigid=rigid, held=held, ratio=ratio, plain_ratio=min(lam) / max(lam) if lam else 1.0)


def rollout(a, s0, v0, T):
    """s, v [N + 1, B] of the double integrator driven by the accelerations a [B, N] from (s0, v0) with the steps T [N]"""
    B, N = a.shape
    s = np.empty((N + 1, B)); v = np.empty((N + 1, B))
    s[0], v[0] = s0, v0
    for k in range(N):
        s[k + 1] = s[k] + T[k] * v[k] + 0.5 * T[k] * T[k] * a[:, k]
        v[k + 1] = v[k] + T[k] * a[:, k]
    return s, v


# ------------------------------------------------------------------------------------------------ certified optimum
PVIOL_MAX, STAT_MAX = 1e-14, 1e-13            # the thresholds of tests/test_qp_cert_cpu.py
BAR = dict(a=1e-9, v=1e-9, slack=1e-9, s=1e-8)
COST_BAR = dict(ABO=1e-8, ORIG=1e-6)          # relative to 1 + |cost|


def objective(H, g, x):
    """1/2 x'Hx + g'x in long double"""
    import qp_cert as Q
    xl = np.asarray(x, dtype=np.float64).astype(Q.LD)
    return float(0.5 * xl @ (H.astype(Q.LD) @ xl) + g.astype(Q.LD) @ xl)


def certify(H, g, A, lba, uba, x0, stage, typ, N, OPT):
    """x* = refined_solution started from x0, its certificate and what read_certificate says of it.  singular: the
    refinement did not reach a point the certificate accepts (the KKT system of the positive multipliers has no unique
    solution); degenerate: that, or a multiplier ratio below DEGENERATE_RATIO."""
    import qp_cert as Q
    p = (H, g, A, lba, uba, None, None)
    xs, _ = Q.refined_solution(*p, x0)
    finite = bool(np.isfinite(xs).all())
    c = Q.certificate(*p, xs if finite else x0)
    R = read_certificate(c, stage, typ, N, OPT)
    singular = not finite or not (c["pviol"] <= PVIOL_MAX and c["stat"] <= STAT_MAX)
    R.update(x=xs, cert=c, singular=singular, degenerate=singular or R["ratio"] < DEGENERATE_RATIO, f=objective(H, g, xs))
    return R


def full_point(A, lba, uba, a):
    """The point of a problem that has the accelerations a [N] and every slack at the smallest value that satisfies the
    rows of its group and its own lower bound.  A slack's column holds its bound row and the rows it softens: -1 in a row
    with an upper bound, +1 in a row with a lower bound; none of them has the other side."""
    nC, nV = A.shape
    x = np.zeros(nV)
    x[0::5] = a
    w = A @ x                                     # every row with the slacks at zero
    for c in range(nV):
        if c % 5 == 0:
            continue
        need = -np.inf
        for r in np.nonzero(A[:, c])[0]:
            al = A[r, c]
            lo, hi = (lba[r], uba[r]) if al > 0.0 else (-uba[r], -lba[r])     # lo <= |al| slack + sign(al) w <= hi
            assert np.isfinite(lo) and not np.isfinite(hi)
            need = max(need, (lo - np.sign(al) * w[r]) / abs(al))
        x[c] = need
    return x


def row_violation(A, lba, uba, x):
    """max(lba - Ax, Ax - uba, 0) per row"""
    ax = A @ x
    return np.maximum(np.maximum(lba - ax, ax - uba), 0.0)
