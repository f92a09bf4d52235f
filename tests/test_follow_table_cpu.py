"""report.follow_table -- the vehicle-following and cost key figures of a batch, the executable specification of
eepacc_follow_kpis -- on the CPU: its cost fields against the reference's own saved cost_* series, its headway fields
against independent numpy, the edge cases by hand, the enum mirror and the argument checks that need no device.

Tolerances.  Counts, the index, the minima and the maximum must be equal.  A sum of n terms taken in two orders differs by
at most about 2 (n - 1) u sum|terms|, u = 2^-53: the bar for a cost is 4 n u |w| sum|terms| (tests/test_gpu_kpis.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, load_golden, make_case
from eepacc_mpc_casadi_matlab_amd import report
from eepacc_mpc_casadi_matlab_amd._abi import FKPI, FKPI_FIELDS, FKPI_N, FKPI_WEIGHTS

U = 2.0 ** -53
INF = np.inf
COSTS = FKPI_FIELDS[FKPI["cost_P"]:]
HEADWAY = ("lead_samples", "h_min_m", "h_min_index", "thw_min_s", "margin_min_m", "margin_viol_steps", "ttc_min_s")
SAVED = ("abo_abmpc", "orig_abmpc", "abo_fbmpc", "orig_fbmpc")


def _saved(name):
    """A saved solution of the reference as [n, 1] columns, with its tree's settings, weights and the lead it was run on."""
    OPT, V, s_tv, v_tv = make_case("ABO" if name.startswith("abo") else "ORIG", 20)
    G = load_golden(name)
    n = G["s_opt"].size
    col = lambda x: np.asarray(x, dtype=np.float64).reshape(-1, 1)[:n]
    rows = [col(G[k + "_opt"]) for k in ("s", "v", "Fm", "a", "xi_v", "xi_h", "xi_s", "xi_f")] + [col(s_tv), col(v_tv)]
    W = report.follow_weights(OPT, "ab" if name.endswith("abmpc") else "fb")
    return OPT, V, G, rows, W


def _table(rows, OPT, V, W):
    return report.follow_table(*rows, OPT["Tvec"][0], OPT["h_min"], OPT["tau_min"], W, OPT["b_fifthOrder"], V["phi"])


@pytest.mark.parametrize("name", SAVED)
def test_costs_against_the_saved_series(name):
    """The cost fields are the last entries of the reference's cumulative cost_* (RunOpt_ABMPC.m:391-398,
    RunOpt_FBMPC.m:382-390), cost_P from the saved Fm_opt and the speed behind the saved rpm_opt."""
    OPT, V, G, rows, W = _saved(name)
    s, v, Fm, a, xi_v, xi_h, xi_s, xi_f = [r[:, 0] for r in rows[:8]]
    n = s.size
    T = _table(rows, OPT, V, W)
    assert T.shape == (FKPI_N, 1)
    rpm = 30.0 / np.pi * v * V["phi"]
    assert np.abs(rpm - G["rpm_opt"]).max() <= 4 * U * np.abs(rpm).max()           # the surface is fed the saved motor speed
    j = np.diff(a) / float(OPT["Tvec"][0])
    terms = {"cost_P": report.power_surface(OPT["b_fifthOrder"], Fm, rpm) ** 2, "cost_a": a ** 2, "cost_j": j ** 2,
             "cost_xi_v": xi_v, "cost_xi_h": xi_h, "cost_xi_s": xi_s, "cost_xi_f": xi_f}
    for w, key in zip(W, COSTS):
        got = T[FKPI[key], 0]
        if key == "cost_P" and name.endswith("abmpc"):
            assert "cost_P" not in G.files and got == 0.0                         # RunOpt_ABMPC defines none
            continue
        assert G[key].size == n - 1
        bar = 4 * n * U * abs(w) * np.abs(terms[key][:n - 1]).sum()
        print(name, key, got, "saved", G[key][-1], "difference", abs(got - G[key][-1]), "bar", bar)
        assert abs(got - G[key][-1]) <= bar, (name, key, got, G[key][-1], bar)
    assert T[FKPI["cost_a"], 0] > 0 and T[FKPI["cost_xi_v"], 0] > 0


def test_ab_weights_are_the_users_W_1_to_5():
    """RunOpt_ABMPC.m:383-388: W(1..5) of OPTsettings.W_AB with w_f = W(5), in both trees -- in ABO's seven entries W(1) is
    w_FC, and the reference's cost_a uses it all the same."""
    abo = dict(W_AB=[7.0, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0], W_FB=np.arange(10.0, 17.0))
    orig = dict(W_AB=[1.0, 2.0, 3.0, 4.0, 5.0, 6.0], W_FB=np.arange(10.0, 17.0))
    assert np.array_equal(report.follow_weights(abo, "ab"), [0.0, 7.0, 1.0, 2.0, 3.0, 4.0, 4.0])
    assert np.array_equal(report.follow_weights(orig, "ab"), [0.0, 1.0, 2.0, 3.0, 4.0, 5.0, 5.0])
    assert np.array_equal(report.follow_weights(abo, "fb"), np.arange(10.0, 17.0))
    assert np.array_equal(report.follow_weights(abo, "none"), [0.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])
    with pytest.raises(ValueError):
        report.follow_weights(abo, "bl")


def _independent_headway(s, v, s_tv, v_tv, h_min, tau_min):
    """The headway fields of one instance with numpy's own reductions over a mask."""
    lead = s_tv < 1e6
    h = s_tv - s
    if not lead.any():
        return [0.0, INF, -1.0, INF, INF, 0.0, INF]
    m = h - np.maximum(h_min, v * tau_min)
    with np.errstate(divide="ignore", invalid="ignore"):
        thw, ttc = h / v, h / (v - v_tv)
    mv, mc = lead & (v > 0), lead & (v - v_tv > 0)
    return [float(lead.sum()), np.min(h[lead]), float(np.flatnonzero(lead & (h == np.min(h[lead])))[0]),
            np.min(thw[mv]) if mv.any() else INF, np.min(m[lead]), float((m[lead] < 0).sum()), np.min(ttc[mc]) if mc.any() else INF]


@pytest.mark.parametrize("name", SAVED)
def test_headway_against_independent_numpy(name):
    OPT, V, G, rows, W = _saved(name)
    T = _table(rows, OPT, V, W)
    s, v, s_tv, v_tv = rows[0][:, 0], rows[1][:, 0], rows[8][:, 0], rows[9][:, 0]
    want = _independent_headway(s, v, s_tv, v_tv, OPT["h_min"], OPT["tau_min"])
    got = [T[FKPI[k], 0] for k in HEADWAY]
    assert got == want, (got, want)
    assert T[FKPI["xi_h_max"], 0] == np.max(rows[5])
    assert got[0] == s.size and 1.9 < got[1] < 3.0 and got[3] > 1.0            # the saved runs follow the lead at about h_min


def _hand(s, v, s_tv, v_tv, a=None, xi=None, W=None, h_min=2.0, tau_min=0.5, Ts=0.5):
    """One instance by hand: lists in, the column of the table out as a dict."""
    col = lambda x: np.asarray(x, dtype=np.float64).reshape(-1, 1)
    n = len(s)
    a = [0.0] * n if a is None else a
    xi = [0.0] * n if xi is None else xi
    OPT, V, _, _ = make_case("ABO", 20)
    T = report.follow_table(col(s), col(v), col([100.0] * n), col(a), col(xi), col(xi), col(xi), col(xi), col(s_tv), col(v_tv), Ts,
                            h_min, tau_min, report.follow_weights(OPT, "none") if W is None else W, OPT["b_fifthOrder"], V["phi"])
    return {k: T[i, 0] for k, i in FKPI.items()}


def test_no_lead_at_all():
    r = _hand([0.0, 5.0, 10.0], [10.0, 10.0, 10.0], [INF] * 3, [0.0] * 3, xi=[0.25, 0.5, 0.125])
    assert [r[k] for k in HEADWAY] == [0.0, INF, -1.0, INF, INF, 0.0, INF]
    assert r["xi_h_max"] == 0.5 and r["cost_xi_h"] == 0.75                      # what needs no lead is there
    # the reference's "no lead" is a lead at 1e6 m or more (Main.m:288), and a NaN is no lead sample either
    assert [_hand([0.0, 5.0], [1.0, 1.0], far, [0.0, 0.0])["lead_samples"] for far in ([1e6, 2e6], [np.nan, np.nan], [999999.0, 1e6])] == [0.0, 0.0, 1.0]


def test_lead_that_appears_mid_run():
    """The cut-in of use case 10: no lead, then one 12 m ahead that the ego closes in on."""
    r = _hand(s=[0.0, 10.0, 20.0, 30.0, 40.0], v=[20.0] * 5, s_tv=[INF, INF, 32.0, 41.0, 50.0], v_tv=[0.0, 0.0, 18.0, 18.0, 18.0])
    assert [r[k] for k in HEADWAY] == [3.0, 10.0, 4.0, 0.5, 0.0, 0.0, 5.0]       # gaps 12, 11, 10 m; policy 10 m; closing at 2 m/s
    r = _hand(s=[0.0, 10.0, 20.0, 30.0, 40.0], v=[20.0] * 5, s_tv=[INF, INF, 29.0, 38.0, 50.0], v_tv=[0.0, 0.0, 18.0, 18.0, 18.0])
    assert [r[k] for k in HEADWAY] == [3.0, 8.0, 3.0, 0.4, -2.0, 2.0, 4.0]       # gaps 9, 8, 10 m: two samples inside the policy


def test_standstill_samples():
    """v = 0: no headway time and no time to collision from such a sample, the policy is h_min."""
    r = _hand(s=[0.0, 0.0, 1.0], v=[0.0, 0.0, 2.0], s_tv=[3.0, 3.5, 6.0], v_tv=[0.0, 1.0, 3.0])
    assert [r[k] for k in HEADWAY] == [3.0, 3.0, 0.0, 2.5, 1.0, 0.0, INF]
    r = _hand(s=[0.0, 0.0], v=[0.0, 0.0], s_tv=[1.5, 1.0], v_tv=[0.0, 0.0])
    assert [r[k] for k in HEADWAY] == [2.0, 1.0, 1.0, INF, -1.0, 2.0, INF]


def test_never_closing():
    r = _hand(s=[0.0, 5.0, 10.0], v=[10.0, 10.0, 10.0], s_tv=[20.0, 26.0, 31.0], v_tv=[10.0, 12.0, 10.0])
    assert r["ttc_min_s"] == INF and r["thw_min_s"] == 2.0 and r["h_min_m"] == 20.0 and r["h_min_index"] == 0.0


def test_repeated_minimum_reports_the_first_index():
    r = _hand(s=[0.0, 1.0, 2.0, 3.0, 4.0], v=[1.0] * 5, s_tv=[9.0, 8.0, 10.0, 10.0, 11.0], v_tv=[1.0] * 5)
    assert r["h_min_m"] == 7.0 and r["h_min_index"] == 1.0                       # gaps 9, 7, 8, 7, 7


def test_one_and_two_steps():
    """n = 1: the sums of k = 1:N_sim are empty, seven zeros; n = 2: one term each, of sample 0, and one jerk."""
    W = np.array([2.0, 3.0, 5.0, 7.0, 11.0, 13.0, 17.0])
    r = _hand(s=[1.0], v=[4.0], s_tv=[9.0], v_tv=[2.0], a=[1.5], xi=[0.25], W=W)
    assert [r[k] for k in COSTS] == [0.0] * 7
    assert [r[k] for k in HEADWAY] == [1.0, 8.0, 0.0, 2.0, 6.0, 0.0, 4.0] and r["xi_h_max"] == 0.25
    r = _hand(s=[1.0, 2.0], v=[4.0, 4.0], s_tv=[9.0, 9.5], v_tv=[2.0, 2.0], a=[1.5, -0.5], xi=[0.25, 0.75], W=W)
    OPT, V, _, _ = make_case("ABO", 20)
    P0 = report.power_surface(OPT["b_fifthOrder"], np.array([100.0]), np.array([30.0 / np.pi * 4.0 * V["phi"]]))[0]
    assert [r[k] for k in COSTS] == [2.0 * (P0 * P0), 3.0 * 2.25, 5.0 * 16.0, 7.0 * 0.25, 11.0 * 0.25, 13.0 * 0.25, 17.0 * 0.25]
    assert r["xi_h_max"] == 0.75 and r["h_min_m"] == 7.5 and r["h_min_index"] == 1.0
    assert _hand(s=[1.0, 2.0], v=[4.0, 4.0], s_tv=[9.0, 9.5], v_tv=[2.0, 2.0], a=[1.5, -0.5], W=W * [0, 1, 1, 1, 1, 1, 1])["cost_P"] == 0.0


def test_summarise_table_takes_the_table():
    """summarise_table reduces this table by class too; +inf (no lead in an instance) stays +inf in max and mean, no NaN."""
    T = np.zeros((FKPI_N, 4))
    T[FKPI["h_min_m"]] = [3.0, INF, 5.0, 4.0]
    T[FKPI["lead_samples"]] = [10.0, 0.0, 10.0, 10.0]
    S = report.summarise_table(T, [0, 0, 1, 1])
    assert S["mean"].shape == (2, FKPI_N) and not np.isnan(S["mean"]).any()
    h = FKPI["h_min_m"]
    assert np.array_equal(S["min"][:, h], [3.0, 4.0]) and np.array_equal(S["max"][:, h], [INF, 5.0]) and np.array_equal(S["mean"][:, h], [INF, 4.5])
    assert "+inf" in report.summarise_table.__doc__


def test_enum_mirror_equals_the_header():
    hdr = open(os.path.join(ROOT, "include", "eepacc.h")).read()
    body = re.search(r"enum \{\s*EEPACC_FKPI_LEAD_SAMPLES = 0,(.*?)\};", hdr, re.S).group(0)
    names = re.findall(r"^\s*(EEPACC_FKPI_[A-Z_]+)", body, re.M)
    assert names == ["EEPACC_FKPI_" + f.upper() for f in FKPI_FIELDS] + ["EEPACC_FKPI_N"] and FKPI_N == 15
    body = re.search(r"enum \{\s*EEPACC_FKPI_W_AB = 0,(.*?)\};", hdr, re.S).group(0)
    names = re.findall(r"^\s*(EEPACC_FKPI_W_[A-Z]+)", body, re.M)
    assert names == ["EEPACC_FKPI_W_AB", "EEPACC_FKPI_W_FB", "EEPACC_FKPI_W_NONE"]
    assert FKPI_WEIGHTS == {"ab": 0, "fb": 1, "none": 2}


def test_argument_checks_that_need_no_device():
    """weights, n_steps and the five buffers are checked before the handle is looked at: EEPACC_EINVAL with the argument's name."""
    from eepacc_mpc_casadi_matlab_amd import engine
    lib = engine.load_library()
    buf = (C.c_double * 16)()
    p = C.addressof(buf)
    ok = dict(B=1, n_steps=1, weights=0, traj=p, status=p, s_tv=p, v_tv=p, fkpi=p)
    order = ("B", "n_steps", "weights", "traj", "status", "s_tv", "v_tv", "fkpi")

    def call(**kw):
        rc = lib.eepacc_follow_kpis(None, *[dict(ok, **kw)[k] for k in order], None)
        return rc, lib.eepacc_last_error().decode()
    for bad in (3, -1, 7):
        rc, msg = call(weights=bad)
        assert rc == -1 and "eepacc_follow_kpis: weights = %d" % bad in msg, msg
    for bad in (0, -2):
        rc, msg = call(n_steps=bad)
        assert rc == -1 and "eepacc_follow_kpis: n_steps = %d" % bad in msg, msg
    for name in ("traj", "status", "s_tv", "v_tv", "fkpi"):
        rc, msg = call(**{name: None})
        assert rc == -1 and "eepacc_follow_kpis: %s is NULL" % name in msg, msg
    rc, msg = call()
    assert rc == -1 and "NULL handle" in msg, msg                                  # everything else is in order
