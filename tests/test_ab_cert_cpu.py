"""The case table of tests/ab_cert_cases.py is valid and reaches the rows it is written for: proven on the CPU oracle's dense
problem (Oracle.ab_step(..., want_dense=True)) with the KKT certificate of tests/qp_cert.py, without the code under test.

A row type counts as covered in a configuration when some case has a row of that type with a strictly positive multiplier in
the certificate of the refined solution.  Measured (the test prints the table): both trees cover every type of their
catalogue but `s`; every edge horizon covers a_min, a jerk type and a safety or headway row; the largest set of rigid rows
(rows that are no slack bound) with positive multipliers at N = 63 is 86 (ORIG, brake_below_limit; ABO 76, brake_closing) and
at N = 32, 33 between 55 and 67; the largest set of *held* rows, rigid rows whose slack sits on its bound or that have none
(26 at N = 63), is printed next to it.  States with larger sets at N = 63 (117 rigid, 54 held: ABO brake_late) are degenerate
there and stay out (ab_cert_cases.LEFT_OUT).

Exempt type: `s`.  CreateQP_AB.m:256-259 bounds s_k below by s_min = 0 and above by s_goal = inf (Settings.m:143).  With
s_0 >= 0 and the rows 0 <= v_k of :260-263, s_k = s_0 + sum T (v_j + v_j+1) / 2 >= s_0 >= 0: the row can be tight only at
s_0 = 0 with every speed up to stage k on its own bound, where its normal is a combination of those speed rows' normals and
the multiplier can be carried by them; at every state with s_0 > 0, as in this table, it is inactive.

Degenerate cases.  The issue's measure (smallest positive multiplier below 1e-6 of the largest) is asserted, with its cap of
one case in eight, in the ten configurations where the weights allow it: the ABO tree with its unit weights and ORIG at N = 2
and 3.  In the other nine (ISSUE_MEASURE_UNMET below: ORIG at N >= 20 and the three ICE-map configurations) it is replaced
by a scaled measure, and this is a substitution, not the issue's check: each multiplier is compared with the cost of its
row's slack, which caps it (read_certificate); the threshold 1e-6 and the cap of one case in eight stay.  Why: with the ORIG
and ICE weights the largest multiplier of every feasible case is w_s = 9e7, carried by the bound of xi_s at any stage
without a safety violation (the hard terminal rows force such stages), so the unscaled measure calls every multiplier below
90 degenerate.
* ICE-map weights: the bound of xi_h and the headway row share 100 w_h + 2 w_h xi_h = 10 + 0.2 xi_h per stage; one of the two
  is positive at every stage and below 90 unless xi_h > 400 m, which the terminal rows exclude.  Every state is flagged.
* ORIG at N >= 20: a soft row's multiplier runs from 0 to its cap (v_inc and the bound of xi_v share w_v = 800, hwp and the
  bound of xi_h share 1000 + 20 xi_h) over the stages where the row passes from slack to tight; a value below 90, or within 90
  of the cap, is 5 to 10 % of the range and far from zero, but it is flagged.  With >= 20 stages most cases have such a
  passage (the smallest multiplier of the flagged cases is a headway row's 1 ... 88 in 38 of them, printed by
  test_degenerate_cases_are_rare).  With MB20 the last stage is blocked and a_19 enters only its own cost: the blocked row
  carries |2 w_a a_19 + ...| = 60 |a_19|, below 90 unless the horizon ends braking or pulling harder than 1.5 m/s^2.
Cases the unscaled measure flags, of the cases of the table as it stands (asserted as a record): see ISSUE_MEASURE_UNMET.
Shrinking the ORIG tables to the unflagged states would leave 14, 7, 11, 4, 1 and 3 states (orig20, 32, 33, 63, 20_mb, 24_tvec)
and take out the pair of states that exposed the solver error fixed with these tests.  On the device every case the scaled
measure accepts is compared point by point and by its objective, which is stricter than the objective-only comparison the
issue prescribes for degenerate cases.
"""
import numpy as np
import pytest

import ab_cert_cases as T
import qp_cert as Q

EXEMPT = ("s",)
NO_EXCEPTION = ("a_max", "a_min", "j_max", "j_min", "safe1", "safe2", "hwp", "v_lim", "v_curv", "v_stop", "v_tl", "blocked")
# configuration -> cases flagged by the issue's unscaled degeneracy measure (see the docstring); the scaled one is asserted there
ISSUE_MEASURE_UNMET = {"orig20": 3, "orig32": 9, "orig33": 8, "orig63": 7, "orig20_mb": 14, "orig24_tvec": 10,
                       "abo20_ice": 24, "abo33_ice": 23, "abo20_ice_mb": 23}
JERK = ("j_max", "j_min")
FOLLOW = ("safe1", "safe2", "hwp")


@pytest.fixture(scope="module")
def table():
    """config -> list of per-case dicts (name, oracle result, certified optimum of the oracle's problem)"""
    from oracle import Oracle
    out = {}
    for cfg, (tree, N, _) in T.CONFIGS.items():
        OPT, V = T.settings(cfg)
        orc = Oracle(OPT, V)
        stage, typ = T.config_row_map(cfg)
        names, cols = T.cases(cfg)
        rows = []
        for i, nm in enumerate(names):
            r = orc.ab_step(**{n: float(cols[n][i]) for n in T.INS}, want_dense=True)
            assert r["G"].shape[0] == stage.size
            R = dict(name=nm, status=r["status"], x_oracle=r["x"].copy(), r=r)
            if r["status"] == 0:
                R["cert_oracle"] = Q.certificate(r["H"], r["c"], r["G"], r["lb"], r["ub"], None, None, r["x"])
                R.update(T.certify(r["H"], r["c"], r["G"], r["lb"], r["ub"], r["x"], stage, typ, N, OPT))
            rows.append(R)
        out[cfg] = rows
    return out


def _covered(rows):
    return {t for R in rows for _, _, t, _ in R["rows"]}


def test_table_shape():
    assert len(T.CONFIGS) == 19
    for cfg, (tree, N, over) in T.CONFIGS.items():
        names, cols = T.cases(cfg)
        assert 0 < len(names) <= 32 and len(set(names)) == len(names)
        OPT, _ = T.settings(cfg)
        assert OPT["paramEstSetting"] in (0, 1) and OPT["TVestSetting"] in (0, 1)
        assert set(T.LEFT_OUT.get(cfg, ())) <= {r[0] for r in T.STATES}
    assert {N for _, N, _ in T.CONFIGS.values()} == {2, 3, 20, 24, 32, 33, 63}


def test_every_case_is_solved_and_certified(table):
    for cfg, rows in table.items():
        for R in rows:
            assert R["status"] == 0, (cfg, R["name"])
            c = R["cert_oracle"]
            assert c["pviol"] <= T.PVIOL_MAX and c["stat"] <= T.STAT_MAX, (cfg, R["name"], c["pviol"], c["stat"])


def test_coverage_of_row_types(table):
    print()
    cfgs = list(table)
    print("%-8s" % "type" + "".join(" %5s" % c.replace("orig", "o").replace("abo", "a")[:5] for c in cfgs))
    for t in T.AB_ROW_TYPES:
        print("%-8s" % t + "".join(" %5s" % (sum(any(x[2] == t for x in R["rows"]) for R in table[c]) if t in T.catalogue(c) else "-")
                                   for c in cfgs))
    assert len(EXEMPT) <= 2 and not set(EXEMPT) & set(NO_EXCEPTION)
    for tree in ("ABO", "ORIG"):
        mine = [c for c in cfgs if T.CONFIGS[c][0] == tree]
        want = {t for c in mine for t in T.catalogue(c)} - set(EXEMPT)
        got = set().union(*[_covered(table[c]) for c in mine])
        assert want <= got, (tree, sorted(want - got))
        assert "blocked" in want and set(NO_EXCEPTION) - set(T.ROUTE_TYPES if tree == "ABO" else ()) <= want
    # at the edge horizons the issue's three; the table reaches them, and the deceleration limit, in every configuration
    for c in cfgs:
        got = _covered(table[c])
        assert got & {"a_min", "a_max"} and got & set(JERK) and got & set(FOLLOW), (c, sorted(got))
        assert "a_min" in got, c


def test_hard_braking_cases_carry_the_coverage(table):
    """Without the hard-braking cases the coverage assertion above fails: no other case reaches the deceleration limit in
    the ABO tree at N >= 20."""
    rest = {c: _covered([R for R in rows if not R["name"].startswith("brake")]) for c, rows in table.items()}
    assert any("a_min" not in got for got in rest.values())
    assert "a_min" not in rest["abo20"] and "a_min" not in rest["abo33"]


def test_stage_edges(table):
    for tree in ("ABO", "ORIG"):
        first = last = terminal = False
        for c, rows in table.items():
            N = T.CONFIGS[c][1]
            if T.CONFIGS[c][0] != tree:
                continue
            for R in rows:
                ks = {k for _, k, _, _ in R["rigid"]}
                first |= 0 in ks; last |= N - 1 in ks; terminal |= N in ks
        assert first and last and terminal, (tree, first, last, terminal)


def test_large_rigid_working_sets(table):
    """N = 32, 33, 63: a case with N / 2 or more rigid rows carrying a multiplier.  Largest at N = 63 (measured): 86 rigid
    rows (ORIG), 76 (ABO); the solver's capacity of 64 rows counts what it holds after the exact slack elimination."""
    print()
    for c, rows in table.items():
        N = T.CONFIGS[c][1]
        if N not in (32, 33, 63):
            continue
        best = max(rows, key=lambda R: len(R["rigid"]))
        held = max(rows, key=lambda R: len(R["held"]))
        print("%-12s N %2d: most rigid rows %3d (%s), most held rows %3d (%s)" % (c, N, len(best["rigid"]), best["name"],
                                                                                    len(held["held"]), held["name"]))
        assert len(best["rigid"]) >= N / 2, c


def test_degenerate_cases_are_rare(table):
    """At most one case in eight per configuration: by the issue's unscaled measure where the weights allow it, by the scaled
    one in ISSUE_MEASURE_UNMET, where the number of cases the unscaled measure flags is pinned as a record."""
    print()
    for c, rows in table.items():
        scaled = [R["name"] for R in rows if R["degenerate"]]
        plain = [R for R in rows if R["singular"] or R["plain_ratio"] < T.DEGENERATE_RATIO]
        print("%-12s %2d cases, degenerate: scaled measure %d %s, issue's measure %d; smallest ratio scaled %.1e plain %.1e" % (
            c, len(rows), len(scaled), scaled, len(plain), min(R["ratio"] for R in rows), min(R["plain_ratio"] for R in rows)))
        for R in plain:
            l, t, k = min((l, t, k) for _, k, t, l in R["rows"])
            print("      %-18s smallest multiplier %.3g (%s, stage %d)" % (R["name"], l, t, k))
        assert not any(R["singular"] for R in rows), c
        assert 8 * len(scaled) <= len(rows), (c, scaled)
        if c in ISSUE_MEASURE_UNMET:
            assert len(plain) == ISSUE_MEASURE_UNMET[c], (c, len(plain))
        else:
            assert 8 * len(plain) <= len(rows), (c, [R["name"] for R in plain])


def test_oracle_distance_to_the_certified_optimum(table):
    """The yardstick of the device's bars: the CPU oracle's distance to x* on its own problem, per configuration.  No case
    comes near one eighth of a bar, so tests/test_gpu_ab_cert.py widens none."""
    print()
    for c, rows in table.items():
        tree, N, _ = T.CONFIGS[c]
        OPT, _ = T.settings(c)
        names, cols = T.cases(c)
        Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
        xs = np.stack([R["x"] for R in rows]); xo = np.stack([R["x_oracle"] for R in rows])
        d_a = np.abs(xs[:, 0::5] - xo[:, 0::5]).max()
        d_xi = max(np.abs(xs[:, j::5] - xo[:, j::5]).max() for j in (1, 2, 3, 4))
        ss, vs = T.rollout(xs[:, 0::5], cols["s"], cols["v"], Tv)
        so = np.stack([R["r"]["s_pred"] for R in rows], axis=1); vo = np.stack([R["r"]["v_pred"] for R in rows], axis=1)
        d_s, d_v = np.abs(ss - so).max(), np.abs(vs - vo).max()
        d_f = max(abs(T.objective(R["r"]["H"], R["r"]["c"], R["x_oracle"]) - R["f"]) / (1 + abs(R["f"])) for R in rows)
        print("%-12s oracle to x*: a %.1e slacks %.1e s_pred %.1e v_pred %.1e cost %.1e" % (c, d_a, d_xi, d_s, d_v, d_f))
        assert d_a <= T.BAR["a"] / 8 and d_xi <= T.BAR["slack"] / 8 and d_v <= T.BAR["v"] / 8 and d_s <= T.BAR["s"] / 8, c
        assert d_f <= T.COST_BAR[tree] / 8, c
