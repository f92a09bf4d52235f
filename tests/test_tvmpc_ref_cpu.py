"""Target-vehicle MPC (RunOpt_TVMPC / CreateQP_TV) on the CPU: the numpy restatement tests/tvmpc_ref.py that the GPU tests
compare against.  The reference holds no saved TVMPC solution, so parity pinned by restatement only; here the restatement
itself is checked: its structure against CreateQP_TV.m and against the oracle's CreateQP_BL, and its LP solutions against an
independent solver (HiGHS through scipy.optimize.linprog, as tests/test_bl_lp_independent.py does for the baseline LP)."""
import numpy as np
import pytest
from scipy.optimize import linprog

import tvmpc_ref as tvr
from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV, default_opt


def _case(uc, tree="ABO", **over):
    o = default_opt(); o["useCaseNum"] = uc
    OPT = Settings(o, tree=tree, N_hor=20)
    OPT.update(over)
    return OPT, SetVehicleParameters(tree)


# (use case, s, v, a_prev, t0): start of use case 1; 60 m before the stop of use case 2; use case 5's first traffic light
# (at 250 m, red while mod(t - 9, 29) < 17) from 50 m at t = 10 s; inside the first curve of use case 6 (100 .. 130 m)
LP_STEPS = [(1, 10.0, 0.0, 0.0, 0.0), (2, 240.0, 12.0, -0.5, 12.0), (5, 200.0, 14.0, 0.0, 10.0), (6, 95.0, 9.0, 0.2, 14.0)]


def _highs(r):
    G, lb, ub = r["G"], r["lb"], r["ub"]
    fu, fl = np.isfinite(ub), np.isfinite(lb)
    A = np.vstack([G[fu], -G[fl]]); b = np.concatenate([ub[fu], -lb[fl]])
    res = linprog(r["c"], A_ub=A, b_ub=b, bounds=[(None, None)] * r["c"].size, method="highs")
    assert res.status == 0, res.message
    return res


@pytest.mark.parametrize("uc,s,v,a_prev,t0", LP_STEPS)
def test_restated_lp_equals_highs(uc, s, v, a_prev, t0):
    OPT, V = _case(uc)
    ref = tvr.TVRef(OPT, V)
    r = ref.step(s, v, a_prev, t0)
    assert r["status"] == 0 and not r["H"].any()                  # W_TV of the reference: a linear program
    res = _highs(r)
    # 1e-8 relative: the curvature 1e-4 puts the least-norm point 4e-9 above the optimum on a face (measured for the baseline LP)
    assert abs(r["c"] @ r["x"] - res.fun) <= 1e-8 * max(1.0, abs(res.fun)), (r["c"] @ r["x"], res.fun)
    assert abs(r["out"][tvr.OUT["cost"]] - res.fun) <= 1e-8 * max(1.0, abs(res.fun))
    y = r["G"] @ r["x"]
    assert np.maximum(np.maximum(y - r["ub"], r["lb"] - y), 0.0).max() < 1e-8


def test_row_count_and_cap_factors():
    OPT, V = _case(6)
    N = OPT["TV_N_hor"]
    s_est = np.linspace(90.0, 200.0, N + 1)
    H, c, G, lb, ub = tvr.create_qp_tv(OPT, V, s_est, 3.0, 0.1)
    assert G.shape == (11 * N, 4 * N + 2) and G.any(axis=1).all()                # RunOpt_TVMPC.m:185-190: 11 rows per stage
    v_lim, v_stop, v_TL, v_curv, *_ = tvr.route_and_comfort_bounds(OPT, s_est, np.zeros(N), 3.0, N)
    assert v_curv.min() < 0.5 * v_lim.max()                                      # the curve is inside the horizon
    for kk in range(N):
        np.testing.assert_array_equal(ub[11 * kk + 7:11 * kk + 11], [0.8 * v_lim[kk], 0.8 * v_curv[kk], v_stop[kk], v_TL[kk]])
    assert c[4 * N + 1] == -OPT["W_TV"][0] and (c[1::4] == -OPT["W_TV"][0]).all()     # CreateQP_TV.m:130,291-292


def test_limits_do_not_depend_on_the_measured_speed():
    OPT, V = _case(1)
    ref = tvr.TVRef(OPT, V)
    N = ref.N
    for v in (0.0, 7.0, 18.0, 30.0):
        *_, lb, ub, _, _, _ = ref.dense_qp(50.0, v, 0.0, 0.0)
        for kk in range(N):        # rows 3..6 of a stage: a_min, a_max, jerk (dense rows of a_k, a_{k-1}, xi: no state part)
            assert lb[11 * kk + 3] == -OPT["TV_a_LimLowVel"] and ub[11 * kk + 4] == OPT["TV_a_LimLowVel"]
            assert lb[11 * kk + 5] == -0.5 * OPT["TV_j_LimLowVel"] and ub[11 * kk + 6] == 0.5 * OPT["TV_j_LimLowVel"]


@pytest.mark.parametrize("uc", [2, 5, 6])
def test_equals_create_qp_bl_without_headway_rows(uc):
    """With the baseline limits set to the target-vehicle limits (speed independent: low = high) and the 0.8 factors undone,
    CreateQP_TV is CreateQP_BL (the oracle's orc_create_qp_bl through TransformToDense) without its headway rows."""
    from oracle import Oracle
    OPT, V = _case(uc, TV_a_LimHighVel=1.0, TV_j_LimHighVel=2.0)
    OPT.update(BL_a_LimLowVel=1.0, BL_a_LimHighVel=1.0, BL_j_LimLowVel=2.0, BL_j_LimHighVel=2.0)
    N = 20
    s, v, a_prev, t0 = 180.0, 11.0, 0.3, 10.0
    r = Oracle(Settings_BL(OPT), V).ab_step(s, v, a_prev, t0, 1e6, 0.0, 0.0, want_dense=True)
    keep = np.array([i for i in range(13 * N) if i % 13 < 11])
    s_est, _ = tvr.estimate_trajectory(OPT, s, v, a_prev, np.zeros(N + 1), np.zeros(N + 1))
    H, c, G, lb, ub = tvr.create_qp_tv(OPT, V, s_est, t0, a_prev, cap_scale=1.0)
    Hd, cd, Gd, lbd, ubd, _, _ = tvr.transform_to_dense(N, 0.5, H, c, G, lb, ub, s, v)
    np.testing.assert_allclose(Gd, r["G"][keep], rtol=0, atol=1e-12)
    np.testing.assert_allclose(cd, r["c"], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(Hd, r["H"], rtol=0, atol=1e-12)
    for mine, theirs in ((lbd, r["lb"][keep]), (ubd, r["ub"][keep])):
        fin = np.isfinite(mine)
        assert (fin == (np.abs(theirs) < 1e19)).all()
        np.testing.assert_allclose(mine[fin], theirs[fin], rtol=1e-12, atol=1e-9)


def test_settings_tv_view():
    OPT, V = _case(1)
    for tree in ("ABO", "ORIG"):
        o = Settings(tree=tree)
        assert list(o["W_TV"]) == [1e2, 0.0, 0.0, 1e7] and o["TV_N_hor"] == 20 and o["TV_Ts"] == 0.5 and o["TV_trajEstSett"] == 1
        assert (o["TV_a_LimLowVel"], o["TV_a_LimHighVel"], o["TV_j_LimLowVel"], o["TV_j_LimHighVel"]) == (1.0, 0.5, 2.0, 0.5)
    T = Settings_TV(OPT)
    assert T["bl_mode"] == 2 and T["N_hor"] == 20 and T["BL_a_LimLowVel"] == 1.0 and T["BL_j_LimLowVel"] == 2.0
    bad = dict(OPT); bad["TV_Ts"] = 0.25
    with pytest.raises(ValueError, match="TV_Ts"):
        Settings_TV(bad)
