"""Target-vehicle MPC (RunOpt_TVMPC / CreateQP_TV) on MI355X through the C-ABI (a handle created with bl_mode = 2) against
the CPU restatement tests/tvmpc_ref.py.  The reference holds no saved TVMPC solution: parity pinned by restatement only
(the restatement itself is checked against CreateQP_BL and HiGHS in tests/test_tvmpc_ref_cpu.py).

Tolerances are those of tests/test_gpu_bl.py against the oracle: forces 1e-2 N, a 5e-6, xi_f 1e-6, predictions 1e-3 m /
1e-4 m/s with a unique optimum (strictly convex weights W_TV = [1e2, 1, 1, 1e7]); with the reference's LP weights the
point where the optimum is unique and the objective value where it is not (at most 10 % of the compared steps), and the
closed-loop band 25 m / 5 m/s of test_gpu_bl.py:241."""
import numpy as np
import pytest

import tvmpc_ref as tvr
from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV, default_opt

pytestmark = pytest.mark.gpu

W_CONVEX = np.array([1e2, 1.0, 1.0, 1e7])
N_LOOP = 80


def _case(uc, tree="ABO", N=20, convex=False):
    o = default_opt(); o["useCaseNum"] = uc
    OPT = Settings(o, tree=tree, N_hor=max(N, 20))
    OPT["TV_N_hor"] = N
    if convex:
        OPT["W_TV"] = W_CONVEX.copy()
    return OPT, SetVehicleParameters(tree)


def _engine(OPT, V, max_batch=64):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


_loops = {}


def ref_loop(uc, tree="ABO", N=20, convex=False, n_steps=N_LOOP):
    """Restated closed loop (computed once per configuration, shared, never modified)."""
    key = (uc, tree, N, convex, n_steps)
    if key not in _loops:
        OPT, V = _case(uc, tree, N, convex)
        ref = tvr.TVRef(OPT, V)
        v0 = OPT["v_init"]                   # a moving start reaches the route features within the 80 steps
        traj, st, aprev = ref.run(n_steps, v0=v0)
        for a in (traj, st, aprev):
            a.setflags(write=False)
        _loops[key] = (OPT, V, ref, traj, st, aprev)
    return _loops[key]


def test_tv_handle_and_wrong_handle_refusals():
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    OPT, V = _case(1)
    tv = _engine(Settings_TV(OPT), V, 2)               # fails on a library that knows bl_mode 0 and 1 only
    assert tv.h
    z, stv = np.zeros(1), np.full((4, 1), 1e3)
    for call in (lambda: tv.run_abmpc(z, z, z, stv, stv), lambda: tv.run_blmpc(z, z, z, stv, stv), lambda: tv.run_fbmpc(z, z, z, stv, stv),
                 lambda: tv.ab_step(z, z, z, z, z, z, z), lambda: tv.run_abmpc_host(z, z, z, stv, stv)):
        with pytest.raises(EepaccError, match="bl_mode"):
            call()
    for other in (_engine(OPT, V, 2), _engine(Settings_BL(OPT), V, 2)):
        with pytest.raises(EepaccError, match="bl_mode = 2"):
            other.run_tvmpc(z, z, z, 4)
        with pytest.raises(EepaccError, match="bl_mode = 2"):
            other.tv_step(z, z, z, z)
    bad = Settings_TV(OPT); bad["solverToUse"] = 2
    with pytest.raises(EepaccError, match="solverToUse"):
        _engine(bad, V, 2)


def _steps_of(traj, aprev, Ts, every):
    ks = np.arange(0, traj.shape[0], every)
    return ks, traj[ks, OUT["s"]].copy(), traj[ks, OUT["v"]].copy(), aprev[ks].copy(), Ts * ks


@pytest.mark.parametrize("uc", [1, 2, 3, 4, 5, 6, 7])
def test_tv_step_convex_vs_restatement(uc):
    """Cold, independent steps sampled along the restated closed loop; strictly convex weights: a unique optimum."""
    OPT, V, ref, traj, st, aprev = ref_loop(uc, convex=True)
    ks, s, v, ap, t0 = _steps_of(traj, aprev, 0.5, 4)
    eng = _engine(Settings_TV(OPT), V)
    out, sp, vp, status = eng.tv_step(s, v, ap, t0)
    o = out.cpu().numpy(); stat = status.cpu().numpy(); sp = sp.cpu().numpy(); vp = vp.cpu().numpy()
    assert ks.size == 20
    for i, k in enumerate(ks):
        r = ref.step(s[i], v[i], ap[i], t0[i])
        assert (r["status"] != 0) == (stat[i] != 0), (uc, k)
        if r["status"] != 0:
            continue
        d = {n: abs(o[OUT[n], i] - r["out"][OUT[n]]) for n in ("Fm", "Fb", "a", "xi_f", "cost", "DistHor")}
        print(uc, k, d)
        assert d["Fm"] < 1e-2 and d["Fb"] < 1e-2, (uc, k, d)
        assert d["a"] < 5e-6 and d["xi_f"] < 1e-6 and d["DistHor"] < 1e-9, (uc, k, d)
        assert d["cost"] < 1e-6 * max(1.0, abs(r["out"][OUT["cost"]])) + 10.0, (uc, k, d)
        assert np.abs(sp[:, i] - r["s_pred"]).max() < 1e-3 and np.abs(vp[:, i] - r["v_pred"]).max() < 1e-4, (uc, k)
        assert o[OUT["xi_v"], i] == 0.0 and o[OUT["xi_h"], i] == 0.0 and o[OUT["xi_s"], i] == 0.0


@pytest.mark.parametrize("N", [3, 40])
def test_tv_step_other_horizons(N):
    """N = 3 (smallest sensible horizon) and N = 40 (the N <= 63 kernel) on the stop approach of use case 2."""
    OPT, V, ref, traj, st, aprev = ref_loop(2, N=N, convex=True, n_steps=48)
    ks, s, v, ap, t0 = _steps_of(traj, aprev, 0.5, 4)
    eng = _engine(Settings_TV(OPT), V)
    out, sp, vp, status = eng.tv_step(s, v, ap, t0)
    o = out.cpu().numpy(); stat = status.cpu().numpy()
    for i, k in enumerate(ks):
        r = ref.step(s[i], v[i], ap[i], t0[i])
        assert (r["status"] != 0) == (stat[i] != 0), (N, k)
        if r["status"] == 0:
            assert abs(o[OUT["Fm"], i] - r["out"][OUT["Fm"]]) < 1e-2 and abs(o[OUT["Fb"], i] - r["out"][OUT["Fb"]]) < 1e-2, (N, k)
            assert abs(o[OUT["a"], i] - r["out"][OUT["a"]]) < 5e-6 and abs(o[OUT["xi_f"], i] - r["out"][OUT["xi_f"]]) < 1e-6, (N, k)


def test_tv_step_lp_vs_restatement():
    """The reference's LP weights: the point where the optimum is unique, the objective value where it is not (BL's rule,
    test_gpu_bl.py:222-240)."""
    n_cmp = n_face = 0
    for uc in (1, 2, 3, 4, 5, 6, 7):
        OPT, V, ref, traj, st, aprev = ref_loop(uc)
        ks, s, v, ap, t0 = _steps_of(traj, aprev, 0.5, 4)
        eng = _engine(Settings_TV(OPT), V)
        out, _, _, status = eng.tv_step(s, v, ap, t0, want_pred=False)
        o = out.cpu().numpy(); stat = status.cpu().numpy()
        for i, k in enumerate(ks):
            r = ref.step(s[i], v[i], ap[i], t0[i])
            assert (r["status"] != 0) == (stat[i] != 0), (uc, k)
            if r["status"] != 0:
                continue
            co, ck = r["out"][OUT["cost"]], o[OUT["cost"], i]
            print(uc, k, "cost", ck - co, "a_qp", o[OUT["a_qp"], i] - r["out"][OUT["a_qp"]])
            n_cmp += 1
            if abs(o[OUT["a_qp"], i] - r["out"][OUT["a_qp"]]) > 1e-4:
                # a face of optima: two optimal points, one objective value (test_gpu_bl.py:237)
                n_face += 1
                assert abs(ck - co) < 1e-7 * max(1.0, abs(co)) + 1e-5, (uc, k, ck, co)
            else:
                # a unique optimum: the point, with the bands of test_gpu_bl.py:92-96,214 (the cost carries w_f = 1e7 times
                # the slack's 1e-6; measured on use case 3, step 32: xi_f = 6.8e-3, the two costs 0.24 apart at 6.8e4)
                assert abs(o[OUT["Fm"], i] - r["out"][OUT["Fm"]]) < 1e-1 and abs(o[OUT["Fb"], i] - r["out"][OUT["Fb"]]) < 1e-1, (uc, k)
                assert abs(o[OUT["a"], i] - r["out"][OUT["a"]]) < 3e-5 and abs(o[OUT["xi_f"], i] - r["out"][OUT["xi_f"]]) < 1e-6, (uc, k)
                assert abs(ck - co) < 1e-6 * max(1.0, abs(co)) + 10.0, (uc, k, ck, co)
    assert n_cmp >= 130, n_cmp                       # 7 use cases x 20 steps, minus steps the restatement calls infeasible
    assert n_face <= 0.1 * n_cmp, (n_face, n_cmp)


def _physical(OPT, tr, st):
    v, s, xi = tr[:, OUT["v"]], tr[:, OUT["s"]], tr[:, OUT["xi_f"]]
    assert v.min() >= -1e-5                                      # state_bound_tol of a baseline-type handle
    N = OPT["TV_N_hor"]
    n_checked = 0
    for k in range(tr.shape[0]):
        if xi[k] == 0.0 and st[k] == 0:
            v_lim, _, _, v_curv, *_ = tvr.route_and_comfort_bounds(OPT, np.full(N + 1, s[k]), np.zeros(N), 0.0, 1)
            assert v[k] <= 0.8 * min(v_lim[0], v_curv[0]) + 1e-6, k
            n_checked += 1
    assert n_checked >= tr.shape[0] // 4, n_checked              # the slack is off its bound on a minority of the steps only


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
@pytest.mark.parametrize("uc", [1, 2, 5])
def test_tv_closed_loop_vs_restatement(uc, tree):
    B = 5
    for convex in (True, False):
        OPT, V, ref, traj, rst, _ = ref_loop(uc, tree=tree, convex=convex)
        eng = _engine(Settings_TV(OPT), V)
        s0 = np.full(B, OPT["TVinitDist"]); v0 = np.full(B, OPT["v_init"]); a0 = np.zeros(B)
        t1, s1 = eng.run_tvmpc(s0, v0, a0, N_LOOP)
        tr = t1.cpu().numpy(); st = s1.cpu().numpy()
        t2, s2 = eng.run_tvmpc(s0, v0, a0, N_LOOP)
        assert np.array_equal(t2.cpu().numpy(), tr) and np.array_equal(s2.cpu().numpy(), st)      # deterministic
        assert np.abs(tr - tr[:, :, :1]).max() == 0.0
        if convex:
            assert np.array_equal(st[:, 0] != 0, rst != 0)
        else:
            # the LP loops may part on a face of optima, so the status is not compared step by step: both solve every step
            assert int((st != 0).sum()) == 0 and int((rst != 0).sum()) == 0, (uc, tree, np.flatnonzero(st[:, 0]), np.flatnonzero(rst))
        d = {n: np.abs(tr[:, OUT[n], 0] - traj[:, OUT[n]]).max() for n in ("s", "v", "a", "Fm", "Fb", "xi_f")}
        print(uc, tree, convex, d)
        if convex:
            for n, tol in (("s", 1e-5), ("v", 1e-5), ("a", 2e-5), ("Fm", 5e-2), ("Fb", 5e-2), ("xi_f", 1e-5)):
                assert d[n] < tol, (uc, tree, n, d[n])
        else:
            assert d["s"] < 25.0 and d["v"] < 5.0, (uc, tree, d)
        _physical(OPT, tr[:, :, 0], st[:, 0])
        assert np.all(tr[:, OUT["xi_v"]] == 0) and np.all(tr[:, OUT["xi_h"]] == 0) and np.all(tr[:, OUT["xi_s"]] == 0)


def test_tv_full_stop_and_batch_permutation():
    """Use case 2 (stop at 300 m) from different starts: a full stop is reached at the stop location; results do not depend
    on the position of an instance in the batch."""
    OPT, V = _case(2)
    eng = _engine(Settings_TV(OPT), V)
    B = 7
    s0 = 10.0 + 20.0 * np.arange(B); v0 = np.linspace(5.0, 17.0, B); a0 = np.zeros(B)
    t1, s1 = eng.run_tvmpc(s0, v0, a0, 80)
    tr = t1.cpu().numpy()
    p = np.array([3, 0, 6, 1, 5, 2, 4])
    t2, s2 = eng.run_tvmpc(s0[p], v0[p], a0[p], 80)
    assert np.array_equal(t2.cpu().numpy(), tr[:, :, p]) and np.array_equal(s2.cpu().numpy(), s1.cpu().numpy()[:, p])
    assert int((s1.cpu().numpy() != 0).sum()) == 0
    # the stop cap is stopVel = 0.2 m/s at the stop location and rises with the distance from it (1 m/s per m)
    # (a target vehicle creeps through the stop at that speed and leaves again: CreateQP_TV has no dwell time)
    for b in range(B):
        k = int(np.argmin(np.abs(tr[:, OUT["s"], b] - 300.0)))
        dist = abs(tr[k, OUT["s"], b] - 300.0)
        # the stage-0 row is v_0 - xi_f <= stopVel + dist (CreateQP_TV.m:275-278): the slack of the step is part of the bound
        assert dist < 0.5 and tr[k, OUT["v"], b] <= 0.2 + dist + tr[k, OUT["xi_f"], b] + 1e-6 and tr[k, OUT["v"], b] < 0.5, \
            (b, k, dist, tr[k, OUT["v"], b], tr[k, OUT["xi_f"], b])


@pytest.mark.parametrize("N", [20, 40])
def test_tv_chunked_launch(N):
    OPT, V = _case(5, N=N)
    eng = _engine(Settings_TV(OPT), V)
    B = 6
    s0 = np.linspace(10.0, 200.0, B); v0 = np.full(B, 15.0); a0 = np.zeros(B)
    t, s = eng.run_tvmpc(s0, v0, a0, 40)
    ta, sa = eng.run_tvmpc(s0, v0, a0, 20)
    tb, sb = eng.run_tvmpc(s0, v0, a0, 20, resume=True)
    assert np.array_equal(np.concatenate([ta.cpu().numpy(), tb.cpu().numpy()], 0), t.cpu().numpy())
    assert np.array_equal(np.concatenate([sa.cpu().numpy(), sb.cpu().numpy()], 0), s.cpu().numpy())


def test_tv_device_chaining_and_refusal():
    """Main.m:82-89 on the device: ABMPC fed the device-resident TVMPC trace equals ABMPC fed the same trace through the host."""
    from eepacc_mpc_casadi_matlab_amd.engine import generate_lead_and_run
    OPT, V = _case(2)
    OPT["t_sim"] = 20.0
    B = 4
    tv = _engine(Settings_TV(OPT), V, B); ego = _engine(OPT, V, B)
    tv0 = (np.full(B, 10.0) + 5.0 * np.arange(B), np.zeros(B), np.zeros(B))
    traj, status, s_tv, v_tv = generate_lead_and_run(OPT, V, kind="ab", batch=B, tv_init=tv0, engines=(tv, ego))
    assert s_tv.is_cuda and s_tv.shape == (41, B)
    lead, _ = tv.run_tvmpc(*tv0, 41)
    lead = lead.cpu().numpy()
    assert np.array_equal(s_tv.cpu().numpy(), lead[:, OUT["s"]] - OPT["TVlength"]) and np.array_equal(v_tv.cpu().numpy(), lead[:, OUT["v"]])
    t2, s2 = ego.run_abmpc(np.zeros(B), np.full(B, OPT["v_init"]), np.zeros(B), s_tv.cpu().numpy(), v_tv.cpu().numpy())
    assert np.array_equal(t2.cpu().numpy(), traj.cpu().numpy()) and np.array_equal(s2.cpu().numpy(), status.cpu().numpy())
    bad = dict(OPT); bad["TV_Ts"] = 0.25
    with pytest.raises(ValueError, match="TV_Ts"):
        generate_lead_and_run(bad, V, kind="ab", batch=B)


def test_runopt_tvmpc_mirror():
    from eepacc_mpc_casadi_matlab_amd.engine import RunOpt_TVMPC
    OPT, V = _case(1)
    s_opt, v_opt, n_err = RunOpt_TVMPC(OPT, V)
    assert s_opt.shape == v_opt.shape == (61,) and n_err == 0              # t_sim/TV_Ts + 1 steps of use case 1
    assert s_opt[0] == OPT["TVinitDist"] and v_opt[0] == OPT["TVinitVel"]
    assert v_opt.max() <= 0.8 * 80 / 3.6 + 1e-6 and v_opt[-1] > 15.0       # settles at 0.8 of the 80 km/h limit
