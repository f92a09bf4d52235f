"""ICE-map fuel term (CreateQP_AB.m:154-159, OPT["fuel_map"] = "ICE") at long horizons and with move blocking.

The kernel variant `ice` builds the step's condensed Hessian in LDS and inverts it there: on the packed triangle for
N > 32 and folded into the leader-indexed layout E'HE when Mb != 0.  Everything is compared against the oracle, which
states CreateQP_AB.m literally (ICE term and the Mb equality rows included).  Tolerances are those of
test_golden_icemap_step_varying_hessian: forces to 1e-5 N, ten times the per-step figures on closed loops.
"""
import numpy as np
import pytest

from conftest import make_case, load_golden, GOLDEN_AB_ICEMAP
from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1, make_s2

pytestmark = pytest.mark.gpu

TOL = dict(s=1e-8, v=1e-9, Fm=1e-5, Fb=1e-5, a=1e-9, xi_v=1e-9, xi_h=1e-9, xi_s=1e-9, xi_f=1e-9,
           DistHor=1e-8, a_qp=1e-9)
CLOSED = ("s", "v", "Fm", "Fb", "a", "xi_v", "xi_h", "xi_s", "xi_f")
MB_TEST = [0, 0, 0, 0, 0, 1, 0, 1, 0, 1, 0, 1, 0, 1, 1, 0, 1, 1, 0, 1]      # test_move_blocking's mask, N = 20


def reference_long_mask():
    """ABO/Settings.m:100 (the commented alternative) expanded as Settings.m:243-250: N = 50, 25 blocked stages."""
    mb = []
    for n in [1] * 10 + [2] * 10 + [4] * 5:
        mb += [0] + [1] * (n - 1)
    return np.array(mb, dtype=np.int32)


def _ice_case(N, Mb=None):
    OPT, V, s_tv, v_tv = make_case("ABO", N)
    OPT = dict(OPT)
    OPT["W_AB"] = np.array(GOLDEN_AB_ICEMAP["W_AB"])
    OPT["fuel_map"] = "ICE"
    if Mb is not None:
        OPT["Mb"] = np.asarray(Mb, dtype=np.int32)
    return OPT, V, s_tv, v_tv


def _engine(OPT, V, max_batch):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _closed_loop_vs_oracle(OPT, V, sc, tr, st, idx, gears=None):
    from oracle import Oracle
    orc = Oracle(OPT, V)
    n_steps = tr.shape[0]
    for i in idx:
        ref, rst, _ = orc.run("ab", n_steps, 0.0, float(sc["v0"][i]), 0.0, sc["s_tv"][:, i].copy(), sc["v_tv"][:, i].copy())
        assert rst.sum() == 0 and st[:, i].sum() == 0, i
        for n in CLOSED:
            err = np.abs(tr[:, OUT[n], i] - ref[:, OUT[n]]).max()
            assert err < 10 * TOL[n], (i, n, err)
        if gears is not None:
            gears |= {orc.lib_lut(v) for v in ref[:, OUT["v"]]}
    return orc


@pytest.mark.parametrize("N", [33, 60, 63])
def test_open_loop_s1_long_horizon(N, torch_mod):
    """S1 batch, one cold step each: N = 33 and 63 are the edges of the large (packed) configuration."""
    from oracle import Oracle
    OPT, V, s_tv, v_tv = _ice_case(N)
    B = 24
    s1 = make_s1(B, load_golden("abo_abmpc_icemap"), s_tv, v_tv)
    args = {k: s1[k] for k in ("s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev")}
    out, sp, vp, status = _engine(OPT, V, B).ab_step(**args)
    o = out.cpu().numpy(); sp = sp.cpu().numpy(); vp = vp.cpu().numpy(); st = status.cpu().numpy()
    orc = Oracle(OPT, V)
    for i in range(B):
        r = orc.ab_step(**{k: float(v[i]) for k, v in args.items()})
        assert r["status"] == st[i] == 0, i
        for n, t in TOL.items():
            assert abs(o[OUT[n], i] - r["out"][OUT[n]]) < t, (N, i, n)
        assert abs(o[OUT["cost"], i] - r["out"][OUT["cost"]]) < 1e-8 * (1 + abs(r["out"][OUT["cost"]])), (N, i)
        assert np.abs(sp[:, i] - r["s_pred"]).max() < 1e-8, (N, i)
        assert np.abs(vp[:, i] - r["v_pred"]).max() < 1e-9, (N, i)


def test_closed_loop_s2_n60(torch_mod, lead_trace):
    """Config 4's horizon: S2 closed loops against the oracle; the gears along the trajectories vary, so does H."""
    OPT, V, _, _ = _ice_case(60)
    B, n_steps = 4, 60
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"])
    traj, status = _engine(OPT, V, 8).run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    gears = set()
    _closed_loop_vs_oracle(OPT, V, sc, traj.cpu().numpy(), status.cpu().numpy(), range(B), gears)
    assert len(gears) >= 3, gears


def test_move_blocking_n20(torch_mod, lead_trace):
    """ICE + Mb (small configuration): closed loop against the oracle's equality rows, blocked predicted accelerations."""
    OPT, V, _, _ = _ice_case(20, MB_TEST)
    B, n_steps = 3, 80
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"], seed=2)
    eng = _engine(OPT, V, 4)
    traj, status = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    tr = traj.cpu().numpy()
    orc = _closed_loop_vs_oracle(OPT, V, sc, tr, status.cpu().numpy(), range(B))
    a_prev = float((tr[40, OUT["v"], 0] - tr[39, OUT["v"], 0]) / 0.5)
    a_tv = float((sc["v_tv"][40, 0] - sc["v_tv"][39, 0]) / 0.5)
    inp = (float(tr[40, OUT["s"], 0]), float(tr[40, OUT["v"], 0]), a_prev, 20.0, float(sc["s_tv"][40, 0]),
           float(sc["v_tv"][40, 0]), a_tv)
    r = orc.ab_step(*inp)
    _, _, vp, st1 = eng.ab_step(*[[x] for x in inp])
    assert int(st1.cpu().numpy()[0]) == 0
    vp = vp.cpu().numpy()[:, 0]
    assert np.abs(vp - r["v_pred"]).max() < 1e-7
    acc = np.diff(vp) / 0.5
    blocked = np.nonzero(OPT["Mb"])[0]
    assert np.abs(acc[blocked] - acc[blocked - 1]).max() < 1e-9


def test_reference_long_horizon_mask(torch_mod, lead_trace):
    """The reference's long-horizon recipe: N = 50 with 25 blocked stages (both limits of the old build at once)."""
    mb = reference_long_mask()
    assert mb.size == 50 and mb.sum() == 25
    OPT, V, _, _ = _ice_case(50, mb)
    B, n_steps = 3, 60
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"], seed=11)      # (the oracle's dense solver gives up on a step of some seeds)
    traj, status = _engine(OPT, V, 4).run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    _closed_loop_vs_oracle(OPT, V, sc, traj.cpu().numpy(), status.cpu().numpy(), range(B))


def test_full_size_batch_n60(torch_mod, lead_trace):
    """N = 60 x 8192: more instances than resident waves, so the per-wave scratch of the base inverse is reused.  The ABO
    weights of Settings.m (as bench.py's N = 60 entry): with the saved ICE solution's weights (up to 1e7) a few hundredths
    of a percent of these steps fail at the iteration limit 60 N + 200, with the efficiency map as well."""
    OPT, V, _, _ = make_case("ABO", 60)
    OPT = dict(OPT)
    OPT["fuel_map"] = "ICE"
    B, n_steps, k = 8192, 20, 7
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"])
    eng = _engine(OPT, V, B)
    traj, status = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    tr = traj.cpu().numpy(); st = status.cpu().numpy()
    assert st.sum() == 0
    assert np.isfinite(tr).all()
    traj2, _ = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    assert np.array_equal(traj2.cpu().numpy(), tr)
    perm = np.random.default_rng(0).permutation(B)
    trp, _ = eng.run_abmpc(sc["s0"][perm], sc["v0"][perm], sc["a_minus1"][perm],
                           np.ascontiguousarray(sc["s_tv"][:, perm]), np.ascontiguousarray(sc["v_tv"][:, perm]))
    assert np.array_equal(trp.cpu().numpy(), tr[:, :, perm])
    t1, _ = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][:k], sc["v_tv"][:k])
    t2, _ = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][k:], sc["v_tv"][k:], resume=True)
    assert np.array_equal(np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()]), tr)
    idx = np.random.default_rng(1).choice(B, 8, replace=False)
    _closed_loop_vs_oracle(OPT, V, sc, tr, st, idx)
