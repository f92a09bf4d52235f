"""eepacc_bl_build_qp: the condensed QP of a BLMPC step (bl_mode = 1) or a TVMPC step (bl_mode = 2), built on the device.

The five arrays are held against the CPU oracle's literal condensing (orc_create_qp_bl -> orc_transform_to_dense, per
instance), against tests/tvmpc_ref.py for the target-vehicle problem, and against the H and G the reference saved with
both of its BLMPC solutions.  The round trip build -> dense QP operator is compared with eepacc_bl_step by objective
value: with the reference's weights the problem is a linear program with faces of optima, so points are not compared.
Then what the entry point promises: the row catalogue, independence of the batch, no side effects, refusals.

Tolerances (bl_qp_ref.compare): those of tests/test_gpu_ab_build.py, A 1e-13 absolute, H 1e-12 max|H| (an all-zero
reference H, the linear program, must be met with zeros), g 1e-12 max|g|, finite bounds 1e-12 max(1, max|finite bound|),
infinite bounds in place.  Round trip: the objective check of tests/test_gpu_bl.py for oracle against kernel,
|cost - cost_ref| < 1e-7 max(1, |cost_ref|) + 1e-5.
"""
import ctypes as C

import numpy as np
import pytest

import bl_qp_ref as blr
from conftest import make_case, load_golden, golden_step_inputs
from eepacc_mpc_casadi_matlab_amd._abi import OUT, BL_ROW_TYPES
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1
from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV, default_opt
from qp_build_helpers import INS, _cols, _engine, _np
from bl_qp_ref import _bl_case, GEOM24, QP_WEIGHTS, STATES, KEYS, ROUND_TRIP_STEPS, cost_bar

pytestmark = pytest.mark.gpu

assert INS == KEYS           # bl_qp_ref's states are keyed by the builder's inputs, in argument order


def _states(tree, B, seed=1234):
    """The fixed states of the CPU test (standstill, a speed on the 5 m/s knot of the comfort limits, one on the 20 m/s knot)
    and perturbed states of the saved baseline run (scenarios.make_s1) up to B."""
    c = _cols([dict(zip(KEYS, st)) for st in STATES[:B]])
    if B > len(STATES):
        _, _, s_tv, v_tv = make_case(tree, 20)
        s1 = make_s1(B - len(STATES), load_golden(f"{tree.lower()}_blmpc"), s_tv, v_tv, seed=seed)
        c = {n: np.concatenate([c[n], np.asarray(s1[n], dtype=np.float64)]) for n in INS}
    return c


def _bl_step(eng, c):
    return eng._step(eng.lib.eepacc_bl_step, [c[n] for n in INS], True)


def _against_oracle(BL, V, cols, eng=None, preds=None):
    """All five arrays of every instance against the oracle's dense problem; preds = (s_pred, v_pred) [N+1, B] of the step
    before (estimator mode 2)."""
    from oracle import Oracle
    B = cols["s"].size
    eng = eng or _engine(BL, V, max(B, 1))
    orc = Oracle(BL, V)
    H, g, A, lba, uba = _np(eng.bl_build_qp(**cols))
    nV, nC = eng.bl_qp_size()
    assert (nV, nC) == (orc.nV("ab"), orc.nC("ab")) == (2 * eng.N, 13 * eng.N + 2)
    assert H.shape == (B, nV, nV) and A.shape == (B, nC, nV) and lba.shape == uba.shape == (B, nC) and g.shape == (B, nV)
    worst = dict(A=0.0, H=0.0, g=0.0, b=0.0)
    for i in range(B):
        inp = {n: float(cols[n][i]) for n in INS}
        r = blr.oracle_dense(orc, inp, *((preds[0][:, i], preds[1][:, i]) if preds else ()))
        e = blr.compare((H[i], g[i], A[i], lba[i], uba[i]), (r["H"], r["c"], r["G"], r["lb"], r["ub"]))
        assert max(e.values()) <= 1.0, (i, e)
        for n in worst:
            worst[n] = max(worst[n], e[n])
        # nothing is left of a buffer's earlier contents: the +-inf entries are the only non-finite ones, where the oracle has them
        assert np.isfinite(H[i]).all() and np.isfinite(g[i]).all() and np.isfinite(A[i]).all()
        assert np.array_equal(np.isfinite(lba[i]), np.isfinite(r["lb"])) and np.array_equal(np.isfinite(uba[i]), np.isfinite(r["ub"]))
    print("worst over %d instances: A %.3g, H %.3g, g %.3g, bounds %.3g (fractions of the bar)" % (B, worst["A"], worst["H"], worst["g"], worst["b"]))
    return worst


# ------------------------------------------------------------------------------------------------ 1  the oracle's dense problem
@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
@pytest.mark.parametrize("N", [2, 3, 20, 33, 63])
def test_horizon_sizes_vs_oracle(tree, N):
    """N = 2, 3: the first-stage jerk rows meet the terminal rows; 33: the first size above one half-wave's stages; 63: the
    limit.  B = 3: the standstill and both knots of the comfort limits."""
    BL, V = _bl_case(N, tree)
    _against_oracle(BL, V, _states(tree, 3))
    if N in (3, 33):
        BL, V = _bl_case(N, tree, W_BL=QP_WEIGHTS)
        _against_oracle(BL, V, _states(tree, 3))


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
@pytest.mark.parametrize("B", [1, 65])
def test_batch_sizes_vs_oracle(tree, B):
    """B = 65: more than one wave's worth of workgroups with a tail."""
    BL, V = _bl_case(20, tree, W_BL=QP_WEIGHTS) if B == 65 else _bl_case(20, tree)
    _against_oracle(BL, V, _states(tree, B))


@pytest.mark.parametrize("est", [0, 1])
def test_estimator_modes_vs_oracle(est):
    BL, V = _bl_case(20, "ABO", paramEstSetting=est, TVestSetting=est)
    _against_oracle(BL, V, _states("ABO", 8))


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_shifted_previous_solution_vs_oracle(tree):
    """Estimator mode 2: a bl_step leaves its predictions in the handle; the build of the next step reads them."""
    BL, V = _bl_case(20, tree, paramEstSetting=2)
    OPT, _, s_tv, v_tv = make_case(tree, 20)
    G = load_golden(f"{tree.lower()}_blmpc")
    ks = (40, 150, 333, 600, 868)
    eng = _engine(BL, V, 8)
    out, sp, vp, st = _bl_step(eng, _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ks]))
    assert np.isfinite(sp.cpu().numpy()).all() and np.isfinite(vp.cpu().numpy()).all()
    _against_oracle(BL, V, _cols([golden_step_inputs(G, s_tv, v_tv, k + 1) for k in ks]), eng, (sp.cpu().numpy(), vp.cpu().numpy()))


def test_variable_time_steps_vs_oracle():
    """Geometric Tvec: the sums of Ss and d in the reference's order; the jerk terms keep Ts = Tvec(1) (CreateQP_BL.m:31)."""
    for tree, kw in (("ABO", {}), ("ORIG", dict(W_BL=QP_WEIGHTS, paramEstSetting=0, TVestSetting=0))):
        BL, V = _bl_case(24, tree, Tvec=GEOM24, **kw)
        _against_oracle(BL, V, _states(tree, 6))


def test_route_features_vs_oracle():
    """Speed-limit steps, curves, stops and traffic lights switched on: the four caps carry real bounds."""
    for tree in ("ABO", "ORIG"):
        BL, V = _bl_case(20, tree, route=True)
        c = _states(tree, 8)
        c["s"] = np.array([10.0, 85.0, 150.0, 190.0, 290.0, 320.0, 400.0, 590.0])      # 150, 400: knots of the speed-limit table
        c["s_tv"] = c["s"] + np.array([5.0, 20.0, 60.0, 150.0, 1e4, 30.0, 8.0, 12.0])
        _against_oracle(BL, V, c)


# ------------------------------------------------------------------------------------------------ 2  other references
def _tv_case(N, uc=6, **kw):
    o = default_opt(); o["useCaseNum"] = uc
    OPT = Settings(o, tree="ABO", N_hor=N)
    OPT["TV_N_hor"] = N
    OPT.update(kw)
    return OPT, SetVehicleParameters("ABO")


# Before the first curve of use case 6 (100 .. 130 m); a state whose estimates 10 + 2.5 k land exactly on the curve's knots at
# 100 and 130 m (in exact arithmetic on both sides); at a standstill inside the curve.  The first state is kept off the knots
# on purpose: from s = 95, v = 9, a = 0.2 the reference's repeated sums reach the knot at 251 m exactly at stage 33 while the
# device's estimator (eepacc_stage.h: one product with tau instead of repeated sums) gives 251 - 3e-14, so the two sides read
# different rows of the curve table there, as the step kernels that share the estimator do.
TV_STATES = [(95.3, 9.0, 0.2, 14.0), (10.0, 5.0, 0.0, 0.0), (118.0, 0.0, -0.4, 30.0)]


def _against_tvref(OPT, V, cols, eng=None, preds=None):
    import tvmpc_ref as tvr
    ref = tvr.TVRef(OPT, V)
    eng = eng or _engine(Settings_TV(OPT), V, 8)
    H, g, A, lba, uba = _np(eng.bl_build_qp(cols["s"], cols["v"], cols["a_prev"], cols["t0"]))
    N = ref.N
    assert eng.bl_qp_size() == (2 * N, 11 * N) and A.shape[1:] == (11 * N, 2 * N)
    for i in range(cols["s"].size):
        a = [float(cols[n][i]) for n in ("s", "v", "a_prev", "t0")]
        Hd, cd, Gd, lbd, ubd, _, _, _ = ref.dense_qp(*a, *((preds[0][:, i], preds[1][:, i]) if preds else ()))
        e = blr.compare((H[i], g[i], A[i], lba[i], uba[i]), (Hd, cd, Gd, lbd, ubd))
        print("instance %d: A %.3g, H %.3g, g %.3g, bounds %.3g (fractions of the bar)" % (i, e["A"], e["H"], e["g"], e["b"]))
        assert max(e.values()) <= 1.0, (i, e)


@pytest.mark.parametrize("N", [2, 3, 20, 33, 63])
def test_target_vehicle_vs_tvmpc_ref(N):
    c = {n: np.array([st[j] for st in TV_STATES]) for j, n in enumerate(("s", "v", "a_prev", "t0"))}
    OPT, V = _tv_case(N)
    _against_tvref(OPT, V, c)
    if N in (3, 20):
        OPT, V = _tv_case(N, W_TV=QP_WEIGHTS, TV_trajEstSett=0)
        _against_tvref(OPT, V, c)


def test_target_vehicle_shifted_previous_solution():
    OPT, V = _tv_case(20, uc=2, TV_trajEstSett=2)
    eng = _engine(Settings_TV(OPT), V, 8)
    c = dict(s=np.array([200.0, 240.0]), v=np.array([10.0, 12.0]), a_prev=np.array([0.1, -0.5]), t0=np.array([10.0, 12.0]))
    out, sp, vp, st = eng.tv_step(c["s"], c["v"], c["a_prev"], c["t0"])
    assert np.isfinite(sp.cpu().numpy()).all() and np.isfinite(out.cpu().numpy()).all()
    o = out.cpu().numpy()
    nxt = dict(s=c["s"] + 0.5 * c["v"], v=c["v"] + 0.5 * o[OUT["a_qp"]], a_prev=o[OUT["a_qp"]].copy(), t0=c["t0"] + 0.5)
    _against_tvref(OPT, V, nxt, eng, (sp.cpu().numpy(), vp.cpu().numpy()))


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_saved_matrices_of_the_reference(tree):
    """optSol.H (40 x 40) and optSol.G (262 x 40) of both saved BLMPC solutions; neither depends on the state."""
    OPT, V, s_tv, v_tv = make_case(tree, 20)
    G = load_golden(f"{tree.lower()}_blmpc")
    eng = _engine(Settings_BL(OPT), V, 4)
    H, g, A, lba, uba = _np(eng.bl_build_qp(**_cols([golden_step_inputs(G, s_tv, v_tv, k) for k in (0, 333, 870)])))
    for i in range(3):
        assert A[i].shape == G["G"].shape and H[i].shape == G["H"].shape
        eA = np.abs(A[i] - G["G"]).max()
        print("%s: max|A - G_saved| = %.3g, max|H_saved| = %.3g, max|H| = %.3g" % (tree, eA, np.abs(G["H"]).max(), np.abs(H[i]).max()))
        assert eA <= 1e-13
        if np.abs(G["H"]).max() > 0.0:
            assert np.abs(H[i] - G["H"]).max() <= 1e-12 * np.abs(G["H"]).max()
        else:
            assert not H[i].any()                                      # the reference's weights: a linear program


# ------------------------------------------------------------------------------------------------ 3  round trip
@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_round_trip_objective_against_bl_step(tree):
    """build -> qp_solve_batched_dual (nV = 40, nC = 262) against eepacc_bl_step on 8 states of the saved run, the step with a
    face of optima (41) among them: the objective values, not the points.  First the oracle's own solve of the built problem
    against EEPACC_OUT_COST, then the operator's at the same bar.  An instance may be left out only where the oracle's solve
    reports failure too, and at most 1 of 8 (tests/test_bl_build_cpu.py checks that the oracle leaves out none)."""
    from oracle import Oracle
    OPT, V, s_tv, v_tv = make_case(tree, 20)
    G = load_golden(f"{tree.lower()}_blmpc")
    BL = Settings_BL(OPT)
    eng = _engine(BL, V, 8)
    c = _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ROUND_TRIP_STEPS])
    q = eng.bl_build_qp(**c)
    assert q.H.shape[1:] == (40, 40) and q.A.shape[1:] == (262, 40)
    r = eng.qp_solve_batched_dual(q.H, q.g, q.A, q.lba, q.uba)
    out, sp, vp, status = _bl_step(eng, c)
    o = out.cpu().numpy()
    assert int(status.cpu().numpy().sum()) == 0
    H, g, A, lba, uba = _np(q)
    x = r.x.cpu().numpy(); st = r.status.cpu().numpy()
    orc = Oracle(BL, V)
    left_out = 0
    for i, k in enumerate(ROUND_TRIP_STEPS):
        ref = o[OUT["cost"], i]
        xo, _, so = orc.qp_solve(H[i], g[i], A[i], lba[i], uba[i])
        gap_o = abs(0.5 * xo @ H[i] @ xo + g[i] @ xo - ref)
        gap_g = abs(0.5 * x[i] @ H[i] @ x[i] + g[i] @ x[i] - ref)
        print("step %d: cost %.9g, oracle's solve status %d gap %.3g, operator status %d gap %.3g, bar %.3g"
              % (k, ref, so["status"], gap_o, st[i], gap_g, cost_bar(ref)))
        if so["status"] != 0:
            left_out += 1                                              # only with the oracle's failure
            continue
        assert gap_o < cost_bar(ref), (k, gap_o)
        assert st[i] == 0, (k, st[i])
        assert gap_g < cost_bar(ref), (k, gap_g)
        y = A[i] @ x[i]
        assert np.maximum(np.maximum(y - uba[i], lba[i] - y), 0.0).max() < 1e-6, k
    assert left_out <= 1, left_out


# ------------------------------------------------------------------------------------------------ 4  catalogue
def test_row_catalogue():
    N = 20
    BL, V = _bl_case(N)
    eng = _engine(BL, V, 4)
    nV, nC = eng.bl_qp_size()
    stage, typ = eng.bl_qp_rows()
    assert (nV, nC) == (2 * N, 13 * N + 2)
    assert stage.shape == typ.shape == (nC,) and stage.dtype == typ.dtype == np.int32
    rs, rt = blr.rows_of(N)
    assert np.array_equal(stage, rs) and np.array_equal(typ, rt)
    for t, n in enumerate(BL_ROW_TYPES):
        assert (typ == t).sum() == N + (1 if n in ("safe1", "safe2") else 0), n
    assert list(stage[-2:]) == [N, N] and [BL_ROW_TYPES[t] for t in typ[-2:]] == ["safe1", "safe2"]
    # a row typed SAFE2 is s_k + tau_min v_k - xi_f through the condensing: a_i for i < k, xi_k (none at the terminal stage)
    q = eng.bl_build_qp(**_states("ABO", 2))
    A = q.A.cpu().numpy()[0]
    lo = np.isfinite(q.lba.cpu().numpy()[0]); hi = np.isfinite(q.uba.cpu().numpy()[0])
    T, tau_min = np.asarray(BL["Tvec"]), BL["tau_min"]
    for r in np.where(typ == BL_ROW_TYPES.index("safe2"))[0]:
        k = int(stage[r])
        want = np.zeros(nV, dtype=bool)
        want[0:2 * k:2] = True
        if k < N:
            want[2 * k + 1] = True
            assert A[r, 2 * k + 1] == -1.0
        assert np.array_equal(A[r] != 0.0, want), (r, k)
        for i in range(k):
            assert A[r, 2 * i] == 0.5 * T[i] ** 2 + T[i] * T[i + 1:k].sum() + tau_min * T[i]      # exact at Ts = 0.5
    two, lower = {"s", "v"}, {"xi_f", "a_min", "j_min"}
    for i in range(nC):
        n = BL_ROW_TYPES[typ[i]]
        want = (True, True) if n in two else (True, False) if n in lower else (False, True)
        if n == "s":
            want = (True, bool(np.isfinite(BL["s_goal"])))
        assert (bool(lo[i]), bool(hi[i])) == want, (i, n)
    # bl_mode = 2: the same enum without the safe-distance types, no terminal rows
    OPT, V = _tv_case(N)
    tv = _engine(Settings_TV(OPT), V, 4)
    stage, typ = tv.bl_qp_rows()
    rs, rt = blr.rows_of(N, tv=True)
    assert tv.bl_qp_size() == (2 * N, 11 * N) and np.array_equal(stage, rs) and np.array_equal(typ, rt)
    assert typ.max() == BL_ROW_TYPES.index("v_tl") and stage.max() == N - 1


# ------------------------------------------------------------------------------------------------ 5  independence, side effects
def test_instances_are_independent():
    import torch
    BL, V = _bl_case(20, "ORIG", W_BL=QP_WEIGHTS)
    eng = _engine(BL, V)
    c = _states("ORIG", 65)
    full = _np(eng.bl_build_qp(**c))
    again = _np(eng.bl_build_qp(**c))
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for i in (0, 7, 63, 64):
        one = _np(eng.bl_build_qp(**{n: c[n][i:i + 1] for n in INS}))
        for a, b in zip(full, one):
            assert np.array_equal(a[i:i + 1], b), i
    perm = np.random.default_rng(0).permutation(65)
    shuffled = _np(eng.bl_build_qp(**{n: np.ascontiguousarray(c[n][perm]) for n in INS}))
    for a, b in zip(full, shuffled):
        assert np.array_equal(a[perm], b)
    # every entry is written: buffers pre-filled with NaN hold none afterwards and equal the first build
    nV, nC = eng.bl_qp_size()
    B = 65
    f64 = dict(dtype=torch.float64, device="cuda")
    ins = [torch.as_tensor(c[n], **f64) for n in INS]
    outs = [torch.full((B * n,), float("nan"), **f64) for n in (nV * nV, nV, nV * nC, nC, nC)]
    assert eng.lib.eepacc_bl_build_qp(eng.h, B, *[x.data_ptr() for x in ins + outs], None) == 0
    torch.cuda.synchronize()
    got = [x.cpu().numpy() for x in outs]
    assert not any(np.isnan(a).any() for a in got)
    assert np.array_equal(got[0].reshape(B, nV, nV), full[0]) and np.array_equal(got[1].reshape(B, nV), full[1])
    assert np.array_equal(got[2].reshape(B, nV, nC).transpose(0, 2, 1), full[2])
    assert np.array_equal(got[3].reshape(B, nC), full[3]) and np.array_equal(got[4].reshape(B, nC), full[4])


@pytest.mark.parametrize("est", [1, 2])
def test_build_has_no_side_effects(est):
    """A build between two bl_step calls (estimator mode 2 included: the carried predictions are read, not written) leaves
    the second call's outputs unchanged; the same between two closed-loop launches and between two tv_step calls."""
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    G = load_golden("abo_blmpc")
    BL = Settings_BL(OPT); BL["paramEstSetting"] = est
    c1 = _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in (40, 150, 333, 600)])
    c2 = _cols([golden_step_inputs(G, s_tv, v_tv, k + 1) for k in (40, 150, 333, 600)])
    other = _states("ABO", 7)

    def steps(with_build):
        eng = _engine(BL, V, 8)
        _bl_step(eng, c1)
        if with_build:
            eng.bl_build_qp(**other); eng.bl_build_qp(**c2)
        return [x.cpu().numpy() for x in _bl_step(eng, c2)]
    for a, b in zip(steps(False), steps(True)):
        assert np.array_equal(a, b)

    n = 12
    stv = np.repeat(s_tv[:n, None], 3, 1); vtv = np.repeat(v_tv[:n, None], 3, 1)

    def loop(with_build):
        eng = _engine(BL, V, 8)
        z = np.zeros(3)
        t1, s1 = eng.run_blmpc(z, np.array([0.0, 2.0, 5.0]), z, stv[:6], vtv[:6])
        if with_build:
            eng.bl_build_qp(**other)
        t2, s2 = eng.run_blmpc(z, np.array([0.0, 2.0, 5.0]), z, stv[6:], vtv[6:], resume=True)
        return np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()]), np.concatenate([s1.cpu().numpy(), s2.cpu().numpy()])
    ta, sa = loop(False)
    tb, sb = loop(True)
    assert np.array_equal(ta, tb) and np.array_equal(sa, sb) and np.isfinite(ta).all()

    OPT, V = _tv_case(20, uc=2, TV_trajEstSett=est)
    tvc = dict(s=np.array([200.0, 240.0]), v=np.array([10.0, 12.0]), a_prev=np.array([0.1, -0.5]), t0=np.array([10.0, 12.0]))

    def tv_steps(with_build):
        eng = _engine(Settings_TV(OPT), V, 8)
        eng.tv_step(**tvc)
        if with_build:
            eng.bl_build_qp(**tvc)
        return [x.cpu().numpy() for x in eng.tv_step(**tvc)]
    for a, b in zip(tv_steps(False), tv_steps(True)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6  refusals
def test_refusals():
    import torch
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, EepaccError
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    G = load_golden("abo_blmpc")
    eng = _engine(Settings_BL(OPT), V, 8)
    lib = eng.lib
    nV, nC = eng.bl_qp_size()
    B = 3
    c = _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in (60, 333, 600)])
    twin = _engine(Settings_BL(OPT), V, 8)                 # the same bl_step calls without the refused ones in between
    _bl_step(eng, c); _bl_step(twin, c)                   # (a step starts from the working set the handle's last step left)

    def unchanged():
        for a, b in zip(_bl_step(twin, c), _bl_step(eng, c)):
            assert np.array_equal(a.cpu().numpy(), b.cpu().numpy())
    f64 = dict(dtype=torch.float64, device="cuda")
    ins = [torch.zeros(B, **f64) for _ in range(7)]
    outs = [torch.empty(B * n, **f64) for n in (nV * nV, nV, nV * nC, nC, nC)]
    names = list(INS) + ["H", "g", "A", "lba", "uba"]
    for j, name in enumerate(names):                      # every buffer in turn, by name
        ptrs = [x.data_ptr() for x in ins + outs]
        ptrs[j] = None
        assert lib.eepacc_bl_build_qp(eng.h, B, *ptrs, None) == -1
        assert ("eepacc_bl_build_qp: %s is NULL" % name) == lib.eepacc_last_error().decode()
        unchanged()
    ptrs = [x.data_ptr() for x in ins + outs]
    for bad in (9, -1):
        assert lib.eepacc_bl_build_qp(eng.h, bad, *ptrs, None) == -1
        assert "B = %d" % bad in lib.eepacc_last_error().decode()
        unchanged()
    with pytest.raises(EepaccError, match="max_batch"):
        eng.bl_build_qp(**_states("ABO", 9))
    unchanged()
    assert lib.eepacc_bl_build_qp(eng.h, 0, *([None] * 12), None) == 0
    q = eng.bl_build_qp(*[np.zeros(0)] * 7)
    assert q.H.shape == (0, nV, nV) and q.A.shape == (0, nC, nV) and q.lba.shape == (0, nC)
    n1, n2 = C.c_int(), C.c_int()
    assert lib.eepacc_bl_qp_size(eng.h, None, C.byref(n2)) == -1 and "nV" in lib.eepacc_last_error().decode()
    assert lib.eepacc_bl_qp_size(eng.h, C.byref(n1), None) == -1 and "nC" in lib.eepacc_last_error().decode()
    assert lib.eepacc_bl_qp_rows(eng.h, None, None) == -1 and "stage" in lib.eepacc_last_error().decode()
    unchanged()
    # bl_mode = 2: the lead arrays may be NULL, every other buffer may not
    TVO, TVV = _tv_case(20)
    tv = _engine(Settings_TV(TVO), TVV, 8)
    tnV, tnC = tv.bl_qp_size()
    touts = [torch.empty(B * n, **f64) for n in (tnV * tnV, tnV, tnV * tnC, tnC, tnC)]
    tptrs = [x.data_ptr() for x in ins[:4]] + [None] * 3 + [x.data_ptr() for x in touts]
    assert lib.eepacc_bl_build_qp(tv.h, B, *tptrs, None) == 0
    for j in (0, 1, 2, 3, 7, 8, 9, 10, 11):
        p = list(tptrs); p[j] = None
        assert lib.eepacc_bl_build_qp(tv.h, B, *p, None) == -1
        assert ("eepacc_bl_build_qp: %s is NULL" % names[j]) == lib.eepacc_last_error().decode()
    # a bl_mode = 0 handle and a class handle: EEPACC_ENOTSUP; the AB entry refuses the baseline handle and names this one
    ab = _engine(OPT, V, 8)
    cls = Engine.from_classes([OPT], [V], max_batch=8)
    cls.set_classes(np.zeros(B, dtype=np.int32))
    for e, words in ((ab, ("bl_mode = 0", "eepacc_ab_build_qp", "eepacc_fb_build_qp")), (cls, ("eepacc_create_classes",))):
        assert lib.eepacc_bl_build_qp(e.h, B, *ptrs, None) == -4
        for w in words:
            assert w in lib.eepacc_last_error().decode()
        assert lib.eepacc_bl_qp_size(e.h, C.byref(n1), C.byref(n2)) == -4
        with pytest.raises(EepaccError):
            e.bl_qp_rows()
    assert lib.eepacc_ab_build_qp(eng.h, B, *ptrs, None) == -4 and "eepacc_bl_build_qp" in lib.eepacc_last_error().decode()
    unchanged()
    torch.cuda.synchronize()
