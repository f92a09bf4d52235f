"""eepacc_fb_build_qp: the condensed QP of an FBMPC step, built on the device.

Independent checks of the five arrays: the H and G the reference saved with both FBMPC solutions, the CPU oracle's literal
condensing (Oracle.fb_step(..., want_dense=True)) over the settings and horizon lengths, with the model A(k)/D(k) taken from
the handle's carried state (both stores of it) and passed explicitly, and the round trip build -> dense QP operator against
the structured FBMPC kernel.  Then what the entry point promises about side effects, independence of the batch, the row
catalogue and refusals.

Tolerances.  A: 1e-12 absolute and H: 1e-11 max|H|, what the oracle itself meets against the saved matrices
(test_oracle_golden.py::test_fb_final_step_dense_H_G); g: 1e-12 max|g|; finite bounds: 1e-12 max(1, max|finite bound|), the
bars of test_gpu_ab_build.py; infinite bounds in place.  Round trip: those of test_gpu_fb.py (_compare_fb).

The oracle's dense problem at N = 63: orc_fb_step also solves the QP it returns, which takes up to 20 s per instance at
that size.  _oracle_dense(solve=False) calls the same two functions of the oracle (orc_create_qp_fb,
orc_transform_to_dense) around the model update of orc_fb_step restated here; test_oracle_routes_agree pins the two routes
to each other bit for bit.
"""
import ctypes as C
import math

import numpy as np
import pytest

import qp_build_helpers
from conftest import make_case, load_golden, golden_step_inputs
from eepacc_mpc_casadi_matlab_amd._abi import OUT, FB_ROW_TYPES, SettingsPOD, Vehicle, c_double_p, as_dptr
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1, make_s2
from qp_build_helpers import INS, _cols, _np

pytestmark = pytest.mark.gpu

MB20 = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1]          # that of test_gpu_ab_build.py


def _engine(OPT, V, max_batch=8):
    return qp_build_helpers._engine(OPT, V, max_batch)


def _case(tree, N, **kw):
    OPT, V, s_tv, v_tv = make_case(tree, N)
    OPT = dict(OPT); OPT.update(kw)
    return OPT, V, s_tv, v_tv


def _s1(tree, B, seed=1234):
    """Perturbed golden states (scenarios.make_s1), valid inputs at every horizon length."""
    _, _, s_tv, v_tv = make_case(tree, 20)
    s1 = make_s1(B, load_golden(f"{tree.lower()}_abmpc"), s_tv, v_tv, seed=seed)
    return {n: np.ascontiguousarray(s1[n], dtype=np.float64) for n in INS}


def _fb_step(eng, c):
    """Engine.fb_step on the inputs of the build (v_prev, Fm_prev, Fb_prev are accepted and unused, CreateQP_FB.m:1)."""
    z = np.zeros_like(c["s"])
    return eng.fb_step(c["s"], c["v"], z, c["a_prev"], z, z, c["t0"], c["s_tv"], c["v_tv"], c["a_tv_prev"])


# ---------------------------------------------------------------------------------------- the oracle's side
def _fresh_state(OPT, V, v0):
    """The loop state before step 0: A(k), D(k) of ABO/RunOpt_FBMPC.m:78-90 (orc_run_fbmpc)."""
    from oracle.loader import LoopState
    st = LoopState()
    lm, za, T = V["lambda"] * V["m"], V["zeta_a"], np.asarray(OPT["Tvec"], dtype=np.float64)
    for k in range(int(OPT["N_hor"])):
        if OPT["FBuseTaylor"]:
            st.fbA22[k] = 1.0 - 2.0 * T[k] * za * v0 * v0 / lm
            st.fbD2[k] = T[k] / lm * (za * v0 * v0)
        else:
            st.fbA22[k] = 1.0
            st.fbD2[k] = T[k] / lm * (-za * v0 * v0)
    st.k = 0
    return st


def _oracle_dense(orc, V, st, inp, pred=None, solve=True):
    """The oracle's dense problem of the step with the inputs inp at the loop state st, whose model it updates as
    orc_fb_step does.  pred = (s_pred, v_pred) of the previous step for paramEstSetting = 2."""
    from oracle.loader import StepIO
    N = orc.N
    if solve and pred is None:
        return orc.fb_step(st, inp["s"], inp["v"], 0.0, inp["a_prev"], 0.0, 0.0, inp["t0"], inp["s_tv"], inp["v_tv"],
                           inp["a_tv_prev"], want_dense=True)
    nV, nC = orc.nV("fb"), orc.nC("fb")
    if solve:                                              # Oracle.fb_step with the previous predictions filled in
        io = StepIO()
        for n in INS:
            setattr(io, n, float(inp[n]))
        for k in range(N + 1):
            io.s_pred[k] = float(pred[0][k]); io.v_pred[k] = float(pred[1][k])
        dense = np.zeros(nV * nV + nV + nC * nV + 2 * nC + nV)
        rc = orc.lib.orc_fb_step(C.byref(orc.S), C.byref(orc.V), C.byref(st), C.byref(io), as_dptr(dense))
        return orc._unpack(io, rc, dense, "fb")
    L, dp, dbl = orc.lib, c_double_p, C.c_double
    L.orc_create_qp_fb.argtypes = [C.POINTER(SettingsPOD), C.POINTER(Vehicle), dbl, dbl, dp, dp, dp] + [dbl] * 5 + [dp] * 6
    L.orc_transform_to_dense.argtypes = [C.c_int] * 3 + [dp] * 8 + [dbl, dbl] + [dp] * 7
    L.orc_create_qp_fb.restype = None; L.orc_transform_to_dense.restype = None
    nz = 8 * N + 2
    s_est, v_est, stv_est, vtv_est = (np.zeros(N + 1) for _ in range(4))
    sp, vp = (c_double_p(), c_double_p()) if pred is None else (as_dptr(np.ascontiguousarray(pred[0])), as_dptr(np.ascontiguousarray(pred[1])))
    L.orc_estimate_vehicle_trajectory(C.byref(orc.S), 0, inp["s"], inp["v"], inp["a_prev"], sp, vp, as_dptr(s_est), as_dptr(v_est))
    L.orc_estimate_vehicle_trajectory(C.byref(orc.S), 1, inp["s_tv"], inp["v_tv"], inp["a_tv_prev"], c_double_p(), c_double_p(),
                                      as_dptr(stv_est), as_dptr(vtv_est))
    Hs, cs, Gs, glb, gub, theta = np.zeros(nz * nz), np.zeros(nz), np.zeros(nC * nz), np.zeros(nC), np.zeros(nC), np.zeros(N)
    L.orc_create_qp_fb(C.byref(orc.S), C.byref(orc.V), inp["s"], inp["v"], as_dptr(s_est), as_dptr(v_est), as_dptr(stv_est),
                       inp["t0"], 0.0, inp["a_prev"], 0.0, 0.0, as_dptr(Hs), as_dptr(cs), as_dptr(Gs), as_dptr(glb), as_dptr(gub),
                       as_dptr(theta))
    lm, za, T = V["lambda"] * V["m"], V["zeta_a"], [float(x) for x in orc.OPT["Tvec"]]
    zrg = lambda i: V["m"] * V["g"] * (V["c_r"] * math.cos(theta[i]) + math.sin(theta[i]))
    if orc.OPT["FBuseTaylor"]:                             # oracle/eepacc_oracle.c, orc_fb_step: RunOpt_FBMPC.m:247-259
        if st.k < N:
            i = N - 1
            st.fbA22[st.k] = 1.0 - 2.0 * T[i] * za * float(v_est[i]) / lm
            st.fbD2[st.k] = T[i] / lm * (za * float(v_est[i]) * float(v_est[i]) - zrg(i))
    else:
        for i in range(N):
            st.fbD2[i] = T[i] / lm * (-za * float(v_est[i]) * float(v_est[i]) - zrg(i))
    A, Bm, Dm = np.zeros(4 * N), np.zeros(12 * N), np.zeros(2 * N)
    for k in range(N):
        A[4 * k:4 * k + 4] = (1.0, T[k], 0.0, st.fbA22[k])
        Bm[12 * k + 6] = Bm[12 * k + 7] = T[k] / lm
        Dm[2 * k + 1] = st.fbD2[k]
    Hd, cd, Gd, lbd, ubd = np.zeros(nV * nV), np.zeros(nV), np.zeros(nC * nV), np.zeros(nC), np.zeros(nC)
    Psi, d = np.zeros(nz * nV), np.zeros(nz)
    L.orc_transform_to_dense(N, 6, nC, as_dptr(A), as_dptr(Bm), as_dptr(Dm), as_dptr(Hs), as_dptr(cs), as_dptr(Gs), as_dptr(glb),
                             as_dptr(gub), inp["s"], inp["v"], as_dptr(Hd), as_dptr(cd), as_dptr(Gd), as_dptr(lbd), as_dptr(ubd),
                             as_dptr(Psi), as_dptr(d))
    return dict(H=Hd.reshape(nV, nV), c=cd, G=Gd.reshape(nC, nV), lb=lbd, ub=ubd)


def _compare(q, i, r, what=""):
    """Instance i of a built problem (numpy arrays H, g, A, lba, uba) against the oracle's dense problem r."""
    H, g, A, lba, uba = q[:5]
    assert H[i].shape == r["H"].shape and A[i].shape == r["G"].shape and lba[i].shape == r["lb"].shape
    eA = np.abs(A[i] - r["G"]).max()
    eH = np.abs(H[i] - r["H"]).max() / np.abs(r["H"]).max()
    eg = np.abs(g[i] - r["c"]).max() / np.abs(r["c"]).max()
    fin_all = np.concatenate([r["lb"][np.isfinite(r["lb"])], r["ub"][np.isfinite(r["ub"])]])
    bscale = max(1.0, np.abs(fin_all).max())
    eb = 0.0
    for mine, ref in ((lba[i], r["lb"]), (uba[i], r["ub"])):
        fin = np.isfinite(ref)
        assert np.array_equal(mine[~fin], ref[~fin]), (what, i)          # infinite entries: same place, same sign
        assert np.isfinite(mine[fin]).all(), (what, i)
        eb = max(eb, np.abs(mine[fin] - ref[fin]).max() / bscale)
    print("%s instance %d: max|A - G| %.3g, H %.3g of max|H|, g %.3g of max|g|, bounds %.3g of their scale" % (what, i, eA, eH, eg, eb))
    assert eA < 1e-12 and eH < 1e-11 and eg <= 1e-12 and eb <= 1e-12, (what, i, eA, eH, eg, eb)


def _fresh_vs_oracle(OPT, V, cols, eng=None, solve=True, what=""):
    """Step 0 on a fresh handle: all five arrays of every instance against the oracle's dense problem of a fresh loop."""
    from oracle import Oracle
    eng = eng or _engine(OPT, V)
    orc = Oracle(OPT, V)
    q = _np(eng.fb_build_qp(**cols))
    assert eng.fb_qp_size() == (orc.nV("fb"), orc.nC("fb"))
    for i in range(q[0].shape[0]):
        inp = {n: float(cols[n][i]) for n in INS}
        _compare(q, i, _oracle_dense(orc, V, _fresh_state(OPT, V, inp["v"]), inp, solve=solve), what)
    return eng


# ------------------------------------------------------------------------------------------------ 1
def _replayed_model(OPT, V, G, s_tv, v_tv, N=20, Ts=0.5):
    """The A(k), D(k) the reference's loop holds at step 870: at MPC step k < N entry k was frozen from v_est(N_hor) of that
    step (the replay of tests/test_oracle_golden.py::test_fb_final_step_dense_H_G over the saved trajectory)."""
    from oracle import Oracle
    orc = Oracle(OPT, V)
    lm = V["lambda"] * V["m"]
    A22, D2 = np.ones(N), np.zeros(N)
    for k in range(N):
        inp = golden_step_inputs(G, s_tv, v_tv, k)
        s_est = np.zeros(N + 1); v_est = np.zeros(N + 1)
        orc.lib.orc_estimate_vehicle_trajectory(C.byref(orc.S), 0, inp["s"], inp["v"], inp["a_prev"], c_double_p(), c_double_p(),
                                                as_dptr(s_est), as_dptr(v_est))
        i = N - 1
        theta = OPT["slope"][0]
        A22[k] = 1.0 - 2.0 * Ts * V["zeta_a"] * v_est[i] / lm
        D2[k] = Ts / lm * (V["zeta_a"] * v_est[i] ** 2 - V["m"] * V["g"] * (V["c_r"] * np.cos(theta) + np.sin(theta)))
    return A22, D2


@pytest.mark.parametrize("name", ["abo_fbmpc", "orig_fbmpc"])
def test_saved_matrices_of_the_reference(name):
    """Step 870 of both saved FBMPC solutions: the H (120 x 120) and G (522 x 120) the reference wrote with them."""
    tree = name.split("_")[0].upper()
    OPT, V, s_tv, v_tv = _case(tree, 20)
    G = load_golden(name)
    A22, D2 = _replayed_model(OPT, V, G, s_tv, v_tv)
    eng = _engine(OPT, V, 4)
    q = eng.fb_build_qp(**_cols([golden_step_inputs(G, s_tv, v_tv, 870)]), A22=A22[:, None], D2=D2[:, None], want_model=True)
    H, g, A, lba, uba, A22_used, D2_used = _np(q)
    assert np.array_equal(A22_used[:, 0], A22) and np.array_equal(D2_used[:, 0], D2)
    assert A[0].shape == G["G"].shape == (522, 120) and H[0].shape == G["H"].shape == (120, 120)
    eA = np.abs(A[0] - G["G"]).max()
    eH = np.abs(H[0] - G["H"]).max() / np.abs(G["H"]).max()
    print("%s: max|A - G| = %.3g, max|H - H_gold| / max|H_gold| = %.3g" % (name, eA, eH))
    assert eA < 1e-12
    assert eH < 1e-11


# ------------------------------------------------------------------------------------------------ 2
def test_oracle_routes_agree():
    """No GPU work: _oracle_dense without the solve returns the arrays of Oracle.fb_step(want_dense=True) bit for bit and
    leaves the same model behind, at a step that replaces an entry (k = 3) and with FBuseTaylor = 0."""
    from oracle import Oracle
    for kw in ({}, dict(FBuseTaylor=False)):
        OPT, V, s_tv, v_tv = _case("ABO", 20, **kw)
        G = load_golden("abo_fbmpc")
        orc = Oracle(OPT, V)
        inp = golden_step_inputs(G, s_tv, v_tv, 60)
        sa, sb = _fresh_state(OPT, V, 3.0), _fresh_state(OPT, V, 3.0)
        sa.k = sb.k = 3
        ra = _oracle_dense(orc, V, sa, inp)
        rb = _oracle_dense(orc, V, sb, inp, solve=False)
        for n in ("H", "c", "G", "lb", "ub"):
            assert np.array_equal(ra[n], rb[n]), n
        assert list(sa.fbA22[:20]) == list(sb.fbA22[:20]) and list(sa.fbD2[:20]) == list(sb.fbD2[:20])


@pytest.mark.parametrize("dense_path", [False, True], ids=["structured", "dense_path"])
@pytest.mark.parametrize("N", [20, 3])
def test_carried_model_from_the_handle_vs_oracle(N, dense_path):
    """Engine.fb_step and the oracle walk through golden steps 0, 1, 2, ... with one loop state; before the steps
    k = 0, 1, N-1, N, N+5 the build with A22 = D2 = None must pose the oracle's problem of that step: initialisation, the
    replacement of entry k == k_step < N, the freeze from k_step >= N on.  A structured handle keeps the entries in its
    per-instance state block, a handle with blocked moves (dense path) in stage-major arrays."""
    from oracle import Oracle
    mb = (MB20 if N == 20 else [0, 0, 1]) if dense_path else None
    OPT, V, s_tv, v_tv = _case("ABO", N, **({} if mb is None else dict(Mb=np.array(mb))))
    G = load_golden("abo_fbmpc")
    eng = _engine(OPT, V, 4)
    orc = Oracle(OPT, V)
    assert eng.fb_qp_size() == (6 * N, 26 * N + 2 + (2 * sum(mb) if mb else 0))
    st = _fresh_state(OPT, V, float(G["v_opt"][0]))
    checked = []
    for k in range(N + 6):
        inp = golden_step_inputs(G, s_tv, v_tv, k)
        c = _cols([inp, inp])
        st.k = k
        q = _np(eng.fb_build_qp(**c)) if k in (0, 1, N - 1, N, N + 5) else None
        r = _oracle_dense(orc, V, st, inp)                                # the oracle's step: its model moves on
        if q is not None:
            _compare(q, 0, r, "N=%d step %d" % (N, k))
            assert all(np.array_equal(a[0], a[1]) for a in q)
            checked.append(k)
        _fb_step(eng, c)                                                  # the engine's step: its model moves on
    assert checked == sorted({0, 1, N - 1, N, N + 5})


@pytest.mark.parametrize("est", [0, 1])
@pytest.mark.parametrize("tree,N", [("ABO", 2), ("ORIG", 2), ("ABO", 3), ("ORIG", 3), ("ABO", 33), ("ORIG", 33),
                                    ("ABO", 63), ("ORIG", 63)])
def test_horizon_sizes_vs_oracle(tree, N, est):
    """N = 2, 3: the first-stage jerk rows beside the terminal rows, the k + 1 < N coupling block absent or single; 33; 63:
    the limit and the LDS budget.  Both estimator modes on the ego and the lead, step 0."""
    OPT, V, _, _ = _case(tree, N, paramEstSetting=est, TVestSetting=est)
    _fresh_vs_oracle(OPT, V, _s1(tree, 2 if N == 63 else 4, seed=100 + N), solve=N < 63, what="%s N=%d est=%d" % (tree, N, est))


def test_blocked_moves_vs_oracle():
    OPT, V, _, _ = _case("ABO", 20, Mb=np.array(MB20))
    eng = _engine(OPT, V)
    assert eng.fb_qp_size() == (120, 26 * 20 + 2 + 2 * sum(MB20))
    _fresh_vs_oracle(OPT, V, _s1("ABO", 4), eng, what="Mb")
    stage, typ = eng.fb_qp_rows()
    for name in ("blocked_fm", "blocked_fb"):
        assert [int(k) for k in stage[typ == FB_ROW_TYPES.index(name)]] == [k for k in range(20) if MB20[k]]
    lba, uba = _np(eng.fb_build_qp(**_s1("ABO", 2)))[3:5]
    blocked = (typ == FB_ROW_TYPES.index("blocked_fm")) | (typ == FB_ROW_TYPES.index("blocked_fb"))
    assert (lba[:, blocked] == 0.0).all() and (uba[:, blocked] == 0.0).all()


def test_no_taylor_vs_oracle():
    """FBuseTaylor = 0: A22 = 1 and D2 from this step's estimate at every step, nothing carried."""
    OPT, V, _, _ = _case("ABO", 20, FBuseTaylor=False)
    c = _s1("ABO", 4)
    eng = _fresh_vs_oracle(OPT, V, c, what="FBuseTaylor=0")
    q = eng.fb_build_qp(**c, want_model=True)
    assert (q.A22_used.cpu().numpy() == 1.0).all()
    _fb_step(eng, c)                                                      # a step later the problem of these inputs is the same
    for a, b in zip(_np(q), _np(eng.fb_build_qp(**c, want_model=True))):
        assert np.array_equal(a, b)


def test_power_fit_with_fm_squared_vs_oracle():
    """b_quadr(4) != 0: the Fm^2 term of the power fit (a dense-path handle)."""
    bq = np.array([185, 1.296e-20, 2.301, 2.5e-4, 0.003728, -0.000181])
    OPT, V, _, _ = _case("ABO", 20, b_quadr=bq)
    _fresh_vs_oracle(OPT, V, _s1("ABO", 4), what="b_quadr(4)")


def test_variable_time_steps_vs_oracle():
    N = 24
    OPT, V, _, _ = _case("ABO", N, Tvec=0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1)))
    _fresh_vs_oracle(OPT, V, _s1("ABO", 4), what="Tvec")
    OPT, V, _, _ = _case("ORIG", N, Tvec=0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1)), paramEstSetting=0, TVestSetting=0)
    _fresh_vs_oracle(OPT, V, _s1("ORIG", 2), what="Tvec")


def test_route_features_vs_oracle():
    """Speed-limit steps, curves, stops and traffic lights switched on (the case of test_gpu_ab_build.py)."""
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, default_opt
    OPT = default_opt()
    OPT.update(slopes=np.array([[3.0, 40, 160], [-2.0, 300, 420]]),
               speedLimZones=np.array([[50.0, 0.0], [30.0, 150.0], [70.0, 400.0]]),
               curves=np.array([[-1 / 25.0, 90, 120], [1 / 60.0, 250, 300]]),
               stopLoc=np.array([200.0, 520.0]),
               TLLoc=np.array([[330.0, 5.0, 20.0, 25.0], [600.0, 0.0, 15.0, 15.0]]))
    OPT = Settings(OPT, tree="ORIG", N_hor=20)
    V = SetVehicleParameters("ORIG")
    c = _s1("ORIG", 8)
    c["s"] = np.array([10.0, 85.0, 140.0, 190.0, 290.0, 320.0, 395.0, 590.0])
    c["s_tv"] = c["s"] + np.array([5.0, 20.0, 60.0, 150.0, 1e4, 30.0, 8.0, 12.0])
    _fresh_vs_oracle(OPT, V, c, what="route")


@pytest.mark.parametrize("dense_path", [False, True], ids=["structured", "dense_path"])
def test_shifted_previous_solution_vs_oracle(dense_path):
    """paramEstSetting = 2: one fb_step leaves its predictions in the handle; the build of the next step reads them (and
    the model of step 1), as the next fb_step does."""
    from oracle import Oracle
    OPT, V, s_tv, v_tv = _case("ABO", 20, paramEstSetting=2, **(dict(Mb=np.array(MB20)) if dense_path else {}))
    G = load_golden("abo_fbmpc")
    ks = (40, 150, 333, 600)
    eng = _engine(OPT, V)
    orc = Oracle(OPT, V)
    c0 = _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ks])
    q0 = _np(eng.fb_build_qp(**c0))                                       # step 0: the predictions are zero
    _, sp, vp, _ = _fb_step(eng, c0)
    sp, vp = sp.cpu().numpy(), vp.cpu().numpy()
    assert np.abs(vp).max() > 1.0
    c1 = _cols([golden_step_inputs(G, s_tv, v_tv, k + 1) for k in ks])
    q1 = _np(eng.fb_build_qp(**c1))
    zero = np.zeros(21)
    for i in range(len(ks)):
        # the oracle's own loop state walks through step 0 (without the QP solve, which the model does not depend on) and
        # carries its model into step 1; of the engine only the predictions of its step 0 enter, as the reference's loop
        # hands them on
        st = _fresh_state(OPT, V, float(c0["v"][i]))
        _compare(q0, i, _oracle_dense(orc, V, st, {n: float(c0[n][i]) for n in INS}, pred=(zero, zero), solve=False), "paramEst=2 step 0")
        st.k = 1
        _compare(q1, i, _oracle_dense(orc, V, st, {n: float(c1[n][i]) for n in INS}, pred=(sp[:, i], vp[:, i])), "paramEst=2 step 1")


# ------------------------------------------------------------------------------------------------ 3
# Golden steps whose saved exitMessage is 0 and whose dense problem (posed at step 0 of a fresh loop, as the round trip
# poses it) Oracle.qp_solve solves with status 0, from the same point as the oracle's own solver, with v well above the
# 1e-3 m/s below which the force split is undetermined.  Checked on the CPU for both trees.
ROUND_TRIP_STEPS = (40, 60, 100, 150, 333, 400, 500, 600)


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_round_trip_against_the_structured_kernel(tree):
    OPT, V, s_tv, v_tv = _case(tree, 20)
    G = load_golden(f"{tree.lower()}_fbmpc")
    assert int(np.abs(G["exitMessage"][list(ROUND_TRIP_STEPS)]).sum()) == 0
    c = _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ROUND_TRIP_STEPS])
    eng = _engine(OPT, V)
    q = eng.fb_build_qp(**c)
    x, cost, status = eng.qp_solve_batched(q.H, q.g, q.A, q.lba, q.uba)
    out, _, _, st2 = _fb_step(_engine(OPT, V), c)
    x, cost, o = x.cpu().numpy(), cost.cpu().numpy(), out.cpu().numpy()
    print("status: operator %s, fb_step %s" % (status.cpu().numpy(), st2.cpu().numpy()))
    assert int(np.abs(status.cpu().numpy()).sum()) == 0 and int(np.abs(st2.cpu().numpy()).sum()) == 0
    Fr = o[OUT["Fm"]] + o[OUT["Fb"]]
    ftol = 1e-6 + 1e-8 * np.abs(Fr).max()                                 # test_gpu_fb.py::_compare_fb
    print("Fm %.3g Fb %.3g (bar %.3g)" % (np.abs(x[:, 0] - o[OUT["Fm"]]).max(), np.abs(x[:, 1] - o[OUT["Fb"]]).max(), ftol))
    assert np.abs(x[:, 0] - o[OUT["Fm"]]).max() < ftol
    assert np.abs(x[:, 1] - o[OUT["Fb"]]).max() < ftol
    for j, n in enumerate(("xi_v", "xi_h", "xi_s", "xi_f")):
        err = np.abs(x[:, 2 + j] - o[OUT[n]]).max()
        rel = 1e-11 * np.abs(o[OUT[n]]).max() if n == "xi_f" else 0.0
        print("%s %.3g" % (n, err))
        assert err < 1e-9 + rel, n
    H, g = q.H.cpu().numpy(), q.g.cpu().numpy()
    obj = 0.5 * np.einsum("bi,bij,bj->b", x, H, x) + np.einsum("bi,bi->b", g, x)
    cerr = np.abs(obj - o[OUT["cost"]]).max() / np.abs(o[OUT["cost"]]).max()
    print("cost (relative) %.3g; operator's own %.3g" % (cerr, np.abs(cost - o[OUT["cost"]]).max() / np.abs(o[OUT["cost"]]).max()))
    assert cerr < 1e-9


# ------------------------------------------------------------------------------------------------ 4
@pytest.mark.parametrize("dense_path", [False, True], ids=["structured", "dense_path"])
def test_build_has_no_side_effects(lead_trace, dense_path):
    """run_fbmpc of 2n steps against n steps, a build, n steps resumed; the same around two fb_step calls."""
    OPT, V, _, _ = _case("ABO", 20, **(dict(Mb=np.array(MB20)) if dense_path else {}))
    B, n = 5, 12
    sc = make_s2(B, 2 * n, lead_trace["V_TO_2Hz"], seed=5)
    c = _s1("ABO", B)

    def loop(with_build):
        eng = _engine(OPT, V, 8)
        t1, s1 = eng.run_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][:n], sc["v_tv"][:n])
        if with_build:
            eng.fb_build_qp(**c)
            eng.fb_build_qp(**c, A22=np.ones((20, B)), D2=np.zeros((20, B)), want_model=True)
        t2, s2 = eng.run_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][n:], sc["v_tv"][n:], resume=True)
        eng.synchronize()
        return np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()]), np.concatenate([s1.cpu().numpy(), s2.cpu().numpy()])

    def steps(with_build):
        eng = _engine(OPT, V, 8)
        res = []
        for j in range(2):
            cj = _s1("ABO", B, seed=40 + j)
            if with_build:
                eng.fb_build_qp(**c)
            res += _np(_fb_step(eng, cj))
        if with_build:
            eng.fb_build_qp(**c)
        res += _np(_fb_step(eng, _s1("ABO", B, seed=42)))
        return res
    eng = _engine(OPT, V, 8)
    tf, sf = eng.run_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    ta, sa = loop(False)
    tb, sb = loop(True)
    assert np.array_equal(tf.cpu().numpy(), ta) and np.array_equal(sf.cpu().numpy(), sa)
    assert np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert np.isfinite(ta).all()
    for a, b in zip(steps(False), steps(True)):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 5
def test_instances_are_independent():
    OPT, V, _, _ = _case("ORIG", 20, Mb=np.array(MB20))
    eng = _engine(OPT, V)
    c = _s1("ORIG", 8)
    full = _np(eng.fb_build_qp(**c, want_model=True))
    again = _np(eng.fb_build_qp(**c, want_model=True))
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for i in (0, 3, 7):
        alone = _np(eng.fb_build_qp(**{n: c[n][i:i + 1] for n in INS}, want_model=True))
        for a, b in zip(full[:5], alone[:5]):
            assert np.array_equal(a[i:i + 1], b), i
        for a, b in zip(full[5:], alone[5:]):
            assert np.array_equal(a[:, i:i + 1], b), i
    fed = _np(eng.fb_build_qp(**c, A22=full[5], D2=full[6], want_model=True))
    for a, b in zip(full, fed):
        assert np.array_equal(a, b)
    assert all(np.isfinite(a).all() for a in full[:3])
    # the same after two steps on a structured handle: the model from the handle, then fed back, by then not the initial one
    OPT, V, _, _ = _case("ABO", 20)
    eng = _engine(OPT, V)
    c = _s1("ABO", 8)
    first = eng.fb_build_qp(**c, want_model=True)
    _fb_step(eng, c); _fb_step(eng, c)
    full = _np(eng.fb_build_qp(**c, want_model=True))
    assert not np.array_equal(full[5], first.A22_used.cpu().numpy())
    fed = _np(eng.fb_build_qp(**c, A22=full[5], D2=full[6], want_model=True))
    for a, b in zip(full, fed):
        assert np.array_equal(a, b)


# ------------------------------------------------------------------------------------------------ 6
SLACK_OF = dict(xi_v=2, xi_h=3, xi_s=4, xi_f=5, tm_min=5, tm_max=5, axle_min=5, axle_max=5, fric_max=5, fric_min=5, a_max=5,
                a_min=5, j_max=5, j_min=5, v_lim=5, v_curv=5, v_stop=4, v_tl=4, v_inc=2, safe1=4, safe2=4, hwp=3)


@pytest.mark.parametrize("tree,mb", [("ABO", None), ("ORIG", MB20)])
def test_row_catalogue_shape(tree, mb):
    N = 20
    OPT, V, _, _ = _case(tree, N, **({} if mb is None else dict(Mb=np.array(mb))))
    eng = _engine(OPT, V, 2)
    nV, nC = eng.fb_qp_size()
    stage, typ = eng.fb_qp_rows()
    assert nV == 6 * N and nC == 26 * N + 2 + (2 * sum(mb) if mb else 0)
    assert stage.shape == typ.shape == (nC,) and stage.dtype == typ.dtype == np.int32
    assert (np.diff(stage) >= 0).all() and stage[0] == 0 and list(stage[-2:]) == [N, N]
    assert [FB_ROW_TYPES[t] for t in typ[-2:]] == ["safe1", "safe2"]
    assert typ.min() >= 0 and typ.max() < len(FB_ROW_TYPES)
    for k in range(N):
        tk = typ[stage == k]
        assert (np.diff(tk) > 0).all(), k                                 # types ascend within a stage
        assert tk.size == (28 if mb and mb[k] else 26), k
        assert (FB_ROW_TYPES.index("blocked_fm") in tk) == bool(mb and mb[k]), k
    # the catalogue names the data: the non-zero slack column of a row of the built A is the one its type names
    A = eng.fb_build_qp(**_s1(tree, 2)).A.cpu().numpy()[0]
    for i in range(nC):
        n, k = FB_ROW_TYPES[typ[i]], int(stage[i])
        slack = A[i].reshape(N, 6)[:, 2:]
        want = np.zeros((N, 4))
        if n in SLACK_OF and k < N:
            want[k, SLACK_OF[n] - 2] = 1.0
        assert np.array_equal(slack != 0.0, want != 0.0), (i, n, k)


def test_multipliers_read_row_by_row():
    """eepacc_qp_solve_batched_dual on built golden steps, read as test_gpu_ab_build.py::test_multipliers_read_row_by_row
    reads them: stationarity in CasADi's sign at the bar of tests/test_gpu_qp_dual.py (qp_dual_check.dual_check: r <= 1e-9
    of max(1, |g|, |lam|), no multiplier of the wrong sign), and a multiplier only on a row the working set holds."""
    import qp_dual_check as D
    OPT, V, s_tv, v_tv = _case("ABO", 20)
    G = load_golden("abo_fbmpc")
    eng = _engine(OPT, V)
    q = eng.fb_build_qp(**_cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ROUND_TRIP_STEPS]))
    r = eng.qp_solve_batched_dual(q.H, q.g, q.A, q.lba, q.uba)
    assert int(np.abs(r.status.cpu().numpy()).sum()) == 0
    H, g, A, lba, uba = _np(q)
    x, lam, ws = r.x.cpu().numpy(), r.lam_a.cpu().numpy(), r.ws_a.cpu().numpy()
    lam_x, ws_x = r.lam_x.cpu().numpy(), r.ws_x.cpu().numpy()
    stage, typ = eng.fb_qp_rows()
    assert ws.shape[1] == stage.size
    for i in range(x.shape[0]):
        d = D.dual_check((H[i], g[i], A[i], lba[i], uba[i], None, None), x[i], lam[i], lam_x[i], ws[i], ws_x[i])
        print("step %d: stationarity r = %.3g, held rows %d" % (ROUND_TRIP_STEPS[i], d["r"], (ws[i] != 0).sum()))
        assert d["r"] <= 1e-9, (i, d["r"])
        assert not d["sign"], (i, d["sign"])
    assert (lam[ws == 0] == 0.0).all()                                    # every row with lam_a != 0 has ws_a != 0
    assert np.isfinite(lba[ws == -1]).all() and np.isfinite(uba[ws == 1]).all()
    assert (ws != 0).any() and (ws_x == 0).all()
    for n in ("xi_v", "xi_h", "xi_s", "xi_f"):                            # a slack bound has a lower side only
        assert (ws[:, typ == FB_ROW_TYPES.index(n)] <= 0).all(), n


# ------------------------------------------------------------------------------------------------ 7
def test_refusals():
    import torch
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, EepaccError
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV
    OPT, V, _, _ = _case("ABO", 20)
    eng = _engine(OPT, V, 8)
    lib = eng.lib
    nV, nC = eng.fb_qp_size()
    B, N = 3, 20
    f64 = dict(dtype=torch.float64, device="cuda")
    ins = [torch.zeros(B, **f64) for _ in range(7)]
    model = [torch.ones(N * B, **f64), torch.zeros(N * B, **f64)]
    outs = [torch.empty(B * n, **f64) for n in (nV * nV, nV, nV * nC, nC, nC)]
    used = [torch.empty(N * B, **f64) for _ in range(2)]

    def call(h, nB, ptrs):
        return lib.eepacc_fb_build_qp(h, nB, *ptrs, None)
    full = [x.data_ptr() for x in ins + model + outs + used]
    names = list(INS) + ["A22", "D2", "H", "g", "A", "lba", "uba", "A22_used", "D2_used"]
    for j, name in enumerate(names):                      # every required buffer in turn, by name
        if name in ("A22", "D2", "A22_used", "D2_used"):
            continue
        ptrs = list(full); ptrs[j] = None
        assert call(eng.h, B, ptrs) == -1
        assert ("eepacc_fb_build_qp: %s is NULL" % name) == lib.eepacc_last_error().decode()
    for j, name in ((7, "A22"), (8, "D2")):               # only one of the two
        ptrs = list(full); ptrs[j] = None
        assert call(eng.h, B, ptrs) == -1
        assert ("eepacc_fb_build_qp: %s is NULL" % name) in lib.eepacc_last_error().decode()
    for drop in ((7, 8), (14, 15), (7, 8, 14, 15)):       # the optional ones may be absent
        ptrs = list(full)
        for j in drop:
            ptrs[j] = None
        assert call(eng.h, B, ptrs) == 0
    for bad in (9, -1):
        assert call(eng.h, bad, full) == -1
        assert "B = %d" % bad in lib.eepacc_last_error().decode()
    with pytest.raises(EepaccError, match="max_batch"):
        eng.fb_build_qp(**_s1("ABO", 9))
    assert call(eng.h, 0, [None] * 16) == 0
    q = eng.fb_build_qp(*[np.zeros(0)] * 7)
    assert q.H.shape == (0, nV, nV) and q.A.shape == (0, nC, nV) and q.lba.shape == (0, nC)
    n1, n2 = C.c_int(), C.c_int()
    assert lib.eepacc_fb_qp_size(eng.h, None, C.byref(n2)) == -1 and "nV" in lib.eepacc_last_error().decode()
    assert lib.eepacc_fb_qp_size(eng.h, C.byref(n1), None) == -1 and "nC" in lib.eepacc_last_error().decode()
    assert lib.eepacc_fb_qp_rows(eng.h, None, None) == -1 and "stage" in lib.eepacc_last_error().decode()
    assert call(None, B, full) == -1 and "NULL handle" in lib.eepacc_last_error().decode()
    # FBuseTaylor = 0 carries no model: given arrays are refused
    nt = _engine(dict(OPT, FBuseTaylor=False), V, 8)
    assert call(nt.h, B, full) == -1
    assert "A22" in lib.eepacc_last_error().decode() and "FBuseTaylor" in lib.eepacc_last_error().decode()
    # a dense-path handle reads its carried model with the stride of the FBMPC steps that wrote it: another B is refused,
    # whatever ABMPC calls on the handle did in between (they write the handle's last B, not the FBMPC store's)
    mb = _engine(dict(OPT, Mb=np.array(MB20)), V, 8)
    nCm = mb.fb_qp_size()[1]
    outs8 = [torch.empty(8 * n, **f64) for n in (nV * nV, nV, nV * nCm, nCm, nCm)]
    c8 = _s1("ABO", 8)
    ins8 = [torch.as_tensor(c8[n], **f64) for n in INS]
    from_handle = [x.data_ptr() for x in ins8] + [None, None] + [x.data_ptr() for x in outs8] + [None, None]
    assert call(mb.h, 8, from_handle) == 0                                   # before the first step nothing is carried: any B
    _fb_step(mb, {n: c8[n][:2] for n in INS})                            # the store now holds 2 instances
    mb.ab_step(**c8)                                                      # last B of the handle: 8
    assert call(mb.h, 8, from_handle) == -1
    msg = lib.eepacc_last_error().decode()
    assert "eepacc_fb_build_qp: B = 8 differs from the B = 2 of the FBMPC steps" in msg
    assert call(mb.h, 2, from_handle) == 0
    mb.ab_step(**{n: c8[n][:3] for n in INS})                             # last B of the handle: 3
    assert call(mb.h, 3, from_handle) == -1 and "B = 3 differs from the B = 2" in lib.eepacc_last_error().decode()
    assert call(mb.h, 2, from_handle) == 0
    model8 = [torch.ones(N * 8, **f64), torch.zeros(N * 8, **f64)]
    given = [x.data_ptr() for x in ins8 + model8 + outs8] + [None, None]
    assert call(mb.h, 8, given) == 0                                     # a given model needs nothing of the store
    mb.reset()
    assert call(mb.h, 8, from_handle) == 0                                   # after a reset nothing is carried
    cls = Engine.from_classes([OPT], [V], max_batch=8)
    cls.set_classes(np.zeros(B, dtype=np.int32))
    bl = _engine(Settings_BL(OPT), V, 8)
    tv = _engine(Settings_TV(OPT), V, 8)
    for e, word in ((cls, "eepacc_create_classes"), (bl, "bl_mode = 1"), (tv, "bl_mode = 2")):
        assert call(e.h, B, full) == -4
        assert word in lib.eepacc_last_error().decode()
        assert lib.eepacc_fb_qp_size(e.h, C.byref(n1), C.byref(n2)) == -4
        with pytest.raises(EepaccError):
            e.fb_qp_rows()
    torch.cuda.synchronize()


def test_longest_horizon_with_blocked_moves_vs_oracle():
    """N = 63 with blocked stages, the last one among them: the longest row table and the largest LDS footprint."""
    mb = np.zeros(63, dtype=np.int64); mb[5] = mb[40] = mb[62] = 1
    OPT, V, _, _ = _case("ABO", 63, Mb=mb)
    eng = _engine(OPT, V, 2)
    assert eng.fb_qp_size() == (378, 26 * 63 + 2 + 6)
    _fresh_vs_oracle(OPT, V, _s1("ABO", 2, seed=163), eng, solve=False, what="N=63 Mb")
