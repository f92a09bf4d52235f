"""eepacc_ab_build_qp: the condensed QP of an ABMPC step, built on the device.

Three independent checks of the five arrays: the H and G the reference saved with six solutions, the CPU oracle's
literal condensing (want_dense=True), and the round trip build -> dense QP operator against the structured ABMPC
kernel, which shares neither the builder nor the oracle's QP method.  Then what the entry point promises about side
effects, independence of the batch, the row catalogue and refusals.

Tolerances.  A: 1e-13 absolute and H: 1e-12 max|H|, what the oracle itself meets against the saved matrices
(test_oracle_golden.py); g: 1e-12 max|g|; finite bounds: 1e-12 max(1, max|finite bound|); infinite bounds in place.
Round trip: those of test_gpu_ab.py::test_open_loop_seeded_batch_vs_oracle.
"""
import ctypes as C

import numpy as np
import pytest

from ab_cert_cases import rollout
from conftest import make_case, load_golden, golden_step_inputs, GOLDEN_AB_VARIANTS, GOLDEN_AB_ICEMAP
from eepacc_mpc_casadi_matlab_amd._abi import OUT, AB_ROW_TYPES
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1, make_s2
from qp_build_helpers import INS, _cols, _engine, _np

pytestmark = pytest.mark.gpu

ICE = dict(W_AB=np.array(GOLDEN_AB_ICEMAP["W_AB"]), fuel_map=GOLDEN_AB_ICEMAP["fuel_map"])
MB20 = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1]


def _case(tree, N, **kw):
    OPT, V, s_tv, v_tv = make_case(tree, N)
    OPT = dict(OPT); OPT.update(kw)
    return OPT, V, s_tv, v_tv


def _s1(tree, B, seed=1234):
    """Perturbed golden states (scenarios.make_s1), valid inputs at every horizon length."""
    _, _, s_tv, v_tv = make_case(tree, 20)
    s1 = make_s1(B, load_golden(f"{tree.lower()}_abmpc"), s_tv, v_tv, seed=seed)
    return {n: np.ascontiguousarray(s1[n], dtype=np.float64) for n in INS}


def _against_oracle(OPT, V, cols, eng=None):
    """All five arrays of every instance against the oracle's dense problem; returns the largest errors seen, each as a
    fraction of its bound."""
    from oracle import Oracle
    eng = eng or _engine(OPT, V)
    orc = Oracle(OPT, V)
    H, g, A, lba, uba = _np(eng.ab_build_qp(**cols))
    nV, nC = eng.ab_qp_size()
    assert (nV, nC) == (orc.nV("ab"), orc.nC("ab"))
    assert H.shape[1:] == (nV, nV) and A.shape[1:] == (nC, nV) and lba.shape[1:] == (nC,)
    worst = dict(A=0.0, H=0.0, g=0.0, b=0.0)
    for i in range(H.shape[0]):
        r = orc.ab_step(**{n: float(cols[n][i]) for n in INS}, want_dense=True)
        eA = np.abs(A[i] - r["G"]).max() / 1e-13
        eH = np.abs(H[i] - r["H"]).max() / (1e-12 * np.abs(r["H"]).max())
        eg = np.abs(g[i] - r["c"]).max() / (1e-12 * np.abs(r["c"]).max())
        eb = 0.0
        fin_all = np.concatenate([r["lb"][np.isfinite(r["lb"])], r["ub"][np.isfinite(r["ub"])]])
        btol = 1e-12 * max(1.0, np.abs(fin_all).max())
        for mine, ref in ((lba[i], r["lb"]), (uba[i], r["ub"])):
            fin = np.isfinite(ref)
            assert np.array_equal(mine[~fin], ref[~fin]), i          # infinite entries: same place, same sign
            assert np.isfinite(mine[fin]).all(), i
            eb = max(eb, np.abs(mine[fin] - ref[fin]).max() / btol)
        print("instance %d: A %.3g, H %.3g, g %.3g, bounds %.3g (fractions of the bound)" % (i, eA, eH, eg, eb))
        assert eA <= 1.0 and eH <= 1.0 and eg <= 1.0 and eb <= 1.0, (i, eA, eH, eg, eb)
        for n, e in (("A", eA), ("H", eH), ("g", eg), ("b", eb)):
            worst[n] = max(worst[n], e)
    return worst


# ------------------------------------------------------------------------------------------------ 1
GOLDENS = {
    "abo_abmpc": ("ABO", {}),
    "orig_abmpc": ("ORIG", {}),
    "abo_abmpc_effmap": ("ABO", dict(W_AB=np.array(GOLDEN_AB_VARIANTS["abo_abmpc_effmap"]))),
    "abo_abmpc_fcopt": ("ABO", dict(W_AB=np.array(GOLDEN_AB_VARIANTS["abo_abmpc_fcopt"]))),
    "abo_abmpc_nofcopt": ("ABO", dict(W_AB=np.array(GOLDEN_AB_VARIANTS["abo_abmpc_nofcopt"]))),
    "abo_abmpc_icemap": ("ABO", ICE),
}


@pytest.mark.parametrize("name", sorted(GOLDENS))
def test_saved_matrices_of_the_reference(name):
    """Step 870 of every saved ABMPC solution: the H and G the reference wrote with it."""
    tree, kw = GOLDENS[name]
    OPT, V, s_tv, v_tv = _case(tree, 20, **kw)
    G = load_golden(name)
    eng = _engine(OPT, V, 4)
    H, g, A, lba, uba = _np(eng.ab_build_qp(**_cols([golden_step_inputs(G, s_tv, v_tv, 870)])))
    assert A[0].shape == G["G"].shape and H[0].shape == G["H"].shape
    eA = np.abs(A[0] - G["G"]).max()
    eH = np.abs(H[0] - G["H"]).max() / np.abs(G["H"]).max()
    print("%s: max|A - G| = %.3g, max|H - H_gold| / max|H_gold| = %.3g" % (name, eA, eH))
    assert eA <= 1e-13
    assert eH <= 1e-12


# ------------------------------------------------------------------------------------------------ 2
@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_golden_steps_vs_oracle(tree):
    OPT, V, s_tv, v_tv = _case(tree, 20)
    G = load_golden(f"{tree.lower()}_abmpc")
    _against_oracle(OPT, V, _cols([golden_step_inputs(G, s_tv, v_tv, k) for k in (0, 1, 60, 333, 870)]))


@pytest.mark.parametrize("est", [0, 1])
@pytest.mark.parametrize("tree,N", [("ABO", 2), ("ORIG", 2), ("ABO", 3), ("ORIG", 3), ("ABO", 33), ("ORIG", 33),
                                    ("ABO", 63), ("ORIG", 63)])
def test_horizon_sizes_vs_oracle(tree, N, est):
    """N = 2, 3: the first-stage jerk rows meet the terminal rows; 33: the first size above one half-wave's stages;
    63: the limit.  Both estimator modes on the ego and the lead."""
    OPT, V, _, _ = _case(tree, N, paramEstSetting=est, TVestSetting=est)
    _against_oracle(OPT, V, _s1(tree, 4 if N == 63 else 6, seed=100 + N))


def test_blocked_moves_vs_oracle():
    OPT, V, _, _ = _case("ABO", 20, Mb=np.array(MB20))
    eng = _engine(OPT, V)
    assert eng.ab_qp_size() == (100, 14 * 20 + 2 + sum(MB20))
    _against_oracle(OPT, V, _s1("ABO", 6), eng)
    OPT, V, _, _ = _case("ORIG", 20, Mb=np.array(MB20))
    _against_oracle(OPT, V, _s1("ORIG", 3))


def test_variable_time_steps_vs_oracle():
    """Geometric Tvec (the commented option of ABO/Settings.m:120-121): the sums of Ss and d in the reference's order."""
    N = 24
    OPT, V, _, _ = _case("ABO", N, Tvec=0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1)))
    _against_oracle(OPT, V, _s1("ABO", 6))
    OPT, V, _, _ = _case("ORIG", N, Tvec=0.5 * (1.5 / 0.5) ** (np.arange(N) / (N - 1)), paramEstSetting=0, TVestSetting=0)
    _against_oracle(OPT, V, _s1("ORIG", 3))


def test_ice_map_vs_oracle():
    OPT, V, _, _ = _case("ABO", 33, **ICE)
    _against_oracle(OPT, V, _s1("ABO", 6))


def test_route_features_vs_oracle():
    """Speed-limit steps, curves, stops and traffic lights switched on: the four ORIG caps carry real bounds."""
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
    _against_oracle(OPT, V, c)


# ------------------------------------------------------------------------------------------------ 3, 6
def _round_trip(OPT, V, cols, tree, eng=None):
    """ab_step and build -> qp_solve_batched_dual (cold) on the same inputs, on a fresh handle; returns what test 6 reads."""
    eng = eng or _engine(OPT, V)
    q = eng.ab_build_qp(**cols)
    r = eng.qp_solve_batched_dual(q.H, q.g, q.A, q.lba, q.uba)
    out, sp, vp, status = eng.ab_step(**cols)
    o = out.cpu().numpy(); sp = sp.cpu().numpy(); vp = vp.cpu().numpy()
    x = r.x.cpu().numpy()
    H, g, A, lba, uba = _np(q)
    assert int(status.cpu().numpy().sum()) == 0
    assert int(r.status.cpu().numpy().sum()) == 0
    orig = tree == "ORIG"
    B, N = x.shape[0], eng.N
    T = np.asarray(OPT["Tvec"], dtype=np.float64)
    err = np.abs(x[:, 0] - o[OUT["a_qp"]]).max()
    print("a_qp %.3g" % err)
    assert err < 1e-9
    for j, n in enumerate(("xi_v", "xi_h", "xi_s", "xi_f")):
        err = np.abs(x[:, 1 + j] - o[OUT[n]]).max()
        print("%s %.3g" % (n, err))
        assert err < 1e-9, n
    cost = 0.5 * np.einsum("bi,bij,bj->b", x, H, x) + np.einsum("bi,bi->b", g, x)
    cerr = np.abs(cost - o[OUT["cost"]]) / (1 + np.abs(o[OUT["cost"]]))
    print("cost (relative) %.3g" % cerr.max())
    assert cerr.max() < (1e-6 if orig else 1e-8)
    s, v = rollout(x[:, 0:5 * N:5], cols["s"], cols["v"], T)
    print("s_pred %.3g v_pred %.3g" % (np.abs(s - sp).max(), np.abs(v - vp).max()))
    assert np.abs(s - sp).max() < (1e-6 if orig else 1e-8)
    assert np.abs(v - vp).max() < (1e-7 if orig else 1e-9)
    return dict(eng=eng, lam_a=r.lam_a.cpu().numpy(), ws_a=r.ws_a.cpu().numpy(), lba=lba, uba=uba)


ROUND_TRIPS = {
    "abo": ("ABO", 20, {}),
    "orig": ("ORIG", 20, {}),
    "abo_mb": ("ABO", 20, dict(Mb=np.array(MB20))),
    "orig_mb": ("ORIG", 20, dict(Mb=np.array(MB20))),
    "abo_ice": ("ABO", 20, ICE),
}
_solved = {}


def _solved_case(name):
    if name not in _solved:
        tree, N, kw = ROUND_TRIPS[name]
        OPT, V, _, _ = _case(tree, N, **kw)
        _solved[name] = _round_trip(OPT, V, _s1(tree, 24), tree)
    return _solved[name]


@pytest.mark.parametrize("name", sorted(ROUND_TRIPS))
def test_round_trip_against_the_structured_kernel(name):
    _solved_case(name)


def test_round_trip_shifted_previous_solution():
    """paramEstSetting = 2: one ab_step leaves its predictions in the handle; the build of the next step reads them, as the
    next ab_step does."""
    OPT, V, s_tv, v_tv = _case("ABO", 20, paramEstSetting=2)
    G = load_golden("abo_abmpc")
    ks = (40, 150, 333, 600, 869)
    eng = _engine(OPT, V)
    _, _, _, st = eng.ab_step(**_cols([golden_step_inputs(G, s_tv, v_tv, k) for k in ks]))
    assert int(st.cpu().numpy().sum()) == 0
    _round_trip(OPT, V, _cols([golden_step_inputs(G, s_tv, v_tv, k + 1) for k in ks]), "ABO", eng)


# ------------------------------------------------------------------------------------------------ 4
def test_build_has_no_side_effects(lead_trace):
    OPT, V, _, _ = _case("ABO", 20, paramEstSetting=2)
    B, n = 5, 12
    sc = make_s2(B, n, lead_trace["V_TO_2Hz"], seed=5)
    c = _s1("ABO", B)

    def loop(with_build):
        eng = _engine(OPT, V, 8)
        t1, s1 = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][:6], sc["v_tv"][:6])
        if with_build:
            eng.ab_build_qp(**c)
        t2, s2 = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"][6:], sc["v_tv"][6:], resume=True)
        eng.synchronize()
        return (np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()]), np.concatenate([s1.cpu().numpy(), s2.cpu().numpy()]))
    ta, sa = loop(False)
    tb, sb = loop(True)
    assert np.array_equal(ta, tb) and np.array_equal(sa, sb)
    assert np.isfinite(ta).all()


# ------------------------------------------------------------------------------------------------ 5
def test_instances_are_independent():
    OPT, V, _, _ = _case("ORIG", 20, Mb=np.array(MB20))
    eng = _engine(OPT, V)
    c = _s1("ORIG", 65)
    full = _np(eng.ab_build_qp(**c))
    again = _np(eng.ab_build_qp(**c))
    for a, b in zip(full, again):
        assert np.array_equal(a, b)
    for B in (1, 5):
        part = _np(eng.ab_build_qp(**{n: c[n][:B] for n in INS}))
        for a, b in zip(full, part):
            assert np.array_equal(a[:B], b), B
    perm = np.random.default_rng(0).permutation(65)
    shuffled = _np(eng.ab_build_qp(**{n: np.ascontiguousarray(c[n][perm]) for n in INS}))
    for a, b in zip(full, shuffled):
        assert np.array_equal(a[perm], b)
    assert all(np.isfinite(a).all() for a in full[:3])


# ------------------------------------------------------------------------------------------------ 6
@pytest.mark.parametrize("tree,mb", [("ABO", None), ("ORIG", None), ("ABO", MB20), ("ORIG", MB20)])
def test_row_catalogue_shape(tree, mb):
    OPT, V, _, _ = _case(tree, 20, **({} if mb is None else dict(Mb=np.array(mb))))
    eng = _engine(OPT, V, 2)
    nV, nC = eng.ab_qp_size()
    stage, typ = eng.ab_qp_rows()
    assert nV == 100 and nC == (18 if tree == "ORIG" else 14) * 20 + 2 + (sum(mb) if mb else 0)
    assert stage.shape == typ.shape == (nC,) and stage.dtype == typ.dtype == np.int32
    assert (np.diff(stage) >= 0).all() and stage[0] == 0 and list(stage[-2:]) == [20, 20]
    assert [AB_ROW_TYPES[t] for t in typ[-2:]] == ["safe1", "safe2"]
    assert typ.min() >= 0 and typ.max() < len(AB_ROW_TYPES)
    blocked = [int(k) for k in stage[typ == AB_ROW_TYPES.index("blocked")]]
    assert blocked == ([k for k in range(20) if mb[k]] if mb else [])
    assert ((typ == AB_ROW_TYPES.index("v_lim")).sum() == 20) == (tree == "ORIG")
    # the catalogue names the data: a row's type says which sides the built problem bounds
    c = _s1(tree, 2)
    q = eng.ab_build_qp(**c)
    lo = np.isfinite(q.lba.cpu().numpy()[0]); hi = np.isfinite(q.uba.cpu().numpy()[0])
    two, lower = {"s", "v", "blocked"}, {"xi_v", "xi_h", "xi_s", "xi_f", "a_min", "j_min", "v_inc"}
    for i in range(nC):
        n = AB_ROW_TYPES[typ[i]]
        want = (True, True) if n in two else (True, False) if n in lower else (False, True)
        if n == "s":
            want = (True, bool(np.isfinite(OPT["s_goal"])))             # Settings.m:143 has no goal: s_goal = inf
        assert (bool(lo[i]), bool(hi[i])) == want, (i, n)


@pytest.mark.parametrize("name", sorted(ROUND_TRIPS))
def test_multipliers_read_row_by_row(name):
    R = _solved_case(name)
    stage, typ = R["eng"].ab_qp_rows()
    ws, lam = R["ws_a"], R["lam_a"]
    assert ws.shape[1] == stage.size
    assert (lam[ws == 0] == 0.0).all()
    assert np.isfinite(R["lba"][ws == -1]).all()          # a row held at its lower side has one
    assert np.isfinite(R["uba"][ws == 1]).all()
    assert (ws != 0).any()
    # every held slack-bound row is one the catalogue calls a slack bound: held at the lower side, the only one it has
    for n in ("xi_v", "xi_h", "xi_s", "xi_f"):
        assert (ws[:, typ == AB_ROW_TYPES.index(n)] <= 0).all(), n


# ------------------------------------------------------------------------------------------------ 7
def test_refusals():
    import torch
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, EepaccError
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL
    OPT, V, _, _ = _case("ABO", 20)
    eng = _engine(OPT, V, 8)
    lib = eng.lib
    nV, nC = eng.ab_qp_size()
    B = 3
    f64 = dict(dtype=torch.float64, device="cuda")
    ins = [torch.zeros(B, **f64) for _ in range(7)]
    outs = [torch.empty(B * n, **f64) for n in (nV * nV, nV, nV * nC, nC, nC)]
    names = list(INS) + ["H", "g", "A", "lba", "uba"]
    for j, name in enumerate(names):                      # every buffer in turn, by name
        ptrs = [x.data_ptr() for x in ins + outs]
        ptrs[j] = None
        assert lib.eepacc_ab_build_qp(eng.h, B, *ptrs, None) == -1
        assert ("eepacc_ab_build_qp: %s is NULL" % name) == lib.eepacc_last_error().decode()
    ptrs = [x.data_ptr() for x in ins + outs]
    for bad in (9, -1):
        assert lib.eepacc_ab_build_qp(eng.h, bad, *ptrs, None) == -1
        assert "B = %d" % bad in lib.eepacc_last_error().decode()
    with pytest.raises(EepaccError, match="max_batch"):
        eng.ab_build_qp(**_s1("ABO", 9))
    assert lib.eepacc_ab_build_qp(eng.h, 0, *([None] * 12), None) == 0
    q = eng.ab_build_qp(*[np.zeros(0)] * 7)
    assert q.H.shape == (0, nV, nV) and q.A.shape == (0, nC, nV) and q.lba.shape == (0, nC)
    n1, n2 = C.c_int(), C.c_int()
    assert lib.eepacc_ab_qp_size(eng.h, None, C.byref(n2)) == -1 and "nV" in lib.eepacc_last_error().decode()
    assert lib.eepacc_ab_qp_rows(eng.h, None, None) == -1 and "stage" in lib.eepacc_last_error().decode()
    cls = Engine.from_classes([OPT], [V], max_batch=8)
    cls.set_classes(np.zeros(B, dtype=np.int32))
    bl = _engine(Settings_BL(OPT), V, 8)
    for e, word in ((cls, "eepacc_create_classes"), (bl, "bl_mode = 1")):
        assert lib.eepacc_ab_build_qp(e.h, B, *ptrs, None) == -4
        assert word in lib.eepacc_last_error().decode()
        assert lib.eepacc_ab_qp_size(e.h, C.byref(n1), C.byref(n2)) == -4
        with pytest.raises(EepaccError):
            e.ab_qp_rows()
    torch.cuda.synchronize()
