"""eepacc_fb_step_est, eepacc_fb_build_qp_est and eepacc_run_fbmpc_preview: FBMPC with the horizon guesses supplied by the
caller.  Inputs: tests/fb_est_cases.py (tests/test_fb_est_cpu.py proves off the GPU what they are and that the oracle solves the
problem of every instance).

f1   the built problem against the oracle's CreateQP_FB + condensing on the same arrays (bars of test_gpu_fb_build.py::_compare),
     every configuration, and on a dense-path handle with Mb
f2   the step against the built problem solved by the dense QP operator (bars of
     test_gpu_fb_build.py::test_round_trip_against_the_structured_kernel), cold and on stale codes; status 0 everywhere
f3   all three arrays NULL: bit for bit eepacc_fb_step / eepacc_fb_build_qp, the two entries alternating, mode 2 included
f4   one side supplied, the other estimated: equals the call with both sides supplied (bars of f2; bit equality reported)
f5   the carried model entry after a step: made of the supplied v_est[N-1] (4 ulp of the entry)
f6   preview loop against a host loop of eepacc_fb_step_est fed scenarios.lead_preview; the bar is the larger of the _compare_fb
     bars of test_gpu_fb.py and twice the distance measured between run_fbmpc and a loop of fb_step on the same inputs
f7   one preview launch against two resumed launches, bit for bit (inside f6's loop over the cases)
f8   constant-speed lead with TVestSetting = 0: preview loop against run_fbmpc
f9   refusals
f10  instances are independent
Row N_hor of s_tv_est is handed over as NaN throughout: it is not read.

Figures of f6 (MI355X, multiples of the _compare_fb bars, largest over the cases): run_fbmpc against a loop of fb_step
s 2.8e-6, v 4.4e-6, xi_v 3.6e-6, F 1.8e-7, cost 1.5e-6; run_fbmpc_preview against a loop of fb_step_est s 4.3e-6, v 1.4e-5,
xi_v 1.4e-5, F 8.2e-7, cost 1.1e-6.
"""
import numpy as np
import pytest

import fb_est_cases as E
import stage_ref
from bl_est_cases import braking_lead
from conftest import make_case
from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.scenarios import lead_preview

pytestmark = pytest.mark.gpu

MB20 = [0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 1, 0, 0, 1, 1, 1, 0, 0, 1]          # that of test_gpu_fb_build.py
FB_TOL = dict(s=1e-8, v=1e-9, a=1e-9, xi_v=1e-9, xi_h=1e-9, xi_s=1e-9, xi_f=1e-9, DistHor=1e-8)      # tests/test_gpu_fb.py
_cache = {}


def _engine(OPT, V, max_batch=8):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _np(xs):
    return [x.cpu().numpy() for x in xs]


def _fb_args(c):
    z = np.zeros_like(c["s"])
    return (c["s"], c["v"], z, c["a_prev"], z, z, c["t0"], c["s_tv"], c["v_tv"], c["a_tv_prev"])


def _step(eng, c, **sup):
    out, sp, vp, st = eng.fb_step_est(*_fb_args(c), **sup)
    return dict(out=out.cpu().numpy(), s_pred=sp.cpu().numpy(), v_pred=vp.cpu().numpy(), status=st.cpu().numpy())


def _plain(eng, c):
    out, sp, vp, st = eng.fb_step(*_fb_args(c))
    return dict(out=out.cpu().numpy(), s_pred=sp.cpu().numpy(), v_pred=vp.cpu().numpy(), status=st.cpu().numpy())


def _compare_problem(q, i, r, what):
    """test_gpu_fb_build.py::_compare"""
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


# ------------------------------------------------------------------------------------------------ f1
@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_built_problem_against_the_oracle(cfg):
    OPT, V = E.settings(cfg)
    cols = E.inputs(cfg)
    q = _np(_engine(OPT, V).fb_build_qp_est(**cols, **E.device_arrays(cfg), want_model=True))
    _, probs = E.oracle_problems(cfg)
    assert len(probs) == E.B == q[0].shape[0]
    for i, r in enumerate(probs):
        _compare_problem(q, i, r, cfg)
        # the model that went into the problem: the last bit of the entry made in this step may differ (header)
        assert np.abs(q[5][:, i] - r["A22"]).max() <= 4 * np.spacing(1.0) and np.abs(q[6][:, i] - r["D2"]).max() <= 4 * np.spacing(np.abs(r["D2"]).max())
    assert np.isposinf(q[4][E.B - 1]).any() and np.isposinf(q[4][E.B - 2]).any()


def test_built_problem_on_a_dense_path_handle():
    """Mb: the handle's FBMPC steps go through the dense path; the builder entry serves it.  The rows of the blocked moves apart,
    the problem is that of the abo20 configuration on the same arrays."""
    OPT, V = E.settings("abo20")
    cols = E.inputs("abo20")
    eng = _engine(dict(OPT, Mb=np.array(MB20)), V)
    q = _np(eng.fb_build_qp_est(**cols, **E.device_arrays("abo20")))
    stage, typ = eng.fb_qp_rows()
    from eepacc_mpc_casadi_matlab_amd._abi import FB_ROW
    keep = (typ != FB_ROW["blocked_fm"]) & (typ != FB_ROW["blocked_fb"])
    assert int((~keep).sum()) == 2 * sum(MB20)
    _, probs = E.oracle_problems("abo20")
    for i, r in enumerate(probs):
        _compare_problem((q[0], q[1], q[2][:, keep], q[3][:, keep], q[4][:, keep]), i, r, "abo20 with Mb")
    assert (q[3][:, ~keep] == 0.0).all() and (q[4][:, ~keep] == 0.0).all()


# ------------------------------------------------------------------------------------------------ f2
def _solved(cfg):
    """The built problem of the configuration on the supplied arrays, solved by the dense QP operator (computed once)"""
    if cfg not in _cache:
        OPT, V = E.settings(cfg)
        eng = _engine(OPT, V)
        q = eng.fb_build_qp_est(**E.inputs(cfg), **E.device_arrays(cfg))
        x, cost, status = eng.qp_solve_batched(q.H, q.g, q.A, q.lba, q.uba)
        H, g = q.H.cpu().numpy(), q.g.cpu().numpy()
        x = x.cpu().numpy()
        obj = 0.5 * np.einsum("bi,bij,bj->b", x, H, x) + np.einsum("bi,bi->b", g, x)
        _cache[cfg] = dict(x=x, obj=obj, status=status.cpu().numpy())
    return _cache[cfg]


def _against_the_solved_problem(cfg, R, res, what, idx=None):
    """bars of test_gpu_fb_build.py::test_round_trip_against_the_structured_kernel"""
    idx = np.arange(E.B) if idx is None else idx
    x, obj, o = R["x"][idx], R["obj"][idx], res["out"]
    print("%s %s status: operator %s, fb_step_est %s" % (cfg, what, R["status"][idx], res["status"]))
    assert int(np.abs(R["status"]).sum()) == 0 and int(np.abs(res["status"]).sum()) == 0, (cfg, what)
    Fr = o[OUT["Fm"]] + o[OUT["Fb"]]
    ftol = 1e-6 + 1e-8 * np.abs(Fr).max()
    eFm, eFb = np.abs(x[:, 0] - o[OUT["Fm"]]).max(), np.abs(x[:, 1] - o[OUT["Fb"]]).max()
    print("%s %s: Fm %.3g Fb %.3g (bar %.3g)" % (cfg, what, eFm, eFb, ftol))
    assert eFm < ftol and eFb < ftol, (cfg, what, eFm, eFb)
    for j, n in enumerate(("xi_v", "xi_h", "xi_s", "xi_f")):
        err = np.abs(x[:, 2 + j] - o[OUT[n]]).max()
        rel = 1e-11 * np.abs(o[OUT[n]]).max() if n == "xi_f" else 0.0
        print("%s %s: %s %.3g" % (cfg, what, n, err))
        assert err < 1e-9 + rel, (cfg, what, n, err)
    cerr = np.abs(obj - o[OUT["cost"]]).max() / np.abs(o[OUT["cost"]]).max()
    print("%s %s: cost (relative) %.3g" % (cfg, what, cerr))
    assert cerr < 1e-9, (cfg, what, cerr)


@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_step_against_the_built_problem(cfg):
    OPT, V = E.settings(cfg)
    cols, sup = E.inputs(cfg), E.device_arrays(cfg)
    R = _solved(cfg)
    _against_the_solved_problem(cfg, R, _step(_engine(OPT, V), cols, **sup), "cold")
    # stale codes: first a step on another instance's state and arrays in the same slot (the table's own, rotated by one).  That
    # step moves the handle's step counter and model on, so the reference of the second step is the problem built for step 1 on
    # this handle's carried model (entry 0 made by the first step, entry 1 made now of the supplied v_est[N-1]).
    eng = _engine(OPT, V)
    rot = np.roll(np.arange(E.B), 1)
    first = _step(eng, E.take(cols, rot), **E.device_arrays(cfg, rot))
    assert int(np.abs(first["status"]).sum()) == 0
    q = eng.fb_build_qp_est(**cols, **sup)                               # step 1 of this handle: its carried model
    x, cost, status = eng.qp_solve_batched(q.H, q.g, q.A, q.lba, q.uba)
    H, g, x = q.H.cpu().numpy(), q.g.cpu().numpy(), x.cpu().numpy()
    R1 = dict(x=x, obj=0.5 * np.einsum("bi,bij,bj->b", x, H, x) + np.einsum("bi,bi->b", g, x), status=status.cpu().numpy())
    _against_the_solved_problem(cfg, R1, _step(eng, cols, **sup), "stale codes")


# ------------------------------------------------------------------------------------------------ f3
@pytest.mark.parametrize("cfg,mode", [("abo20", None), ("orig33", None), ("abo3", None), ("abo20", 2), ("grade20", None)])
def test_null_arrays_are_the_estimators(cfg, mode):
    OPT, V = E.settings(cfg)
    if mode is not None:
        OPT = dict(OPT, paramEstSetting=mode)
    cols = E.inputs(cfg)
    a, b = _engine(OPT, V), _engine(OPT, V)

    def same_state():
        qa, qb = a.fb_build_qp(**cols, want_model=True), b.fb_build_qp(**cols, want_model=True)    # model, predictions (mode 2), step counter
        for x, y in zip(qa, qb):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    for k in range(3):                                                   # later steps start from the carried codes and model
        for x, y in zip(a.fb_build_qp_est(**cols, want_model=True), b.fb_build_qp(**cols, want_model=True)):
            assert np.array_equal(x.cpu().numpy(), y.cpu().numpy()), (cfg, k)
        ra = _step(a, cols) if k != 1 else _plain(a, cols)               # the two entries alternate on handle a
        rb = _plain(b, cols)
        for n in ("out", "s_pred", "v_pred", "status"):
            assert np.array_equal(ra[n], rb[n], equal_nan=True), (cfg, k, n)
        assert not ra["status"].any()
        same_state()
    # the working-set codes are not visible through the builder: one more step on each shows them equal
    ra, rb = _step(a, cols), _step(b, cols)
    for n in ("out", "s_pred", "v_pred", "status"):
        assert np.array_equal(ra[n], rb[n], equal_nan=True), (cfg, n)


# ------------------------------------------------------------------------------------------------ f4
@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    import cfg_harness
    import stage_harness
    return stage_harness.load(str(tmp_path_factory.mktemp("stage_harness"))), cfg_harness.load(str(tmp_path_factory.mktemp("cfg_harness")))


@pytest.mark.parametrize("cfg,mode", [("abo20", 0), ("abo20", 1), ("orig33", 1)])
def test_one_side_supplied(cfg, mode, harnesses):
    """Only s_tv_est, and only s_est / v_est: each equals the call in which the other side holds the device's own estimate."""
    H, CH = harnesses
    tree, N, _ = E.CONFIGS[cfg]
    OPT, V = E.settings(cfg)
    OPT = dict(OPT, paramEstSetting=mode, TVestSetting=mode)
    built = CH.build(OPT, V)
    assert built.rc == 0, built.msg
    cols = E.inputs(cfg)
    B = E.B
    lane = np.repeat(np.arange(N + 1), B)
    rep = lambda a: np.tile(a, N + 1)
    se, ve = H.estimate(built.cfg, mode, OPT["tConstACC_ego"], rep(cols["s"]), rep(cols["v"]), rep(cols["a_prev"]), lane)
    st, _ = H.estimate(built.cfg, mode, OPT["tConstACC_tar"], rep(cols["s_tv"]), rep(cols["v_tv"]), rep(cols["a_tv_prev"]), lane)
    own = dict(s_est=se.reshape(N + 1, B), v_est=ve.reshape(N + 1, B), s_tv_est=st.reshape(N + 1, B))
    sup = E.device_arrays(cfg)
    for what, part, full in (("lead only", dict(s_tv_est=sup["s_tv_est"]), dict(s_est=own["s_est"], v_est=own["v_est"], s_tv_est=sup["s_tv_est"])),
                             ("ego only", dict(s_est=sup["s_est"], v_est=sup["v_est"]), dict(s_est=sup["s_est"], v_est=sup["v_est"], s_tv_est=own["s_tv_est"]))):
        a, b = _step(_engine(OPT, V), cols, **part), _step(_engine(OPT, V), cols, **full)
        assert not a["status"].any() and not b["status"].any(), (cfg, what)
        equal = all(np.array_equal(a[n], b[n]) for n in ("out", "s_pred", "v_pred"))
        print("%s mode %d, %s: %s" % (cfg, mode, what, "bit-equal" if equal else "not bit-equal"))
        o, r = a["out"], b["out"]
        Fr = r[OUT["Fm"]] + r[OUT["Fb"]]
        ftol = 1e-6 + 1e-8 * np.abs(Fr).max()
        assert np.abs(o[OUT["Fm"]] - r[OUT["Fm"]]).max() < ftol and np.abs(o[OUT["Fb"]] - r[OUT["Fb"]]).max() < ftol, (cfg, what)
        for n in ("xi_v", "xi_h", "xi_s", "xi_f"):
            rel = 1e-11 * np.abs(r[OUT[n]]).max() if n == "xi_f" else 0.0
            assert np.abs(o[OUT[n]] - r[OUT[n]]).max() < 1e-9 + rel, (cfg, what, n)
        assert np.abs(o[OUT["cost"]] - r[OUT["cost"]]).max() < 1e-9 * np.abs(r[OUT["cost"]]).max(), (cfg, what)


# ------------------------------------------------------------------------------------------------ f5
@pytest.mark.parametrize("cfg", ["abo20", "orig33", "grade20"])
def test_carried_model_entry_is_made_of_the_supplied_guess(cfg):
    """The bar is 4 ulp of the carried entry, A22 and D2 alike.  D2 = T / lm (za v^2 - zeta_rg) is a difference of air drag and
    rolling / grade resistance, which cancel at v_c = sqrt(zeta_rg / za) (14.5 m/s on the flat route, 28.4 m/s on the grade).
    The step kernels contract products into fused multiply-adds and numpy does not, so the two sides differ by roundings at the
    size of the terms; near v_c that is many ulps of the difference.  The guesses of this test are free, so v_est[N-1] is put
    away from v_c: 0.3 to 0.44 v_c on three instances and 2.0 to 2.54 v_c on the other three, another value at every step.  There
    the larger term is at most 1.33 times the difference, and every contraction the compiler may choose for za v v - zeta_rg and
    c_r cos + sin stays within 2 ulp of numpy's D2 (exact rational arithmetic, all combinations); 4 ulp is asserted.
    A fourth step on the table's own v_est + 0.25, which comes within a per cent of v_c on one instance, is printed and not
    asserted: there the last bits of the terms show as up to 21 ulp of D2 (abo20, instance 1)."""
    import math
    OPT, V = E.settings(cfg)
    za = V["zeta_a"]
    th = float(np.asarray(OPT["slope"], dtype=np.float64)[0])
    v_c = math.sqrt(V["m"] * V["g"] * (V["c_r"] * math.cos(th) + math.sin(th)) / za)
    cols, sup = E.inputs(cfg), E.device_arrays(cfg)
    N = E.CONFIGS[cfg][1]
    eng = _engine(OPT, V)
    factors = np.array([0.3, 0.35, 0.4, 2.0, 2.25, 2.5])
    for k in range(4):
        v_k = sup["v_est"].copy()
        if k < 3:
            v_k[N - 1] = v_c * (factors + 0.02 * k)
        else:
            v_k = v_k + 0.25
        _step(eng, cols, s_est=sup["s_est"], v_est=v_k, s_tv_est=sup["s_tv_est"])
        q = eng.fb_build_qp(**cols, want_model=True)
        A22, D2 = q.A22_used.cpu().numpy(), q.D2_used.cpu().numpy()
        worst = 0.0
        for i in range(E.B):
            wantA, wantD = E.model_step0(OPT, V, float(cols["v"][i]), v_k[:, i])       # entry 0 of this function: made of v_k[N-1]
            dA = abs(A22[k, i] - wantA[0]) / np.spacing(abs(wantA[0]))
            dD = abs(D2[k, i] - wantD[0]) / np.spacing(abs(wantD[0]))
            worst = max(worst, dD)
            if k < 3:
                assert dA <= 4 and dD <= 4, (cfg, k, i, dA, dD, D2[k, i], wantD[0])
        print("%s step %d%s: D2 entry against numpy, worst distance %.0f ulp of D2" % (cfg, k, "" if k < 3 else " (near v_c, not asserted)", worst))


# ------------------------------------------------------------------------------------------------ f6, f7
def _host_loop(OPT, V, s0, v0, am1, s_tv, v_tv, n_steps, preview):
    """eepacc_fb_step_est fed scenarios.lead_preview (preview) or eepacc_fb_step, closed by the plant of tests/stage_ref.py
    (measurement block RunOpt_FBMPC.m:161-191).  The step operator has no previous speed and reports a = 0; the loop's
    a = (v - v_prev) / Ts (:316-318) is stated here."""
    eng = _engine(OPT, V)
    Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
    Ts, B = Tv[0], s0.size
    traj = np.zeros((n_steps, len(OUT), B)); status = np.zeros((n_steps, B), dtype=np.int32)
    s, v, a_prev, vtv_prev = s0.copy(), v0.copy(), am1.copy(), np.zeros(B)
    z = np.zeros(B)
    for k in range(n_steps):
        if k == 0:
            vtv, atv = np.zeros(B), np.zeros(B)
        else:
            u = traj[k - 1, OUT["Fm"]] + traj[k - 1, OUT["Fb"]]
            nxt = [stage_ref.plant_rk4(OPT, V, s[i], v[i], u[i]) for i in range(B)]
            s_new, v_new = np.array([x[0] for x in nxt]), np.array([x[1] for x in nxt])
            a_prev = (v_new - v) / Ts
            s, v = s_new, v_new
            vtv = v_tv[k].copy(); atv = (vtv - vtv_prev) / Ts; vtv_prev = vtv
        args = (s, v, z, a_prev, z, z, np.full(B, k * Ts), s_tv[k].copy(), vtv, atv)
        if preview:
            st_est = lead_preview(s_tv, v_tv, k, Tv); st_est[-1] = np.nan
            out, _, _, st = eng.fb_step_est(*args, s_tv_est=st_est, want_pred=False)
        else:
            out, _, _, st = eng.fb_step(*args, want_pred=False)
        traj[k] = out.cpu().numpy(); status[k] = st.cpu().numpy()
        traj[k, OUT["a"]] = a_prev if k > 0 else 0.0
    return traj, status


FIELDS = ("s", "v", "a", "xi_v", "xi_h", "xi_s", "xi_f", "DistHor", "F", "Fm", "Fb", "cost")


def _distance(t, st, r, rst):
    """Per field of _compare_fb, the distance of two loops [steps, fields, B] as a multiple of that field's _compare_fb bar, the
    largest over the instances.  As _compare_fb does, an instance is compared up to the first step on which a QP fails (status
    1: a measured speed below zero after the stop behind the standing lead, the hard row v_0 >= 0 of CreateQP_FB.m:315); both
    loops must fail on that same step, after which each applies its own last iterate.  Returns the distances and the compared
    steps per instance."""
    worst, steps = {n: 0.0 for n in FIELDS}, []
    for i in range(t.shape[2]):
        bad = (st[:, i] != 0) | (rst[:, i] != 0)
        n = int(np.argmax(bad)) if bad.any() else len(bad)
        if bad.any():
            assert st[n, i] != 0 and rst[n, i] != 0, ("exit flags differ at the first failing step", i, n, st[n, i], rst[n, i])
        steps.append(n)
        assert n >= 10, (i, n)
        for k, x in _distance_one(t[:n, :, i], r[:n, :, i]).items():
            worst[k] = max(worst[k], x)
    return worst, steps


def _distance_one(t, r):
    d = {}
    for n in ("s", "v", "a", "xi_v", "xi_h", "xi_s", "xi_f", "DistHor"):
        rel = 1e-11 * np.abs(r[:, OUT[n]]).max() if n == "xi_f" else 0.0
        d[n] = np.abs(t[:, OUT[n]] - r[:, OUT[n]]).max() / (FB_TOL[n] + rel)
    Fr = r[:, OUT["Fm"]] + r[:, OUT["Fb"]]
    ftol = 1e-6 + 1e-8 * np.abs(Fr).max()
    d["F"] = np.abs(t[:, OUT["Fm"]] + t[:, OUT["Fb"]] - Fr).max() / ftol
    mv = r[:, OUT["v"]] > 1e-3
    d["Fm"] = np.abs(t[:, OUT["Fm"]] - r[:, OUT["Fm"]])[mv].max() / ftol if mv.any() else 0.0
    d["Fb"] = np.abs(t[:, OUT["Fb"]] - r[:, OUT["Fb"]])[mv].max() / ftol if mv.any() else 0.0
    d["cost"] = np.abs(t[:, OUT["cost"]] - r[:, OUT["cost"]]).max() / (1e-9 * np.abs(r[:, OUT["cost"]]).max())
    return d


@pytest.mark.parametrize("name,N,tvec", [("uniform20", 20, False), ("uniform33", 33, False), ("geometric24", 24, True)])
def test_preview_loop_against_host_loop(name, N, tvec):
    over = dict(Tvec=0.5 * 3.0 ** (np.arange(N) / (N - 1)), paramEstSetting=0) if tvec else {}
    OPT, V, _, _ = make_case("ABO", N, **over)
    n_steps, B = 30, 3
    s_all, v_all = braking_lead(n_steps + N, B, 0.5)
    s0, v0, am1 = np.zeros(B), np.array([3.0, 6.0, 9.0]), np.zeros(B)
    # the parent's two entries on the same inputs: how far a launch of run_fbmpc is from a loop of fb_step
    base, bst = _engine(OPT, V).run_fbmpc(s0, v0, am1, s_all[:n_steps], v_all[:n_steps])
    base, bst = base.cpu().numpy(), bst.cpu().numpy()
    href, hst = _host_loop(OPT, V, s0, v0, am1, s_all[:n_steps], v_all[:n_steps], n_steps, preview=False)
    d0, n0 = _distance(base, bst, href, hst)
    print("%s: run_fbmpc against a loop of fb_step (steps compared per instance %s), multiples of the _compare_fb bars: " % (name, n0) +
          " ".join("%s %.3g" % (n, d0[n]) for n in FIELDS))
    for what, n_lead in (("n_lead = n_steps", n_steps), ("n_lead = n_steps + N", n_steps + N)):
        s_tv, v_tv = s_all[:n_lead], v_all[:n_lead]
        one, ost = _engine(OPT, V).run_fbmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=n_steps)
        one, ost = one.cpu().numpy(), ost.cpu().numpy()
        eng = _engine(OPT, V)
        h = 13
        t1, st1 = eng.run_fbmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=h)
        t2, st2 = eng.run_fbmpc_preview(s0, v0, am1, s_tv[h:], v_tv[h:], n_steps=n_steps - h, resume=True)
        two = np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()])
        assert np.array_equal(one, two) and np.array_equal(ost, np.concatenate([st1.cpu().numpy(), st2.cpu().numpy()])), (name, what)   # f7
        ref, rst = _host_loop(OPT, V, s0, v0, am1, s_tv, v_tv, n_steps, preview=True)
        d, nd = _distance(one, ost, ref, rst)
        print("%s, %s: preview launch against a loop of fb_step_est (steps compared per instance %s), multiples of the _compare_fb bars: "
              % (name, what, nd) + " ".join("%s %.3g" % (n, d[n]) for n in FIELDS))
        assert not np.array_equal(one[:, OUT["Fm"]], base[:, OUT["Fm"]])                  # the preview changes the drive
        for n in FIELDS:
            assert d[n] <= max(1.0, 2.0 * d0[n]), (name, what, n, d[n], d0[n])


# ------------------------------------------------------------------------------------------------ f8
def test_preview_of_a_constant_speed_lead_is_the_estimator():
    """v_tv = 8, Ts = 0.5, gap 24 on dyadic numbers with TVestSetting = 0.  The measurement block reports v_tv = 0 at step 0
    (RunOpt_FBMPC.m:161-172), so there the estimator guesses a standing lead while the preview sees it move: step 0 of both
    handles is eepacc_run_fbmpc's, and steps 1 .. 29 are resumed with the one loop and the other, where the guesses are the same
    trajectory (tests/test_gpu_ab_est.py, a5)."""
    OPT, V, _, _ = make_case("ABO", 20, TVestSetting=0)
    n, B = 30, 4
    v_tv = np.full((n + 20, B), 8.0)
    s_tv = 24.0 + 4.0 * np.arange(n + 20)[:, None] + np.zeros((1, B))
    s0, v0, am1 = np.zeros(B), np.array([2.0, 4.0, 6.0, 8.0]), np.zeros(B)
    a, b = _engine(OPT, V), _engine(OPT, V)
    res = []
    for eng, run in ((a, a.run_fbmpc), (b, None)):
        t0, st0 = eng.run_fbmpc(s0, v0, am1, s_tv[:1], v_tv[:1])
        if run is not None:
            t1, st1 = eng.run_fbmpc(s0, v0, am1, s_tv[1:n], v_tv[1:n], resume=True)
        else:
            t1, st1 = eng.run_fbmpc_preview(s0, v0, am1, s_tv[1:], v_tv[1:], n_steps=n - 1, resume=True)
        res.append((np.concatenate([t0.cpu().numpy(), t1.cpu().numpy()]), np.concatenate([st0.cpu().numpy(), st1.cpu().numpy()])))
    (ta, sa), (tb, sb) = res
    assert not sa.any() and not sb.any()
    print("constant-speed lead: preview loop against run_fbmpc: %s" % ("bit-equal" if np.array_equal(ta, tb) else "not bit-equal"))
    d, _ = _distance(tb, sb, ta, sa)
    print("multiples of the _compare_fb bars: " + " ".join("%s %.3g" % (n, d[n]) for n in FIELDS))
    for n in FIELDS:
        assert d[n] <= 1.0, (n, d[n])


# ------------------------------------------------------------------------------------------------ f9
def _refused(fn, code, *words):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    with pytest.raises(EepaccError) as e:
        fn()
    msg = str(e.value)
    assert ("libeepacc error %d:" % code) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _build_raw(e, B=1):
    """eepacc_fb_build_qp_est itself (Engine.fb_build_qp_est asks eepacc_fb_qp_size first, which has refusals of its own); the
    handle is checked before any buffer"""
    from eepacc_mpc_casadi_matlab_amd.engine import _check
    _check(e.lib.eepacc_fb_build_qp_est(e.h, B, *[None] * 19, None))


def test_refusals(monkeypatch):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV
    ENOTSUP, EINVAL = -4, -1
    OPT, V = E.settings("abo20")
    cols, sup = E.inputs("abo20"), E.device_arrays("abo20")
    B = E.B
    lead = (np.zeros((4, B)) + 50.0, np.zeros((4, B)))
    eng = _engine(OPT, V)
    lib = eng.lib
    step = lambda e: ("eepacc_fb_step_est", lambda: e.fb_step_est(*_fb_args(cols), **sup))
    build = lambda e: ("eepacc_fb_build_qp_est", lambda: _build_raw(e))
    run = lambda e: ("eepacc_run_fbmpc_preview", lambda: e.run_fbmpc_preview(cols["s"], cols["v"], cols["a_prev"], *lead))
    for e, word in ((Engine.from_classes([OPT], [V], max_batch=8), "eepacc_create_classes"),
                    (_engine(Settings_BL(OPT), V), "bl_mode = 1"), (_engine(Settings_TV(OPT), V), "bl_mode = 2")):
        for name, fn in (step(e), build(e), run(e)):
            _refused(fn, ENOTSUP, name, word)
    bq = np.array([185, 1.296e-20, 2.301, 2.5e-4, 0.003728, -0.000181])
    monkeypatch.setenv("EEPACC_FB_DENSE", "1")
    forced = _engine(OPT, V)
    monkeypatch.delenv("EEPACC_FB_DENSE")
    for e, word in ((_engine(dict(OPT, Mb=np.array(MB20)), V), "Mb[2]"), (_engine(dict(OPT, b_quadr=bq), V), "b_quadr(4)"),
                    (forced, "EEPACC_FB_DENSE=1")):
        for name, fn in (step(e), run(e)):
            _refused(fn, ENOTSUP, name, word, "dense path", "eepacc_fb_build_qp_est still builds")
        q = e.fb_build_qp_est(**cols, **sup)                             # the builder entry serves such a handle
        assert np.isfinite(q.H.cpu().numpy()).all()
    for name, fn in (("eepacc_fb_step_est", lambda: lib.eepacc_fb_step_est(eng.h, B, *[1] * 10, 1, None, None, *[1] * 4, None)),
                     ("eepacc_fb_build_qp_est", lambda: lib.eepacc_fb_build_qp_est(eng.h, B, *[1] * 7, None, 1, None, None, None, *[1] * 5, None, None, None))):
        assert fn() == EINVAL                                            # (refused before any pointer is read)
        msg = lib.eepacc_last_error().decode()
        assert name in msg and "s_est" in msg and "v_est" in msg
    with pytest.raises(ValueError, match="s_est and v_est"):
        eng.fb_step_est(*_fb_args(cols), s_est=sup["s_est"])
    big = {n: np.tile(cols[n], 2) for n in cols}
    _refused(lambda: eng.fb_step_est(*_fb_args(big)), EINVAL, "eepacc_fb_step_est", "max_batch")
    _refused(lambda: _build_raw(eng, 9), EINVAL, "eepacc_fb_build_qp_est", "max_batch")
    _refused(lambda: eng.run_fbmpc_preview(np.zeros(16), np.zeros(16), np.zeros(16), np.zeros((4, 16)) + 50.0, np.zeros((4, 16))),
             EINVAL, "eepacc_run_fbmpc_preview", "max_batch")
    _refused(lambda: eng.run_fbmpc_preview(cols["s"], cols["v"], cols["a_prev"], *lead, n_steps=5), EINVAL,
             "eepacc_run_fbmpc_preview", "n_lead = 4", "n_steps = 5")
    # a NULL required buffer, through the C-ABI itself
    t = eng.torch
    d = [eng._d(cols[n], B) for n in E.INS]
    out = t.empty((len(OUT), B), dtype=t.float64, device=eng.device); st = t.empty((B,), dtype=t.int32, device=eng.device)
    ten = [x.data_ptr() for x in (d[0], d[1], d[0], d[2], d[0], d[0], d[3], d[4], d[5], d[6])]
    rc = lib.eepacc_fb_step_est(eng.h, B, *ten, None, None, None, None, None, None, st.data_ptr(), None)
    assert rc == EINVAL and b"eepacc_fb_step_est: out is NULL" in lib.eepacc_last_error()
    nV, nC = eng.fb_qp_size()
    bufs = [t.empty(n, dtype=t.float64, device=eng.device) for n in (B * nV * nV, B * nV, B * nV * nC, B * nC, B * nC)]
    ptrs = [x.data_ptr() for x in bufs]; ptrs[3] = None
    rc = lib.eepacc_fb_build_qp_est(eng.h, B, *[x.data_ptr() for x in d], None, None, None, None, None, *ptrs, None, None, None)
    assert rc == EINVAL and b"eepacc_fb_build_qp_est: lba is NULL" in lib.eepacc_last_error()
    ptrs[3] = bufs[3].data_ptr()
    rc = lib.eepacc_fb_build_qp_est(eng.h, B, *[x.data_ptr() for x in d], None, None, None, bufs[3].data_ptr(), None, *ptrs, None, None, None)
    assert rc == EINVAL and b"eepacc_fb_build_qp_est: D2 is NULL" in lib.eepacc_last_error()
    rc = lib.eepacc_run_fbmpc_preview(eng.h, B, 4, 4, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, None, out.data_ptr(), st.data_ptr(), None)
    assert rc == EINVAL and b"eepacc_run_fbmpc_preview: NULL buffer" in lib.eepacc_last_error()
    assert lib.eepacc_fb_step_est(None, B, *[None] * 17, None) == EINVAL and b"NULL handle" in lib.eepacc_last_error()
    # B = 0 is nothing to do
    assert lib.eepacc_fb_step_est(eng.h, 0, *[None] * 17, None) == 0
    assert lib.eepacc_fb_build_qp_est(eng.h, 0, *[None] * 19, None) == 0
    assert lib.eepacc_run_fbmpc_preview(eng.h, 0, 4, 4, *[None] * 7, None) == 0
    # generate_lead_and_run(kind="fb", preview=True) keeps raising: the new path is Engine.run_fbmpc_preview
    from eepacc_mpc_casadi_matlab_amd import engine as en
    with pytest.raises(ValueError, match="preview"):
        en.generate_lead_and_run(OPT, kind="fb", preview=True)
    t.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ f10
@pytest.mark.parametrize("cfg", ["abo20", "orig33"])
def test_instances_are_independent(cfg):
    OPT, V = E.settings(cfg)
    cols, sup = E.inputs(cfg), E.device_arrays(cfg)
    perm = np.array([3, 5, 0, 4, 1, 2])
    full = _step(_engine(OPT, V), cols, **sup)
    shuf = _step(_engine(OPT, V), E.take(cols, perm), **E.device_arrays(cfg, perm))
    for n in ("out", "s_pred", "v_pred"):
        assert np.array_equal(full[n][:, perm], shuf[n]), (cfg, n)
    assert np.array_equal(full["status"][perm], shuf["status"])
    qa = _np(_engine(OPT, V).fb_build_qp_est(**cols, **sup))
    qb = _np(_engine(OPT, V).fb_build_qp_est(**E.take(cols, perm), **E.device_arrays(cfg, perm)))
    for x, y in zip(qa, qb):
        assert np.array_equal(x[perm], y), cfg
    n_steps, N = 12, E.CONFIGS[cfg][1]
    s_tv, v_tv = braking_lead(n_steps + N, E.B, 0.5)
    s0, v0, am1 = np.zeros(E.B), np.linspace(3.0, 9.0, E.B), np.zeros(E.B)
    ta, sa = _engine(OPT, V).run_fbmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=n_steps)
    tb, sb = _engine(OPT, V).run_fbmpc_preview(s0[perm], v0[perm], am1[perm], s_tv[:, perm], v_tv[:, perm], n_steps=n_steps)
    assert np.array_equal(ta.cpu().numpy()[:, :, perm], tb.cpu().numpy()) and np.array_equal(sa.cpu().numpy()[:, perm], sb.cpu().numpy())
