"""eepacc_ab_step_est, eepacc_ab_build_qp_est and eepacc_run_abmpc_preview: ABMPC with the horizon guesses supplied by the
caller.  Inputs: tests/ab_est_cases.py (tests/test_ab_est_cpu.py proves off the GPU what they are and that few are degenerate).

a1  the built problem against the oracle's CreateQP_AB + condensing on the same arrays (bars of tests/test_gpu_ab_build.py)
a2  the step against the certified optimum of the built problem: cold, on stale codes, with B = 5 (bars of
    tests/test_gpu_ab_cert.py: ab_cert_cases.BAR / COST_BAR)
a3  all three arrays NULL: bit for bit eepacc_ab_step / eepacc_ab_build_qp
a4  the device's own estimates supplied: eepacc_ab_step within the step bars of tests/test_gpu_ab.py (bit equality is reported)
a5  preview loop where the estimator's guess is the future exactly (constant-speed lead on dyadic numbers; no lead)
a6  preview loop on a lead that brakes to a stop and pulls away: the device loop against a host loop of eepacc_ab_step_est fed
    scenarios.lead_preview and closed by the plant of tests/stage_ref.py; one launch against two, bit for bit
a7  refusals
Row N_hor of s_tv_est is handed over as NaN throughout: it is not read.
"""
import numpy as np
import pytest

import ab_cert_cases as T
import ab_est_cases as E
import stage_ref
from conftest import make_case
from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.scenarios import lead_preview

pytestmark = pytest.mark.gpu

TOL = dict(s=1e-8, v=1e-9, Fm=1e-6, Fb=1e-6, a=1e-9, xi_v=1e-9, xi_h=1e-9, xi_s=1e-9, xi_f=1e-9, a_qp=1e-9)   # tests/test_gpu_ab.py
_cache = {}


def _engine(OPT, V, max_batch=16):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _sup(cfg, idx=None):
    """the supplied arrays of a configuration for the device: row N of s_tv_est is NaN"""
    se, ve, st = E.supplied(cfg)
    st = st.copy(); st[-1] = np.nan
    if idx is not None:
        se, ve, st = se[:, idx], ve[:, idx], st[:, idx]
    return dict(s_est=np.ascontiguousarray(se), v_est=np.ascontiguousarray(ve), s_tv_est=np.ascontiguousarray(st))


def _step(eng, cols, **sup):
    out, sp, vp, st = eng.ab_step_est(**cols, **sup)
    return dict(out=out.cpu().numpy(), s_pred=sp.cpu().numpy(), v_pred=vp.cpu().numpy(), status=st.cpu().numpy())


# ------------------------------------------------------------------------------------------------ a1
@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_built_problem_against_the_oracle(cfg):
    OPT, V = T.settings(cfg)
    _, cols = E.inputs(cfg)
    eng = _engine(OPT, V)
    H, g, A, lba, uba = [x.cpu().numpy() for x in eng.ab_build_qp_est(**cols, **_sup(cfg))]
    _, probs = E.oracle_problems(cfg)
    for i, r in enumerate(probs):
        eA = np.abs(A[i] - r["G"]).max() / 1e-13
        eH = np.abs(H[i] - r["H"]).max() / (1e-12 * np.abs(r["H"]).max())
        eg = np.abs(g[i] - r["c"]).max() / (1e-12 * np.abs(r["c"]).max())
        fin_all = np.concatenate([r["lb"][np.isfinite(r["lb"])], r["ub"][np.isfinite(r["ub"])]])
        btol = 1e-12 * max(1.0, np.abs(fin_all).max())
        eb = 0.0
        for mine, ref in ((lba[i], r["lb"]), (uba[i], r["ub"])):
            fin = np.isfinite(ref)
            assert np.array_equal(mine[~fin], ref[~fin]), (cfg, i)        # infinite entries: same place, same sign
            assert np.isfinite(mine[fin]).all(), (cfg, i)
            eb = max(eb, np.abs(mine[fin] - ref[fin]).max() / btol)
        print("%s instance %d: A %.3g, H %.3g, g %.3g, bounds %.3g (fractions of the bound)" % (cfg, i, eA, eH, eg, eb))
        assert eA <= 1.0 and eH <= 1.0 and eg <= 1.0 and eb <= 1.0, (cfg, i, eA, eH, eg, eb)


# ------------------------------------------------------------------------------------------------ a2
def _certified(cfg):
    if cfg in _cache:
        return _cache[cfg]
    tree, N, _ = T.CONFIGS[cfg]
    OPT, V = T.settings(cfg)
    names, cols = E.inputs(cfg)
    stage, typ = T.config_row_map(cfg)
    eng = _engine(OPT, V)
    q = eng.ab_build_qp_est(**cols, **_sup(cfg))
    r = eng.qp_solve_batched_dual(q.H, q.g, q.A, q.lba, q.uba)
    H, g, A, lba, uba = [np.ascontiguousarray(x.cpu().numpy()) for x in q]
    x0, st0 = r.x.cpu().numpy(), r.status.cpu().numpy()
    opt = []
    for i, nm in enumerate(names):
        start = x0[i]
        if st0[i] != 0:
            D, probs = E.oracle_problems(cfg)
            start, _, so = D.solve(probs[i])
            assert so["status"] == 0, (cfg, nm)
        R = T.certify(H[i], g[i], A[i], lba[i], uba[i], start, stage, typ, N, OPT)
        assert R["degenerate"] or (R["cert"]["pviol"] <= T.PVIOL_MAX and R["cert"]["stat"] <= T.STAT_MAX), (cfg, nm)
        opt.append(R)
    xs = np.stack([R["x"] for R in opt])
    Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
    s_ref, v_ref = T.rollout(xs[:, 0::5], cols["s"], cols["v"], Tv)
    C = dict(cfg=cfg, tree=tree, names=names, cols=cols, x=xs, s_ref=s_ref, v_ref=v_ref, f=np.array([R["f"] for R in opt]),
             degenerate=np.array([R["degenerate"] for R in opt]), settings=(OPT, V), problems=(H, g, A, lba, uba), opt=opt)
    _cache[cfg] = C
    return C


def distances(C, res, idx):
    """Largest distances of a step's results to the certified optima of the instances idx (tests/test_gpu_ab_cert.py)"""
    o = res["out"]
    ok = ~C["degenerate"][idx]
    x, f = C["x"][idx], C["f"][idx]
    d = dict(cost=float((np.abs(o[OUT["cost"]] - f) / (1 + np.abs(f))).max()))
    if ok.any():
        d["a"] = float(np.abs(o[OUT["a_qp"]] - x[:, 0])[ok].max())
        d["slack"] = float(max(np.abs(o[OUT[n]] - x[:, 1 + j])[ok].max() for j, n in enumerate(T.SLACK_BOUNDS)))
        d["s"] = float(np.abs(res["s_pred"] - C["s_ref"][:, idx])[:, ok].max())
        d["v"] = float(np.abs(res["v_pred"] - C["v_ref"][:, idx])[:, ok].max())
    return d


def _assert_within_bars(C, res, idx, what):
    assert int(np.abs(res["status"]).sum()) == 0, (C["cfg"], what, res["status"])
    d = distances(C, res, idx)
    print("%s %s: worst distances to x* " % (C["cfg"], what) + " ".join("%s %.2e" % kv for kv in sorted(d.items())))
    for n, e in d.items():
        bar = T.COST_BAR[C["tree"]] if n == "cost" else T.BAR[n]
        assert e <= bar, (C["cfg"], what, n, e)


@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_step_is_the_certified_optimum(cfg):
    C = _certified(cfg)
    OPT, V = C["settings"]
    n = len(C["names"])
    print("%s: %d cases, degenerate %d" % (cfg, n, int(C["degenerate"].sum())))
    assert int(C["degenerate"].sum()) <= E.MAX_DROPPED * n
    every = np.arange(n)
    _assert_within_bars(C, _step(_engine(OPT, V), C["cols"], **_sup(cfg)), every, "cold")
    # after a step on another problem in the same slot: the table's own states, rotated by one, through eepacc_ab_step
    eng = _engine(OPT, V)
    eng.ab_step(**T.take(C["cols"], np.roll(every, 1)))
    _assert_within_bars(C, _step(eng, C["cols"], **_sup(cfg)), every, "stale codes")
    five = np.arange(n - 5, n)                                           # a batch that is no multiple of 4, the +inf leads in it
    _assert_within_bars(C, _step(_engine(OPT, V), T.take(C["cols"], five), **_sup(cfg, five)), five, "B = 5")


# ------------------------------------------------------------------------------------------------ a3
@pytest.mark.parametrize("cfg", ["abo20", "orig33", "abo3"])
def test_null_arrays_are_the_estimators(cfg):
    OPT, V = T.settings(cfg)
    _, cols = E.inputs(cfg)
    a, b = _engine(OPT, V), _engine(OPT, V)
    for _ in range(2):                                                   # the second step starts from the carried codes
        ra = _step(a, cols)
        out, sp, vp, st = b.ab_step(**cols)
        for x, y in ((ra["out"], out), (ra["s_pred"], sp), (ra["v_pred"], vp), (ra["status"], st)):
            assert np.array_equal(x, y.cpu().numpy(), equal_nan=True)
    for x, y in zip(a.ab_build_qp_est(**cols), b.ab_build_qp(**cols)):
        assert np.array_equal(x.cpu().numpy(), y.cpu().numpy())
    # the two entry points alternate on one handle
    r1 = _step(a, cols); out, *_ = a.ab_step(**cols); r2 = _step(b, cols); out2, *_ = b.ab_step_est(**cols)
    assert np.array_equal(r1["out"], r2["out"]) and np.array_equal(out.cpu().numpy(), out2.cpu().numpy())


# ------------------------------------------------------------------------------------------------ a4
@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    import cfg_harness
    import stage_harness
    return stage_harness.load(str(tmp_path_factory.mktemp("stage_harness"))), cfg_harness.load(str(tmp_path_factory.mktemp("cfg_harness")))


@pytest.mark.parametrize("cfg,mode", [("abo20", 0), ("abo20", 1), ("orig33", 0), ("orig33", 1)])
def test_supplied_equals_computed(cfg, mode, harnesses):
    H, CH = harnesses
    tree, N, _ = T.CONFIGS[cfg]
    OPT, V = T.settings(cfg)
    OPT = dict(OPT, paramEstSetting=mode, TVestSetting=mode)
    built = CH.build(OPT, V)
    assert built.rc == 0, built.msg
    _, cols = E.inputs(cfg)
    B = cols["s"].size
    lane = np.repeat(np.arange(N + 1), B)
    rep = lambda a: np.tile(a, N + 1)
    se, ve = H.estimate(built.cfg, mode, OPT["tConstACC_ego"], rep(cols["s"]), rep(cols["v"]), rep(cols["a_prev"]), lane)
    st, _ = H.estimate(built.cfg, mode, OPT["tConstACC_tar"], rep(cols["s_tv"]), rep(cols["v_tv"]), rep(cols["a_tv_prev"]), lane)
    sup = dict(s_est=se.reshape(N + 1, B), v_est=ve.reshape(N + 1, B), s_tv_est=st.reshape(N + 1, B))
    got = _step(_engine(OPT, V), cols, **sup)
    out, sp, vp, status = _engine(OPT, V).ab_step(**cols)
    o = out.cpu().numpy()
    assert np.array_equal(got["status"], status.cpu().numpy()) and not got["status"].any()
    equal = np.array_equal(got["out"], o) and np.array_equal(got["s_pred"], sp.cpu().numpy()) and np.array_equal(got["v_pred"], vp.cpu().numpy())
    print("%s estimator mode %d: supplied estimates against computed ones: %s" % (cfg, mode, "bit-equal" if equal else "not bit-equal"))
    orig = tree == "ORIG"
    for n, tol in TOL.items():
        tol = 1e-5 if orig and n in ("Fm", "Fb") else tol                # tests/test_gpu_ab.py: forces to 1e-5 N in the ORIG tree
        err = np.abs(got["out"][OUT[n]] - o[OUT[n]]).max()
        assert err < tol, (cfg, mode, n, err)
    assert np.abs(got["s_pred"] - sp.cpu().numpy()).max() < (1e-6 if orig else 1e-8)
    assert np.abs(got["v_pred"] - vp.cpu().numpy()).max() < (1e-7 if orig else 1e-9)


# ------------------------------------------------------------------------------------------------ a5
@pytest.mark.parametrize("lead", ["constant_speed", "none"])
def test_preview_loop_where_the_guess_is_the_future(lead):
    """v_tv = 8, Ts = 0.5, gap 16 on dyadic numbers with TVestSetting = 0, and no lead at all: 40 steps of both loops.

    Without a lead the two loops are compared launch against launch.  With the constant-speed lead the premise (the
    estimator's guess is the future) does not hold at step 0: the measurement block reports v_tv = 0 there
    (RunOpt_ABMPC.m:159-172), so the estimator loop's first step guesses a standing lead while the preview sees it move, and the
    two launches differ from the first force on (measured: 1296 N at step 0, 3.68 m after 40 steps).  From step 1 on the premise
    holds.  So step 0 of both handles is eepacc_run_abmpc's, and steps 1 .. 39 are resumed with the one loop and the other: all
    40 rows are compared, within the bars the issue sets, and 39 of them are the preview kernel's."""
    OPT, V, _, _ = make_case("ABO", 20, TVestSetting=0)
    n_steps, B = 40, 3
    k = np.arange(n_steps + 20)[:, None]
    if lead == "constant_speed":
        v_tv = np.full((k.size, B), 8.0)
        s_tv = 16.0 + 4.0 * k + np.zeros((1, B))
    else:
        v_tv = np.zeros((k.size, B)); s_tv = np.full((k.size, B), np.inf)
    s0, v0, am1 = np.zeros(B), np.array([0.0, 0.5, 1.0]), np.zeros(B)
    ref, rst = _engine(OPT, V).run_abmpc(s0, v0, am1, s_tv[:n_steps], v_tv[:n_steps])
    eng = _engine(OPT, V)
    if lead == "constant_speed":
        g0, st0 = eng.run_abmpc(s0, v0, am1, s_tv[:1], v_tv[:1])
        g1, st1 = eng.run_abmpc_preview(s0, v0, am1, s_tv[1:], v_tv[1:], n_steps=n_steps - 1, resume=True)
        a = np.concatenate([g0.cpu().numpy(), g1.cpu().numpy()]); gst = np.concatenate([st0.cpu().numpy(), st1.cpu().numpy()])
    else:
        got, gst = eng.run_abmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=n_steps)
        a, gst = got.cpu().numpy(), gst.cpu().numpy()
    b = ref.cpu().numpy()
    for n in ("s", "v", "Fm", "Fb"):
        print("%s %s: %.3e" % (lead, n, np.abs(a[:, OUT[n]] - b[:, OUT[n]]).max()))
    assert np.array_equal(gst, rst.cpu().numpy())
    for n in ("s", "v", "Fm", "Fb"):
        err = np.abs(a[:, OUT[n]] - b[:, OUT[n]]).max()
        assert err < TOL[n], (lead, n, err)


# ------------------------------------------------------------------------------------------------ a6
def _braking_lead(n_rows, B, Ts):
    """a lead that brakes to a stop and pulls away again, one phase shift per instance"""
    t = Ts * np.arange(n_rows)[:, None] + 1.5 * np.arange(B)[None, :]
    v = np.clip(np.minimum(10.0 - 2.0 * (t - 6.0), 1.5 * (t - 16.0)), 0.0, 10.0)
    v = np.where(t < 6.0, 10.0, np.maximum(v, 0.0))
    s = 25.0 + Ts * np.concatenate([np.zeros((1, B)), np.cumsum(v[:-1], axis=0)])
    return np.ascontiguousarray(s), np.ascontiguousarray(v)


def _host_loop(OPT, V, s0, v0, am1, s_tv, v_tv, n_steps):
    """eepacc_ab_step_est fed scenarios.lead_preview, closed by the plant of tests/stage_ref.py (RunOpt_ABMPC.m:159-191)"""
    eng = _engine(OPT, V)
    Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
    Ts, B = Tv[0], s0.size
    traj = np.zeros((n_steps, len(OUT), B)); status = np.zeros((n_steps, B), dtype=np.int32)
    s, v, a_prev, vtv_prev = s0.copy(), v0.copy(), am1.copy(), np.zeros(B)
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
        st_est = lead_preview(s_tv, v_tv, k, Tv); st_est[-1] = np.nan
        out, _, _, st = eng.ab_step_est(s, v, a_prev, np.full(B, k * Ts), s_tv[k].copy(), vtv, atv, s_tv_est=st_est, want_pred=False)
        traj[k] = out.cpu().numpy(); status[k] = st.cpu().numpy()
    return traj, status


@pytest.mark.parametrize("name,N,tvec", [("geometric24", 24, True), ("uniform20", 20, False), ("uniform33", 33, False)])
def test_preview_loop_against_host_loop(name, N, tvec):
    over = dict(Tvec=0.5 * 3.0 ** (np.arange(N) / (N - 1)), paramEstSetting=0) if tvec else {}
    OPT, V, _, _ = make_case("ABO", N, **over)
    n_steps, B = 36, 3
    s_all, v_all = _braking_lead(n_steps + N, B, 0.5)
    s0, v0, am1 = np.zeros(B), np.array([3.0, 6.0, 9.0]), np.zeros(B)
    for what, n_lead in (("n_lead = n_steps", n_steps), ("n_lead = n_steps + N", n_steps + N)):
        s_tv, v_tv = s_all[:n_lead], v_all[:n_lead]
        one, ost = _engine(OPT, V).run_abmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=n_steps)
        one, ost = one.cpu().numpy(), ost.cpu().numpy()
        assert not ost.any(), (name, what)
        eng = _engine(OPT, V)
        h = 17
        t1, st1 = eng.run_abmpc_preview(s0, v0, am1, s_tv, v_tv, n_steps=h)
        t2, st2 = eng.run_abmpc_preview(s0, v0, am1, s_tv[h:], v_tv[h:], n_steps=n_steps - h, resume=True)
        two = np.concatenate([t1.cpu().numpy(), t2.cpu().numpy()])
        assert np.array_equal(one, two) and np.array_equal(ost, np.concatenate([st1.cpu().numpy(), st2.cpu().numpy()])), (name, what)
        ref, rst = _host_loop(OPT, V, s0, v0, am1, s_tv, v_tv, n_steps)
        assert not rst.any()
        for n in ("s", "v", "Fm", "Fb", "a", "xi_v", "xi_h", "xi_s", "xi_f"):
            err = np.abs(one[:, OUT[n]] - ref[:, OUT[n]]).max()
            print("%s, %s, %s: %.3e" % (name, what, n, err))
            assert err < 10 * TOL[n], (name, what, n, err)              # the closed-loop bars of test_closed_loop_s2_vs_oracle


# ------------------------------------------------------------------------------------------------ a7
def _refused(fn, code, *words):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    with pytest.raises(EepaccError) as e:
        fn()
    msg = str(e.value)
    assert ("libeepacc error %d:" % code) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def _build_raw(e):
    """eepacc_ab_build_qp_est itself (Engine.ab_build_qp_est asks eepacc_ab_qp_size first, which has refusals of its own); the
    handle is checked before any buffer"""
    from eepacc_mpc_casadi_matlab_amd.engine import _check
    _check(e.lib.eepacc_ab_build_qp_est(e.h, 1, *[None] * 15, None))


def test_refusals():
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL
    ENOTSUP, EINVAL = -4, -1
    OPT, V = T.settings("abo20")
    _, cols = E.inputs("abo20")
    sup = _sup("abo20")
    B = cols["s"].size
    lead = (np.zeros((4, B)) + 50.0, np.zeros((4, B)))
    eng = _engine(OPT, V)
    lib = eng.lib
    calls = lambda e: (("eepacc_ab_step_est", lambda: e.ab_step_est(**cols, **sup)),
                       ("eepacc_ab_build_qp_est", lambda: _build_raw(e)),
                       ("eepacc_run_abmpc_preview", lambda: e.run_abmpc_preview(cols["s"], cols["v"], cols["a_prev"], *lead)))
    kinds = [(Engine.from_classes([OPT], [V], max_batch=16), "eepacc_create_classes"),
             (_engine(dict(OPT, Mb=np.array(T.MB20)), V), "Mb[2]"),
             (_engine(*T.settings("abo20_ice")), "ab_fuel_term == 2")]
    kinds.append((_engine(Settings_BL(OPT), V), "bl_mode = 1"))
    for e, word in kinds:
        for name, fn in calls(e):
            _refused(fn, ENOTSUP, name, word)
    for name, fn in (("eepacc_ab_step_est", lambda: eng.ab_step_est(**cols, s_est=sup["s_est"])),
                     ("eepacc_ab_build_qp_est", lambda: eng.ab_build_qp_est(**cols, v_est=sup["v_est"]))):
        _refused(fn, EINVAL, name, "s_est", "v_est")
    big = {n: np.tile(cols[n], 2) for n in cols}
    _refused(lambda: eng.ab_step_est(**big), EINVAL, "eepacc_ab_step_est", "max_batch")
    _refused(lambda: eng.ab_build_qp_est(**big), EINVAL, "eepacc_ab_build_qp_est", "max_batch")
    _refused(lambda: eng.run_abmpc_preview(np.zeros(32), np.zeros(32), np.zeros(32), np.zeros((4, 32)) + 50.0, np.zeros((4, 32))),
             EINVAL, "eepacc_run_abmpc_preview", "max_batch")
    _refused(lambda: eng.run_abmpc_preview(cols["s"], cols["v"], cols["a_prev"], *lead, n_steps=5), EINVAL,
             "eepacc_run_abmpc_preview", "n_lead = 4", "n_steps = 5")
    # a NULL required buffer, through the C-ABI itself
    t = eng.torch
    d = [eng._d(cols[n], B) for n in T.INS]
    out = t.empty((len(OUT), B), dtype=t.float64, device=eng.device); st = t.empty((B,), dtype=t.int32, device=eng.device)
    rc = lib.eepacc_ab_step_est(eng.h, B, *[x.data_ptr() for x in d], None, None, None, None, None, None, st.data_ptr(), None)
    assert rc == EINVAL and b"eepacc_ab_step_est: NULL buffer" in lib.eepacc_last_error()
    nV, nC = eng.ab_qp_size()
    bufs = [t.empty(n, dtype=t.float64, device=eng.device) for n in (B * nV * nV, B * nV, B * nV * nC, B * nC, B * nC)]
    ptrs = [x.data_ptr() for x in bufs]; ptrs[3] = None
    rc = lib.eepacc_ab_build_qp_est(eng.h, B, *[x.data_ptr() for x in d], None, None, None, *ptrs, None)
    assert rc == EINVAL and b"eepacc_ab_build_qp_est: lba is NULL" in lib.eepacc_last_error()
    rc = lib.eepacc_run_abmpc_preview(eng.h, B, 4, 4, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), None, None, out.data_ptr(), st.data_ptr(), None)
    assert rc == EINVAL and b"eepacc_run_abmpc_preview: NULL buffer" in lib.eepacc_last_error()
    # B = 0 is nothing to do
    assert lib.eepacc_ab_step_est(eng.h, 0, *[None] * 14, None) == 0
    assert lib.eepacc_ab_build_qp_est(eng.h, 0, *[None] * 15, None) == 0
    assert lib.eepacc_run_abmpc_preview(eng.h, 0, 4, 4, *[None] * 7, None) == 0
