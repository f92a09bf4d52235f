"""Supplied horizon guesses on class handles: eepacc_classes_step_est and eepacc_run_classes_preview (kernels clsest for a
handle of eepacc_create_classes, blclsest for one of eepacc_create_classes_bl with bl_mode = 1), and
generate_lead_and_run_mix(preview=True).

The reference throughout is existing code: a plain single-class Engine per class running ab_step_est / bl_step_est /
run_abmpc_preview / run_blmpc_preview, themselves pinned against certified optima and host loops by tests/test_gpu_ab_est.py and
tests/test_gpu_bl_est.py.  The new kernels are the same source with the same flags and an instance's arithmetic depends on no
neighbour, so the bar is np.array_equal for traj, out, predictions, status and last_iterations: a difference means a value read
from the DevCfg of another class, or a supplied array read at another place, not rounding.

c1  preview closed loop, ABMPC      c2  the same for the baseline controller      c3  one launch against two, alternation
c4  step entry                      c5  all three arrays NULL                     c6  wrong-class sensitivity
c7  generate_lead_and_run_mix       c8  refusals                                  c9  determinism

On c4's "stale codes with the class map permuted between the two calls": eepacc_set_classes resets the handle's carried state
(include/eepacc.h), so codes cannot outlive a change of the map.  The test therefore has both halves: stale codes under an
unchanged map (a step on the neighbour's inputs in the same slot first) against plain engines doing the same, and a step under
a permuted map followed by eepacc_set_classes back to the map, which must give the cold result.
"""
import numpy as np
import pytest

import ab_cert_cases as T
import ab_est_cases as E
from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, SetVehicleParameters
from test_gpu_classes import _use_case, scenario
from test_gpu_classes_bl import _mixed, bl_route_classes, bl_solver_classes

pytestmark = pytest.mark.gpu

ENOTSUP, EINVAL = -4, -1
N_STEPS = 25
H_SPLIT = 11


def _single(OPT, V, max_batch=32):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


# ---- classes ------------------------------------------------------------------------------------------------------------
def ab_classes(N, tree):
    """Five ABMPC classes that differ in route (use cases 3, 6, 7, 12), weights, vehicle mass and estimator mode
    (paramEstSetting 1, 0 and 2)."""
    V = SetVehicleParameters(tree)
    uc = {c: _use_case(c, N, tree) for c in (3, 6, 7, 12)}
    w = np.ones(np.size(uc[6]["W_AB"])); w[:4] = [3.0, 0.5, 1.0, 2.0]
    OPTs = [uc[3], dict(uc[6], W_AB=np.asarray(uc[6]["W_AB"]) * w), uc[7], dict(uc[12], paramEstSetting=0, TVestSetting=0),
            dict(uc[3], paramEstSetting=2)]
    Vs = [V, V, dict(V, m=V["m"] + 350.0), V, V]
    assert sorted({int(o["paramEstSetting"]) for o in OPTs}) == [0, 1, 2]
    return OPTs, Vs


def bl_classes(which, N, tree):
    if which == "solver":
        OPTs, Vs = bl_solver_classes(N)
        keep = [0, 1, 2, 4, 5, 6, 9]        # reference weights, convex W_BL, bl_lp_eps, bl_prox_iter 40 and -1, mass, estimator 2
        return [OPTs[i] for i in keep], [Vs[i] for i in keep]
    OPTs, Vs = bl_route_classes(N, tree)
    OPTs, Vs = OPTs[:5], list(Vs[:5])
    Vs[2] = dict(Vs[2], m=Vs[2]["m"] + 300.0)
    return OPTs, Vs


def _scene(K, n_rows, lead_trace, seed, no_lead_class=1):
    """Two instances per class, interleaved (the waves of a block hold different classes; B = 2 K is no multiple of the 4 or 3
    waves of a block for the K used here), S2 leads from tight following to a free road, and one class without a lead."""
    sc = scenario(K, 2, n_rows, lead_trace, seed=seed)
    B = sc["class_of"].size
    assert B % 4 and B % 3
    none = sc["class_of"] == no_lead_class
    sc["s_tv"] = np.array(sc["s_tv"]); sc["v_tv"] = np.array(sc["v_tv"])
    sc["s_tv"][:, none] = np.inf; sc["v_tv"][:, none] = 0.0
    for a in (sc["s_tv"], sc["v_tv"]):
        a.setflags(write=False)
    return sc


def _pv(eng, entry, sc, n_steps, n_lead, idx=slice(None), row0=0, resume=False):
    """A preview launch of n_steps steps from row row0 of the scene's traces, which end at row n_lead."""
    rows = slice(row0, n_lead)
    traj, status = getattr(eng, entry)(sc["s0"][idx], sc["v0"][idx], sc["a_minus1"][idx], np.array(sc["s_tv"][rows, idx]),
                                       np.array(sc["v_tv"][rows, idx]), n_steps=n_steps, resume=resume)
    eng.synchronize()
    return traj.cpu().numpy(), status.cpu().numpy(), eng.last_iterations(sc["s0"][idx].size)


def _plain(eng, entry, sc, n_steps, idx, row0=0, resume=False):
    """The estimator loop (run_abmpc / run_blmpc) on rows row0 .. row0 + n_steps."""
    rows = slice(row0, row0 + n_steps)
    traj, status = getattr(eng, entry)(sc["s0"][idx], sc["v0"][idx], sc["a_minus1"][idx], np.array(sc["s_tv"][rows, idx]),
                                       np.array(sc["v_tv"][rows, idx]), resume=resume)
    eng.synchronize()
    return traj.cpu().numpy(), status.cpu().numpy(), eng.last_iterations(sc["s0"][idx].size)


def _equal_per_class(got, sc, refs, what):
    tr, st, it = got
    for k, (rt, rs, ri) in enumerate(refs):
        idx = np.nonzero(sc["class_of"] == k)[0]
        assert np.array_equal(tr[:, :, idx], rt, equal_nan=True), (what, "traj", k, float(np.nanmax(np.abs(tr[:, :, idx] - rt))))
        assert np.array_equal(st[:, idx], rs), (what, "status", k)
        assert np.array_equal(it[idx], ri), (what, "last_iterations", k)


_loops = {}


def closed_loop(kind, which, tree, N, lead_trace):
    """The scene, the mixed engine and the plain engines' preview loops of one configuration, for n_lead = n_steps and
    n_steps + N: computed once, read by c1 / c2, c3, c6 and c9 and left unchanged."""
    key = (kind, which, tree, N)
    if key in _loops:
        return _loops[key]
    OPTs, Vs = ab_classes(N, tree) if kind == "ab" else bl_classes(which, N, tree)
    sc = _scene(len(OPTs), N_STEPS + N, lead_trace, seed=31 + N)
    ref_entry = "run_abmpc_preview" if kind == "ab" else "run_blmpc_preview"
    plain = [_single(o, v) for o, v in zip(OPTs, Vs)]
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    L = dict(OPT=OPTs, V=Vs, sc=sc, eng=eng, plain=plain, ref_entry=ref_entry, ref={}, mixed={})
    for n_lead in (N_STEPS, N_STEPS + N):
        L["mixed"][n_lead] = _pv(eng, "run_classes_preview", sc, N_STEPS, n_lead)
        L["ref"][n_lead] = [_pv(p, ref_entry, sc, N_STEPS, n_lead, np.nonzero(sc["class_of"] == k)[0]) for k, p in enumerate(plain)]
        for a in L["mixed"][n_lead] + tuple(x for r in L["ref"][n_lead] for x in r):
            a.setflags(write=False)
    _loops[key] = L
    return L


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


# ------------------------------------------------------------------------------------------------ c1
@pytest.mark.parametrize("tree,N", [("ORIG", 20), ("ABO", 20), ("ORIG", 40), ("ABO", 33)])
def test_preview_closed_loop_abmpc(tree, N, torch_mod, lead_trace):
    L = closed_loop("ab", "route", tree, N, lead_trace)
    assert L["eng"].num_classes == 5
    for n_lead in (N_STEPS, N_STEPS + N):
        tr = L["mixed"][n_lead][0]
        lead = np.isfinite(L["sc"]["s_tv"][0])
        assert np.isfinite(tr[:, OUT["v"]]).all() and lead.sum() == 8
        _equal_per_class(L["mixed"][n_lead], L["sc"], L["ref"][n_lead], (tree, N, n_lead))
    # the future past the launch's rows is read: the two n_lead differ where a lead exists
    a, b = L["mixed"][N_STEPS][0], L["mixed"][N_STEPS + N][0]
    assert not np.array_equal(a[:, :, lead], b[:, :, lead]) and np.array_equal(a[:, :, ~lead], b[:, :, ~lead])


# ------------------------------------------------------------------------------------------------ c2
@pytest.mark.parametrize("which,tree,N", [("route", "ORIG", 20), ("route", "ABO", 20), ("route", "ORIG", 40), ("solver", "ORIG", 20)])
def test_preview_closed_loop_baseline(which, tree, N, torch_mod, lead_trace):
    L = closed_loop("bl", which, tree, N, lead_trace)
    assert all(int(o["bl_mode"]) == 1 for o in L["OPT"])
    if which == "solver":
        assert len({np.asarray(o["W_BL"]).tobytes() for o in L["OPT"]}) > 1
        assert len({float(o.get("bl_lp_eps", -7.0)) for o in L["OPT"]}) > 1 and len({int(o.get("bl_prox_iter", -7)) for o in L["OPT"]}) > 2
    for n_lead in (N_STEPS, N_STEPS + N):
        _equal_per_class(L["mixed"][n_lead], L["sc"], L["ref"][n_lead], (which, tree, N, n_lead))
    if which == "solver":                                               # the classes do differ in what they compute
        tr, c = L["mixed"][N_STEPS][0], L["sc"]["class_of"]
        assert len({tr[:, OUT["a"], c == k].tobytes() for k in range(len(L["OPT"]))}) >= 4


# ------------------------------------------------------------------------------------------------ c3
@pytest.mark.parametrize("kind,N", [("ab", 20), ("bl", 20), ("ab", 40)])
def test_one_launch_against_two_and_alternation(kind, N, torch_mod, lead_trace):
    L = closed_loop(kind, "route", "ORIG", N, lead_trace)
    sc, eng, h = L["sc"], L["eng"], H_SPLIT
    for n_lead in (N_STEPS, N_STEPS + N):
        one = L["mixed"][n_lead]
        p1 = _pv(eng, "run_classes_preview", sc, h, n_lead)
        p2 = _pv(eng, "run_classes_preview", sc, N_STEPS - h, n_lead, row0=h, resume=True)
        assert np.array_equal(np.concatenate([p1[0], p2[0]]), one[0], equal_nan=True), (kind, n_lead)
        assert np.array_equal(np.concatenate([p1[1], p2[1]]), one[1]), (kind, n_lead)
    # the estimator loop for h steps, then the preview on the same handle; the plain engines do the same
    n_lead = N_STEPS + N
    est_entry = "run_abmpc" if kind == "ab" else "run_blmpc"
    a1 = _plain(eng, est_entry, sc, h, slice(None))
    a2 = _pv(eng, "run_classes_preview", sc, N_STEPS - h, n_lead, row0=h, resume=True)
    for k, p in enumerate(L["plain"]):
        idx = np.nonzero(sc["class_of"] == k)[0]
        r1 = _plain(p, est_entry, sc, h, idx)
        r2 = _pv(p, L["ref_entry"], sc, N_STEPS - h, n_lead, idx, row0=h, resume=True)
        assert np.array_equal(a1[0][:, :, idx], r1[0], equal_nan=True) and np.array_equal(a1[1][:, idx], r1[1]), (kind, k)
        assert np.array_equal(a2[0][:, :, idx], r2[0], equal_nan=True) and np.array_equal(a2[1][:, idx], r2[1]), (kind, k)
        assert np.array_equal(a2[2][idx], r2[2]), (kind, k)
    # (the alternated loop is another loop than the preview's own: its first h steps had no preview)
    lead = np.isfinite(sc["s_tv"][0])
    assert not np.array_equal(a2[0][:, :, lead], L["mixed"][n_lead][0][h:][:, :, lead])


# ------------------------------------------------------------------------------------------------ c4
STEP_CONFIGS = list(E.CONFIGS) + ["abo24_tvec", "orig24_tvec"]


@pytest.mark.parametrize("cfg", ["abo24_tvec", "orig24_tvec"])
def test_geometric_configurations_are_what_they_are_called(cfg):
    Tv = np.asarray(T.settings(cfg)[0]["Tvec"])
    assert Tv.size == 24 and np.ptp(Tv) > 0.5


def _step_inputs(cfg):
    """names, step inputs and supplied arrays of a configuration: those of tests/ab_est_cases.py (lead acceleration reversing
    within the horizon, +inf from mid-horizon in column B - 2 of the batches of 12, +inf throughout in column B - 1), built by
    the same rule for the two geometric-Tvec configurations, which that module does not list; row N of s_tv_est is NaN."""
    tree, N, _ = T.CONFIGS[cfg]
    if cfg in E.CONFIGS:
        _, cols = E.inputs(cfg)
        se, ve, st = E.supplied(cfg)
    else:
        names, cols = T.cases(cfg)
        cols = T.take(cols, np.arange(min(12, len(names))))
        B = cols["s"].size
        Tv = np.asarray(T.settings(cfg)[0]["Tvec"], dtype=np.float64)
        rng = np.random.default_rng([E.SEED, N, int(tree == "ORIG"), 24])
        se = np.empty((N + 1, B)); ve = np.empty((N + 1, B)); st = np.empty((N + 1, B))
        se[0], ve[0], st[0] = cols["s"], cols["v"], cols["s_tv"]
        a_ego = rng.uniform(-1.5, 1.5, (N, B))
        a_lead = rng.uniform(0.3, 1.2, B) * min(1.0, 5.0 / Tv.sum())
        v_lead = cols["v_tv"].copy()
        for k in range(N):
            ve[k + 1] = np.maximum(ve[k] + Tv[k] * a_ego[k], 0.0)
            se[k + 1] = se[k] + Tv[k] * ve[k]
            st[k + 1] = st[k] + Tv[k] * v_lead
            v_lead = v_lead + Tv[k] * (a_lead if 2 * k < N else -a_lead)
        st[N // 2:, B - 2] = np.inf
        st[:, B - 1] = np.inf
    st = st.copy(); st[-1] = np.nan
    B = cols["s"].size
    assert np.isposinf(st[:-1, B - 1]).all() and (B < 8 or (np.isposinf(st[N // 2:-1, B - 2]).all() and np.isfinite(st[:N // 2, B - 2]).all()))
    if N >= 20:
        dd = np.diff(st[:-1, :B - 2], n=2, axis=0)
        assert (dd[:N // 2 - 1] > 0).any() and (dd[N // 2 + 1:] < 0).any()      # the lead's acceleration reverses in the horizon
    return cols, dict(s_est=np.ascontiguousarray(se), v_est=np.ascontiguousarray(ve), s_tv_est=np.ascontiguousarray(st))


def _step_classes(cfg, kind):
    """Three classes on the settings of a configuration: itself, other weights (ABMPC) or bl_lp_eps (baseline) with estimator
    mode 0, and another vehicle mass with the previous solution as the ego estimate (mode 2)."""
    OPT, V = T.settings(cfg)
    if kind == "bl":
        base = Settings_BL(OPT)
        base["Tvec"] = np.asarray(OPT["Tvec"], dtype=np.float64).copy()          # (the geometric grid, where the configuration has one)
        OPTs = [base, dict(base, bl_lp_eps=0.1, paramEstSetting=0), dict(base, paramEstSetting=2)]
    else:
        w = np.ones(np.size(OPT["W_AB"])); w[:4] = [3.0, 0.5, 1.0, 2.0]
        OPTs = [OPT, dict(OPT, W_AB=np.asarray(OPT["W_AB"]) * w, paramEstSetting=0), dict(OPT, paramEstSetting=2)]
    return OPTs, [V, V, dict(V, m=V["m"] + 350.0)]


def _take(cols, sup, idx):
    return T.take(cols, idx), {n: np.ascontiguousarray(a[:, idx]) for n, a in sup.items()}


def _np_step(res, eng, B):
    out, sp, vp, st = res
    eng.synchronize()
    return dict(out=out.cpu().numpy(), s_pred=sp.cpu().numpy(), v_pred=vp.cpu().numpy(), status=st.cpu().numpy(), iters=eng.last_iterations(B))


def _plain_step(eng, kind, cols, sup=None):
    """The plain handle's step: with supplied arrays ab_step_est / bl_step_est, without ab_step / eepacc_bl_step."""
    B = cols["s"].size
    if sup is not None:
        return _np_step((eng.bl_step_est if kind == "bl" else eng.ab_step_est)(**cols, **sup), eng, B)
    if kind == "bl":
        return _np_step(eng._step(eng.lib.eepacc_bl_step, [cols[n] for n in T.INS], True), eng, B)
    return _np_step(eng.ab_step(**cols), eng, B)


def _same_step(got, ref, idx, what):
    for n in ("out", "s_pred", "v_pred", "status", "iters"):
        assert np.array_equal(got[n][..., idx], ref[n], equal_nan=True), (what, n)


@pytest.mark.parametrize("kind", ["ab", "bl"])
@pytest.mark.parametrize("cfg", STEP_CONFIGS)
def test_step_entry(cfg, kind, torch_mod):
    cols, sup = _step_inputs(cfg)
    OPTs, Vs = _step_classes(cfg, kind)
    B, K = cols["s"].size, len(OPTs)
    every = np.arange(B)
    class_of = (every % K).astype(np.int32)
    plain = [_single(o, v) for o, v in zip(OPTs, Vs)]
    eng = _mixed(OPTs, Vs)
    eng.set_classes(class_of)
    # cold
    cold = _np_step(eng.classes_step_est(**cols, **sup), eng, B)
    print(cfg, kind, "steps that report a failure:", int((cold["status"] != 0).sum()), "of", B)
    refs = []
    for k, p in enumerate(plain):
        idx = every[class_of == k]
        refs.append(_plain_step(p, kind, *_take(cols, sup, idx)))
        _same_step(cold, refs[k], idx, (cfg, kind, "cold", k))
    # the second step in a row starts from the carried codes and, in the class with paramEstSetting 2, from the stored solution
    warm = _np_step(eng.classes_step_est(**cols, **sup), eng, B)
    for k, p in enumerate(plain):
        idx = every[class_of == k]
        _same_step(warm, _plain_step(p, kind, *_take(cols, sup, idx)), idx, (cfg, kind, "second step", k))
    # stale codes: the neighbour's inputs in the same slot first, through the plain step entry, then the supplied step
    eng.reset()
    roll = np.roll(every, 1)
    _plain_step(eng, kind, T.take(cols, roll))
    stale = _np_step(eng.classes_step_est(**cols, **sup), eng, B)
    for k, p in enumerate(plain):
        idx = every[class_of == k]
        p.reset()
        _plain_step(p, kind, T.take(cols, roll[idx]))
        _same_step(stale, _plain_step(p, kind, *_take(cols, sup, idx)), idx, (cfg, kind, "stale codes", k))
    # a step under a permuted map, then the map again (which resets the handle): the cold result
    perm = np.roll(class_of, 1)
    eng.set_classes(perm)
    other = _np_step(eng.classes_step_est(**T.take(cols, roll), **sup), eng, B)
    eng.set_classes(class_of)
    again = _np_step(eng.classes_step_est(**cols, **sup), eng, B)
    _same_step(again, cold, every, (cfg, kind, "after a permuted map"))
    assert other["out"].shape == cold["out"].shape
    # a smaller B after a larger one: the last five instances (the +inf leads among them), with their own classes
    five = every[B - 5:]
    eng.set_classes(class_of[five])
    small = _np_step(eng.classes_step_est(*[cols[n][five] for n in T.INS], **{n: np.ascontiguousarray(a[:, five]) for n, a in sup.items()}), eng, 5)
    for k in range(K):
        sel = np.nonzero(class_of[five] == k)[0]
        idx = every[class_of == k]
        pos = np.nonzero(np.isin(idx, five))[0]                          # where the class's reference holds these instances
        for n in ("out", "s_pred", "v_pred", "status", "iters"):
            assert np.array_equal(small[n][..., sel], refs[k][n][..., pos], equal_nan=True), (cfg, kind, "B = 5", k, n)


# ------------------------------------------------------------------------------------------------ c5
@pytest.mark.parametrize("kind", ["ab", "bl"])
@pytest.mark.parametrize("cfg", ["abo20", "orig33", "abo3"])
def test_null_arrays_are_the_class_handles_own_step(cfg, kind, torch_mod):
    cols, _ = _step_inputs(cfg)
    OPTs, Vs = _step_classes(cfg, kind)
    B = cols["s"].size
    class_of = (np.arange(B) % len(OPTs)).astype(np.int32)
    a, b = _mixed(OPTs, Vs), _mixed(OPTs, Vs)
    a.set_classes(class_of); b.set_classes(class_of)
    every = np.arange(B)
    for _ in range(2):                                                   # the second step starts from the carried state
        _same_step(_np_step(a.classes_step_est(**cols), a, B), _plain_step(b, kind, cols), every, (cfg, kind))
    # the two entries alternate on one handle
    r1 = _np_step(a.classes_step_est(**cols), a, B); r2 = _plain_step(a, kind, cols)
    r3 = _plain_step(b, kind, cols); r4 = _np_step(b.classes_step_est(**cols), b, B)
    _same_step(r1, r3, every, (cfg, kind, "alternating")); _same_step(r2, r4, every, (cfg, kind, "alternating"))


# ------------------------------------------------------------------------------------------------ c6
@pytest.mark.parametrize("kind", ["ab", "bl"])
def test_a_wrong_class_shows(kind, torch_mod, lead_trace):
    """The map rotated by one class: every instance is solved with its neighbour's settings, and the comparison of c1 / c2 sees
    it in at least one column (in fact in most)."""
    L = closed_loop(kind, "route", "ORIG", 20, lead_trace)
    sc, K = L["sc"], len(L["OPT"])
    eng = _mixed(L["OPT"], L["V"])
    eng.set_classes((sc["class_of"] + 1) % K)
    tr, st, it = _pv(eng, "run_classes_preview", sc, N_STEPS, N_STEPS)
    differs = [not np.array_equal(tr[:, :, np.nonzero(sc["class_of"] == k)[0]], L["ref"][N_STEPS][k][0], equal_nan=True) for k in range(K)]
    print(kind, "classes whose columns differ under the rotated map:", differs)
    assert any(differs)


# ------------------------------------------------------------------------------------------------ c7
@pytest.mark.parametrize("kind", ["ab", "bl"])
def test_generate_lead_and_run_mix_with_preview(kind, torch_mod):
    from eepacc_mpc_casadi_matlab_amd.engine import generate_lead_and_run_mix
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_use_case_mix
    cases = [2, 10, 5, 6]
    mix = make_use_case_mix(cases, 2, "ORIG", 20, n_steps=20, controller=kind)
    B = mix["class_of"].size
    res = generate_lead_and_run_mix(mix, kind=kind, preview=True)
    assert res[2].is_cuda and tuple(res[2].shape) == (20, B)
    traj, status, s_tv, v_tv = [x.cpu().numpy() for x in res]
    assert np.isfinite(traj).all()
    ten = mix["class_of"] == cases.index(10)
    assert np.array_equal(s_tv[:, ten], mix["s_tv"][:, ten]) and np.array_equal(v_tv[:, ten], mix["v_tv"][:, ten])
    # it is run_classes_preview on the traces it returns, n_lead = n_steps
    eng = _mixed(mix["OPT"], mix["V"])
    eng.set_classes(mix["class_of"])
    want, wst = eng.run_classes_preview(mix["s0"], mix["v0"], mix["a_minus1"], s_tv, v_tv)
    assert tuple(want.shape) == traj.shape
    assert np.array_equal(traj, want.cpu().numpy()) and np.array_equal(status, wst.cpu().numpy())
    # preview=False and the default are today's call
    plain = [x.cpu().numpy() for x in generate_lead_and_run_mix(mix, kind=kind, preview=False)]
    default = [x.cpu().numpy() for x in generate_lead_and_run_mix(mix, kind=kind)]
    for x, y in zip(plain, default):
        assert np.array_equal(x, y)
    assert np.array_equal(plain[2], s_tv) and np.array_equal(plain[3], v_tv)
    want, wst = (eng.run_blmpc if kind == "bl" else eng.run_abmpc)(mix["s0"], mix["v0"], mix["a_minus1"], s_tv, v_tv)
    assert np.array_equal(plain[0], want.cpu().numpy()) and np.array_equal(plain[1], wst.cpu().numpy())
    # knowing the lead's future changes the loop of an instance whose lead moves
    moving = np.ptp(v_tv, axis=0) > 0.5
    assert moving.any()
    changed = [i for i in np.nonzero(moving)[0] if not np.array_equal(traj[:, :, i], plain[0][:, :, i])]
    print(kind, "instances with a moving lead:", np.nonzero(moving)[0].tolist(), "changed by the preview:", changed)
    assert changed


# ------------------------------------------------------------------------------------------------ c8
def _refused(fn, code, *words):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    with pytest.raises(EepaccError) as e:
        fn()
    msg = str(e.value)
    assert ("libeepacc error %d:" % code) in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_refusals(torch_mod, lead_trace):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, _check
    from test_gpu_classes_bl import tv_classes
    STEP, RUN = "eepacc_classes_step_est", "eepacc_run_classes_preview"
    ab_OPTs, ab_Vs = ab_classes(20, "ORIG")
    ab_OPTs, ab_Vs = ab_OPTs[:3], ab_Vs[:3]
    bl_OPTs, bl_Vs = bl_route_classes(20, "ORIG")
    bl_OPTs, bl_Vs = bl_OPTs[:3], bl_Vs[:3]
    _, TVs, TVV = tv_classes(20)
    sc = scenario(3, 2, 12, lead_trace)
    B, N = 6, 20
    z = np.zeros(B)
    step_in = (sc["s0"], sc["v0"], sc["a_minus1"], z, sc["s_tv"][0], sc["v_tv"][0], z)
    lead = (np.ascontiguousarray(sc["s_tv"][:4]), np.ascontiguousarray(sc["v_tv"][:4]))
    good = np.zeros((N + 1, B)) + 100.0
    raw_step = lambda e: _check(e.lib.eepacc_classes_step_est(e.h, 1, *[None] * 14, None))       # the handle is checked first
    raw_run = lambda e: _check(e.lib.eepacc_run_classes_preview(e.h, 1, 4, 4, *[None] * 7, None))
    # handles without classes: the message points to the plain entries of the handle's mode
    for e, words in ((_single(ab_OPTs[0], ab_Vs[0]), ("no settings classes", "bl_mode = 0", "eepacc_ab_step_est", "eepacc_run_abmpc_preview")),
                     (_single(bl_OPTs[0], bl_Vs[0]), ("no settings classes", "bl_mode = 1", "eepacc_bl_step_est", "eepacc_run_blmpc_preview")),
                     (_single(TVs[0], TVV[0]), ("no settings classes", "bl_mode = 2", "target-vehicle"))):
        _refused(lambda: raw_step(e), ENOTSUP, STEP, *words)
        _refused(lambda: raw_run(e), ENOTSUP, RUN, *words)
        _refused(lambda: e.classes_step_est(*step_in), ENOTSUP, STEP)
        _refused(lambda: e.run_classes_preview(z, z, z, *lead), ENOTSUP, RUN)
    # a target-vehicle class handle: no lead
    tv = _mixed(TVs[:3], TVV[:3], max_batch=8)
    tv.set_classes(sc["class_of"])
    _refused(lambda: tv.classes_step_est(*step_in), ENOTSUP, STEP, "bl_mode = 2", "no lead")
    _refused(lambda: tv.run_classes_preview(z, z, z, *lead), ENOTSUP, RUN, "bl_mode = 2", "no lead")
    for OPTs, Vs in ((ab_OPTs, ab_Vs), (bl_OPTs, bl_Vs)):
        eng = _mixed(OPTs, Vs, max_batch=8)
        lib = eng.lib
        # before eepacc_set_classes, and with another B than the map's
        _refused(lambda: eng.classes_step_est(*step_in), EINVAL, STEP, "eepacc_set_classes has not been called")
        _refused(lambda: eng.run_classes_preview(z, z, z, *lead), EINVAL, RUN, "eepacc_set_classes has not been called")
        eng.set_classes(sc["class_of"])
        _refused(lambda: eng.classes_step_est(*[x[:4] for x in step_in]), EINVAL, STEP, "B = 4 differs")
        _refused(lambda: eng.run_classes_preview(z[:4], z[:4], z[:4], lead[0][:, :4], lead[1][:, :4]), EINVAL, RUN, "B = 4 differs")
        # B outside [0, max_batch]
        _refused(lambda: eng.classes_step_est(*[np.tile(x, 2) for x in step_in]), EINVAL, STEP, "max_batch")
        _refused(lambda: eng.run_classes_preview(np.zeros(12), np.zeros(12), np.zeros(12), np.zeros((4, 12)) + 50.0, np.zeros((4, 12))),
                 EINVAL, RUN, "max_batch")
        assert lib.eepacc_classes_step_est(eng.h, -1, *[None] * 14, None) == EINVAL and "B = -1" in lib.eepacc_last_error().decode()
        assert lib.eepacc_run_classes_preview(eng.h, -1, 4, 4, *[None] * 7, None) == EINVAL and RUN in lib.eepacc_last_error().decode()
        # n_lead < n_steps
        _refused(lambda: eng.run_classes_preview(z, z, z, *lead, n_steps=5), EINVAL, RUN, "n_lead = 4", "n_steps = 5")
        # half a pair and NULL required buffers, through the C-ABI itself (Engine refuses half a pair before the call)
        t = eng.torch
        d = [eng._d(x, B).data_ptr() for x in step_in]
        keep = [eng._d(good, (N + 1) * B) for _ in range(2)]
        out = t.empty((len(OUT), B), dtype=t.float64, device=eng.device); st = t.empty((B,), dtype=t.int32, device=eng.device)
        for half in ((keep[0].data_ptr(), None), (None, keep[1].data_ptr())):
            rc = lib.eepacc_classes_step_est(eng.h, B, *d, *half, None, out.data_ptr(), None, None, st.data_ptr(), None)
            msg = lib.eepacc_last_error().decode()
            assert rc == EINVAL and STEP in msg and "s_est" in msg and "v_est" in msg, msg
        rc = lib.eepacc_classes_step_est(eng.h, B, *d, None, None, None, None, None, None, st.data_ptr(), None)
        assert rc == EINVAL and b"eepacc_classes_step_est: NULL buffer" in lib.eepacc_last_error()
        rc = lib.eepacc_classes_step_est(eng.h, B, *d[:4], None, *d[5:], None, None, None, out.data_ptr(), None, None, st.data_ptr(), None)
        assert rc == EINVAL and b"eepacc_classes_step_est: NULL buffer" in lib.eepacc_last_error()
        traj = t.empty((4, len(OUT), B), dtype=t.float64, device=eng.device); st4 = t.empty((4, B), dtype=t.int32, device=eng.device)
        rc = lib.eepacc_run_classes_preview(eng.h, B, 4, 4, d[0], d[1], d[2], None, None, traj.data_ptr(), st4.data_ptr(), None)
        assert rc == EINVAL and b"eepacc_run_classes_preview: NULL buffer" in lib.eepacc_last_error()
        rc = lib.eepacc_run_classes_preview(eng.h, B, 4, 4, d[0], d[1], d[2], d[4], d[5], None, st4.data_ptr(), None)
        assert rc == EINVAL and b"eepacc_run_classes_preview: NULL buffer" in lib.eepacc_last_error()
        # B = 0 is nothing to do
        assert lib.eepacc_classes_step_est(eng.h, 0, *[None] * 14, None) == 0
        assert lib.eepacc_run_classes_preview(eng.h, 0, 4, 4, *[None] * 7, None) == 0
        # the QP builders stay refused on class handles, and the entries for plain handles keep their answers (what
        # tests/test_gpu_ab_est.py, tests/test_gpu_bl_est.py and tests/test_gpu_classes_bl.py::test_refusals assert)
        word = "eepacc_create_classes"                                  # (either creation entry; the old tests ask for this much)
        for name, n_null in (("eepacc_ab_step_est", 14), ("eepacc_ab_build_qp_est", 15), ("eepacc_bl_step_est", 14), ("eepacc_bl_build_qp_est", 15)):
            _refused(lambda: _check(getattr(lib, name)(eng.h, 1, *[None] * n_null, None)), ENOTSUP, name, "eepacc_create_classes")
        for name in ("eepacc_run_abmpc_preview", "eepacc_run_blmpc_preview"):
            _refused(lambda: _check(getattr(lib, name)(eng.h, 1, 4, 4, *[None] * 7, None)), ENOTSUP, name, "eepacc_create_classes")
        for call in (lambda: eng.ab_step_est(*step_in), lambda: eng.ab_build_qp_est(*step_in), lambda: eng.run_abmpc_preview(z, z, z, *lead),
                     lambda: eng.ab_build_qp(*step_in), lambda: eng.bl_build_qp(*step_in), lambda: eng.ab_qp_size(), lambda: eng.bl_qp_size()):
            _refused(call, ENOTSUP)
            assert word in lib.eepacc_last_error().decode()
        # a refused call leaves the handle's state alone: the next step is the twin's
        twin = _mixed(OPTs, Vs, max_batch=8)
        twin.set_classes(sc["class_of"])
        sup = dict(s_tv_est=np.ascontiguousarray(sc["s_tv"][0][None, :] + 4.0 * np.arange(N + 1)[:, None]))
        a = _np_step(eng.classes_step_est(*step_in, **sup), eng, B); b = _np_step(twin.classes_step_est(*step_in, **sup), twin, B)
        _same_step(a, b, np.arange(B), "after refusals")
    t.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ c9
@pytest.mark.parametrize("kind", ["ab", "bl"])
def test_determinism_and_independence_of_the_neighbours(kind, torch_mod, lead_trace):
    L = closed_loop(kind, "route", "ORIG", 20, lead_trace)
    sc, n_lead = L["sc"], N_STEPS + 20
    B = sc["class_of"].size
    one = L["mixed"][n_lead]
    # a second handle, the same inputs
    eng = _mixed(L["OPT"], L["V"])
    eng.set_classes(sc["class_of"])
    two = _pv(eng, "run_classes_preview", sc, N_STEPS, n_lead)
    for x, y in zip(one, two):
        assert np.array_equal(x, y, equal_nan=True)
    # instances permuted together with their classes: other classes share an instance's block, its column is the same
    perm = np.random.default_rng(7).permutation(B)
    assert not np.array_equal(sc["class_of"][perm], sc["class_of"])
    eng.set_classes(sc["class_of"][perm])
    tp, sp, ip = _pv(eng, "run_classes_preview", sc, N_STEPS, n_lead, perm)
    assert np.array_equal(tp, one[0][:, :, perm], equal_nan=True) and np.array_equal(sp, one[1][:, perm]) and np.array_equal(ip, one[2][perm])
