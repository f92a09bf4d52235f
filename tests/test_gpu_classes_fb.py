"""FBMPC on settings classes (eepacc_classes_fb_step, eepacc_run_classes_fbmpc / Engine.classes_fb_step, run_classes_fbmpc): one
launch for instances that differ in route, W_FB, FBuseTaylor, estimator and vehicle.

The class kernels are the structured FBMPC kernels compiled once more with the DevCfg bound per wave (csrc/eepacc_fbs_cls.hip):
the same source with another DevCfg pointer.  The bar is bit equality (np.array_equal) with the plain engine of every class,
Engine(OPT[k], V[k]), which runs the WHOLE batch's inputs with the same B and n_steps (the same launch geometry: grid, work-unit
length); only the columns of class k are compared.  The oracle checks one mixed launch as a whole, at the tolerances of
tests/test_gpu_fb.py (_compare_fb with scale = 10, its closed-loop use there), on a mix of the settings that file compares with the
oracle.  Inputs, and the reasons for them: tests/classes_fb_cases.py.
"""
import numpy as np
import pytest

import classes_fb_cases as T

pytestmark = pytest.mark.gpu

ENOTSUP = "libeepacc error -4"
EINVAL = "libeepacc error -1"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


def _mixed(OPTs, Vs, max_batch=16):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine.from_classes(OPTs, Vs, device=0, max_batch=max_batch)


def _plain(OPT, V, max_batch=16):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _np(xs):
    return [None if x is None else x.cpu().numpy() for x in xs]


def _run(eng, entry, sc, rows=slice(None), resume=False):
    traj, status = getattr(eng, entry)(sc["s0"], sc["v0"], sc["a_minus1"], np.ascontiguousarray(sc["s_tv"][rows]),
                                       np.ascontiguousarray(sc["v_tv"][rows]), resume=resume)
    eng.synchronize()
    return traj.cpu().numpy(), status.cpu().numpy()


def _same(x, r):
    return np.array_equal(x, r, equal_nan=True)


def _assert_columns_equal_plain_engines(OPTs, Vs, sc, got, plain_fn, what):
    """got: arrays whose last axis is the instance; plain_fn(engine of class k) the same arrays for the whole batch."""
    K = int(sc["class_of"].max()) + 1
    for k in range(K):
        idx = np.nonzero(sc["class_of"] == k)[0]
        ref = plain_fn(_plain(OPTs[k], Vs[k]))
        for j, (x, r) in enumerate(zip(got, ref)):
            if x is None:
                assert r is None
                continue
            assert _same(x[..., idx], r[..., idx]), (what, "class", k, "array", j, float(np.nanmax(np.abs(x[..., idx] - r[..., idx]))))


# ------------------------------------------------------------------------------------------------ closed loop
@pytest.mark.parametrize("N,pe2", [(2, False), (3, False), (20, False), (20, True), (32, True), (33, False), (63, True)])
def test_closed_loop_equals_plain_engines(N, pe2, torch_mod):
    """Four classes interleaved over B = 15 (three blocks of the N <= 32 kernel, the last with one wave; a block holds all four
    classes), 30 steps in one launch and the same 30 as 13 + 17 resumed.  N = 32 / 33: the last horizon of the small kernels and
    the first of the large ones.  pe2: class 1 carries its previous solution (paramEstSetting = 2)."""
    OPTs, Vs = T.classes(N, pe2)
    sc = T.scenario(15, 30, 4)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, "run_classes_fbmpc", sc)
    assert (st == 0).any()
    _assert_columns_equal_plain_engines(OPTs, Vs, sc, (tr, st), lambda e: _run(e, "run_fbmpc", sc), "run N=%d" % N)
    a = _run(eng, "run_classes_fbmpc", sc, rows=slice(0, 13))
    b = _run(eng, "run_classes_fbmpc", sc, rows=slice(13, 30), resume=True)
    assert _same(np.concatenate([a[0], b[0]]), tr) and _same(np.concatenate([a[1], b[1]]), st)
    # iteration counts of the last launch, per instance, against the plain engine of class 0 on the same rows
    one = _plain(OPTs[0], Vs[0])
    _run(one, "run_fbmpc", sc, rows=slice(0, 13)); _run(one, "run_fbmpc", sc, rows=slice(13, 30), resume=True)
    idx = np.nonzero(sc["class_of"] == 0)[0]
    assert np.array_equal(eng.last_iterations(15)[idx], one.last_iterations(15)[idx])


@pytest.mark.parametrize("B", [1, 6, 7, 8, 15])
def test_batch_sizes_with_the_interleaved_map(B, torch_mod):
    """Map 0, 1, 2, 0, 1, 2, ..: one 7-wave block holds several classes, B = 7 fills it, 8 and 15 leave a partial last block."""
    OPTs, Vs = T.classes(20)
    OPTs, Vs = OPTs[:3], Vs[:3]
    sc = T.scenario(B, 12, 3)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, "run_classes_fbmpc", sc)
    _assert_columns_equal_plain_engines(OPTs, Vs, sc, (tr, st), lambda e: _run(e, "run_fbmpc", sc), "B=%d" % B)


def test_long_launch_constant_map_and_one_class(torch_mod):
    """70 steps for B = 6: several work units per instance whatever the unit length.  A constant map to class 2 of 4 and a
    handle with that one class equal the plain engine of the class in every column."""
    OPTs, Vs = T.classes(20)
    sc = T.scenario(6, 70, 3)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, "run_classes_fbmpc", sc)
    _assert_columns_equal_plain_engines(OPTs, Vs, sc, (tr, st), lambda e: _run(e, "run_fbmpc", sc), "70 steps")
    sc8 = T.scenario(8, 20, 1)
    ref = _run(_plain(OPTs[2], Vs[2]), "run_fbmpc", sc8)
    eng.set_classes(np.full(8, 2, dtype=np.int32))
    got = _run(eng, "run_classes_fbmpc", sc8)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])
    one = _mixed(OPTs[2:3], Vs[2:3])
    assert one.num_classes == 1
    one.set_classes(np.zeros(8, dtype=np.int32))
    got = _run(one, "run_classes_fbmpc", sc8)
    assert _same(got[0], ref[0]) and _same(got[1], ref[1])


# ------------------------------------------------------------------------------------------------ step
@pytest.mark.parametrize("N,pe2", [(3, False), (20, True), (32, False), (33, True), (63, False)])
def test_steps_equal_plain_engines(N, pe2, torch_mod):
    """Steps 0, 1, 2 in sequence on inputs that change from call to call: the first is cold, the later ones find the codes of
    another problem and the carried A22 / D2 (frozen stage by stage, RunOpt_FBMPC.m:247-259) and, with pe2, the previous
    predictions.  The second call passes s_pred = v_pred = NULL."""
    B = 15
    OPTs, Vs = T.classes(N, pe2)
    calls = T.step_inputs(B)
    class_of = (np.arange(B) % 4).astype(np.int32)

    def seq(e, fn):
        out = []
        for j, c in enumerate(calls):
            out += _np(getattr(e, fn)(*c, want_pred=(j != 1)))
        return out

    eng = _mixed(OPTs, Vs)
    eng.set_classes(class_of)
    got = seq(eng, "classes_fb_step")
    assert got[5] is None and got[6] is None and got[1] is not None
    _assert_columns_equal_plain_engines(OPTs, Vs, dict(class_of=class_of), got, lambda e: seq(e, "fb_step"), "steps N=%d" % N)
    # reset and set_classes give the cold result again
    eng.reset()
    again = _np(eng.classes_fb_step(*calls[0]))
    assert all(_same(x, r) for x, r in zip(again, got[:4]))
    eng.set_classes(class_of)
    again = _np(eng.classes_fb_step(*calls[0]))
    assert all(_same(x, r) for x, r in zip(again, got[:4]))


# ------------------------------------------------------------------------------------------------ state separation
def test_abmpc_and_fbmpc_state_are_separate(torch_mod):
    OPTs, Vs = T.classes(20, True)
    sc = T.scenario(15, 30, 4)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    fb = _run(eng, "run_classes_fbmpc", sc)
    ab = _run(eng, "run_abmpc", sc)
    B = 15
    ab_in = (sc["s0"] + 3.0, sc["v0"] + 1.0, np.zeros(B), np.zeros(B), sc["s_tv"][3], sc["v_tv"][3], np.zeros(B))
    # FBMPC 13 steps, ABMPC step and closed loop (resume=True: no reset), FBMPC 17 more
    eng.reset()
    a = _run(eng, "run_classes_fbmpc", sc, rows=slice(0, 13), resume=True)
    eng.ab_step(*ab_in)
    _run(eng, "run_abmpc", sc, rows=slice(0, 7), resume=True)
    b = _run(eng, "run_classes_fbmpc", sc, rows=slice(13, 30), resume=True)
    assert _same(np.concatenate([a[0], b[0]]), fb[0]) and _same(np.concatenate([a[1], b[1]]), fb[1])
    # the reverse: ABMPC 13 steps, FBMPC closed loop, ABMPC 17 more
    eng.reset()
    a = _run(eng, "run_abmpc", sc, rows=slice(0, 13), resume=True)
    _run(eng, "run_classes_fbmpc", sc, rows=slice(0, 9), resume=True)
    b = _run(eng, "run_abmpc", sc, rows=slice(13, 30), resume=True)
    assert _same(np.concatenate([a[0], b[0]]), ab[0]) and _same(np.concatenate([a[1], b[1]]), ab[1])
    # steps: an ABMPC step between two FBMPC steps, and an FBMPC step between two ABMPC steps
    calls = T.step_inputs(B)
    eng.reset()
    f0 = _np(eng.classes_fb_step(*calls[0])); f1 = _np(eng.classes_fb_step(*calls[1]))
    eng.reset()
    a0 = _np(eng.ab_step(*ab_in)); a1 = _np(eng.ab_step(*ab_in))
    eng.reset()
    g0 = _np(eng.classes_fb_step(*calls[0])); b0 = _np(eng.ab_step(*ab_in))
    g1 = _np(eng.classes_fb_step(*calls[1])); b1 = _np(eng.ab_step(*ab_in))
    for x, r in zip(g0 + g1 + b0 + b1, f0 + f1 + a0 + a1):
        assert _same(x, r)


# ------------------------------------------------------------------------------------------------ oracle, key figures
def _mix_fixture(OPTs, Vs, sc):
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    traj, status = eng.run_classes_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    eng.synchronize()
    return dict(OPT=OPTs, V=Vs, sc=sc, eng=eng, traj=traj, status=status)


@pytest.fixture(scope="module")
def oracle_mix(torch_mod):
    OPTs, Vs = T.oracle_classes()
    return _mix_fixture(OPTs, Vs, T.oracle_scenario())


@pytest.fixture(scope="module")
def route_mix(torch_mod):
    OPTs, Vs = T.classes(20)
    return _mix_fixture(OPTs[:3], Vs[:3], T.scenario(6, 30, 3))


def test_mixed_launch_against_the_oracle(oracle_mix):
    """Every instance against the oracle's FBMPC closed loop with the settings of its class, as tests/test_gpu_fb.py compares the
    plain engine (_compare_fb: up to the first step that fails on both sides; closed loops there use scale = 10, i.e. s 1e-7 m,
    v and slacks 1e-8, forces 1e-5 N + 1e-8 relative, cost 1e-9 relative).  The mix is drawn from the settings on which that
    file establishes the oracle as a reference for the structured kernels (tests/classes_fb_cases.py says why, and why the
    route classes of the other tests are not in it).  The oracle solves every step of this mix
    (tests/test_classes_fb_cpu.py asserts it), so every step is compared."""
    from oracle import Oracle
    from test_gpu_fb import _compare_fb
    m = oracle_mix
    sc, tr, st = m["sc"], m["traj"].cpu().numpy(), m["status"].cpu().numpy()
    n_steps = tr.shape[0]
    assert tr.shape[2] == T.ORACLE_MIX["B"] and n_steps == T.ORACLE_MIX["n_steps"]
    for i, k in enumerate(sc["class_of"]):
        ref, rst, _ = Oracle(m["OPT"][k], m["V"][k]).run("fb", n_steps, 0.0, float(sc["v0"][i]), 0.0, sc["s_tv"][:, i].copy(), sc["v_tv"][:, i].copy())
        assert rst.sum() == 0, (i, k)
        assert _compare_fb(tr[:, :, i], st[:, i], ref, rst, scale=10.0) == n_steps, (i, k)
    # the classes differ where it shows: the instances of two classes on the same inputs part
    plain = _run(_plain(m["OPT"][1], m["V"][1]), "run_fbmpc", sc)[0]
    assert not _same(plain[:, :, 0], tr[:, :, 0])


def test_key_figures_per_class(route_mix):
    """kpis, follow_kpis(weights="fb") and route_kpis of a mixed trajectory (three route classes, N = 20, B = 6, 30 steps) equal the
    tables of the plain engines of the classes."""
    m = route_mix
    sc, eng, traj, status = m["sc"], m["eng"], m["traj"], m["status"]
    cut = 120.0
    figs = lambda e: _np((e.kpis(traj, status, cut), e.follow_kpis(traj, status, sc["s_tv"], sc["v_tv"], weights="fb"), e.route_kpis(traj, status)))
    got = figs(eng)
    _assert_columns_equal_plain_engines(m["OPT"], m["V"], sc, got, figs, "key figures")
    rpm = _np(eng.postprocess(traj))
    _assert_columns_equal_plain_engines(m["OPT"], m["V"], sc, rpm, lambda e: _np(e.postprocess(traj)), "postprocess")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(torch_mod):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL
    OPTs, Vs = T.classes(20)
    sc = T.scenario(6, 5, 3)
    step = T.step_inputs(6)[0]
    run = lambda e, sc_=sc: e.run_classes_fbmpc(sc_["s0"], sc_["v0"], sc_["a_minus1"], sc_["s_tv"], sc_["v_tv"])
    # a handle of eepacc_create, and one of eepacc_create_classes_bl
    plain = _plain(OPTs[0], Vs[0])
    for call in (lambda: run(plain), lambda: plain.classes_fb_step(*step)):
        with pytest.raises(EepaccError, match=ENOTSUP + r".*eepacc_(run_classes_fbmpc|classes_fb_step): this handle has no settings classes.*eepacc_fb_step / eepacc_run_fbmpc"):
            call()
    bl = _mixed([Settings_BL(o) for o in OPTs[:2]], Vs[:2])
    bl.set_classes(np.zeros(6, dtype=np.int32))
    for call in (lambda: run(bl), lambda: bl.classes_fb_step(*step)):
        with pytest.raises(EepaccError, match=ENOTSUP + r".*eepacc_create_classes_bl.*bl_mode = 1"):
            call()
    # a class the structured kernels do not represent: named with its field
    bq = np.array([185, 1.296e-20, 2.301, 2.5e-4, 0.003728, -0.000181])
    bad = _mixed([OPTs[0], OPTs[1], dict(OPTs[2], b_quadr=bq)], Vs[:3])
    bad.set_classes(sc["class_of"])
    for call in (lambda: run(bad), lambda: bad.classes_fb_step(*step)):
        with pytest.raises(EepaccError, match=ENOTSUP + r".*class 2: b_quadr\(4\) != 0.*no dense path"):
            call()
    w = np.asarray(OPTs[1]["W_FB"], dtype=np.float64).copy(); w[4] = 0.0
    bad = _mixed([OPTs[0], dict(OPTs[1], W_FB=w)], Vs[:2])
    bad.set_classes(np.zeros(6, dtype=np.int32))
    with pytest.raises(EepaccError, match=ENOTSUP + r".*class 1: W_FB"):
        run(bad)
    tr_ab, _ = _run(bad, "run_abmpc", sc)                      # the ABMPC entries of such a handle work as before
    assert np.isfinite(tr_ab).all()
    # the call
    eng = _mixed(OPTs[:3], Vs[:3], max_batch=8)
    for call in (lambda: run(eng), lambda: eng.classes_fb_step(*step)):
        with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_set_classes has not been called"):
            call()
    eng.set_classes(sc["class_of"])
    sc4 = T.scenario(4, 5, 3)
    with pytest.raises(EepaccError, match=EINVAL + r".*eepacc_run_classes_fbmpc: B = 4 differs from the B = 6"):
        run(eng, sc4)
    with pytest.raises(EepaccError, match=EINVAL + r".*eepacc_classes_fb_step: B = 4 differs from the B = 6"):
        eng.classes_fb_step(*[x[:4] for x in step])
    sc9 = T.scenario(9, 5, 3)
    with pytest.raises(EepaccError, match=EINVAL + r".*B = 9 is outside \[0, max_batch = 8\]"):
        run(eng, sc9)
    lib, h, t = eng.lib, eng.h, eng.torch
    d = lambda n: t.zeros(n, dtype=t.float64, device="cuda")
    s0, traj, stat = d(6), d(5 * 12 * 6), t.zeros(30, dtype=t.int32, device="cuda")
    lead = d(30)
    ptr = lambda x: x.data_ptr()
    assert lib.eepacc_run_classes_fbmpc(h, 6, 5, ptr(s0), ptr(s0), ptr(s0), None, ptr(lead), ptr(traj), ptr(stat), None) == -1
    assert "eepacc_run_classes_fbmpc: s_tv is NULL" in lib.eepacc_last_error().decode()
    assert lib.eepacc_classes_fb_step(h, 6, *[ptr(s0)] * 10, None, None, None, ptr(stat), None) == -1
    assert "eepacc_classes_fb_step: out is NULL" in lib.eepacc_last_error().decode()
    assert lib.eepacc_run_classes_fbmpc(h, 6, -1, ptr(s0), ptr(s0), ptr(s0), ptr(lead), ptr(lead), ptr(traj), ptr(stat), None) == -1
    # B = 0 is nothing to do, also before the buffers are looked at
    assert lib.eepacc_run_classes_fbmpc(h, 0, 5, None, None, None, None, None, None, None, None) == 0
    assert lib.eepacc_classes_fb_step(h, 0, *[None] * 10, None, None, None, None, None) == 0
    # a closed loop after a step needs a reset, as on a plain handle
    eng.classes_fb_step(*step)
    with pytest.raises(EepaccError, match=EINVAL + ".*after eepacc_classes_fb_step.*eepacc_reset"):
        eng.run_classes_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"], resume=True)
    # the old entries keep refusing the class handle
    z = np.zeros(6)
    for call in (lambda: eng.run_fbmpc(z, z, z, sc["s_tv"], sc["v_tv"]), lambda: eng.fb_step(*[z] * 10)):
        with pytest.raises(EepaccError, match=ENOTSUP + ".*eepacc_create_classes runs ABMPC only"):
            call()
