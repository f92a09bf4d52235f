"""Settings classes per instance (eepacc_create_classes / Engine.from_classes): one launch for instances that differ in
route, weights, estimator and vehicle.

The class kernels are the plain ABMPC kernels compiled once more with the DevCfg bound per instance: the same source, the
same flags, and results that the project already asserts not to depend on batch size or chunking.  The bar is therefore
bit equality with ordinary single-class engines (np.array_equal), not a tolerance; the oracle is the checker of the mixed
launch as a whole, at the tolerances of tests/test_gpu_ab.py::test_route_features_and_estimator_modes.
"""
import numpy as np
import pytest

from eepacc_mpc_casadi_matlab_amd._abi import OUT
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2

pytestmark = pytest.mark.gpu

ENOTSUP = "libeepacc error -4"
EINVAL = "libeepacc error -1"


def _use_case(case, N, tree="ORIG", **kw):
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, default_opt
    o = default_opt(); o["useCaseNum"] = case
    OPT = Settings(o, tree=tree, N_hor=N)
    OPT.update(kw)
    return OPT


def classes_a(N=20):
    """The classes of the small-kernel tests: five GetUseCase routes of the ORIG tree (its ABMPC has the route rows) and
    five variations of them.  Returns the settings and the vehicle per class."""
    from eepacc_mpc_casadi_matlab_amd.settings import SetVehicleParameters
    V = SetVehicleParameters("ORIG")
    uc = {c: _use_case(c, N) for c in (3, 6, 5, 7, 12)}
    OPTs = [uc[3], uc[6], uc[5], uc[7], uc[12]]
    Vs = [V] * 5
    OPTs.append(dict(uc[6], W_AB=uc[6]["W_AB"] * np.array([3.0, 0.5, 1.0, 2.0, 1.0, 1.0])))       # another inverse Hessian
    Vs.append(V)
    OPTs.append(uc[7]); Vs.append(dict(V, m=V["m"] + 350.0))                                      # another vehicle mass
    OPTs.append(dict(uc[12], paramEstSetting=0, TVestSetting=0)); Vs.append(V)                    # estimator modes 0 / 0
    OPTs.append(dict(uc[3], paramEstSetting=2, b_fifthOrder=1.25 * uc[3]["b_fifthOrder"])); Vs.append(V)   # previous solution; another power fit
    OPTs.append(uc[5]); Vs.append(dict(V, phi=1.1 * V["phi"], eta_TF=0.9))                        # another driveline
    return OPTs, Vs


def scenario(K, per, n_steps, lead_trace, seed=11):
    """per instances of each of K classes, interleaved, on S2 leads from tight following to a free road."""
    B = K * per
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"], seed=seed)
    sc["s_tv"] = np.ascontiguousarray(sc["s_tv"] + np.resize(np.array([5.0, 1e4, 60.0, 150.0, 1e4, 25.0, 400.0]), B)[None, :])
    sc["class_of"] = (np.arange(B) % K).astype(np.int32)
    return sc


def _mixed(OPTs, Vs, max_batch=64):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine.from_classes(OPTs, Vs, device=0, max_batch=max_batch)


def _single(OPT, V, max_batch=64):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _run(eng, sc, idx=slice(None), rows=slice(None), resume=False):
    traj, status = eng.run_abmpc(sc["s0"][idx], sc["v0"][idx], sc["a_minus1"][idx], np.ascontiguousarray(sc["s_tv"][rows, idx]),
                                 np.ascontiguousarray(sc["v_tv"][rows, idx]), resume=resume)
    eng.synchronize()
    return traj.cpu().numpy(), status.cpu().numpy()


def _assert_equals_single_class_engines(OPTs, Vs, sc, tr, st):
    """Every class's instances through an ordinary engine of that class (the existing kernels), bit for bit."""
    for k, (OPT, V) in enumerate(zip(OPTs, Vs)):
        idx = np.nonzero(sc["class_of"] == k)[0]
        rt, rs = _run(_single(OPT, V), sc, idx)
        assert np.array_equal(tr[:, :, idx], rt), ("traj", k, float(np.nanmax(np.abs(tr[:, :, idx] - rt))))
        assert np.array_equal(st[:, idx], rs), ("status", k)


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def mix_a(torch_mod, lead_trace):
    """The mixed launch of (a): N = 20, 60 steps, two instances per class.  Computed once, read by several tests."""
    OPTs, Vs = classes_a()
    sc = scenario(len(OPTs), 2, 60, lead_trace)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, sc)
    tr.setflags(write=False); st.setflags(write=False)
    return dict(OPT=OPTs, V=Vs, sc=sc, eng=eng, traj=tr, status=st)


def test_chosen_classes_have_every_route_feature():
    """(a) asks for a speed-limit step, a curve, a stop, a traffic light and a non-constant slope between the classes, and
    for a constant-slope class next to a table-slope one: read from the tables the kernels get."""
    OPTs, Vs = classes_a()
    assert len(OPTs) == len(Vs) == 10
    assert any(np.ptp(o["v_speedLim"]) > 0 for o in OPTs)
    assert any(np.max(np.abs(o["curvature"])) > 1e-3 for o in OPTs)
    assert any(np.size(o["stopLoc"]) > 0 for o in OPTs)
    assert any(np.size(o["TLLoc"]) > 0 for o in OPTs)
    assert any(np.ptp(o["slope"]) > 0 for o in OPTs) and any(np.ptp(o["slope"]) == 0 for o in OPTs)
    assert len({o["W_AB"].tobytes() for o in OPTs}) > 1 and len({v["m"] for v in Vs}) > 1
    assert any(o["paramEstSetting"] == 0 and o["TVestSetting"] == 0 for o in OPTs)
    assert any(o["paramEstSetting"] == 2 for o in OPTs)


def test_small_kernel_closed_loop_equals_single_class_engines(mix_a):
    """(a): the waves of one block hold different classes (interleaved map, 4 waves per block)."""
    assert mix_a["eng"].num_classes == 10
    assert np.isfinite(mix_a["traj"]).all()
    _assert_equals_single_class_engines(mix_a["OPT"], mix_a["V"], mix_a["sc"], mix_a["traj"], mix_a["status"])


def test_ab_step_and_postprocess_equal_single_class_engines(mix_a):
    """(b): the per-step operator with its predictions, twice in a row (warm start and, for paramEstSetting = 2, the
    stored previous solution), and the post-processing with each instance's own vehicle and power fit."""
    OPTs, Vs, sc, tr = mix_a["OPT"], mix_a["V"], mix_a["sc"], mix_a["traj"]
    B, Ts = sc["class_of"].size, 0.5
    steps = []
    for k in (25, 26):
        v = tr[k, OUT["v"]]
        vtv, vtvp = sc["v_tv"][k], sc["v_tv"][k - 1]
        steps.append((tr[k, OUT["s"]].copy(), v.copy(), (v - tr[k - 1, OUT["v"]]) / Ts, np.full(B, k * Ts), sc["s_tv"][k].copy(),
                      vtv.copy(), (vtv - vtvp) / Ts))
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    got = [[x.cpu().numpy() for x in eng.ab_step(*a)] for a in steps]
    post = [x.cpu().numpy() for x in eng.postprocess(eng.torch.as_tensor(tr.copy(), device="cuda"))]
    assert all(np.isfinite(x).all() for g in got for x in g)
    for k, (OPT, V) in enumerate(zip(OPTs, Vs)):
        idx = np.nonzero(sc["class_of"] == k)[0]
        one = _single(OPT, V)
        for a, g in zip(steps, got):
            ref = [x.cpu().numpy() for x in one.ab_step(*[x[idx] for x in a])]
            for name, x, r in zip(("out", "s_pred", "v_pred", "status"), g, ref):
                assert np.array_equal(x[..., idx], r), (k, name)
        rpost = one.postprocess(one.torch.as_tensor(np.ascontiguousarray(tr[:, :, idx]), device="cuda"))
        for name, x, r in zip(("rpm", "Tm", "P", "E"), post, rpost):
            assert np.array_equal(x[:, idx], r.cpu().numpy()), (k, name)
    # the driveline of a class reaches its instances only: rpm = 30 / pi * v * phi (RunOpt_ABMPC.m:343)
    for i in (2, 9):
        assert np.allclose(post[0][:, i], 30.0 / np.pi * tr[:, OUT["v"], i] * Vs[i]["phi"], rtol=1e-13, atol=0.0)


def test_large_kernel_equals_single_class_engines(torch_mod, lead_trace):
    """(c): N = 40 runs the N <= 63 kernels (3 waves per block)."""
    from eepacc_mpc_casadi_matlab_amd.settings import SetVehicleParameters
    V = SetVehicleParameters("ORIG")
    OPTs = [_use_case(3, 40), _use_case(12, 40, paramEstSetting=2), _use_case(7, 40)]
    Vs = [V, V, dict(V, m=V["m"] + 350.0)]
    sc = scenario(3, 2, 30, lead_trace, seed=12)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, sc)
    assert np.isfinite(tr).all()
    _assert_equals_single_class_engines(OPTs, Vs, sc, tr, st)


@pytest.mark.parametrize("N", [5, 30])
def test_abo_tree_equals_single_class_engines(N, torch_mod, lead_trace):
    """(d): the ABO tree's ABMPC (no route rows; slope and the speed limit of the travel incentive come from the tables):
    classes that differ in route and weights, one without the fuel term (ab_fuel_term = 0) next to two with it."""
    from eepacc_mpc_casadi_matlab_amd._abi import SettingsHolder
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, default_opt
    V = SetVehicleParameters("ABO")
    o1 = default_opt(); o1.update(slopes=np.array([[4.0, 30, 140], [-3.0, 200, 330]]), speedLimZones=np.array([[40.0, 0.0], [70.0, 120.0]]))
    o2 = default_opt(); o2.update(speedLimZones=np.array([[80.0, 0.0], [30.0, 90.0], [60.0, 260.0]]))
    OPTs = [Settings(tree="ABO", N_hor=N), Settings(o1, tree="ABO", N_hor=N), Settings(o2, tree="ABO", N_hor=N)]
    OPTs[0]["W_AB"] = OPTs[0]["W_AB"][1:].copy()                                    # six weights: no w_FC
    OPTs[2]["W_AB"] = OPTs[2]["W_AB"] * np.array([20.0, 3.0, 10.0, 2.0, 1.0, 5.0, 5.0])
    assert [SettingsHolder(o).pod.ab_fuel_term for o in OPTs] == [0, 1, 1]
    assert [SettingsHolder(o).pod.ab_route_rows for o in OPTs] == [0, 0, 0]
    sc = scenario(3, 2, 40, lead_trace, seed=13)
    Vs = [V, V, V]
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    tr, st = _run(eng, sc)
    assert np.isfinite(tr).all()
    _assert_equals_single_class_engines(OPTs, Vs, sc, tr, st)


def test_mixed_launch_against_the_oracle(mix_a):
    """(e): every instance of the mixed launch of (a) against the oracle's closed loop with the settings of its class.
    The set is chosen so that the oracle solves every step of every instance (checked on the CPU), which is asserted."""
    from oracle import Oracle
    sc, tr, st = mix_a["sc"], mix_a["traj"], mix_a["status"]
    n_steps = tr.shape[0]
    tol = dict(s=1e-7, v=1e-8, a=1e-8, xi_v=1e-8, xi_h=1e-8, xi_s=1e-8, xi_f=1e-8, Fm=1e-4, Fb=1e-4)
    worst = {}
    for i, k in enumerate(sc["class_of"]):
        ref, rst, _ = Oracle(mix_a["OPT"][k], mix_a["V"][k]).run("ab", n_steps, 0.0, float(sc["v0"][i]), 0.0, sc["s_tv"][:, i].copy(),
                                                                 sc["v_tv"][:, i].copy())
        assert rst.sum() == 0, (i, k)
        assert np.array_equal(rst != 0, st[:, i] != 0), (i, k)
        for n in tol:
            worst[n] = max(worst.get(n, 0.0), float(np.abs(tr[:, OUT[n], i] - ref[:, OUT[n]]).max()))
    print("largest distances to the oracle:", worst)
    for n, t in tol.items():
        assert worst[n] < t, (n, worst[n])


def test_launch_properties(mix_a):
    """(f): chunked launches, permuted instances, repeated launches."""
    sc, tr, st, eng = mix_a["sc"], mix_a["traj"], mix_a["status"], mix_a["eng"]
    B = sc["class_of"].size
    # two identical launches
    t2, s2 = _run(eng, sc)
    assert np.array_equal(t2, tr) and np.array_equal(s2, st)
    # chunks with resume = True equal one launch (the paramEstSetting = 2 class carries its previous solution across)
    parts = [_run(eng, sc, rows=slice(0, 23))] + [_run(eng, sc, rows=r, resume=True) for r in (slice(23, 24), slice(24, 60))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), tr) and np.array_equal(np.concatenate([p[1] for p in parts]), st)
    # instances permuted together with their classes: the outputs are the permuted outputs
    perm = np.random.default_rng(5).permutation(B)
    eng.set_classes(sc["class_of"][perm])
    tp, sp = _run(eng, sc, perm)
    eng.set_classes(sc["class_of"])
    assert np.array_equal(tp, tr[:, :, perm]) and np.array_equal(sp, st[:, perm])


def test_one_class_and_constant_maps(mix_a):
    """(f): n_classes = 1 still runs the class kernels and equals the ordinary handle; a map that sends every instance to
    class 2 of 5 equals the single handle of class 2."""
    OPTs, Vs, sc = mix_a["OPT"][:5], mix_a["V"][:5], mix_a["sc"]
    idx = np.arange(7)                                       # two blocks, the second partly filled
    ref, rst = _run(_single(OPTs[2], Vs[2]), sc, idx)
    one = _mixed(OPTs[2:3], Vs[2:3])
    assert one.num_classes == 1 and _single(OPTs[2], Vs[2]).num_classes == 1
    one.set_classes(np.zeros(7, dtype=np.int32))
    t1, s1 = _run(one, sc, idx)
    assert np.array_equal(t1, ref) and np.array_equal(s1, rst)
    five = _mixed(OPTs, Vs)
    five.set_classes(np.full(7, 2, dtype=np.int32))
    t5, s5 = _run(five, sc, idx)
    assert np.array_equal(t5, ref) and np.array_equal(s5, rst)
    th, sh = five.run_abmpc_host(sc["s0"][idx], sc["v0"][idx], sc["a_minus1"][idx], sc["s_tv"][:, idx], sc["v_tv"][:, idx])
    assert np.array_equal(th, ref) and np.array_equal(sh, rst)


def test_refusals(torch_mod, lead_trace):
    """(g)"""
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    OPTs, Vs = classes_a()
    OPTs, Vs = OPTs[:3], Vs[:3]
    sc = scenario(3, 2, 12, lead_trace)
    eng = _mixed(OPTs, Vs, max_batch=8)
    step_in = (sc["s0"], sc["v0"], sc["a_minus1"], np.zeros(6), sc["s_tv"][0], sc["v_tv"][0], np.zeros(6))
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_set_classes has not been called"):
        _run(eng, sc)
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_set_classes has not been called"):
        eng.ab_step(*step_in)
    with pytest.raises(EepaccError, match=EINVAL + r".*class_of\[4\] = 3"):
        eng.set_classes([0, 1, 2, 0, 3, 1])
    with pytest.raises(EepaccError, match=EINVAL):
        eng.set_classes([0, 1, -1])
    with pytest.raises(EepaccError, match=EINVAL):
        eng.set_classes(np.zeros(9, dtype=np.int32))          # above max_batch
    eng.set_classes(sc["class_of"])
    full, fst = _run(eng, sc)
    with pytest.raises(EepaccError, match=EINVAL + ".*B = 4 differs"):
        _run(eng, sc, np.arange(4))
    with pytest.raises(EepaccError, match=EINVAL + ".*B = 4 differs"):
        eng.ab_step(*[x[:4] for x in step_in])
    # the other controllers and the dense QP operator are not served
    z = np.zeros(6)
    for call in (lambda: eng.run_fbmpc(z, z, z, sc["s_tv"], sc["v_tv"]), lambda: eng.run_blmpc(z, z, z, sc["s_tv"], sc["v_tv"]),
                 lambda: eng.run_tvmpc(z, z, z, 5), lambda: eng.fb_step(*[z] * 10), lambda: eng.tv_step(z, z, z, z),
                 lambda: eng.run_fbmpc_host(z, z, z, sc["s_tv"], sc["v_tv"]),
                 lambda: eng.qp_solve_batched(np.eye(2)[None], np.zeros((1, 2)), np.ones((1, 1, 2)), lba=np.zeros((1, 1)))):
        with pytest.raises(EepaccError, match=ENOTSUP):
            call()
    # set_classes after a launch resets the loop state: a resumed launch starts at step 0 again
    head, _ = _run(eng, sc, rows=slice(0, 5))
    eng.set_classes(sc["class_of"])
    again, ast = _run(eng, sc, resume=True)
    assert np.array_equal(head, full[:5]) and np.array_equal(again, full) and np.array_equal(ast, fst)


@pytest.mark.parametrize("cfg", ["abo20", "orig20", "abo33", "orig33"])
def test_certified_case_table_equals_the_plain_engine(cfg, torch_mod):
    """The class kernels on active rigid rows: the case table of tests/ab_cert_cases.py (certified against the problem
    itself by tests/test_gpu_ab_cert.py) through two classes with the same settings, the map alternating, bit for bit against
    the plain engine.  eepacc_ab_build_qp refuses a class handle, so this is what carries the certificate over."""
    import ab_cert_cases as T
    OPT, V = T.settings(cfg)
    names, cols = T.cases(cfg)
    B = len(names)
    eng = _mixed([OPT, dict(OPT)], [V, dict(V)])
    eng.set_classes((np.arange(B) % 2).astype(np.int32))
    got = [x.cpu().numpy() for x in eng.ab_step(**cols)]
    ref = [x.cpu().numpy() for x in _single(OPT, V).ab_step(**cols)]
    assert int(np.abs(ref[3]).sum()) == 0
    for name, x, r in zip(("out", "s_pred", "v_pred", "status"), got, ref):
        assert np.array_equal(x, r), (cfg, name)
