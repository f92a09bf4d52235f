"""Without a GPU: the plain-Python reference of the per-stage functions (tests/stage_ref.py) against the restatement the
target-vehicle tests already use, against the oracle's plant on a saved trajectory and against its own 50-digit run; the
device harness (tests/kernels/stage_harness.hip) cross-compiles for gfx950; and every edge-case table of
tests/test_gpu_stage.py (tests/stage_cases.py) still holds a problem on each branch edge it was written for."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import cfg_harness
import stage_cases as sc
import stage_harness as sh
import stage_ref
import tvmpc_ref
from conftest import load_golden, make_case
from eepacc_mpc_casadi_matlab_amd import build as eb

# Largest distance of the fp64 stage_ref.plant_rk4 to its own mpmath run over all of stage_cases.PLANT_VARIANTS (relative to
# max(1, |value|)), as test_plant_fp64_against_mpmath measures it.  The device is allowed 8 times the measured figure.
PLANT_FP64_DISTANCE = 5.5e-16


@pytest.fixture(scope="module")
def CH(tmp_path_factory):
    return cfg_harness.load(str(tmp_path_factory.mktemp("cfg_harness")))


# ---------------------------------------------------------------------------------------------- against tvmpc_ref
@pytest.mark.parametrize("name", sorted(sc.ROUTE_VARIANTS))
def test_route_bounds_equal_tvmpc_ref_on_tv_settings(name):
    """MPCtype 2: selections (v_lim, v_curv, the 1e5 defaults, the constant limits) exact, arithmetic to 1e-15 relative"""
    OPT, V, s, v, t0, i = sc.route_case(name, 2)
    N = int(OPT["TV_N_hor"])
    assert N == int(OPT["N_hor"])
    rng = np.random.default_rng(5)
    for t_0 in (0.0, 7.5, 12.0, 23.5):
        s_est, v_est = rng.choice(s, N + 1), rng.choice(v, N + 1)
        new = stage_ref.route_and_comfort_bounds(OPT, s_est, v_est, t_0, 2)
        v_lim, v_stop, v_TL, v_curv, a_min, a_max, j_min, j_max = tvmpc_ref.route_and_comfort_bounds(OPT, s_est, v_est, t_0, N)
        assert np.array_equal(new["v_lim"], v_lim) and np.array_equal(new["v_curv"], v_curv)
        for a, b in ((new["v_stop"], v_stop), (new["v_TL"], v_TL), (new["a_min"], a_min), (new["a_max"], a_max),
                     (new["j_min"], j_min), (new["j_max"], j_max)):
            assert np.array_equal(a == 1e5, b == 1e5)
            np.testing.assert_allclose(a, b, rtol=1e-15, atol=0)


@pytest.mark.parametrize("mode", [0, 1])
def test_estimator_equals_tvmpc_ref_on_tv_settings(mode):
    OPT, V = sc.route_opt("abo20_five_knots", 2)
    for tc in sc.T_CONST:
        for s0, v0, a0 in sc.STATES_EXACT + sc.STATES_ROUNDED:
            o = dict(OPT, TV_trajEstSett=mode, tConstACC_ego=tc, tConstACC_tar=tc + 1.0)
            s_new, v_new = stage_ref.estimate_trajectory(o, 2, s0, v0, a0)
            s_old, v_old = tvmpc_ref.estimate_trajectory(o, s0, v0, a0, None, None)
            assert np.array_equal(s_new, s_old) and np.array_equal(v_new, v_old)


@pytest.mark.parametrize("name", sorted(sc.INTERP_TABLES))
def test_interp_pwa_equals_tvmpc_ref(name):
    doms, vals, d, exp, tol = sc.interp_case(name)
    assert np.array_equal(exp, [tvmpc_ref.interp_pwa(x, doms, vals) for x in d])


def test_mod_is_exact_on_the_light_phases():
    """x - floor(x / m) m, MATLAB's mod, loses nothing on the dyadic times of the route cases: it equals the exact residue"""
    for name in sc.ROUTE_VARIANTS:
        OPT, V, s, v, t0, i = sc.route_case(name, 0)
        Tvec = np.asarray(OPT["Tvec"], dtype=np.float64)
        for TL in np.asarray(OPT["TLLoc"], dtype=np.float64).reshape(-1, 4):
            m = float(TL[2] + TL[3])
            for q in range(len(s)):
                x = float(t0[q]) + (int(i[q]) + 1) * float(Tvec[i[q]]) - float(TL[1])
                exact = Fraction(t0[q]) + (int(i[q]) + 1) * Fraction(Tvec[i[q]]) - Fraction(TL[1])
                assert Fraction(x) == exact
                assert Fraction(stage_ref.matlab_mod(x, m)) == (exact % Fraction(m) if m else exact)


# ---------------------------------------------------------------------------------------------- plant
@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
def test_plant_equals_oracle_on_golden_trajectory(tree):
    from oracle import Oracle
    OPT, V, s_tv, v_tv = make_case(tree, 20)
    G, orc = load_golden(f"{tree.lower()}_abmpc"), Oracle(OPT, V)
    err = 0.0
    for k in range(870):
        s1, v1 = stage_ref.plant_rk4(OPT, V, G["s_opt"][k], G["v_opt"][k], G["Fm_opt"][k] + G["Fb_opt"][k])
        o0, o1 = orc.plant(G["s_opt"][k], G["v_opt"][k], G["Fm_opt"][k], G["Fb_opt"][k])
        err = max(err, abs(s1 - o0) / max(1.0, abs(s1)), abs(v1 - o1))
        err = max(err, abs(s1 - G["s_opt"][k + 1]) / max(1.0, abs(s1)), abs(v1 - G["v_opt"][k + 1]))
    assert err < 1e-13


def test_plant_fp64_against_mpmath():
    """The fp64 scheme against the same scheme at 50 digits on the inputs of the GPU test.  Measured, largest distance
    relative to max(1, |value|): abo_sloped_m10 5.49e-16, orig_sloped_m1 4.65e-16, abo_flat_m1 3.47e-16, orig_flat_m10
    4.21e-16; 5.49e-16 over all.  This is the yardstick of test_gpu_stage.test_plant_rk4, which allows the device 8 times it."""
    worst = 0.0
    for name in sc.PLANT_VARIANTS:
        f0, f1, m = sc.plant_references(name)
        d = sc.plant_distance(f0, f1, m)
        print("%s: fp64 against mpmath %.3e" % (name, d))
        worst = max(worst, d)
    assert 0.5 * PLANT_FP64_DISTANCE < worst <= PLANT_FP64_DISTANCE


# ---------------------------------------------------------------------------------------------- the harness
def test_harness_cross_compiles_for_gfx950(tmp_path, CH):
    assert "--offload-arch=gfx950" in eb.BASE_FLAGS
    lib = sh.compile_harness(str(tmp_path))
    assert os.path.getsize(lib) > 0 and not sh.is_stale(lib)
    t = os.path.getmtime(lib)
    assert sh.compile_harness(str(tmp_path)) == lib and os.path.getmtime(lib) == t      # up to date: not rebuilt
    os.utime(lib, (t - 10 ** 9, t - 10 ** 9))                                             # older than its inputs
    assert sh.is_stale(lib)
    dll = ctypes.CDLL(lib)
    for s in sh.SYMBOLS:
        assert hasattr(dll, s), s
    dll.sh_sizeof_devcfg.restype = ctypes.c_int
    assert dll.sh_sizeof_devcfg() == CH.sizeof_devcfg


def test_harness_build_follows_another_csrc(monkeypatch, tmp_path):
    monkeypatch.setenv("EEPACC_STAGE_CSRC", str(tmp_path))
    assert sh.inputs() == [sh.SOURCE, str(tmp_path / "eepacc_stage.h"), str(tmp_path / "eepacc_device.h")]
    monkeypatch.delenv("EEPACC_STAGE_CSRC")
    assert sh.inputs()[1] == os.path.join(eb.CSRC, "eepacc_stage.h")


# ---------------------------------------------------------------------------------------------- the case tables
def _assert_all_hit(E, where):
    missing = [k for k, n in E.items() if n < 1]
    assert not missing, "%s: no problem on %s" % (where, missing)


@pytest.mark.parametrize("MPCtype", sc.MPC_TYPES)
@pytest.mark.parametrize("name", sorted(sc.ROUTE_VARIANTS))
def test_route_cases_hit_their_edges(CH, name, MPCtype):
    OPT, V, s, v, t0, i = sc.route_case(name, MPCtype)
    E = sc.route_edges(OPT, s, v, t0, i)
    _assert_all_hit(E, name)
    assert len(s) <= 4096 and i.min() == 0 and i.max() == int(OPT["N_hor"]) - 1
    if "one_knot" not in name:
        for k in ("TL: md == TL[2] (just green), in range", "TL: x < 0 and green where x itself is below TL[2], in range",
                  "TL: red, d < 0", "TL: two red within range", "stop: two within range", "stop: distance == stopRefDist"):
            assert k in E, k
    # the translation takes these settings as they are: one-knot tables, the light with a cycle of length zero
    b = CH.build(OPT, V)
    assert b.rc == 0, b.msg
    assert int(b.field("bl_mode")[0]) == MPCtype and int(b.field("N")[0]) == int(OPT["N_hor"])
    assert int(b.field("n_TL")[0]) == np.asarray(OPT["TLLoc"]).reshape(-1, 4).shape[0]
    assert int(b.field("const_T")[0]) == int(np.all(np.asarray(OPT["Tvec"]) == OPT["Tvec"][0]))


def test_route_variants_cover_the_settings():
    names = sorted(sc.ROUTE_VARIANTS)
    assert {sc.ROUTE_VARIANTS[n][0] for n in names} == {"ABO", "ORIG"} and {sc.ROUTE_VARIANTS[n][1] for n in names} == {2, 20, 63}
    assert {len(sc.ROUTE_VARIANTS[n][2]["s_speedLim"]) for n in names} == {1, 2, 5}
    lights = sc.LIGHTS
    assert np.any(lights[:, 2] + lights[:, 3] == 0)


@pytest.mark.parametrize("name", sorted(sc.ESTIMATE_VARIANTS))
def test_estimate_cases_hit_their_edges(CH, name):
    OPT, V, exact, runs, run, lane = sc.estimate_case(name)
    _assert_all_hit(sc.estimate_edges(OPT, runs, run, lane), name)
    assert len(run) <= 8192
    b = CH.build(OPT, V)
    assert b.rc == 0, b.msg
    Tvec = np.asarray(OPT["Tvec"], dtype=np.float64)
    assert int(b.field("const_T")[0]) == int(np.all(Tvec == Tvec[0]))
    if exact:
        # every sum the reference forms is exact: the repeated adds equal the exact rational sums
        for r in runs:
            s_est, v_est = stage_ref.estimate_trajectory(sc.estimate_run_opt(OPT, r), r[0], *r[3:])
            acc = Fraction(r[3])
            for k in range(1, len(s_est)):
                acc += Fraction(Tvec[k - 1]) * Fraction(v_est[k - 1])
                assert Fraction(s_est[k]) == acc


def test_estimate_variants_cover_the_settings():
    V = sc.ESTIMATE_VARIANTS
    assert {v[1] for v in V.values()} == {2, 20, 63} and {v[0] for v in V.values()} == {"ABO", "ORIG"}
    assert any("non_monotone" in k for k in V) and any("geometric" in k for k in V)
    OPT, _, _ = sc.estimate_opt("abo20_geometric")
    assert np.all(np.diff(OPT["Tvec"]) > 0)


@pytest.mark.parametrize("name", sorted(sc.INTERP_TABLES))
def test_interp_cases_hit_their_edges(name):
    _assert_all_hit(sc.interp_edges(name), name)


def test_interp_tables_cover_the_sizes():
    assert {len(t[0]) for t in sc.INTERP_TABLES.values()} == {1, 2, 5}


@pytest.mark.parametrize("name", sorted(sc.PLANT_VARIANTS))
def test_plant_cases_hit_their_edges(CH, name):
    _assert_all_hit(sc.plant_edges(name), name)
    OPT, V = sc.plant_opt(name)
    b = CH.build(OPT, V)
    assert b.rc == 0, b.msg
    assert int(b.field("const_slope")[0]) == int("flat" in name)
    assert int(b.field("N_integratePlant")[0]) == (1 if name.endswith("m1") else 10)


def test_plant_variants_cover_the_settings():
    names = sorted(sc.PLANT_VARIANTS)
    assert {sc.PLANT_VARIANTS[n][0] for n in names} == {"ABO", "ORIG"}
    assert {int(sc.plant_opt(n)[0]["N_integratePlant"]) for n in names} == {1, 10}
    assert int(sc._settings("ABO", 20)[0]["N_integratePlant"]) == 10
