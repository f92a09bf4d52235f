"""Settings classes of the baseline and target-vehicle controllers (eepacc_create_classes_bl), the parts that need no GPU:
what creation refuses, with the code and a message that names class and field, and the use-case mix of
scenarios.make_use_case_mix for the baseline controller with its target-vehicle classes."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_case, load_golden
from eepacc_mpc_casadi_matlab_amd import build as eb
from eepacc_mpc_casadi_matlab_amd import engine
from eepacc_mpc_casadi_matlab_amd._abi import pack_classes, EEPACC_MAX_CLASSES
from eepacc_mpc_casadi_matlab_amd.scenarios import make_use_case_mix
from eepacc_mpc_casadi_matlab_amd.settings import Settings, Settings_BL, Settings_TV, SetVehicleParameters, default_opt

EINVAL, ENOTSUP = -1, -4


@pytest.fixture(scope="module")
def lib():
    eb.build()
    return engine.load_library()


@pytest.fixture(scope="module")
def case():
    OPT, V, *_ = make_case("ORIG", 20)
    return OPT, Settings_BL(OPT), Settings_TV(OPT), V


def _create(lib, OPTs, Vs, n=None):
    keep, S, V = pack_classes(OPTs, Vs)
    h = C.c_void_p()
    rc = lib.eepacc_create_classes_bl(C.byref(h), S, V, len(OPTs) if n is None else n, 0, 16)
    assert not h.value
    return rc, lib.eepacc_last_error().decode()


def test_the_controller_is_shared(lib, case):
    """Class 0 says which controller the handle runs, 1 or 2; every class has that bl_mode."""
    OPT, BL, TV, V = case
    rc, msg = _create(lib, [BL, BL, TV], [V] * 3)
    assert rc == EINVAL and "class 2" in msg and "bl_mode" in msg, msg
    rc, msg = _create(lib, [TV, BL], [V] * 2)
    assert rc == EINVAL and "class 1" in msg and "bl_mode" in msg, msg
    rc, msg = _create(lib, [BL, OPT], [V] * 2)
    assert rc == EINVAL and "class 1" in msg and "bl_mode" in msg, msg
    # ABMPC classes belong to the other entry, which the message names
    rc, msg = _create(lib, [OPT, OPT], [V] * 2)
    assert rc == EINVAL and "class 0" in msg and "bl_mode" in msg and "eepacc_create_classes" in msg.replace("eepacc_create_classes_bl", ""), msg
    rc, msg = _create(lib, [dict(BL, bl_mode=3)], [V])
    assert rc == EINVAL and "bl_mode" in msg, msg


def test_the_other_entry_names_this_one(lib, case):
    OPT, BL, TV, V = case
    keep, S, Vs = pack_classes([OPT, BL], [V] * 2)
    h = C.c_void_p()
    rc = lib.eepacc_create_classes(C.byref(h), S, Vs, 2, 0, 16)
    msg = lib.eepacc_last_error().decode()
    assert rc == ENOTSUP and not h.value and "class 1" in msg and "bl_mode" in msg and "eepacc_create_classes_bl" in msg, msg


@pytest.mark.parametrize("mode", [1, 2])
def test_fields_that_must_agree(lib, case, mode):
    OPT, BL, TV, V = case
    base = BL if mode == 1 else TV
    other = (Settings_BL if mode == 1 else Settings_TV)(dict(OPT, BL_N_hor=30, TV_N_hor=30))
    rc, msg = _create(lib, [base, base, other], [V] * 3)
    assert rc == EINVAL and "class 2" in msg and "N_hor" in msg, msg
    if mode == 1:                                      # (a target-vehicle class with a non-uniform grid is refused as such)
        o = dict(base); o["Tvec"] = base["Tvec"].copy(); o["Tvec"][7] = 0.75
        rc, msg = _create(lib, [base, o], [V] * 2)
        assert rc == EINVAL and "class 1" in msg and "Tvec[7]" in msg, msg
    o = dict(base); o["Tvec"] = 0.25 * np.ones(20)
    rc, msg = _create(lib, [base, o], [V] * 2)
    assert rc == EINVAL and "class 1" in msg and "Tvec[0]" in msg, msg


def test_what_eepacc_create_refuses_is_refused_per_class(lib, case):
    OPT, BL, TV, V = case
    rc, msg = _create(lib, [BL, dict(BL, solverToUse=2)], [V] * 2)
    assert rc == ENOTSUP and "class 1" in msg and "solverToUse" in msg, msg
    rc, msg = _create(lib, [TV, dict(TV, solverToUse=2)], [V] * 2)
    assert rc == ENOTSUP and "class 1" in msg and "solverToUse" in msg, msg


def test_number_of_classes(lib, case):
    OPT, BL, TV, V = case
    rc, msg = _create(lib, [BL], [V], n=0)
    assert rc == EINVAL and "n_classes" in msg, msg
    assert EEPACC_MAX_CLASSES == 4096
    rc, msg = _create(lib, [BL] * 4097, [V] * 4097)
    assert rc == EINVAL and "n_classes" in msg, msg


@pytest.mark.parametrize("mode", [1, 2])
def test_valid_classes_pass_validation(lib, case, mode):
    """Classes that differ in W_BL, bl_lp_eps, the vehicle mass and the route pass the checks: the call gets as far as the
    device (and fails there where there is none)."""
    OPT, BL, TV, V = case
    base = BL if mode == 1 else TV
    o = default_opt(); o["useCaseNum"] = 5
    route = (Settings_BL if mode == 1 else Settings_TV)(Settings(o, tree="ORIG", N_hor=20))
    W = np.asarray(base["W_BL"], dtype=np.float64)
    OPTs = [base, dict(base, W_BL=W + np.array([0.0, 1.0, 1.0, 0.0])), dict(base, bl_lp_eps=0.5), route]
    keep, S, Vs = pack_classes(OPTs, [V, V, dict(V, m=V["m"] + 300.0), V])
    h = C.c_void_p()
    rc = lib.eepacc_create_classes_bl(C.byref(h), S, Vs, 4, 0, 16)
    msg = lib.eepacc_last_error().decode()
    if rc == 0:
        assert lib.eepacc_num_classes(h) == 4
        lib.eepacc_destroy(h)
    else:
        assert rc == -3 and not h.value and "class" not in msg, msg


def test_from_classes_refuses_mixed_controllers(case):
    """Engine.from_classes picks the entry from the classes' bl_mode and raises where they disagree (before the device)."""
    OPT, BL, TV, V = case
    with pytest.raises(ValueError, match="bl_mode"):
        engine.Engine.from_classes([BL, TV], [V, V], max_batch=4)


def _same(a, b):
    if isinstance(a, dict):
        return set(a) == set(b) and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, np.ndarray) or isinstance(b, np.ndarray):
        return np.array_equal(np.asarray(a), np.asarray(b))
    return a == b


def test_make_use_case_mix_for_the_baseline_controller():
    rec = load_golden("argonne_61505019_lead")
    cases = [3, 8, 10, 12, 7]
    kw = dict(argonne_lead=(rec["t"], rec["v_mph"]))
    ab = make_use_case_mix(cases, 3, "ORIG", 20, **kw)
    bl = make_use_case_mix(cases, 3, "ORIG", 20, controller="bl", **kw)
    K, B = len(cases), 3 * len(cases)
    assert len(bl["OPT"]) == len(bl["V"]) == len(bl["TV"]) == K
    for o, b, tv in zip(ab["OPT"], bl["OPT"], bl["TV"]):
        assert _same(b, Settings_BL(o)) and b["bl_mode"] == 1 and b["N_hor"] == 20 and b["Tvec"].shape == (20,)
        assert _same(tv, Settings_TV(o)) and tv["bl_mode"] == 2
        for key in ("TVlength", "TVinitDist", "TVinitVel"):
            assert tv[key] == o[key]
        assert tv["useCaseNum"] == o["useCaseNum"] and np.array_equal(tv["v_speedLim"], o["v_speedLim"])
    assert _same(ab["TV"], bl["TV"])
    for key in ("class_of", "s0", "v0", "a_minus1", "s_tv", "v_tv", "n_steps", "V"):
        assert _same(ab[key], bl[key]), key
    assert bl["class_of"].tolist() == [0, 1, 2, 3, 4] * 3 and bl["s_tv"].shape == (121, B)
    with pytest.raises(ValueError):
        make_use_case_mix(cases, 3, "ORIG", 20, controller="fb", **kw)


def test_default_mix_is_what_it_was():
    """Without controller the output is the one of before, array for array, restated here from its documentation: the
    settings themselves per class, each instance's start from its use case, the lead of 8 / 9 / 10 and none otherwise."""
    rec = load_golden("argonne_61505019_lead")
    cases = [1, 9, 10, 5]
    mix = make_use_case_mix(cases, 2, "ORIG", 20, argonne_lead=(rec["t"], rec["v_mph"]))
    assert _same({k: v for k, v in mix.items() if k != "TV"},
                 {k: v for k, v in make_use_case_mix(cases, 2, "ORIG", 20, argonne_lead=(rec["t"], rec["v_mph"]), controller="ab").items() if k != "TV"})
    assert set(mix) == {"OPT", "V", "class_of", "s0", "v0", "a_minus1", "s_tv", "v_tv", "n_steps", "TV"}
    OPTs = []
    for c in cases:
        o = default_opt(); o["useCaseNum"] = c; o["argonne_lead"] = (rec["t"], rec["v_mph"])
        OPTs.append(Settings(o, tree="ORIG", N_hor=20))
    n = min(int(round(o["t_sim"] / o["Tvec"][0])) + 1 for o in OPTs)
    assert mix["n_steps"] == n and _same(mix["OPT"], OPTs) and _same(mix["V"], [SetVehicleParameters("ORIG")] * 4)
    assert all("bl_mode" not in o or o["bl_mode"] == 0 for o in mix["OPT"])
    assert mix["class_of"].dtype == np.int32 and mix["class_of"].tolist() == [0, 1, 2, 3] * 2
    for i, k in enumerate(mix["class_of"]):
        o = OPTs[k]
        assert (mix["s0"][i], mix["v0"][i], mix["a_minus1"][i]) == (o["s_init"], o["v_init"], o["a_minus1"])
        if cases[k] in (8, 9, 10):
            assert np.array_equal(mix["s_tv"][:, i], np.asarray(o["s_tv"], dtype=np.float64)[:n])
            assert np.array_equal(mix["v_tv"][:, i], np.asarray(o["v_tv"], dtype=np.float64)[:n])
        else:
            assert np.all(np.isinf(mix["s_tv"][:, i])) and not mix["v_tv"][:, i].any()
