"""Settings classes per instance (eepacc_create_classes), the parts that need no GPU: what creation refuses, with the
code and a message that names class and field, and the use-case mix of scenarios.make_use_case_mix."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_case, load_golden
from eepacc_mpc_casadi_matlab_amd import build as eb
from eepacc_mpc_casadi_matlab_amd import engine
from eepacc_mpc_casadi_matlab_amd._abi import pack_classes, EEPACC_MAX_CLASSES
from eepacc_mpc_casadi_matlab_amd.scenarios import make_use_case_mix

EINVAL, ENOTSUP = -1, -4


@pytest.fixture(scope="module")
def lib():
    eb.build()
    return engine.load_library()


def _create(lib, OPTs, Vs, n=None):
    keep, S, V = pack_classes(OPTs, Vs)
    h = C.c_void_p()
    rc = lib.eepacc_create_classes(C.byref(h), S, V, len(OPTs) if n is None else n, 0, 16)
    assert not h.value
    return rc, lib.eepacc_last_error().decode()


def test_fields_that_must_agree(lib):
    """N_hor and every entry of Tvec select the kernel and the launch geometry: a class that differs from class 0 is
    EEPACC_EINVAL; the message names the class and the field."""
    OPT, V, *_ = make_case("ORIG", 20)
    rc, msg = _create(lib, [OPT, OPT, make_case("ORIG", 30)[0]], [V] * 3)
    assert rc == EINVAL and "class 2" in msg and "N_hor" in msg, msg
    o = dict(OPT); o["Tvec"] = OPT["Tvec"].copy(); o["Tvec"][7] = 0.75
    rc, msg = _create(lib, [OPT, o], [V] * 2)
    assert rc == EINVAL and "class 1" in msg and "Tvec[7]" in msg, msg


def test_settings_without_a_class_variant(lib):
    """Move blocking, the ICE-map fuel term and the baseline controllers have kernels of their own, which the class variant
    does not instantiate: EEPACC_ENOTSUP in whichever class they appear."""
    OPT, V, *_ = make_case("ABO", 20)
    mb = np.zeros(20, dtype=np.int32); mb[5] = 1
    for k, o, field in ((1, dict(OPT, Mb=mb), "Mb"), (2, dict(OPT, bl_mode=1), "bl_mode"), (0, dict(OPT, bl_mode=2), "bl_mode"),
                        (3, dict(OPT, fuel_map="ICE"), "ab_fuel_term")):
        OPTs = [OPT] * 4
        OPTs[k] = o
        rc, msg = _create(lib, OPTs, [V] * 4)
        assert rc == ENOTSUP and ("class %d" % k) in msg and field in msg, (k, field, msg)
    # what eepacc_create refuses in a single handle is refused per class, with the class in front
    rc, msg = _create(lib, [OPT, dict(OPT, solverToUse=2)], [V] * 2)
    assert rc == ENOTSUP and "class 1" in msg and "solverToUse" in msg, msg


def test_number_of_classes(lib):
    OPT, V, *_ = make_case("ABO", 20)
    rc, msg = _create(lib, [OPT], [V], n=0)
    assert rc == EINVAL and "n_classes" in msg, msg
    assert EEPACC_MAX_CLASSES == 4096
    rc, msg = _create(lib, [OPT] * 4097, [V] * 4097)
    assert rc == EINVAL and "n_classes" in msg, msg


def test_valid_classes_pass_validation(lib):
    """Classes that differ only in what may differ pass the checks: the call gets as far as the device (and fails there
    where there is none)."""
    OPT, V, *_ = make_case("ORIG", 20)
    V2 = dict(V, m=V["m"] + 300.0)
    keep, S, Vs = pack_classes([OPT, dict(OPT, paramEstSetting=2), dict(OPT, W_AB=2.0 * OPT["W_AB"])], [V, V2, V])
    h = C.c_void_p()
    rc = lib.eepacc_create_classes(C.byref(h), S, Vs, 3, 0, 16)
    msg = lib.eepacc_last_error().decode()
    if rc == 0:
        assert lib.eepacc_num_classes(h) == 3
        lib.eepacc_destroy(h)
    else:
        assert rc == -3 and not h.value and "class" not in msg, msg


def test_make_use_case_mix():
    rec = load_golden("argonne_61505019_lead")
    cases = [3, 8, 10, 12, 7]
    mix = make_use_case_mix(cases, 3, "ORIG", 20, argonne_lead=(rec["t"], rec["v_mph"]))
    K, B = len(cases), 3 * len(cases)
    assert len(mix["OPT"]) == K and len(mix["V"]) == K
    assert [o["useCaseNum"] for o in mix["OPT"]] == cases
    assert mix["class_of"].dtype == np.int32
    assert mix["class_of"].tolist() == [0, 1, 2, 3, 4] * 3
    # the shortest simulated time of the chosen cases: use case 10, 60 s at Ts = 0.5 s
    assert mix["n_steps"] == 121
    for key in ("s0", "v0", "a_minus1"):
        assert mix[key].shape == (B,)
    assert mix["s_tv"].shape == (121, B) and mix["v_tv"].shape == (121, B)
    for i in range(B):
        o = mix["OPT"][mix["class_of"][i]]
        assert (mix["s0"][i], mix["v0"][i], mix["a_minus1"][i]) == (o["s_init"], o["v_init"], o["a_minus1"])
        if o["useCaseNum"] in (8, 10):
            assert np.array_equal(mix["s_tv"][:, i], np.asarray(o["s_tv"])[:121])
            assert np.array_equal(mix["v_tv"][:, i], np.asarray(o["v_tv"])[:121])
        else:
            assert np.all(np.isinf(mix["s_tv"][:, i])) and not mix["v_tv"][:, i].any()
    assert mix["v0"][0] == 80 / 3.6 and mix["v0"][3] == 0.0
    short = make_use_case_mix([1, 2], 2, "ORIG", 30, n_steps=40)
    assert short["n_steps"] == 40 and short["s_tv"].shape == (40, 4) and short["OPT"][0]["N_hor"] == 30
    with pytest.raises(ValueError):
        make_use_case_mix([1, 2], 2, "ORIG", 30, n_steps=62)          # use case 1 simulates 30 s: 61 steps
