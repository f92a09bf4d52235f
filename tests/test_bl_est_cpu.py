"""What the baseline controller's entry points with supplied horizon guesses (eepacc_bl_step_est, eepacc_bl_build_qp_est,
eepacc_run_blmpc_preview) need that can be checked without a GPU.

c1  The ctypes signatures of the three entries are those of their ABMPC counterparts, the symbols are in the built library and
    the header declares them with the same parameter lists.
c2  Python-side argument errors of Engine.bl_step_est / bl_build_qp_est (s_est without v_est, wrong shapes) and of
    generate_lead_and_run (kind="fb" with preview=True): raised before anything reaches a device.
c3  The inputs of tests/test_gpu_bl_est.py (tests/bl_est_cases.py) are what their docstring says, and the oracle's own solve of
    the oracle's own problem on them fails on at most 1 of 6 instances per configuration: the cap of the GPU test's objective
    comparison (test 4 there) is met by the oracle alone.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import bl_est_cases as E
from eepacc_mpc_casadi_matlab_amd import _abi, engine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
PAIRS = (("eepacc_bl_step_est", "eepacc_ab_step_est"), ("eepacc_bl_build_qp_est", "eepacc_ab_build_qp_est"),
         ("eepacc_run_blmpc_preview", "eepacc_run_abmpc_preview"))


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------------ c1
@pytest.mark.parametrize("bl,ab", PAIRS)
def test_signatures_are_the_ab_counterparts(bl, ab):
    assert _abi.BL_EST_ARGTYPES[bl] == _abi.AB_EST_ARGTYPES[ab]
    assert _params(bl) == _params(ab)                                    # argument names, order and types of the header
    assert len(_params(bl)) == len(_abi.BL_EST_ARGTYPES[bl])
    assert bl in engine.ABI_SYMBOLS


def test_symbols_of_the_built_library():
    from eepacc_mpc_casadi_matlab_amd import build as eb
    lib = C.CDLL(eb.build())
    for bl, _ in PAIRS:
        assert hasattr(lib, bl), bl
    loaded = engine.load_library()
    for bl, _ in PAIRS:
        assert getattr(loaded, bl).argtypes == _abi.BL_EST_ARGTYPES[bl]


# ------------------------------------------------------------------------------------------------ c2
def _bare_engine(N):
    """An Engine without a handle: the argument checks of the bl_ methods come before any use of the library or a device."""
    import torch
    e = engine.Engine.__new__(engine.Engine)
    e.torch, e.N, e.h = torch, N, None
    return e


def test_python_side_argument_errors():
    N, B = 20, 3
    e = _bare_engine(N)
    z = np.zeros(B); good = np.zeros((N + 1, B))
    import torch
    for mk in (np.asarray, torch.as_tensor, lambda a: a.tolist()):      # what the methods accept: numpy, torch, lists
        assert e._est_check(mk(z), mk(good), mk(good), None) is None
        with pytest.raises(ValueError, match=r"s_tv_est has shape \(3, 21\)"):
            e._est_check(mk(z), None, None, mk(good.T.copy()))
    for fn in (e.bl_step_est, e.bl_build_qp_est):
        with pytest.raises(ValueError, match="s_est and v_est"):
            fn(z, z, z, z, z, z, z, s_est=good)
        with pytest.raises(ValueError, match="s_est and v_est"):
            fn(z, z, z, z, z, z, z, v_est=good)
        with pytest.raises(ValueError, match=r"s_tv_est has shape \(20, 3\)"):
            fn(z, z, z, z, z, z, z, s_tv_est=np.zeros((N, B)))
        with pytest.raises(ValueError, match=r"v_est has shape \(3, 21\)"):
            fn(z, z, z, z, z, z, z, s_est=good, v_est=good.T.copy())
        with pytest.raises(ValueError, match=r"s_est has shape \(63,\)"):
            fn(z, z, z, z, z, z, z, s_est=good.ravel(), v_est=good)


def test_fb_has_no_preview():
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, default_opt
    OPT = Settings(default_opt(), tree="ABO", N_hor=20)
    with pytest.raises(ValueError, match="preview"):
        engine.generate_lead_and_run(OPT, kind="fb", preview=True)


# ------------------------------------------------------------------------------------------------ c3
def test_supplied_guesses_are_what_the_docstring_says():
    for cfg, (tree, N) in E.CONFIGS.items():
        BL, _ = E.settings(cfg)
        assert int(BL["N_hor"]) == N and int(BL["bl_mode"]) == 1
        cols = E.inputs(cfg)
        se, ve, st = E.supplied(cfg)
        B = E.B
        assert se.shape == ve.shape == st.shape == (N + 1, B)
        assert np.array_equal(se[0], cols["s"]) and np.array_equal(ve[0], cols["v"])
        assert (np.diff(se, axis=0) >= 0).all() and (ve >= 0).all()
        Tv = np.asarray(BL["Tvec"], dtype=np.float64)
        const_speed = cols["s"][None, :] + np.concatenate([[0.0], np.cumsum(Tv)])[:, None] * cols["v"][None, :]
        if N >= 20:
            assert np.abs(se - const_speed).max() > 1.0                   # unrelated to the constant-speed guess
        fin = st[:, :B - 2]
        assert (np.diff(fin, axis=0) >= 0).all() and np.isfinite(fin).all()
        assert np.isposinf(st[:, B - 1]).all()
        assert np.isposinf(st[N // 2:, B - 2]).all() and np.isfinite(st[:N // 2, B - 2]).all()
        if N >= 20:                                                       # the lead's acceleration reverses inside the horizon
            dd = np.diff(fin, n=2, axis=0)
            assert (dd[:N // 2 - 1] > 0).any() and (dd[N // 2 + 1:] < 0).any()
        dev = E.device_arrays(cfg)
        assert np.isnan(dev["s_tv_est"][-1]).all() and np.array_equal(dev["s_tv_est"][:-1], st[:-1])


@pytest.mark.parametrize("cfg", E.STEP_CONFIGS)
def test_the_oracle_alone_stays_within_the_cap(cfg):
    D, probs = E.oracle_problems(cfg)
    failed = []
    for i, P in enumerate(probs):
        x, _, st = D.orc.qp_solve(P["H"], P["c"], P["G"], P["lb"], P["ub"])
        if st["status"] != 0:
            failed.append(i)
            continue
        y = P["G"] @ x
        assert np.maximum(np.maximum(y - P["ub"], P["lb"] - y), 0.0).max() < 1e-6, (cfg, i)
        assert np.isfinite(E.objective(P["H"], P["c"], x))
    print("%s: the oracle's solve fails on %s of %d" % (cfg, failed, len(probs)))
    assert len(failed) <= E.MAX_LEFT_OUT, (cfg, failed)
