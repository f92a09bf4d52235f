"""What the supplied horizon guesses on class handles (eepacc_classes_step_est, eepacc_run_classes_preview,
generate_lead_and_run_mix(preview=True)) need that can be checked without a GPU.

c1  The ctypes signatures of the two entries are those of eepacc_ab_step_est / eepacc_run_abmpc_preview, the header declares
    them with the same parameter lists, and the built library exports them (the method of tests/test_abi.py and
    tests/test_bl_est_cpu.py).
c2  Python-side argument errors of Engine.classes_step_est / run_classes_preview, raised before anything reaches a device.
c3  generate_lead_and_run_mix refuses an unknown kind and a class without target-vehicle settings before any engine is made,
    with preview=True as without.
c4  scenarios.lead_preview on traces that hold +inf columns (the instances of a mix without a lead) next to finite ones:
    +inf and no NaN at every stage, on sample, between samples and past the last row.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from eepacc_mpc_casadi_matlab_amd import _abi, engine
from eepacc_mpc_casadi_matlab_amd.scenarios import lead_preview, make_use_case_mix

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
PAIRS = (("eepacc_classes_step_est", "eepacc_ab_step_est"), ("eepacc_run_classes_preview", "eepacc_run_abmpc_preview"))


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------------ c1
@pytest.mark.parametrize("cls,ab", PAIRS)
def test_signatures_are_the_ab_counterparts(cls, ab):
    assert _abi.CLASSES_EST_ARGTYPES[cls] == _abi.AB_EST_ARGTYPES[ab]
    assert _params(cls) == _params(ab)                                   # argument names, order and types of the header
    assert len(_params(cls)) == len(_abi.CLASSES_EST_ARGTYPES[cls])
    assert cls in engine.ABI_SYMBOLS


def test_symbols_of_the_built_library():
    from eepacc_mpc_casadi_matlab_amd import build as eb
    lib = C.CDLL(eb.build())
    for cls, _ in PAIRS:
        assert hasattr(lib, cls), cls
    loaded = engine.load_library()
    for cls, _ in PAIRS:
        assert getattr(loaded, cls).argtypes == _abi.CLASSES_EST_ARGTYPES[cls]


def test_engine_methods_have_the_signatures_of_the_plain_ones():
    E = engine.Engine
    for cls, ab in ((E.classes_step_est, E.ab_step_est), (E.run_classes_preview, E.run_abmpc_preview)):
        assert inspect.signature(cls) == inspect.signature(ab)
    p = inspect.signature(engine.generate_lead_and_run_mix).parameters
    assert list(p) == ["mix", "kind", "engines", "device", "preview"] and p["preview"].default is False


# ------------------------------------------------------------------------------------------------ c2
def _bare_engine(N):
    """An Engine without a handle: the argument checks come before any use of the library or a device."""
    import torch
    e = engine.Engine.__new__(engine.Engine)
    e.torch, e.N, e.h = torch, N, None
    return e


def test_python_side_argument_errors():
    N, B = 20, 3
    e = _bare_engine(N)
    z = np.zeros(B); good = np.zeros((N + 1, B))
    with pytest.raises(ValueError, match="s_est and v_est"):
        e.classes_step_est(z, z, z, z, z, z, z, s_est=good)
    with pytest.raises(ValueError, match="s_est and v_est"):
        e.classes_step_est(z, z, z, z, z, z, z, v_est=good)
    with pytest.raises(ValueError, match=r"s_tv_est has shape \(20, 3\)"):
        e.classes_step_est(z, z, z, z, z, z, z, s_tv_est=np.zeros((N, B)))
    with pytest.raises(ValueError, match=r"v_est has shape \(3, 21\)"):
        e.classes_step_est(z, z, z, z, z, z, z, s_est=good, v_est=good.T.copy())
    lead = np.zeros((7, B))
    with pytest.raises(ValueError, match=r"\[n_lead, B\] both"):
        e.run_classes_preview(z, z, z, lead, np.zeros((6, B)))
    with pytest.raises(ValueError, match=r"\[n_lead, B\] both"):
        e.run_classes_preview(z, z, z, lead.ravel(), lead.ravel())
    with pytest.raises(ValueError, match=r"\[n_lead, B\] both"):
        e.run_classes_preview(z, z, z, lead.tolist(), np.zeros((7, B + 1)).tolist())


# ------------------------------------------------------------------------------------------------ c3
@pytest.mark.parametrize("preview", [False, True])
def test_mix_refusals_come_before_any_engine(preview, monkeypatch):
    def no_engine(*a, **k):
        raise AssertionError("an engine was made before the arguments were checked")
    monkeypatch.setattr(engine.Engine, "from_classes", classmethod(no_engine))
    monkeypatch.setattr(engine.Engine, "__init__", no_engine)
    mix = make_use_case_mix([2, 10, 5], 2, "ORIG", 20, n_steps=10)
    for kind in ("fb", "tv", ""):
        with pytest.raises(ValueError, match="kind must be 'ab' or 'bl'"):
            engine.generate_lead_and_run_mix(mix, kind=kind, preview=preview)
    bad = dict(mix, TV=[mix["TV"][0], None, mix["TV"][2]])
    for kind in ("ab", "bl"):
        with pytest.raises(ValueError, match="class 1 has no target-vehicle settings"):
            engine.generate_lead_and_run_mix(bad, kind=kind, preview=preview)
    off = dict(mix, OPT=[dict(o) for o in mix["OPT"]])
    off["OPT"][2]["TV_Ts"] = 0.25
    with pytest.raises(ValueError, match="class 2.*TV_Ts"):
        engine.generate_lead_and_run_mix(off, kind="ab", preview=preview)
    blmix = make_use_case_mix([2, 5], 1, "ORIG", 20, n_steps=10, controller="bl")
    with pytest.raises(ValueError, match="does not fit the classes"):
        engine.generate_lead_and_run_mix(blmix, kind="ab", preview=preview)


# ------------------------------------------------------------------------------------------------ c4
@pytest.mark.parametrize("tvec", ["uniform", "geometric", "multiples"])
def test_lead_preview_keeps_no_lead_columns_infinite(tvec):
    """Columns 0 and 3 have no lead (s_tv = +inf, v_tv = 0, Main.m:77-80), 1 and 2 a moving one; column 4 loses its lead
    half way down the trace.  At every row of the trace, so that the stages fall on samples, between two samples and past
    the last row: a stage is +inf exactly where every sample it reads is, no stage is NaN, and the finite columns are what
    they are without the infinite neighbours."""
    N, n = 12, 9
    Tv = dict(uniform=np.full(N, 0.5), geometric=0.5 * 3.0 ** (np.arange(N) / (N - 1)), multiples=0.3 * (1 + np.arange(N) % 3))[tvec]
    k = np.arange(n, dtype=np.float64)[:, None]
    s = np.full((n, 5), np.inf); v = np.zeros((n, 5))
    s[:, 1:3] = 20.0 + 4.5 * k + np.array([[0.0, 7.0]]); v[:, 1:3] = 9.0
    s[:5, 4] = 30.0 + 3.0 * k[:5, 0]; v[:5, 4] = 6.0
    for r in range(n):
        p = lead_preview(s, v, r, Tv)
        assert p.shape == (N + 1, 5) and not np.isnan(p).any(), (tvec, r)
        assert np.isposinf(p[:, [0, 3]]).all(), (tvec, r)
        assert np.isfinite(p[:, 1:3]).all(), (tvec, r)
        assert np.array_equal(p[:, 1:3], lead_preview(s[:, 1:3], v[:, 1:3], r, Tv)), (tvec, r)
        gone = np.isposinf(p[:N, 4])
        assert gone[-1] and (np.diff(gone.astype(int)) >= 0).all(), (tvec, r)      # once lost, lost for the rest of the horizon
        assert gone[0] == (r >= 5), (tvec, r)
