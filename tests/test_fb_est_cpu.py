"""What the FBMPC entry points with supplied horizon guesses (eepacc_fb_step_est, eepacc_fb_build_qp_est,
eepacc_run_fbmpc_preview) need that can be checked without a GPU.

c1  The ctypes signatures against the header's parameter lists; the symbols are in the built library; the header no longer says
    that supplied guesses are not built for FBMPC and names what stays out.
c2  Python-side argument errors of Engine.fb_step_est / fb_build_qp_est (s_est without v_est, wrong shapes), and
    generate_lead_and_run(kind="fb", preview=True) keeps raising.
c3  The refusal predicate of the three entries (eepacc::fb_est_refusal, csrc/eepacc_cfg.cpp) through a g++-built host harness of
    its own (tests/kernels/fb_est_harness.cpp), on the DevCfg that the settings translation makes: every cause with its code
    and the words of its message; and the ABMPC preview tables it shares (eepacc::preview_tables) on a non-uniform Tvec.  The
    harness with its own main runs as a stand-alone program under -fsanitize=address,undefined.
c4  The inputs of tests/test_gpu_fb_est.py (tests/fb_est_cases.py) are what their docstring says; the oracle's dense problem of
    every instance of every configuration is solved by Oracle.qp_solve with status 0, so that no instance is left out of the
    GPU comparisons; the supplied arrays of every configuration differ from every estimator mode's output by a margin that is
    printed and asserted.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fb_est_cases as E
from eepacc_mpc_casadi_matlab_amd import _abi, engine
from eepacc_mpc_casadi_matlab_amd import build as eb

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
ENTRIES = ("eepacc_fb_step_est", "eepacc_fb_build_qp_est", "eepacc_run_fbmpc_preview")


def _params(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


# ------------------------------------------------------------------------------------------------ c1
def test_signatures_against_the_header():
    step, plain = _params("eepacc_fb_step_est"), _params("eepacc_fb_step")
    assert step[:12] == plain[:12] and step[15:] == plain[12:]           # eepacc_fb_step's list with the three guesses after a_tv_prev
    assert step[12:15] == ["const double* s_est", "const double* v_est", "const double* s_tv_est"]
    build, plain = _params("eepacc_fb_build_qp_est"), _params("eepacc_fb_build_qp")
    assert build[:9] == plain[:9] and build[12:] == plain[9:] and build[9:12] == step[12:15]
    assert _params("eepacc_run_fbmpc_preview") == _params("eepacc_run_abmpc_preview")
    for name in ENTRIES:
        assert len(_params(name)) == len(_abi.FB_EST_ARGTYPES[name]), name
        assert name in engine.ABI_SYMBOLS
    assert _abi.FB_EST_ARGTYPES["eepacc_run_fbmpc_preview"] == _abi.AB_EST_ARGTYPES["eepacc_run_abmpc_preview"]


def test_symbols_of_the_built_library():
    lib = C.CDLL(eb.build())
    for name in ENTRIES:
        assert hasattr(lib, name), name
    loaded = engine.load_library()
    for name in ENTRIES:
        assert getattr(loaded, name).argtypes == _abi.FB_EST_ARGTYPES[name]


def test_header_says_what_is_built():
    assert not re.search(r"Not built:\s*supplied guesses for FBMPC,", HDR)
    m = re.search(r"Not built: supplied guesses for FBMPC steps through the dense path[^.]*\.", HDR)
    assert m and "settings classes" in m.group(0)
    for words in ("Row N_hor of s_tv_est is not read", "All three NULL: bit for bit eepacc_fb_step / eepacc_fb_build_qp",
                  "the builder entry still works"):
        assert words in HDR, words
    for name in ("eepacc_fbs.hip", "eepacc_fbs_est.hip", "eepacc_fb_qp.hip", "eepacc_fb_qp_est.hip"):
        assert name in eb.SOURCES and os.path.exists(os.path.join(eb.CSRC, name)), name


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
    step = lambda **kw: e.fb_step_est(z, z, z, z, z, z, z, z, z, z, **kw)
    build = lambda **kw: e.fb_build_qp_est(z, z, z, z, z, z, z, **kw)
    for fn in (step, build):
        with pytest.raises(ValueError, match="s_est and v_est"):
            fn(s_est=good)
        with pytest.raises(ValueError, match="s_est and v_est"):
            fn(v_est=good)
        with pytest.raises(ValueError, match=r"s_tv_est has shape \(20, 3\)"):
            fn(s_tv_est=np.zeros((N, B)))
        with pytest.raises(ValueError, match=r"v_est has shape \(3, 21\)"):
            fn(s_est=good, v_est=good.T.copy())
        with pytest.raises(ValueError, match=r"s_est has shape \(63,\)"):
            fn(s_est=good.ravel(), v_est=good)


def test_generate_lead_and_run_keeps_refusing_an_fb_preview():
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, default_opt
    OPT = Settings(default_opt(), tree="ABO", N_hor=20)
    with pytest.raises(ValueError, match="preview"):
        engine.generate_lead_and_run(OPT, kind="fb", preview=True)


# ------------------------------------------------------------------------------------------------ c3
HARNESS = os.path.join(ROOT, "tests", "kernels", "fb_est_harness.cpp")
ENOTSUP = -4


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("fb_est_harness"))
    lib = os.path.join(out, "libfb_est_harness.so")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-fPIC", "-shared", "-I", eb.CSRC, HARNESS,
           os.path.join(eb.CSRC, "eepacc_cfg.cpp"), "-o", lib]
    subprocess.run(cmd, check=True, timeout=300)
    L = C.CDLL(lib)
    L.fh_last_error.restype = C.c_char_p
    L.fh_refusal.restype = C.c_int
    L.fh_refusal.argtypes = [C.POINTER(_abi.SettingsPOD), C.POINTER(_abi.Vehicle), C.c_char_p, C.c_int, C.c_int, C.c_int]
    L.fh_preview_tables.argtypes = [_abi.c_double_p, C.c_int, _abi.c_int32_p, _abi.c_double_p]
    return L


def _refusal(L, OPT, V, who, n_classes, structured, needs_structured):
    holder, veh = _abi.SettingsHolder(OPT), _abi.make_vehicle(V)
    rc = L.fh_refusal(C.byref(holder.pod), C.byref(veh), who.encode(), n_classes, int(structured), int(needs_structured))
    return rc, L.fh_last_error().decode()


def test_refusal_predicate(host):
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV
    OPT, V = E.settings("abo20")
    mb = np.zeros(20, dtype=np.int64); mb[[2, 7]] = 1
    bq = np.array([185, 1.296e-20, 2.301, 2.5e-4, 0.003728, -0.000181])
    for who in ENTRIES:
        needs = who != "eepacc_fb_build_qp_est"
        assert _refusal(host, OPT, V, who, 0, True, needs) == (0, "")
        rc, msg = _refusal(host, OPT, V, who, 2, False, needs)
        assert rc == ENOTSUP and msg.startswith(who + ":") and "eepacc_create_classes" in msg
        for S, word in ((Settings_BL(OPT), "bl_mode = 1"), (Settings_TV(OPT), "bl_mode = 2")):
            rc, msg = _refusal(host, S, V, who, 0, False, needs)
            assert rc == ENOTSUP and msg.startswith(who + ":") and word in msg
        for kw, word in ((dict(Mb=mb), "Mb[2] != 0"), (dict(b_quadr=bq), "b_quadr(4) != 0"), ({}, "EEPACC_FB_DENSE=1")):
            rc, msg = _refusal(host, dict(OPT, **kw), V, who, 0, False, needs)
            if needs:
                assert rc == ENOTSUP and msg.startswith(who + ":") and word in msg and "dense path" in msg
                assert "eepacc_fb_build_qp_est still builds the problem" in msg
            else:
                assert (rc, msg) == (0, "")                              # the builder entry serves dense-path handles


def test_sanitized_host_program(tmp_path):
    """tests/kernels/fb_est_harness.cpp with its own main (-DFB_EST_HARNESS_MAIN): the refusal predicate on every cause, Mb on
    the last stage of the mask among them, and the preview tables at N = 63, as a program of its own under AddressSanitizer and
    UndefinedBehaviorSanitizer (tests/test_cfg_cpu.py::test_sanitized_host_program)."""
    exe = str(tmp_path / "fb_est_sanitize")
    cmd = [os.environ.get("CXX", "g++"), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan",     # the runtimes in the program itself
           "-DFB_EST_HARNESS_MAIN", "-I", eb.CSRC, HARNESS, os.path.join(eb.CSRC, "eepacc_cfg.cpp"), "-o", exe]
    subprocess.run(cmd, check=True, timeout=300)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and "0 failed" in r.stdout, (r.returncode, r.stdout, r.stderr)


def test_preview_tables_are_the_specification(host):
    """The tables that eepacc_run_fbmpc_preview shares with eepacc_run_abmpc_preview against scenarios.lead_preview's own rule."""
    for Tv in (np.full(20, 0.5), E.TVEC24, np.full(33, 0.3), 0.5 * np.array([1.0, 1.0, 2.0, 2.5, 4.0])):
        N = Tv.size
        idx, frac = np.zeros(N, dtype=np.int32), np.zeros(N)
        host.fh_preview_tables(_abi.as_dptr(np.ascontiguousarray(Tv)), N, _abi.as_iptr(idx), _abi.as_dptr(frac))
        tau = np.concatenate([[0.0], np.cumsum(Tv)])[:N]
        p = tau / Tv[0]
        assert (frac >= 0.0).all() and (frac < 1.0).all()
        assert np.abs(idx + frac - p).max() < 2e-9 * max(1.0, p.max())
        on_sample = np.abs(p - np.round(p)) < 1e-9
        assert (frac[on_sample] == 0.0).all() and np.array_equal(idx[on_sample], np.round(p[on_sample]).astype(np.int32))


# ------------------------------------------------------------------------------------------------ c4
def test_supplied_guesses_are_what_the_docstring_says():
    assert {N for _, N, _ in E.CONFIGS.values()} == {2, 3, 20, 24, 32, 33, 63}
    for cfg, (tree, N, kw) in E.CONFIGS.items():
        OPT, V = E.settings(cfg)
        assert int(OPT["N_hor"]) == N and len(OPT["Tvec"]) == N
        cols = E.inputs(cfg)
        se, ve, st = E.supplied(cfg)
        B = E.B
        assert se.shape == ve.shape == st.shape == (N + 1, B) and all(cols[n].shape == (B,) for n in E.INS)
        assert (cols["v"] > 1.0).all()                                    # well above 1e-3 m/s
        assert np.array_equal(se[0], cols["s"]) and np.array_equal(ve[0], cols["v"]) and np.array_equal(st[0, :B - 1], cols["s_tv"][:B - 1])
        assert (np.diff(se, axis=0) >= 0).all() and (ve >= 0).all()
        fin = st[:, :B - 2]
        assert (np.diff(fin, axis=0) >= 0).all() and np.isfinite(fin).all()
        assert np.isposinf(st[:, B - 1]).all()
        assert np.isposinf(st[max(N // 2, 1):, B - 2]).all() and np.isfinite(st[:N // 2, B - 2]).all()
        Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
        const_speed = cols["s_tv"][None, :] + np.concatenate([[0.0], np.cumsum(Tv)])[:, None] * cols["v_tv"][None, :]
        assert (fin >= const_speed[:, :B - 2] - 1e-9).all()               # never behind the constant-speed guess
        if N >= 20:                                                       # the lead's acceleration reverses inside the horizon
            dd = np.diff(np.diff(fin, axis=0) / Tv[:, None], axis=0)       # change of the lead's speed from stage to stage
            assert (dd[:N // 2 - 1] > 0).any() and (dd[N // 2 + 1:] < 0).any()
        dev = E.device_arrays(cfg)
        assert np.isnan(dev["s_tv_est"][-1]).all() and np.array_equal(dev["s_tv_est"][:-1], st[:-1])
        idx = np.array([4, 0])
        sub = E.device_arrays(cfg, idx)
        assert np.array_equal(sub["v_est"], ve[:, idx]) and sub["v_est"].flags["C_CONTIGUOUS"]
    assert E.settings("notaylor20")[0]["FBuseTaylor"] in (0, False) and E.settings("abo20")[0]["FBuseTaylor"]
    assert np.ptp(E.settings("tvec24")[0]["Tvec"]) > 0.9
    slope = np.asarray(E.settings("grade20")[0]["slope"])
    assert (slope == E.GRADE).all() and E.GRADE > 0.029


@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_no_estimator_mode_produces_the_supplied_arrays(cfg):
    """Per instance the largest distance of a supplied array to the estimator's, and of those the smallest, must exceed a margin.
    N >= 20: 0.25 m/s and 0.25 m.  N = 2, 3: the ego's speed can depart by at most 0.5 m/s per stage and the lead's by less, so
    the margin is 1e-3 (m/s, m): still five to six orders above the bars of the GPU comparisons (1e-9 m/s, 1e-8 m), which an
    estimator's array in place of the supplied one would miss by as much.  The lead's guess is compared on the rows that are
    read (0 .. N-1).  At N = 2 those are the measurement and one stage at the measured lead speed, which is the constant-speed
    estimate by construction: there the lead side is told from the estimator only by the instances with +inf, and its margin is
    printed, not asserted."""
    N = E.CONFIGS[cfg][1]
    se, ve, st = E.supplied(cfg)
    fin = slice(0, E.B - 2)
    bar = 0.25 if N >= 20 else 1e-3
    for mode in (0, 1):
        oe, ov, ot = E.estimator_outputs(cfg, mode, mode)
        dv, ds = np.abs(ve - ov).max(axis=0).min(), np.abs(se - oe).max(axis=0).min()
        dl = np.abs(st[:N, fin] - ot[:N, fin]).max(axis=0).min()
        print("%s: smallest per-instance distance to estimator mode %d: v_est %.3g m/s, s_est %.3g m, s_tv_est (rows read) %.3g m" % (cfg, mode, dv, ds, dl))
        assert dv > bar and ds > bar, (cfg, mode, dv, ds)
        if N > 2:
            assert dl > bar, (cfg, mode, dl)
    assert np.isposinf(st[:N, E.B - 1]).all() and np.isposinf(st[N // 2:N, E.B - 2]).all()     # no estimator makes these
    # mode 2 (the shifted previous solution) starts from zeros on a fresh handle: further away still
    assert np.abs(ve[1:]).max(axis=0).min() > 1.0


@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_the_oracle_solves_every_instance(cfg):
    D, probs = E.oracle_problems(cfg)
    assert len(probs) == E.B
    for i, P in enumerate(probs):
        x, _, st = D.orc.qp_solve(P["H"], P["c"], P["G"], P["lb"], P["ub"])
        assert st["status"] == 0, (cfg, i, st)
        y = P["G"] @ x
        assert np.maximum(np.maximum(y - P["ub"], P["lb"] - y), 0.0).max() < 1e-6, (cfg, i)
        assert np.isfinite(0.5 * x @ P["H"] @ x + P["c"] @ x)
