"""What the entry points with supplied horizon guesses (eepacc_ab_step_est, eepacc_ab_build_qp_est, eepacc_run_abmpc_preview)
need that can be checked without a GPU.

c1  scenarios.lead_preview / preview_tables, the numpy specification of the preview rule, against hand values.
c2  qp_sens.lead_gradient_from_uba (the arithmetic of ab_lead_gradient) on a synthetic row table against a plain loop.
c3  The inputs of tests/test_gpu_ab_est.py (tests/ab_est_cases.py) on the CPU oracle's dense problem: every case is solved and
    certified by tests/qp_cert.py, and at most a quarter of a configuration's cases is degenerate by the measure of
    tests/ab_cert_cases.py (read_certificate's scaled ratio below DEGENERATE_RATIO, or a singular refinement), so the GPU test's
    point-by-point comparison covers at least three quarters of every configuration.
"""
import numpy as np
import pytest

import ab_cert_cases as T
import ab_est_cases as E
from eepacc_mpc_casadi_matlab_amd import qp_sens
from eepacc_mpc_casadi_matlab_amd._abi import AB_ROW
from eepacc_mpc_casadi_matlab_amd.scenarios import lead_preview, preview_tables


# ------------------------------------------------------------------------------------------------ c1
def test_preview_tables_uniform_and_dyadic():
    idx, frac = preview_tables(np.full(5, 0.5))
    assert idx.tolist() == [0, 1, 2, 3, 4] and frac.tolist() == [0.0] * 5
    idx, frac = preview_tables(np.array([0.5, 0.75, 0.5, 1.0]))           # tau = 0, 0.5, 1.25, 1.75
    assert idx.tolist() == [0, 1, 2, 3] and frac.tolist() == [0.0, 0.0, 0.5, 0.5]


def test_preview_tables_snap_whole_multiples_of_a_non_dyadic_step():
    """Ts = 0.3 and stages of 1, 2 and 3 Ts: tau / Ts is a whole number only up to rounding (0.3 + 0.6 = 0.8999999999999999 in
    double), and the stage still reads a sample with frac exactly 0."""
    Tv = np.array([0.3, 0.6, 0.9, 0.3, 0.6])
    idx, frac = preview_tables(Tv)
    assert idx.tolist() == [0, 1, 3, 6, 7]
    assert frac.tolist() == [0.0] * 5
    assert float(np.float64(0.3) + np.float64(0.6)) != 0.9                # the case does what it says
    idx, frac = preview_tables(np.full(40, 0.3))
    assert idx.tolist() == list(range(40)) and not frac.any()


def test_lead_preview_hand_values():
    s = np.array([10.0, 12.0, 16.0, 24.0, 40.0]); v = np.array([4.0, 8.0, 16.0, 32.0, 3.0])
    Tv = np.array([0.5, 0.75, 0.5, 1.0])                                 # rows ahead: 0, 1, 2.5, 3.5
    p = lead_preview(s, v, 0, Tv)
    assert p.shape == (5, 1)
    assert p[:4, 0].tolist() == [10.0, 12.0, 0.5 * 16.0 + 0.5 * 24.0, 0.5 * 24.0 + 0.5 * 40.0]       # exact sample, fractional index
    p = lead_preview(s, v, 1, Tv)                                         # rows 1, 2, 3.5, 4.5: the last is past the last row
    assert p[:4, 0].tolist() == [12.0, 16.0, 32.0, 40.0 + 3.0 * (1.75 - 3 * 0.5)]
    p = lead_preview(s, v, 3, Tv)                                         # rows 3, 4 (the last row itself: the sample), 5.5, 6.5
    assert p[:4, 0].tolist() == [24.0, 40.0, 40.0 + 3.0 * (1.25 - 0.5), 40.0 + 3.0 * (1.75 - 0.5)]
    p = lead_preview(s, v, 4, Tv)                                         # the step of the last row: everything extrapolated
    assert p[:4, 0].tolist() == [40.0, 40.0 + 3.0 * 0.5, 40.0 + 3.0 * 1.25, 40.0 + 3.0 * 1.75]


def test_lead_preview_no_lead_stays_infinite():
    s = np.full((6, 2), np.inf); s[:, 1] = np.arange(6.0)
    v = np.zeros((6, 2)); v[:, 1] = 2.0
    for r in (0, 3, 5):
        p = lead_preview(s, v, r, np.array([0.5, 0.75, 0.5, 1.0]))
        assert np.isposinf(p[:, 0]).all() and np.isfinite(p[:, 1]).all()


# ------------------------------------------------------------------------------------------------ c2
def test_lead_gradient_from_uba_against_a_plain_loop():
    N, B = 4, 3
    stage, typ = T.row_map("ABO", N)
    tnum = np.array([AB_ROW[t] for t in typ])
    rng = np.random.default_rng(5)
    g = rng.standard_normal((B, stage.size))
    want = np.zeros((B, N + 1))
    for b in range(B):
        for r in range(stage.size):
            if typ[r] in ("safe1", "safe2", "hwp"):
                want[b, min(stage[r], N - 1)] += g[b, r]                  # the terminal rows read stage N - 1
    got = qp_sens.lead_gradient_from_uba(g, stage, tnum, N)
    assert got.shape == (B, N + 1)
    assert np.abs(got - want).max() <= 4 * np.finfo(float).eps * np.abs(g).max() * 5
    assert (got[:, N] == 0.0).all()
    # a stage none of whose lead rows carries a gradient gets exactly 0
    g2 = g.copy(); g2[:, (stage == 1) & np.isin(typ, ("safe1", "safe2", "hwp"))] = 0.0
    assert (qp_sens.lead_gradient_from_uba(g2, stage, tnum, N)[:, 1] == 0.0).all()
    import torch
    gt = qp_sens.lead_gradient_from_uba(torch.as_tensor(g), stage, tnum, N)
    assert np.array_equal(gt.numpy(), got)


# ------------------------------------------------------------------------------------------------ c3
def test_supplied_guesses_are_what_the_docstring_says():
    for cfg in E.CONFIGS:
        N = T.CONFIGS[cfg][1]
        _, cols = E.inputs(cfg)
        se, ve, st = E.supplied(cfg)
        B = cols["s"].size
        assert 5 <= B <= 16 and se.shape == ve.shape == st.shape == (N + 1, B)
        assert np.array_equal(se[0], cols["s"]) and np.array_equal(ve[0], cols["v"])
        assert (np.diff(se, axis=0) >= 0).all() and (ve >= 0).all()
        half = B >= 8                                                     # the instance whose lead ends in mid-horizon
        fin = st[:, :B - 2] if half else st[:, :B - 1]
        assert (np.diff(fin, axis=0) >= 0).all() and np.isfinite(fin).all()
        assert np.isposinf(st[:, B - 1]).all()
        assert not half or (np.isposinf(st[N // 2:, B - 2]).all() and np.isfinite(st[:N // 2, B - 2]).all())
        if N >= 20:                                                       # the lead's acceleration reverses inside the horizon
            dd = np.diff(fin, n=2, axis=0)
            assert (dd[:N // 2 - 1] > 0).any() and (dd[N // 2 + 1:] < 0).any()


@pytest.mark.parametrize("cfg", E.CONFIGS)
def test_cases_are_certified_and_few_are_degenerate(cfg):
    tree, N, _ = T.CONFIGS[cfg]
    OPT, _ = T.settings(cfg)
    D, probs = E.oracle_problems(cfg)
    stage, typ = T.config_row_map(cfg)
    names, _ = E.inputs(cfg)
    dropped = []
    for nm, P in zip(names, probs):
        x, _, st = D.solve(P)
        assert st["status"] == 0, (cfg, nm)
        R = T.certify(P["H"], P["c"], P["G"], P["lb"], P["ub"], x, stage, typ, N, OPT)
        if R["degenerate"]:
            dropped.append(nm)
        else:
            assert R["cert"]["pviol"] <= T.PVIOL_MAX and R["cert"]["stat"] <= T.STAT_MAX, (cfg, nm)
    print("%s: %d cases, degenerate %s" % (cfg, len(names), dropped))
    assert len(dropped) <= E.MAX_DROPPED * len(names), (cfg, dropped)


# ------------------------------------------------------------------------------------------------ sanitizer run
def test_sanitized_preview_tables(tmp_path):
    """tests/kernels/preview_sanitize_main.cpp calls the host-side builder of the preview tables (eepacc_cfg.cpp) at N = 2 and
    63, on the snap rule and on fractional indices, as a program of its own under AddressSanitizer and
    UndefinedBehaviorSanitizer, with the pattern of tests/test_cfg_cpu.py::test_sanitized_host_program."""
    import os
    import subprocess
    import cfg_harness
    from eepacc_mpc_casadi_matlab_amd import build as eb
    exe = str(tmp_path / "preview_sanitize")
    cmd = [cfg_harness.gxx(), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",
           "-I", eb.CSRC, os.path.join(os.path.dirname(os.path.abspath(__file__)), "kernels", "preview_sanitize_main.cpp"),
           cfg_harness.UNIT, "-o", exe]
    subprocess.run(cmd, check=True, timeout=cfg_harness.COMPILE_TIMEOUT_S)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "" and "preview_tables: ok" in r.stdout, (r.returncode, r.stdout, r.stderr)
