"""The MEX gateway mex/RunOpt_TVMPC.c executed end to end without MATLAB, the way tests/test_mex_run.py runs the other
gateways: compiled with the functional stand-in of the MEX runtime (tests/mexstub/mex_mock.c) and libeepacc, run as a process
on an OPTsettings file.  The stand-in calls a gateway for one output struct; RunOpt_TVMPC has the call form
[s_opt, v_opt, numSolverErrors] = RunOpt_TVMPC(OPTsettings), so tests/mexstub/three_outputs.c calls it with nlhs = 3 and
packs the three outputs.  They are bit-equal with RunOpt_TVMPC of the Python layer (same kernels).  Needs the GPU."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_mex_run import _write_struct, _read_struct, PKG
from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, default_opt

pytestmark = pytest.mark.gpu
STUB = os.path.join(ROOT, "tests", "mexstub")


def _build(tmp_path):
    obj, exe = str(tmp_path / "gw.o"), str(tmp_path / "RunOpt_TVMPC")
    inc = ["-I", STUB, "-I", os.path.join(ROOT, "include")]
    r = subprocess.run(["gcc", "-std=c99", "-O1", "-Wall", "-Wextra", "-Werror", "-DmexFunction=gateway_mexFunction", "-c",
                        os.path.join(ROOT, "mex", "RunOpt_TVMPC.c")] + inc + ["-o", obj], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run(["gcc", "-std=c99", "-O1", obj, os.path.join(STUB, "three_outputs.c"), os.path.join(STUB, "mex_mock.c")] + inc +
                       ["-L", PKG, "-leepacc", "-lm", "-Wl,-rpath," + PKG, "-o", exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return exe


@pytest.mark.parametrize("tree,uc", [("ABO", 2), ("ORIG", 5)])
def test_runopt_tvmpc_gateway(tree, uc, tmp_path):
    from eepacc_mpc_casadi_matlab_amd.engine import RunOpt_TVMPC
    o = default_opt(); o["useCaseNum"] = uc
    OPT = Settings(o, tree=tree, N_hor=20)              # no s_tv / v_tv: the controller generates them
    V = SetVehicleParameters(tree)
    exe = _build(tmp_path)
    fin, fout = str(tmp_path / "in.txt"), str(tmp_path / "out.txt")
    _write_struct(fin, OPT, V)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    S = _read_struct(fout)
    s_opt, v_opt, n_err = RunOpt_TVMPC(OPT, V)
    n = int(round(OPT["t_sim"] / OPT["TV_Ts"])) + 1
    assert S["out1"].shape == (n, 1) and S["out2"].shape == (n, 1) and S["out3"].shape == (1, 1)
    np.testing.assert_array_equal(S["out1"].ravel(), s_opt)
    np.testing.assert_array_equal(S["out2"].ravel(), v_opt)
    assert int(S["out3"][0, 0]) == n_err == 0
    assert s_opt[0] == OPT["TVinitDist"] and s_opt[-1] > 100.0
    # TV_Ts != Tvec(1) is refused, not resampled
    bad = dict(OPT); bad["TV_Ts"] = 0.25
    _write_struct(fin, bad, V)
    r = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "TV_Ts must equal Tvec(1)" in r.stderr
