"""qp_sens.ab_lead_gradient: the derivative of the applied acceleration with respect to the lead prediction s_tv_est, against the
central difference of EEPACC_OUT_AQP of eepacc_ab_step_est.

Case: abo20 / brake_slow_lead of tests/ab_cert_cases.py with the supplied guesses of tests/ab_est_cases.py, whose optimum holds
headway or safety rows with multipliers above 1e-3 of the largest (asserted).  Step delta = 1e-3 m on one s_tv_est[k]: once a
stage with an active lead row, once a stage with none, where the gradient has to be exactly 0.  While the working set holds the
solution is affine in the bounds, so the difference between the two figures is the solver's own error over delta: the bar is
10 x (distance of a_qp to the certified optimum, measured for this configuration by test_gpu_ab_est.py's cold step) / delta.
Both numbers are printed.  The working set (read from the dense operator on the perturbed problems) may not change.
"""
import numpy as np
import pytest

import ab_cert_cases as T
import ab_est_cases as E
from eepacc_mpc_casadi_matlab_amd import qp_sens
from eepacc_mpc_casadi_matlab_amd._abi import OUT, AB_ROW
from test_gpu_ab_est import _certified, _engine, _step, _sup, distances

pytestmark = pytest.mark.gpu
CFG, CASE, DELTA = "abo20", "brake_slow_lead", 1e-3


def test_gradient_against_central_difference():
    C = _certified(CFG)
    OPT, V = C["settings"]
    i = C["names"].index(CASE)
    cols = T.take(C["cols"], np.array([i]))
    sup = _sup(CFG, np.array([i]))
    eng = _engine(OPT, V)
    stage, typ = eng.ab_qp_rows()
    lead = np.isin(typ, [AB_ROW["safe1"], AB_ROW["safe2"], AB_ROW["hwp"]])

    def solve(s_tv_est):
        q = eng.ab_build_qp_est(**cols, **dict(sup, s_tv_est=s_tv_est))
        return q, eng.qp_solve_batched_dual(q.H, q.g, q.A, q.lba, q.uba)

    q, sol = solve(sup["s_tv_est"])
    assert int(sol.status.cpu().numpy()[0]) == 0
    lam, ws = sol.lam_a.cpu().numpy()[0], sol.ws_a.cpu().numpy()[0]
    big = np.abs(lam) > 1e-3 * np.abs(lam).max()
    active = sorted(set(np.minimum(stage[lead & big & (ws != 0)], eng.N - 1)))
    idle = [k for k in range(eng.N) if not (ws[lead & (np.minimum(stage, eng.N - 1) == k)] != 0).any()]
    assert active and idle, (active, idle)
    gx = np.zeros((1, q.H.shape[1])); gx[0, 0] = 1.0                     # loss x[0] = EEPACC_OUT_AQP
    grad = qp_sens.ab_lead_gradient(eng, q, sol, (stage, typ), gx).cpu().numpy()[0]
    solver_err = distances(C, C.setdefault("cold", _step(_engine(OPT, V), C["cols"], **_sup(CFG))), np.arange(len(C["names"])))["a"]
    bar = 10.0 * solver_err / DELTA
    print("distance of a_qp to the certified optimum (%s, cold) %.3e; bar 10 x that / delta = %.3e" % (CFG, solver_err, bar))
    for what, k in (("active stage", active[len(active) // 2]), ("idle stage", idle[0])):
        a, sets = [], []
        for sgn in (+1.0, -1.0):
            p = sup["s_tv_est"].copy(); p[k, 0] += sgn * DELTA
            a.append(_step(_engine(OPT, V), cols, **dict(sup, s_tv_est=p))["out"][OUT["a_qp"], 0])
            sets.append(solve(p)[1].ws_a.cpu().numpy()[0])
        assert np.array_equal(sets[0], ws) and np.array_equal(sets[1], ws), (what, k, "the working set changed: use a smaller delta")
        fd = (a[0] - a[1]) / (2 * DELTA)
        print("%s k = %d: gradient %.12e, central difference %.12e, difference %.3e" % (what, k, grad[k], fd, abs(grad[k] - fd)))
        if what == "idle stage":
            assert grad[k] == 0.0
        else:
            assert grad[k] != 0.0
        assert abs(grad[k] - fd) <= bar, (what, k, grad[k], fd, bar)
