"""qp_sens without a GPU: the numpy specification of eepacc_qp_kkt_solve_batched (kkt_solve_reference) and the two recipes
(jvp_rhs, vjp_grads) reproduce central differences of a CPU solver's solution, and are adjoint to each other.

Solver: the CPU oracle's qp_solve followed by qp_cert.refined_solution (tests/qp_sens_cases.cpu_solution).  Problems,
directions and steps: tests/qp_sens_cases.py -- every problem of its six cases, four directions each (g, the bounds, H,
A).  For every one of them the working set of the solver at +-h equals the base one and strict complementarity holds with
the margin 10 h x data scale (asserted, none skipped).

Tolerance of the central difference.  On a fixed working set x is linear in g and the bounds, so the quotient has no
truncation error there; along H and A it has one of O(h^2), and qp_sens_cases.step takes a ten times smaller step there,
which makes it a thousandth of its share at the other step.  What remains is rounding.  The recipe is fed the direction
the two solves actually took (qp_sens_cases.effective_direction: the data are rounded to float64 after the step).  x(+-h)
are the float64 roundings of the long-double refined solutions x_ld(+-h), so the quotient is off by at most
(e+ + e-) / 2h, e+- = |x(+-h) - x_ld(+-h)|_inf (half an ulp of x each) -- the allowance tests/test_gpu_qp_kkt.py uses for the
device; x_ld is good to 1e-19.  The recipe's own dx comes from a long-double solve of a right-hand side formed in float64:
64 eps cond_2(K) max(1, |dx|_inf) for that.  Tolerance = (e+ + e-) / 2h + 64 eps cond_2(K) max(1, |dx|_inf).
Measured (largest |dx_fd - dx|_inf over the problems and directions of the case / smallest tolerance; the largest
tolerance relative to max(1, |dx|_inf) on one problem and direction):
    spd-3x5 6.2e-11 / 3.4e-14 (6.8e-11), spd-9x16 1.3e-10 / 1.2e-11 (2.7e-10), spd-65x130 1.9e-10 / 1.6e-11 (2.5e-10),
    soft-20+43-10-lbx-w10000 4.4e-8 / 2.2e-9 (4.0e-8), soft-20+43-10-row-w1 3.9e-10 / 2.1e-11 (4.4e-10),
    indef-12x9-0.05 1.7e-10 / 9.9e-12 (1.9e-10).
"""
import numpy as np
import pytest

import qp_cert as Q
import qp_sens_cases as SC
from conftest import make_case
from eepacc_mpc_casadi_matlab_amd import qp_sens

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def orc():
    from oracle.loader import Oracle
    return Oracle(*make_case("ABO", 20)[:2])


_BASE = {}


def _base(orc, cid):
    if cid not in _BASE:
        probs = Q.make_case(cid)[1]
        _BASE[cid] = (probs, [SC.cpu_solution(orc.qp_solve, p) for p in probs])
    return _BASE[cid]


def _jvp(p, s, d):
    """(dx, dlam_a, dlam_x) of the recipe with the numpy specification as the linear solver."""
    H, g, A = SC.problem(p)[:3]
    b1 = lambda v: None if v is None else v[None]
    r = qp_sens.jvp_rhs(s["x"][None], s["lam_a"][None], s["ws_a"][None], s["ws_x"][None],
                        *[b1(d.get(k)) for k in ("g", "lba", "uba", "lbx", "ubx", "H", "A")])
    return qp_sens.kkt_solve_reference(H, A, s["ws_a"], s["ws_x"], r[0][0], r[1][0], r[2][0])[:3]


@pytest.mark.parametrize("cid", SC.CASES)
def test_jvp_reproduces_central_differences(cid, orc):
    probs, sols = _base(orc, cid)
    worst, tightest, ratio = 0.0, np.inf, 0.0
    for i, (p, s) in enumerate(zip(probs, sols)):
        m, scale, h = SC.margin(p, *[s[k] for k in ("x", "lam_a", "lam_x", "ws_a", "ws_x")]), SC.data_scale(p), SC.STEP[cid]
        print("%s[%d] held %d + %d, margin %.3e, 10 h scale %.3e" % (cid, i, (s["ws_a"] != 0).sum(), (s["ws_x"] != 0).sum(), m, 10 * h * scale))
        assert m > 10.0 * h * scale, (cid, i, m, scale)
        H, g, A = SC.problem(p)[:3]
        cond = np.linalg.cond(qp_sens.kkt_matrix(H, A, s["ws_a"], s["ws_x"])[0])
        for kind in SC.KINDS:
            d, h = SC.direction(cid, i, kind, p), SC.step(cid, kind)
            pp, pm = SC.perturbed(p, d, h), SC.perturbed(p, d, -h)
            sp, sm = SC.cpu_solution(orc.qp_solve, pp), SC.cpu_solution(orc.qp_solve, pm)
            for side in (sp, sm):
                assert (side["ws_a"] == s["ws_a"]).all() and (side["ws_x"] == s["ws_x"]).all(), (cid, i, kind)
            fd = (sp["x"] - sm["x"]) / (2.0 * h)
            dx = _jvp(p, s, SC.effective_direction(pp, pm, d, h))[0]
            e = [float(np.abs(v["x"].astype(Q.LD) - v["x_ld"]).max()) for v in (sp, sm)]
            tol = (e[0] + e[1]) / (2.0 * h) + 64.0 * EPS * cond * max(1.0, np.abs(dx).max())
            err = np.abs(fd - dx).max()
            print("%s[%d] %-6s h %.0e |dx| %.3e  |fd - dx| %.3e  tol %.3e = (%.1e + %.1e)/2h + %.1e"
                  % (cid, i, kind, h, np.abs(dx).max(), err, tol, e[0], e[1], tol - (e[0] + e[1]) / (2.0 * h)))
            assert err <= tol, (cid, i, kind, err, tol)
            worst, tightest, ratio = max(worst, err), min(tightest, tol), max(ratio, tol / max(1.0, np.abs(dx).max()))
    print("%s largest |fd - dx| %.2e, smallest tolerance %.2e, largest tolerance / max(1, |dx|) %.1e" % (cid, worst, tightest, ratio))


@pytest.mark.parametrize("cid", SC.CASES)
def test_jvp_and_vjp_are_adjoint(cid, orc):
    """<gx, dx> + <glam, dlam> = <dL/dg, dg> + <dL/dlba, dlba> + ... + <dL/dH, dH> + <dL/dA, dA> for random gradients and
    all directions at once; both sides are sums of about n^2 products of O(1) numbers through one solve each, so they
    agree to 64 eps cond_2(K) times the sum of the magnitudes of their terms."""
    probs, sols = _base(orc, cid)
    for i, (p, s) in enumerate(zip(probs, sols)):
        H, g, A = SC.problem(p)[:3]
        d = {}
        for kind in SC.KINDS:
            d.update(SC.direction(cid, i, kind, p))
        rng = np.random.default_rng([SC.CASES.index(cid), i, 31])
        gx, gla, glx = rng.standard_normal(g.shape), rng.standard_normal(A.shape[0]), rng.standard_normal(g.shape)
        dx, dla, dlx = _jvp(p, s, d)
        lhs = gx @ dx + gla @ dla + glx @ dlx            # dlam is zero outside the working set
        u, wa, wx, _ = qp_sens.kkt_solve_reference(H, A, s["ws_a"], s["ws_x"], gx, gla, glx)
        gr = qp_sens.vjp_grads(s["x"][None], s["lam_a"][None], s["ws_a"][None], s["ws_x"][None], u[None], wa[None], wx[None])
        terms = [(gr[k][0] * d[k]).sum() for k in ("g", "lba", "uba", "lbx", "ubx", "H")] + [(gr["A_cm"][0].T * d["A"]).sum()]
        rhs = sum(terms)
        cond = np.linalg.cond(qp_sens.kkt_matrix(H, A, s["ws_a"], s["ws_x"])[0])
        tol = 64.0 * EPS * cond * (sum(abs(t) for t in terms) + abs(gx) @ abs(dx) + abs(gla) @ abs(dla) + abs(glx) @ abs(dlx))
        print("%s[%d] <g, d> %.12e vs %.12e  diff %.2e tol %.2e" % (cid, i, lhs, rhs, abs(lhs - rhs), tol))
        assert abs(lhs - rhs) <= tol, (cid, i, lhs, rhs)
        assert not np.any(gr["lba"][0][s["ws_a"] != -1]) and not np.any(gr["uba"][0][s["ws_a"] != 1])


def test_reference_solves_the_stated_system(orc):
    """kkt_solve_reference against the system as written, several right-hand sides at once, and its refusal of a
    dependent working set."""
    cid = "spd-9x16"
    probs, sols = _base(orc, cid)
    p, s = probs[0], sols[0]
    H, g, A = SC.problem(p)[:3]
    n, m = g.size, A.shape[0]
    rng = np.random.default_rng(5)
    rp, ra, rx = rng.standard_normal((3, n)), rng.standard_normal((3, m)), rng.standard_normal((3, n))
    pp, qa, qx, resid = qp_sens.kkt_solve_reference(H, A, s["ws_a"], s["ws_x"], rp, ra, rx)
    Hs = 0.5 * (H + H.T)
    ha, hx = s["ws_a"] != 0, s["ws_x"] != 0
    assert resid <= 4 * EPS
    assert np.abs(pp @ Hs + qa @ A + qx - rp).max() <= 1e-13 * max(1.0, np.abs(qa).max())
    assert np.abs((pp @ A.T - ra)[:, ha]).max() <= 1e-14 and np.abs((pp - rx)[:, hx]).max() <= 1e-14
    assert not qa[:, ~ha].any() and not qx[:, ~hx].any()
    one = qp_sens.kkt_solve_reference(H, A, s["ws_a"], s["ws_x"], rp[1], ra[1], rx[1])
    np.testing.assert_array_equal(one[0], pp[1])
    # a variable held twice (its bound and a row with that single non-zero): an exactly zero pivot
    A2 = np.zeros((1, n)); A2[0, 2] = 3.0
    with pytest.raises(np.linalg.LinAlgError):
        qp_sens.kkt_solve_reference(H, A2, np.ones(1, dtype=np.int8), np.eye(n, dtype=np.int8)[2], rp[0])
