"""eepacc_qp_kkt_solve_batched (csrc/eepacc_qp_dense.hip, k_qp_kkt) and the derivative layer built on it
(eepacc_mpc_casadi_matlab_amd/qp_sens.py): linear solves with the KKT matrix of a working set, checked against the numpy
specification qp_sens.kkt_solve_reference, which shares nothing with the kernel's method, and the derivatives against
the solver itself and torch's gradcheck.

Bounds.  Residual: qp_sens.kkt_residual, the scaled inf-norm residual of the stated system evaluated in long double from
the problem data, eta = |K z - r|_inf / max(1, |r|_inf, |K|_max |z|_inf).  It must be <= max(1000 x eta of
numpy.linalg.solve in float64 on the same assembled system, 1e-13): margin and floor of tests/test_gpu_qp_dense.py for
differing summation and pivot order.  Solution: |z - z_ref|_inf <= (that bound) x cond_2(K), cond_2 from numpy on the
assembled matrix.
Sensitivity (test 2): |dx - (x(+h) - x(-h)) / 2h|_inf <= (e+ + e-) / 2h + the solution bound above for the derivative's
right-hand side, with e+- = |x(+-h) - refined_solution(x(+-h))|_inf against the long-double refined solution.  Along g and
the bounds the solution on a fixed working set is linear in the step and the quotient has no truncation error; along H and
A it has one of O(h^2), and qp_sens_cases.step takes a ten times smaller step there so that it needs no allowance.  The jvp
is fed the direction the two launches actually took (qp_sens_cases.effective_direction).  Nothing the code under test
returned enters a tolerance.

Measured on an MI355X (largest over the 3 problems of a case; `-s` prints every figure per problem):
                                 residual eta   numpy float64 solve   |z - z_ref|  (smallest tol)   test 2: |fd - dx| (largest, any direction)
    spd-3x5                      8.1e-17        2.4e-16               2.2e-16      (2.4e-13)        2.2e-10
    spd-9x16                     9.9e-17        1.8e-16               3.6e-15      (3.0e-12)        4.4e-10
    spd-65x130                   5.4e-16        1.6e-15               1.4e-14      (2.1e-10)        3.7e-09
    soft-20+43-10-lbx-w10000     1.7e-16        3.3e-16               7.1e-14      (3.9e-11)        1.6e-07  (h = 1e-8 / 1e-9)
    soft-20+43-10-row-w1         2.5e-16        5.4e-16               1.7e-15      (2.3e-11)        5.7e-09
    indef-12x9-0.05              1.1e-16        2.2e-16               1.8e-15      (4.0e-12)        9.7e-10
The residual stays below numpy's own on every problem: the margin of 1000 is not used.  In test 2 the difference is the
rounding of x(+-h) over 2h throughout (e+- of 1e-17 ... 9e-16; the largest figures are those of the H and A directions
with their ten times smaller step); the linear solve's own share of the tolerance is 2e-13 ... 1e-9.  With the H direction
taken from the unsymmetrised arrays the bound is missed (indef-12x9-0.05[2] along H: 1.25e-9 against 1.03e-9), and at the
step of the linear directions the truncation shows (spd-3x5[2] along H at h = 1e-6: 8.9e-12 against 4.6e-12).
The device's working sets at +-h equal the base one on all 6 x 3 x 4 launched pairs.  gradcheck passes on spd-3x5 (3
problems) and on problems 1, 2 of indef-12x9-0.05; nR = 3 equals three nR = 1 calls, and 7 right-hand sides equal the 3
they repeat, bit for bit on all six cases.
"""
import numpy as np
import pytest

import qp_cert as Q
import qp_sens_cases as SC
from conftest import make_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAME = "eepacc_qp_kkt_solve_batched"


@pytest.fixture(scope="module")
def torch_mod():
    import torch
    assert torch.cuda.is_available()
    return torch


@pytest.fixture(scope="module")
def setup():
    return make_case("ABO", 20)[:2]


def _engine(setup, max_batch=8):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(setup[0], setup[1], device=0, max_batch=max_batch)


@pytest.fixture(scope="module")
def eng(torch_mod, setup):
    return _engine(setup)


@pytest.fixture(scope="module")
def sens():
    from eepacc_mpc_casadi_matlab_amd import qp_sens
    return qp_sens


def _stack(probs, k):
    return None if probs[0][k] is None else np.stack([p[k] for p in probs])


_DUAL = {}


def _dual(eng, probs, key=None):
    """One launch of the dual entry (the solver the derivatives belong to); cached per key."""
    if key is None or key not in _DUAL:
        r = eng.qp_solve_batched_dual(*[_stack(probs, k) for k in range(7)])
        eng.synchronize()
        assert (r.status == 0).all()
        if key is None:
            return r
        _DUAL[key] = r
    return _DUAL[key]


def _np(*ts):
    return [t.cpu().numpy() for t in ts]


def _kkt(eng, H, A, wa, wx, rp, ra=None, rx=None):
    out = eng.qp_kkt_solve(H, A, wa, wx, rp, ra, rx)
    eng.synchronize()
    return _np(*out)


def _float64_bound(sens, K, rows, cols, H, A, wa, wx, rp, ra, rx):
    """(residual bound, solution tolerance, z_ref parts) of one problem: 1000 x the residual numpy.linalg.solve reaches
    in float64 on the assembled system, floor 1e-13, and that times cond_2(K)."""
    n, m = H.shape[0], A.shape[0]
    nR = rp.shape[0]
    rhs = np.concatenate([rp, ra[:, rows], rx[:, cols]], axis=1).T
    z = np.linalg.solve(K, rhs)
    p64 = z[:n].T.copy(); qa64 = np.zeros((nR, m)); qx64 = np.zeros((nR, n))
    qa64[:, rows] = z[n:n + len(rows)].T; qx64[:, cols] = z[n + len(rows):].T
    eta64 = sens.kkt_residual(H, A, wa, wx, rp, ra, rx, p64, qa64, qx64)
    bound = max(1000.0 * eta64, 1e-13)
    ref = sens.kkt_solve_reference(H, A, wa, wx, rp, ra, rx)
    return bound, bound * np.linalg.cond(K), ref, eta64


# ------------------------------------------------------------------------------------------- 1. the linear solve
@pytest.mark.parametrize("cid", SC.CASES)
def test_linear_solve_at_size_cases(cid, eng, sens):
    probs = Q.make_case(cid)[1]
    B = len(probs)
    sol = _dual(eng, probs, cid)
    wa, wx = _np(sol.ws_a, sol.ws_x)
    H, A = _stack(probs, 0), _stack(probs, 2)
    n, m = H.shape[1], A.shape[1]
    rng = np.random.default_rng([SC.CASES.index(cid), 99])
    rp, ra, rx = rng.standard_normal((B, 3, n)), rng.standard_normal((B, 3, m)), rng.standard_normal((B, 3, n))
    ra[:, 0] = 0.0; rx[:, 0] = 0.0                  # right-hand side 0: r_p only
    rp[:, 1] = 0.0                                  # right-hand side 1: r_a, r_x only
    p, qa, qx, st = _kkt(eng, H, A, wa, wx, rp, ra, rx)
    assert (st == 0).all()
    worst, tightest = np.zeros(3), np.inf
    for i in range(B):
        K, rows, cols = sens.kkt_matrix(H[i], A[i], wa[i], wx[i])
        bound, tol, ref, eta64 = _float64_bound(sens, K, rows, cols, H[i], A[i], wa[i], wx[i], rp[i], ra[i], rx[i])
        eta = sens.kkt_residual(H[i], A[i], wa[i], wx[i], rp[i], ra[i], rx[i], p[i], qa[i], qx[i])
        dz = max(np.abs(p[i] - ref[0]).max(), np.abs(qa[i] - ref[1]).max(initial=0.0), np.abs(qx[i] - ref[2]).max())
        print("%s[%d] held %d + %d: residual %.2e (float64 solve %.2e, bound %.2e, reference %.2e)  |z - z_ref| %.2e (tol %.2e)"
              % (cid, i, len(rows), len(cols), eta, eta64, bound, ref[3], dz, tol))
        assert np.isfinite(p[i]).all() and np.isfinite(qa[i]).all() and np.isfinite(qx[i]).all()
        assert eta <= bound, (cid, i, eta, bound)
        assert dz <= tol, (cid, i, dz, tol)
        assert not qa[i][:, np.abs(wa[i]) != 1].any() and not qx[i][:, np.abs(wx[i]) != 1].any()
        assert not np.signbit(qa[i][:, np.abs(wa[i]) != 1]).any() and not np.signbit(qx[i][:, np.abs(wx[i]) != 1]).any()
        worst, tightest = np.maximum(worst, [eta, eta64, dz]), min(tightest, tol)
    print("%s largest residual %.2e (float64 solve %.2e), largest |z - z_ref| %.2e (smallest tol %.2e)" % ((cid,) + tuple(worst) + (tightest,)))
    # one right-hand side per call: the same bits
    for r in range(3):
        p1, qa1, qx1, st1 = _kkt(eng, H, A, wa, wx, rp[:, r:r + 1], ra[:, r:r + 1], rx[:, r:r + 1])
        np.testing.assert_array_equal(p1[:, 0], p[:, r]); np.testing.assert_array_equal(qa1[:, 0], qa[:, r])
        np.testing.assert_array_equal(qx1[:, 0], qx[:, r])
    # more right-hand sides than wavefronts: the ones of the second sweep repeat the first
    p7, qa7, qx7, _ = _kkt(eng, H, A, wa, wx, np.tile(rp, (1, 3, 1))[:, :7], np.tile(ra, (1, 3, 1))[:, :7], np.tile(rx, (1, 3, 1))[:, :7])
    for r in range(7):
        np.testing.assert_array_equal(p7[:, r], p[:, r % 3]); np.testing.assert_array_equal(qa7[:, r], qa[:, r % 3])
        np.testing.assert_array_equal(qx7[:, r], qx[:, r % 3])


# ------------------------------------------------------------------------------ 2. sensitivity against the solver
@pytest.mark.parametrize("cid", SC.CASES)
def test_jvp_against_the_solver(cid, eng, sens):
    probs = Q.make_case(cid)[1]
    B = len(probs)
    sol = _dual(eng, probs, cid)
    x, la, lx, wa, wx = _np(sol.x, sol.lam_a, sol.lam_x, sol.ws_a, sol.ws_x)
    H, A = _stack(probs, 0), _stack(probs, 2)
    worst, tightest = 0.0, np.inf
    for kind in SC.KINDS:
        h = SC.step(cid, kind)
        ds = [SC.direction(cid, i, kind, p) for i, p in enumerate(probs)]
        side, data = {}, {}
        for t in (h, -h):
            data[t] = pert = [SC.perturbed(p, d, t) for p, d in zip(probs, ds)]
            r = _dual(eng, pert)
            xs, was, wxs = _np(r.x, r.ws_a, r.ws_x)
            for i in range(B):
                assert (was[i] == wa[i]).all() and (wxs[i] == wx[i]).all(), (cid, i, kind, t, "the chosen step changes the working set")
            # e+-: against the long-double x* of the problem as the device got it (its float64 rounding would hide the
            # half ulp that x(+-h) itself carries, which is all of the error at h = 1e-6)
            side[t] = (xs, [float(np.abs(xs[i].astype(Q.LD) - Q.refined_solution(*pert[i], xs[i])[1]).max()) for i in range(B)])
        ds = [SC.effective_direction(data[h][i], data[-h][i], d, h) for i, d in enumerate(ds)]
        stackd = lambda k: np.stack([d[k] for d in ds]) if k in ds[0] else None
        dx, dla, dlx, st = _np(*sens.qp_jvp(eng, sol, H, A, dg=stackd("g"), dlba=stackd("lba"), duba=stackd("uba"),
                                            dlbx=stackd("lbx"), dubx=stackd("ubx"), dH=stackd("H"), dA=stackd("A")))
        assert (st == 0).all()
        for i in range(B):
            fd = (side[h][0][i] - side[-h][0][i]) / (2.0 * h)
            K, rows, cols = sens.kkt_matrix(H[i], A[i], wa[i], wx[i])
            b1 = lambda v: None if v is None else v[None]
            r = sens.jvp_rhs(x[i][None], la[i][None], wa[i][None], wx[i][None],
                             *[b1(ds[i].get(k)) for k in ("g", "lba", "uba", "lbx", "ubx", "H", "A")])
            tol1 = _float64_bound(sens, K, rows, cols, H[i], A[i], wa[i], wx[i], r[0], r[1], r[2])[1]
            tol = (side[h][1][i] + side[-h][1][i]) / (2.0 * h) + tol1
            err = np.abs(fd - dx[i]).max()
            print("%s[%d] %-6s h %.0e |dx| %.3e  |fd - dx| %.3e  tol %.3e = (%.1e + %.1e)/2h + %.1e"
                  % (cid, i, kind, h, np.abs(dx[i]).max(), err, tol, side[h][1][i], side[-h][1][i], tol1))
            assert err <= tol, (cid, i, kind, err, tol)
            worst, tightest = max(worst, err), min(tightest, tol)
    print("%s largest |fd - dx| %.2e, smallest tolerance %.2e" % (cid, worst, tightest))


# --------------------------------------------------------------------------------------------------- 3. autograd
@pytest.mark.parametrize("cid", ["spd-3x5", "indef-12x9-0.05"])
def test_gradcheck(cid, eng, sens, torch_mod):
    """torch.autograd.gradcheck with its default eps, atol, rtol on qp_layer with respect to g, lba, uba, H, A together.
    gradcheck moves one datum by eps = 1e-6 at a time: the problems of the case whose strict-complementarity margin
    (qp_sens_cases.margin at the device's solution) is at least 1e-3 take part, so that no such step can change the
    working set.  spd-3x5: all three (margins 1.8e-1, 6.4e-2, 5.6e-2); indef-12x9-0.05: problems 1 and 2 (1.1e-2,
    2.6e-2) -- problem 0 has a multiplier of 1.8e-4 and stays with the finite differences of test 2.
    An equality row (lba == uba; row 2 of the indef case) cannot have one of its bounds moved alone: lba + eps > uba is an
    infeasible problem, and the solver's answer to it is no difference quotient.  Such a row takes its two bounds from the
    input lba (uba_eff = where(lba == uba, lba, uba), inside the differentiated function), so gradcheck moves them together
    and sees the sum of the two bound gradients there, and zero for the unused uba entry."""
    t = torch_mod
    probs = Q.make_case(cid)[1]
    sol = _dual(eng, probs, cid)
    parts = _np(sol.x, sol.lam_a, sol.lam_x, sol.ws_a, sol.ws_x)
    margins = [SC.margin(p, *[v[i] for v in parts]) for i, p in enumerate(probs)]
    take = [i for i, m in enumerate(margins) if m >= 1e-3]
    print(cid, "margins", margins, "problems in gradcheck", take)
    assert take == ([0, 1, 2] if cid == "spd-3x5" else [1, 2]), margins
    dev = lambda k, grad: t.tensor(np.stack([SC.problem(probs[i])[k] for i in take]), dtype=t.float64, device=eng.device, requires_grad=grad)
    H, g, A, lba, uba = (dev(k, True) for k in range(5))
    lbx, ubx = dev(5, False), dev(6, False)
    eq = (lba == uba).detach()
    fn = lambda H, g, A, lba, uba: sens.qp_layer(eng, H, g, A, lba, t.where(eq, lba, uba), lbx, ubx)[:3]
    assert t.autograd.gradcheck(fn, (H, g, A, lba, uba))


def test_closed_form_gradients(eng, sens, torch_mod):
    """min 1/2 |x|^2 + g'x  s.t.  a'x >= b with the row active: x = -g + a t, lam_a = -t, t = (b + a'g) / a'a.  For
    L = c'x + m lam_a = -c'g + (c'a - m) t every gradient is known:
      dL/dg = -c + (c'a - m) a / a'a,  dL/db = (c'a - m) / a'a,  dL/da = c t + (c'a - m)(g - 2 a t) / a'a,
      dL/dH = -(v x' + x v')/2 with v = c - a (a'c)/a'a + m a/a'a  (from dx = -P dHs x, dlam = -a'dHs x / a'a)."""
    t = torch_mod
    g0, a0, b0 = np.array([0.5, -0.3, 0.2]), np.array([1.0, 0.25, -0.5]), 1.0
    c, m = np.array([0.7, -1.1, 0.4]), 0.9
    dev = lambda v: t.tensor(np.asarray(v, dtype=np.float64), device=eng.device, requires_grad=True)
    H, g, A, lba = dev(np.eye(3)[None]), dev(g0[None]), dev(a0[None, None]), dev([[b0]])
    x, lam_a, lam_x, status = sens.qp_layer(eng, H, g, A, lba)
    aa = a0 @ a0
    tt = (b0 + a0 @ g0) / aa
    assert status.item() == 0 and tt > 0
    np.testing.assert_allclose(x.detach().cpu().numpy()[0], -g0 + a0 * tt, rtol=0, atol=1e-14)
    np.testing.assert_allclose(lam_a.detach().cpu().numpy()[0], [-tt], rtol=0, atol=1e-14)
    L = (x[0] * t.tensor(c, device=eng.device)).sum() + m * lam_a[0, 0]
    L.backward()
    k = c @ a0 - m
    xs = -g0 + a0 * tt
    v = c - a0 * (a0 @ c) / aa + m * a0 / aa
    want = dict(g=-c + k * a0 / aa, lba=[k / aa], A=[c * tt + k * (g0 - 2 * a0 * tt) / aa], H=-0.5 * (np.outer(v, xs) + np.outer(xs, v)))
    for name, ten in (("g", g), ("lba", lba), ("A", A), ("H", H)):
        got = ten.grad.cpu().numpy()[0]
        print(name, got, want[name])
        np.testing.assert_allclose(got, np.asarray(want[name]), rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------------ 4. edges
def test_empty_and_full_working_sets(eng, sens):
    H, g, A = Q.spd(9, 16, seed=4)[:3]
    n = 9
    Hs = 0.5 * (H + H.T)
    rng = np.random.default_rng(12)
    rp, rx = rng.standard_normal((1, 2, n)), rng.standard_normal((1, 2, n))
    # both NULL: p = Hs^-1 r_p
    p, qa, qx, st = _kkt(eng, H[None], A[None], None, None, rp)
    ref = np.linalg.solve(Hs, rp[0].T).T
    assert st[0] == 0 and not qa.any() and not qx.any()
    assert np.abs(p[0] - ref).max() <= 64 * EPS * np.linalg.cond(Hs) * max(1.0, np.abs(ref).max())
    # nV bounds: p = r_x exactly, q_x = r_p - Hs r_x
    wx = np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int8)[None]
    p, qa, qx, st = _kkt(eng, H[None], A[None], None, wx, rp, None, rx)
    assert st[0] == 0 and not qa.any()
    np.testing.assert_array_equal(p, rx)
    want = rp[0] - rx[0] @ Hs
    assert np.abs(qx[0] - want).max() <= 4 * n * EPS * max(1.0, np.abs(rp).max(), np.abs(Hs).max() * np.abs(rx).max())
    # codes other than +-1 are not held; nC = 0
    p2, _, qx2, st = _kkt(eng, H[None], np.zeros((1, 0, n)), None, 7 * wx, rp, None, rx)
    assert st[0] == 0 and not qx2.any()
    np.testing.assert_array_equal(p2[0], _kkt(eng, H[None], A[None], None, None, rp)[0][0])


def test_singular_instances_do_not_touch_their_neighbours(eng, sens):
    probs = [Q.spd(9, 16, seed=20 + s) for s in range(4)]
    sol = _dual(eng, probs)
    wa, wx = _np(sol.ws_a, sol.ws_x)
    H, A = _stack(probs, 0), _stack(probs, 2).copy()
    rng = np.random.default_rng(13)
    rp, ra, rx = rng.standard_normal((4, 2, 9)), rng.standard_normal((4, 2, 16)), rng.standard_normal((4, 2, 9))
    good = _kkt(eng, H, A, wa, wx, rp, ra, rx)
    assert (good[3] == 0).all()
    # instance 1: a dependent pair of rows; instance 2: more than nV held entries
    A[1, 1] = 2.0 * A[1, 0]
    wa2, wx2 = wa.copy(), wx.copy()
    wa2[1] = 0; wa2[1, :2] = 1; wx2[1] = 0
    wa2[2] = 1; wx2[2] = -1
    p, qa, qx, st = _kkt(eng, H, A, wa2, wx2, rp, ra, rx)
    assert st.tolist() == [0, 1, 1, 0]
    for v, gv in zip((p, qa, qx), good):
        assert np.isnan(v[1]).all() and np.isnan(v[2]).all()
        np.testing.assert_array_equal(v[[0, 3]], gv[[0, 3]])
    # a variable held by its bound and by a row with that single non-zero: an exactly zero pivot
    A1 = np.zeros((1, 1, 9)); A1[0, 0, 2] = 3.0
    st = _kkt(eng, H[:1], A1, np.ones((1, 1), dtype=np.int8), np.eye(9, dtype=np.int8)[2][None], rp[:1])[3]
    assert st[0] == 1


def test_refusals(torch_mod, setup):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, EepaccError
    eng = _engine(setup)
    H, A = np.eye(4)[None], np.zeros((1, 1, 4))
    with pytest.raises(EepaccError, match=NAME + ": bad sizes"):
        eng.qp_kkt_solve(H, A, None, None, np.zeros((1, 0, 4)))
    d = torch_mod.zeros(16, dtype=torch_mod.float64, device=eng.device)
    rc = eng.lib.eepacc_qp_kkt_solve_batched(eng.h, 1, 4, 0, 0, d.data_ptr(), None, None, None, d.data_ptr(), None, None,
                                             d.data_ptr(), None, None, None, eng._stream())
    assert rc == -1 and eng.lib.eepacc_last_error().decode() == NAME + ": bad sizes"
    rc = eng.lib.eepacc_qp_kkt_solve_batched(eng.h, 1, 4, 0, 1, *([None] * 11), eng._stream())
    assert rc == -1 and eng.lib.eepacc_last_error().decode() == NAME + ": NULL buffer"
    with pytest.raises(EepaccError, match=NAME + ": nV/nC above EEPACC_QP_MAX_NV/NC"):
        eng.qp_kkt_solve(np.eye(385)[None], np.zeros((1, 1, 385)), None, None, np.zeros((1, 385)))
    p = eng.qp_kkt_solve(np.zeros((0, 4, 4)), np.zeros((0, 2, 4)), None, None, np.zeros((0, 3, 4)))       # B = 0
    assert p[0].shape == (0, 3, 4) and p[1].shape == (0, 3, 2) and p[3].shape == (0,)
    p, _, _, st = eng.qp_kkt_solve(2.0 * H, A, None, None, np.ones((1, 4)))
    eng.synchronize()
    assert st.item() == 0 and (p.cpu().numpy() == 0.5).all() and p.shape == (1, 4)
    cls = Engine.from_classes([setup[0], setup[0]], [setup[1], setup[1]], device=0, max_batch=8)
    with pytest.raises(EepaccError, match=NAME + ": a handle of eepacc_create_classes runs ABMPC only"):
        cls.qp_kkt_solve(H, A, None, None, np.zeros((1, 4)))
    rc = cls.lib.eepacc_qp_kkt_solve_batched(cls.h, 1, 4, 0, 1, *([None] * 11), cls._stream())
    assert rc == -4                                                                                    # EEPACC_ENOTSUP


def test_mixed_batch_larger_than_the_grid(torch_mod, setup, sens, monkeypatch):
    """One workgroup per CU and more than three instances per workgroup; spd and soft problems of one shape with their
    own working sets, every seventh instance with more held entries than variables.  The same batch in another order
    gives the same bits per instance, and a sample agrees with the specification."""
    monkeypatch.setenv("EEPACC_QP_WGS_PER_CU", "1")
    grid = torch_mod.cuda.get_device_properties(0).multi_processor_count
    B = 3 * grid + 5
    eng = _engine(setup)
    probs = [Q.spd(9, 7, seed=200 + i) if i % 2 == 0 else Q.soft(5, 4, 3, False, 1.0, seed=200 + i) for i in range(B)]
    sol = _dual(eng, probs)
    wa, wx = _np(sol.ws_a, sol.ws_x)
    over = np.arange(B) % 7 == 3
    wa[over] = 1; wx[over] = 1
    H, A = _stack(probs, 0), _stack(probs, 2)
    rng = np.random.default_rng(14)
    rp, ra, rx = rng.standard_normal((B, 2, 9)), rng.standard_normal((B, 2, 7)), rng.standard_normal((B, 2, 9))
    out = _kkt(eng, H, A, wa, wx, rp, ra, rx)
    assert (out[3] == over).all()
    assert np.isnan(out[0][over]).all() and np.isfinite(out[0][~over]).all()
    perm = np.random.default_rng(15).permutation(B)
    out2 = _kkt(eng, H[perm], A[perm], wa[perm], wx[perm], rp[perm], ra[perm], rx[perm])
    for v, v2 in zip(out, out2):
        np.testing.assert_array_equal(v2, v[perm])
    for i in np.random.default_rng(16).choice(np.nonzero(~over)[0], 12, replace=False):
        K, rows, cols = sens.kkt_matrix(H[i], A[i], wa[i], wx[i])
        bound, tol, ref, _ = _float64_bound(sens, K, rows, cols, H[i], A[i], wa[i], wx[i], rp[i], ra[i], rx[i])
        assert sens.kkt_residual(H[i], A[i], wa[i], wx[i], rp[i], ra[i], rx[i], out[0][i], out[1][i], out[2][i]) <= bound
        assert max(np.abs(out[0][i] - ref[0]).max(), np.abs(out[1][i] - ref[1]).max(), np.abs(out[2][i] - ref[2]).max()) <= tol


def test_failed_forward_instance_gets_nan_gradients(eng, sens, torch_mod):
    t = torch_mod
    good = Q.spd(9, 7, seed=1)
    H, g, A, lba, uba, lbx, ubx = [np.array(v, copy=True) for v in Q.spd(9, 7, seed=2)]
    A[2] = 0.0; A[2, 0] = 1.0; lba[2] = 5.0; uba[2] = 6.0                # contradicts ubx[0] <= 0.5
    probs = [good, (H, g, A, lba, uba, lbx, ubx)]
    ins = [t.tensor(_stack(probs, k), dtype=t.float64, device=eng.device, requires_grad=True) for k in range(7)]
    x, lam_a, lam_x, status = sens.qp_layer(eng, *ins)
    assert status.tolist() == [0, 1]
    (x[0].sum() + lam_a[0].sum() + x[1].sum()).backward()
    for k, ten in enumerate(ins):
        gr = ten.grad.cpu().numpy()
        assert np.isfinite(gr[0]).all() and np.isnan(gr[1]).all(), k
    assert np.abs(ins[1].grad[0].cpu().numpy()).max() > 0.0
