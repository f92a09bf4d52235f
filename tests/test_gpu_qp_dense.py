"""The dense QP operator (eepacc_qp_solve_batched, csrc/eepacc_qp_dense.hip) at every size class of its kernel, checked
against the solver-independent optimality certificate of tests/qp_cert.py, a long-double refined solution, and the CPU
oracle -- whose own results on the same problems are certified by tests/test_qp_cert_cpu.py.

Bounds.  Certificate of a kernel result: 1000 x the oracle's value on the same problem, floored at 1e-13 (summation and
pivot order differ).  Distance to the refined x* (spd, soft): 100 x qp_cert.D_REF, the oracle's largest distance to x*
over the table, relative to max(1, ||x*||_inf).  indef: x against the oracle's uniform-rho result at 1e-7 max(1, ||x||_inf)
(the bound of tests/test_gpu_fb.py).

Measured (largest over the case table, 3 problems per case):
                              pviol      stat       ||x - x*||_inf / max(1, ||x*||_inf)
    CPU oracle  spd           3.0e-16    2.5e-14    2.8e-17   (= D_REF["spd"])
                soft          1.8e-16    1.3e-14    2.8e-17   (= D_REF["soft"])
                indef         2.3e-16    4.8e-15    --
    MI355X      not entered yet: this module has not run on an MI355X so far (`-s` prints every figure per problem).
"""
import numpy as np
import pytest

import qp_cert as Q
from conftest import make_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
EINVAL_SIZES = "eepacc_qp_solve_batched: bad sizes"
EINVAL_MAX = "eepacc_qp_solve_batched: nV/nC above EEPACC_QP_MAX_NV/NC"


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
def orc(setup):
    from oracle.loader import Oracle
    return Oracle(*setup)


def _stack(probs, k):
    return None if probs[0][k] is None else np.stack([p[k] for p in probs])


def _launch(eng, probs, x0=None):
    """One launch for problems of one shape; numpy x [B, nV], cost [B], status [B]."""
    x, cost, status = eng.qp_solve_batched(*[_stack(probs, k) for k in range(7)], x0=x0)
    eng.synchronize()
    return x.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy()


def _cert_bound(c_orc):
    return max(1000.0 * c_orc["pviol"], 1e-13), max(1000.0 * c_orc["stat"], 1e-13)


def _reference(orc, fam, p):
    """Oracle result, its certificate and (spd, soft) the refined x* of one problem."""
    x, cost, st = orc.qp_solve(*p)
    c = Q.certificate(*p, x)
    xs = Q.refined_solution(*p, x)[0] if fam in Q.D_REF and st["status"] == 0 else None
    return dict(x=x, cost=cost, status=st["status"], cert=c, xs=xs)


def _check(tag, fam, p, ref, x, status):
    """The size-class assertions for one problem; returns the measured (pviol, stat, distance)."""
    assert ref["status"] == 0, (tag, "the oracle does not solve a table case")
    c = Q.certificate(*p, x)
    pb, sb = _cert_bound(ref["cert"])
    d = float("nan")
    if ref["xs"] is not None:
        d = np.abs(x - ref["xs"]).max() / max(1.0, np.abs(ref["xs"]).max())
    print("%s status %d pviol %.2e (oracle %.2e) stat %.2e (oracle %.2e) |x-x*| %.2e |x-x_oracle| %.2e"
          % (tag, status, c["pviol"], ref["cert"]["pviol"], c["stat"], ref["cert"]["stat"], d, np.abs(x - ref["x"]).max()))
    assert status == 0 == ref["status"], (tag, status)
    assert c["pviol"] <= pb and c["stat"] <= sb, (tag, c["pviol"], pb, c["stat"], sb)
    if ref["xs"] is not None:
        assert d <= 100.0 * Q.D_REF[fam], (tag, d)
    if fam == "indef":
        assert np.abs(x - ref["x"]).max() <= 1e-7 * max(1.0, np.abs(ref["x"]).max()), tag
    return c["pviol"], c["stat"], d


# ----------------------------------------------------------------------------------------------------- size classes
@pytest.mark.parametrize("cid", list(Q.CASES))
def test_size_class(cid, eng, orc):
    """One launch per shape: status 0 like the oracle's, certificate at the oracle's bound, x at the refined x*."""
    fam, probs = Q.make_case(cid)
    refs = Q.solve_all(lambda *p: _reference(orc, fam, p), probs)
    x, cost, status = _launch(eng, probs)
    Q.solve_all(lambda i: _check("%s[%d]" % (cid, i), fam, probs[i], refs[i], x[i], int(status[i])),
                [(i,) for i in range(len(probs))])


# -------------------------------------------------------------------------------------------------- interface edges
def _edge(eng, orc, p, tag, x0=None):
    """Oracle and certificate both on one small problem; returns the kernel's x."""
    ref = _reference(orc, "spd", p)
    x, cost, status = _launch(eng, [p], x0=None if x0 is None else x0[None])
    _check(tag, "spd", p, ref, x[0], int(status[0]))
    _check_cost(p, x[0], cost[0])
    return x[0]


def _check_cost(p, x, cost):
    """cost = 1/2 x'Hx + g'x at the returned x: n + 1 products summed per row and n rows summed, each sum of k terms
    within k eps of the sum of magnitudes -> 4 n eps (1/2 sum |H_ij x_i x_j| + sum |g_i x_i|)."""
    H, g = p[0].astype(Q.LD), p[1].astype(Q.LD)
    xl = x.astype(Q.LD); n = len(x)
    exact = 0.5 * xl @ (H @ xl) + g @ xl
    mag = 0.5 * np.abs(xl) @ (np.abs(H) @ np.abs(xl)) + np.abs(g) @ np.abs(xl)
    assert abs(Q.LD(cost) - exact) <= 4 * n * EPS * mag, (cost, float(exact))


def test_no_rows_with_a_box(eng, orc):
    for n in (1, 6, 70):
        _edge(eng, orc, Q.spd(n, 0, seed=1), "box-%d" % n)


@pytest.mark.parametrize("n", [1, 6, 65, 257])
def test_no_rows_no_bounds_is_a_linear_solve(n, eng, orc):
    """x = -H^-1 g against the long-double refined solve.  The kernel's LU + refinement evaluates the residual Hx + g in
    double: that residual is off by at most 2 n eps ||H|| ||x||, which H^-1 turns into 2 n eps cond(H) ||x||; twice
    that for the refinement's own last correction."""
    H, g = Q.spd(n, 0, seed=2)[:2]
    none = (np.zeros((0, n)), None, None, None, None)
    xs = Q.refined_solution(H, g, *none, np.zeros(n))[0]
    for p in ((H, g) + none, (H, g, np.zeros((0, n)), np.zeros(0), np.zeros(0), np.full(n, -np.inf), np.full(n, np.inf))):
        x, cost, status = _launch(eng, [p])
        assert status[0] == 0
        assert np.abs(x[0] - xs).max() <= 4 * n * EPS * np.linalg.cond(H) * np.abs(xs).max()
        _check_cost(p, x[0], cost[0])
    xo, _, st = orc.qp_solve(H, g, np.zeros((0, n)), None, None)
    assert st["status"] == 0 and np.abs(xo - xs).max() <= 4 * n * EPS * np.linalg.cond(H) * np.abs(xs).max()


@pytest.mark.parametrize("k", [3, 4, 5, 6], ids=["lba", "uba", "lbx", "ubx"])
def test_absent_array_equals_infinite_bounds(k, eng, orc):
    """A bound array passed as NULL is the same problem as that array full of -+inf, bit for bit."""
    probs = []
    for s in range(3):
        p = list(Q.spd(9, 7, seed=10 + s))
        p[k] = np.full_like(p[k], -np.inf if k in (3, 5) else np.inf)
        probs.append(tuple(p))
    full = _launch(eng, probs)
    gone = [tuple(None if j == k else a for j, a in enumerate(p)) for p in probs]
    none = _launch(eng, gone)
    for a, b in zip(full, none):
        np.testing.assert_array_equal(a, b)
    for i, p in enumerate(probs):
        _check("absent-%d[%d]" % (k, i), "spd", p, _reference(orc, "spd", p), none[0][i], int(none[2][i]))


def test_fixed_variable(eng, orc):
    H, g, A, lba, uba, lbx, ubx = Q.spd(8, 7, seed=3)
    lbx[2] = ubx[2] = 0.1
    lbx[5] = ubx[5] = ubx[5]
    x = _edge(eng, orc, (H, g, A, lba, uba, lbx, ubx), "fixed")
    assert x[2] == 0.1 and x[5] == ubx[5]


def _with_duplicate(orc, seed):
    """spd(8, 7) with an inactive row overwritten by a copy of an active one (same bounds)."""
    H, g, A, lba, uba, lbx, ubx = Q.spd(8, 7, seed=seed)
    x = orc.qp_solve(H, g, A, lba, uba, lbx, ubx)[0]
    c = Q.certificate(H, g, A, lba, uba, lbx, ubx, x)
    act = [i for (kind, i, _), lam in zip(c["active"], c["lam"]) if kind == 0 and lam > 0.0]
    idle = [i for i in range(7) if i not in {i for kind, i, _ in c["active"] if kind == 0}]
    assert act and idle
    r, j = act[0], idle[0]
    A[j] = A[r]; lba[j] = lba[r]; uba[j] = uba[r]
    return (H, g, A, lba, uba, lbx, ubx), r, j


def test_duplicated_row(eng, orc):
    """A dependent row in the working set's reach: the problem stays feasible and is solved."""
    for seed in (4, 5):
        p, r, j = _with_duplicate(orc, seed)
        _edge(eng, orc, p, "duplicate-%d" % seed)


def test_duplicated_row_with_contradictory_bounds(eng, orc):
    for seed in (4, 5):
        p, r, j = _with_duplicate(orc, seed)
        H, g, A, lba, uba, lbx, ubx = p
        hi = uba[r] if np.isfinite(uba[r]) else lba[r] + 1.0
        lba[j] = hi + 1.0; uba[j] = hi + 2.0; lba[r] = -np.inf; uba[r] = hi
        x, cost, status = _launch(eng, [p])
        assert status[0] == 1
        assert orc.qp_solve(*p)[2]["status"] == 1


def test_non_symmetric_hessian(eng, orc):
    """H + K with K skew: x'Kx = 0, so the problem is the symmetrised one and its certificate must hold."""
    for n, m, seed in ((9, 7, 6), (65, 30, 7)):
        H, g, A, lba, uba, lbx, ubx = Q.spd(n, m, seed=seed)
        K = np.random.default_rng(seed).standard_normal((n, n)); K = K - K.T
        ps = (H, g, A, lba, uba, lbx, ubx)
        ref = _reference(orc, "spd", ps)
        x, cost, status = _launch(eng, [(H + K,) + ps[1:]])
        _check("skew-%d" % n, "spd", ps, ref, x[0], int(status[0]))
        _check_cost((H + K,) + ps[1:], x[0], cost[0])


def test_start_point_given(eng, orc):
    """x0 is the proximal centre: on a strictly convex problem the result is x* from any start."""
    p = Q.spd(9, 7, seed=8)
    rng = np.random.default_rng(8)
    for x0 in (rng.standard_normal(9), np.full(9, 100.0)):
        _edge(eng, orc, p, "x0", x0=x0)


def test_unbounded_lp_is_not_a_success(eng, orc):
    n = 5
    g = np.random.default_rng(9).standard_normal(n)
    H = np.zeros((n, n))
    for p in ((H, g, np.zeros((0, n)), None, None, None, None),
              (H, g, np.random.default_rng(10).standard_normal((3, n)), np.full(3, -np.inf), np.full(3, np.inf), None, None)):
        x, cost, status = _launch(eng, [p])
        assert status[0] != 0, (status, x)
        assert orc.qp_solve(*p)[2]["status"] != 0


# ------------------------------------------------------------------------------------------------- no false success
@pytest.mark.parametrize("shape", Q.PSD_LP_SHAPES, ids=lambda s: "%dx%d-rank%d" % s)
def test_no_false_success_on_problems_the_method_gives_up_on(shape, eng, orc):
    """Random rank-deficient PSD / LP problems on which the oracle ends with status 1 (the proximal rounds run out).
    Where the kernel says 0 the certificate must hold at the size-class bound (here its floor: there is no oracle
    value); nothing else is asserted."""
    probs = [Q.psd_lp(*shape, seed=s) for s in range(Q.NPROB)]
    x, cost, status = _launch(eng, probs)
    for i, p in enumerate(probs):
        assert status[i] in (0, 1)
        if status[i] == 0:
            c = Q.certificate(*p, x[i])
            assert c["pviol"] <= 1e-13 and c["stat"] <= 1e-13, (shape, i, c["pviol"], c["stat"])


# ------------------------------------------------------------------------------- batch independence and stale state
def _mixed_batch(B):
    """spd, soft, infeasible and unbounded-LP problems of 9 variables and 7 rows in a shuffled order."""
    n, m = 9, 7
    probs, kinds = [], []
    for i in range(B):
        k = i % 4
        if k == 0:
            p = Q.spd(n, m, seed=100 + i)
        elif k == 1:
            p = Q.soft(5, 4, 3, False, 1.0 if i % 8 == 1 else 1e4, seed=100 + i)
        elif k == 2:
            H, g, A, lba, uba, lbx, ubx = Q.spd(n, m, seed=100 + i)
            A[2] = 0.0; A[2, 0] = 1.0; lba[2] = 5.0; uba[2] = 6.0          # contradicts ubx[0] <= 0.5
            p = (H, g, A, lba, uba, lbx, ubx)
        else:
            rng = np.random.default_rng([3, i])
            p = (np.zeros((n, n)), rng.standard_normal(n), rng.standard_normal((m, n)), np.full(m, -np.inf),
                 np.full(m, np.inf), np.full(n, -np.inf), np.full(n, np.inf))
        assert p[0].shape == (n, n) and p[2].shape == (m, n)
        probs.append(p); kinds.append(k)
    order = np.random.default_rng(2024).permutation(B)
    return [probs[i] for i in order], [kinds[i] for i in order]


def test_persistent_workgroups_carry_nothing_over(torch_mod, setup, monkeypatch):
    """One workgroup per CU and more than three problems per workgroup: every workgroup solves problems of different
    kinds one after another.  Results must not depend on what a workgroup solved before: each of 24 sampled problems
    in a launch of its own, and the whole launch repeated, reproduce x, cost and status bit for bit."""
    monkeypatch.setenv("EEPACC_QP_WGS_PER_CU", "1")
    grid = torch_mod.cuda.get_device_properties(0).multi_processor_count
    B = 3 * grid + 5
    probs, kinds = _mixed_batch(B)
    eng = _engine(setup)
    big = _launch(eng, probs)
    x, cost, status = big
    for i, (p, k) in enumerate(zip(probs, kinds)):
        assert (status[i] == 0) == (k < 2), (i, k, status[i])
        if status[i] == 0:
            c = Q.certificate(*p, x[i])
            assert c["pviol"] <= 1e-13 and c["stat"] <= 1e-13, (i, k, c["pviol"], c["stat"])
    for i in np.random.default_rng(7).choice(B, 24, replace=False):
        one = _launch(eng, [probs[i]])
        for a, b in zip(big, one):
            np.testing.assert_array_equal(a[i], b[0])
    for a, b in zip(big, _launch(eng, probs)):
        np.testing.assert_array_equal(a, b)
    # another shape on the same engine (the workspace grows), then the first shape again
    other = [Q.spd(65, 130, seed=s) for s in range(3)]
    xo, _, so = _launch(eng, other)
    assert (so == 0).all()
    for a, b in zip(big, _launch(eng, probs)):
        np.testing.assert_array_equal(a, b)
    xo2, _, _ = _launch(eng, other)
    np.testing.assert_array_equal(xo, xo2)


# ---------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable(torch_mod, setup, orc):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    eng = _engine(setup)
    p = Q.spd(4, 4, seed=1)
    good = _launch(eng, [p])
    assert good[2][0] == 0

    def still_works():
        for a, b in zip(good, _launch(eng, [p])):
            np.testing.assert_array_equal(a, b)

    with pytest.raises(EepaccError, match=EINVAL_MAX):
        eng.qp_solve_batched(np.eye(385)[None], np.zeros((1, 385)), np.zeros((1, 1, 385)))
    still_works()
    with pytest.raises(EepaccError, match=EINVAL_MAX):
        eng.qp_solve_batched(np.eye(4)[None], np.zeros((1, 4)), np.zeros((1, 2049, 4)))
    still_works()
    with pytest.raises(EepaccError, match=EINVAL_SIZES):
        eng.qp_solve_batched(np.zeros((1, 0, 0)), np.zeros((1, 0)), np.zeros((1, 0, 0)))
    still_works()
    x, cost, status = eng.qp_solve_batched(np.zeros((0, 4, 4)), np.zeros((0, 4)), np.zeros((0, 4, 4)))      # B = 0
    assert x.shape == (0, 4) and status.shape == (0,)
    still_works()
    # the largest size the contract admits is solved (nV = 384, nC = 2048 is a table case; here the limits one by one)
    for n, m in ((384, 1), (1, 2048)):
        pp = Q.spd(n, m, seed=2)
        xx, _, st = _launch(eng, [pp])
        assert st[0] == 0
        c = Q.certificate(*pp, xx[0])
        assert c["pviol"] <= 1e-13 and c["stat"] <= 1e-13
