"""eepacc_qp_solve_batched_dual (csrc/eepacc_qp_dense.hip, k_qp_dense<true>): multipliers in CasADi's convention, the final
working set, and the warm start from a working set -- checked with tests/qp_dual_check.py and the solver-independent
certificate of tests/qp_cert.py, which share nothing with the kernel's method.

Bounds.  Stationarity of the returned multipliers, r = ||Hs x + g + A'lam_a + lam_x||_inf / max(1, ||g||_inf, ||lam||_inf):
max(1000 x qp_cert.certificate(p, x)["stat"], 1e-13) at the kernel's own x -- the best any non-negative multipliers do at
that point, with the margin tests/test_gpu_qp_dense.py gives for differing summation and pivot order; the hard ceiling is
the kernel's acceptance threshold, 1e-9.  Signs and complementarity: none may be off.  Certificate of x (warm-start
tests): the bounds of tests/test_gpu_qp_dense.py, 1000 x the CPU oracle's value on the same problem, floor 1e-13.
Unique multipliers (spd; the two sides of an equality merged into one signed multiplier mu; active normals N of full
column rank): the reference is the certificate's non-negative least-squares solution mu_ref with residual res_ref.  Any
mu that meets the stationarity bound above at the reference's scale den_ref = max(1, ||g||_inf, ||mu_ref||_inf) has
||grad - N mu||_2 <= sqrt(n) bound den_ref, and N (mu_ref - mu) is the difference of the two residuals, so
||mu - mu_ref||_2 <= (sqrt(n) bound den_ref + ||res_ref||_2) / sigma_min(N).  That is the tolerance: it is made of the
problem, the reference and the asserted bound only; nothing the kernel returned enters it.

Measured on an MI355X (largest over the 3 problems of a case; `-s` prints every figure per problem):
                                      r          certificate stat at the same x    held rows with lam == 0
    spd-3x5                           2.0e-16    3.1e-17                           0
    spd-9x16                          1.3e-16    8.3e-16                           0
    spd-65x130                        9.1e-16    2.3e-15                           0
    spd-257x100                       1.7e-15    4.6e-15                           0
    soft-20+43-10-lbx-w10000          4.0e-16    2.2e-15                           0
    soft-20+43-10-row-w1              3.7e-16    3.0e-15                           0
    soft-40+88-30-lbx-w1              7.5e-16    3.0e-15                           0
    indef-12x9-0.05                   2.0e-16    2.6e-16                           0
    indef-70x40-0.001                 5.3e-16    2.2e-15                           0
Unique multipliers, largest ||mu_kernel - mu_ref||_2 (smallest tolerance of the case): spd-3x5 4.5e-16 (1.7e-13), spd-9x16
4.1e-15 (4.4e-12), spd-65x130 7.5e-15 (1.2e-10), spd-257x100 2.0e-14 (9.5e-10); the active normals were independent on all
twelve problems.
r stays below the certificate's own value nearly everywhere (inf-norm against 2-norm): the margin of 1000 is not used.
x, cost and status of the new entry without a warm start equal eepacc_qp_solve_batched bit for bit on both cases of
test_same_primal_as_the_old_entry_point.
Warm start from the own working set, iterations cold -> warm (round of the exact exit by the CPU oracle): spd-65x130
107/86/83 -> 0/0/0 (1/1/1); soft-40+88-30-lbx-w1 88/117/86 -> 0/0/0 (1/1/1); indef-12x9-0.05 12/14/14 -> 0/14/14 (1/2/3: a
set that shows a negative multiplier in round 0 is discarded whole).  Mixed launch: all 211 warm instances with cold
iterations need none.  After the perturbation of test_warm_start_after_a_perturbation: spd-65x130 98/89/79 -> 0/0/79,
soft-40+88-30-lbx-w1 86/105/84 -> 86/105/1.
"""
import numpy as np
import pytest

import qp_cert as Q
import qp_dual_check as D
from conftest import make_case

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
NAME = "eepacc_qp_solve_batched_dual"
SIZE_CASES = ["spd-3x5", "spd-9x16", "spd-65x130", "spd-257x100",
              "soft-20+43-10-lbx-w10000", "soft-20+43-10-row-w1", "soft-40+88-30-lbx-w1",
              "indef-12x9-0.05", "indef-70x40-0.001"]


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


def _dual(eng, probs, x0=None, ws0=None):
    """One launch of the new entry for problems of one shape; a dict of numpy arrays."""
    r = eng.qp_solve_batched_dual(*[_stack(probs, k) for k in range(7)], x0=x0, ws0=ws0)
    eng.synchronize()
    return {k: v.cpu().numpy() for k, v in r._asdict().items()}


def _old(eng, probs, x0=None):
    x, cost, status = eng.qp_solve_batched(*[_stack(probs, k) for k in range(7)], x0=x0)
    eng.synchronize()
    return x.cpu().numpy(), cost.cpu().numpy(), status.cpu().numpy()


_REF = {}


def _oracle_bounds(orc, key, p):
    """(pviol bound, stat bound) of tests/test_gpu_qp_dense.py for one problem: 1000 x the oracle's certificate, floor
    1e-13.  Computed once per key."""
    if key not in _REF:
        x, _, st = orc.qp_solve(*p)
        assert st["status"] == 0, (key, "the oracle does not solve the case")
        c = Q.certificate(*p, x)
        _REF[key] = (max(1000.0 * c["pviol"], 1e-13), max(1000.0 * c["stat"], 1e-13))
    return _REF[key]


def _check_duals(tag, p, o, i, fam=None):
    """The assertions on the multipliers and the working set of instance i; returns (r, certificate stat, held zeros)."""
    assert o["status"][i] == 0, (tag, o["status"][i])
    x, la, lx, wa, wx = (o[k][i] for k in ("x", "lam_a", "lam_x", "ws_a", "ws_x"))
    assert np.isfinite(la).all() and np.isfinite(lx).all(), tag
    d = D.dual_check(p, x, la, lx, wa, wx)
    c = Q.certificate(*p, x)
    held0 = int(((wa != 0) & (la == 0.0)).sum() + ((wx != 0) & (lx == 0.0)).sum())
    bound = max(1000.0 * c["stat"], 1e-13)
    print("%s r %.2e (certificate stat %.2e, bound %.2e) held %d of them with lam == 0: %d iters %d"
          % (tag, d["r"], c["stat"], bound, (wa != 0).sum() + (wx != 0).sum(), held0, o["iters"][i]))
    assert not d["sign"], (tag, d["sign"])
    assert not d["comp"], (tag, d["comp"])
    assert not ((la != 0.0) & (wa == 0)).any() and not ((lx != 0.0) & (wx == 0)).any(), tag
    assert d["r"] <= 1e-9, (tag, d["r"])                      # the kernel's own acceptance threshold: the hard ceiling
    assert d["r"] <= bound, (tag, d["r"], bound)
    if fam == "spd" and c["active"]:
        N, mu_c, mu_k = D.net_multipliers(p, c, la, lx)
        sv = np.linalg.svd(N, compute_uv=False)
        if N.shape[1] <= N.shape[0] and sv[-1] > 1e-8 * sv[0]:
            # reference side only: multipliers that meet the stationarity bound asserted above, with the scale of the
            # REFERENCE multipliers, leave ||grad - N mu||_2 <= sqrt(n) bound den_ref; N (mu_ref - mu) is the difference
            # of the two residuals
            res_c = np.asarray(c["grad"] - N.astype(Q.LD) @ mu_c.astype(Q.LD), dtype=np.float64)
            den_ref = max(1.0, np.abs(p[1]).max(), np.abs(mu_c).max())
            tol = (np.sqrt(N.shape[0]) * bound * den_ref + np.linalg.norm(res_c)) / sv[-1]
            dl = np.linalg.norm(mu_k - mu_c)
            print("%s unique multipliers: |lam - lam_nnls|_2 %.2e (bound %.2e, sigma_min %.2e)" % (tag, dl, tol, sv[-1]))
            assert dl <= tol, (tag, dl, tol)
        else:
            print("%s active normals dependent (sigma_min %.2e of %.2e): multipliers not unique, not compared" % (tag, sv[-1], sv[0]))
    return d["r"], c["stat"], held0


def _check_x(tag, orc, key, p, o, i):
    """Certificate of x at the bounds of a cold solve (the oracle's, as tests/test_gpu_qp_dense.py sets them)."""
    pb, sb = _oracle_bounds(orc, key, p)
    c = Q.certificate(*p, o["x"][i])
    print("%s pviol %.2e (bound %.2e) stat %.2e (bound %.2e)" % (tag, c["pviol"], pb, c["stat"], sb))
    assert o["status"][i] == 0, (tag, o["status"][i])
    assert c["pviol"] <= pb and c["stat"] <= sb, (tag, c["pviol"], pb, c["stat"], sb)


# ----------------------------------------------------------------------------------------------------- size classes
@pytest.mark.parametrize("cid", SIZE_CASES)
def test_duals_at_size_classes(cid, eng):
    fam, probs = Q.make_case(cid)
    o = _dual(eng, probs)
    worst = np.zeros(3)
    for i, p in enumerate(probs):
        worst = np.maximum(worst, _check_duals("%s[%d]" % (cid, i), p, o, i, fam))
    print("%s largest r %.2e, certificate stat %.2e, held rows with lam == 0: %d" % ((cid,) + tuple(worst[:2]) + (int(worst[2]),)))


@pytest.mark.parametrize("cid", ["spd-9x16", "soft-20+43-10-lbx-w10000"])
def test_same_primal_as_the_old_entry_point(cid, eng):
    fam, probs = Q.make_case(cid)
    o = _dual(eng, probs)
    x, cost, status = _old(eng, probs)
    np.testing.assert_array_equal(o["x"], x)
    np.testing.assert_array_equal(o["cost"], cost)
    np.testing.assert_array_equal(o["status"], status)


# -------------------------------------------------------------------------------------------------------- warm start
@pytest.mark.parametrize("cid", ["spd-65x130", "soft-40+88-30-lbx-w1", "indef-12x9-0.05"])
def test_warm_start_from_own_working_set(cid, eng, orc):
    """Cold, then again from the working set the cold solve ended with.  Which status-0 exit an instance took is not an
    output of the entry point; the CPU oracle restates the method and reports it (polished == 1: the exact solve
    accepted the point; prox_iterations: in which proximal round).  An instance whose exact exit came in the first
    round must need no iteration at all when warm.  One accepted in a later round ended on the working set of a
    proximal problem re-centred at its last iterate; warm-started, round 0 is centred at x0 again, that set's
    multipliers are another problem's and may be negative, and the set is then discarded: only <= holds there."""
    fam, probs = Q.make_case(cid)
    cold = _dual(eng, probs)
    warm = _dual(eng, probs, ws0=(cold["ws_a"], cold["ws_x"]))
    n_zero = 0
    for i, p in enumerate(probs):
        tag = "%s[%d]" % (cid, i)
        st = orc.qp_solve(*p)[2]
        print("%s iters cold %d warm %d (oracle: polished %d in round %d)"
              % (tag, cold["iters"][i], warm["iters"][i], st["polished"], st["prox_iterations"]))
        _check_x(tag, orc, (cid, i), p, warm, i)
        _check_duals(tag, p, warm, i)
        assert warm["iters"][i] <= cold["iters"][i], tag
        if cold["iters"][i] > 0 and st["status"] == 0 and st["polished"] == 1 and st["prox_iterations"] == 1:
            assert warm["iters"][i] == 0, tag
            n_zero += 1
    assert n_zero >= 1, cid                                   # every case has such an instance


def _perturbed(p, seed):
    H, g, A, lba, uba, lbx, ubx = [np.array(a, copy=True) for a in p]
    d = np.random.default_rng(seed).standard_normal(g.shape)
    g = g + 0.01 * np.linalg.norm(g) * d / np.linalg.norm(d)
    return H, g, A, lba, uba + 1e-3, lbx, ubx


@pytest.mark.parametrize("cid", ["spd-65x130", "soft-40+88-30-lbx-w1"])
def test_warm_start_after_a_perturbation(cid, eng, orc):
    fam, probs = Q.make_case(cid)
    base = _dual(eng, probs)
    pert = [_perturbed(p, i) for i, p in enumerate(probs)]
    cold = _dual(eng, pert)
    warm = _dual(eng, pert, ws0=(base["ws_a"], base["ws_x"]))
    for i, p in enumerate(pert):
        tag = "%s-perturbed[%d]" % (cid, i)
        print("%s iters cold %d warm %d" % (tag, cold["iters"][i], warm["iters"][i]))
        _check_x(tag, orc, (cid, "perturbed", i), p, warm, i)
        _check_duals(tag, p, warm, i)


def test_bad_warm_starts_cannot_hurt(eng, orc):
    cid = "spd-9x16"
    fam, probs = Q.make_case(cid)
    B, n, m = len(probs), 9, 16
    own = _dual(eng, probs)
    other = _dual(eng, [Q.spd(n, m, seed=50 + s) for s in range(B)])
    ones_a, ones_x = np.ones((B, m), dtype=np.int8), np.ones((B, n), dtype=np.int8)
    alt = (np.where(np.arange(m) % 2 == 0, 1, -1).astype(np.int8) * ones_a, np.where(np.arange(n) % 2 == 0, 1, -1).astype(np.int8) * ones_x)
    lo_inf = np.stack([np.where(np.isfinite(p[3]), 0, -1) for p in probs]).astype(np.int8)      # only sides without a bound
    hi_inf = np.stack([np.where(np.isfinite(p[4]), 0, 1) for p in probs]).astype(np.int8)
    feeds = {"all +1": (ones_a, ones_x), "all -1": (-ones_a, -ones_x),
             "alternating": alt, "alternating, sides swapped": (-alt[0], -alt[1]),
             "entries of value 7": (7 * ones_a, 7 * ones_x),
             "infinite lower sides": (lo_inf, 0 * ones_x), "infinite upper sides": (hi_inf, 0 * ones_x),
             "more than nV rows": (-ones_a, ones_x),
             "another problem's working set": (other["ws_a"], other["ws_x"]),
             "rows only": (own["ws_a"], None), "variables only": (None, own["ws_x"])}
    assert (np.abs(ones_a).sum(1) > n).all()
    for name, ws0 in feeds.items():
        o = _dual(eng, probs, ws0=ws0)
        for i, p in enumerate(probs):
            tag = "%s, %s [%d]" % (cid, name, i)
            print("%s iters %d (cold %d)" % (tag, o["iters"][i], own["iters"][i]))
            _check_x(tag, orc, (cid, i), p, o, i)
            _check_duals(tag, p, o, i)
    # entries that are no request at all leave the cold solve, bit for bit
    for name in ("entries of value 7", "infinite lower sides", "infinite upper sides"):
        o = _dual(eng, probs, ws0=feeds[name])
        for k in own:
            np.testing.assert_array_equal(o[k], own[k], err_msg=name + " " + k)
    # the unbounded LP of test_gpu_qp_dense.test_unbounded_lp_is_not_a_success stays a failure when warm-started
    nl = 5
    g = np.random.default_rng(9).standard_normal(nl)
    A = np.random.default_rng(10).standard_normal((3, nl))
    p = (np.zeros((nl, nl)), g, A, np.full(3, -np.inf), np.full(3, np.inf), None, None)
    for ws0 in (None, (np.ones((1, 3), dtype=np.int8), np.ones((1, nl), dtype=np.int8))):
        o = _dual(eng, [p], ws0=ws0)
        assert o["status"][0] == 1
        assert np.isnan(o["lam_a"]).all() and np.isnan(o["lam_x"]).all()
        assert (o["ws_a"] == 0).all() and (o["ws_x"] == 0).all()


# ------------------------------------------------------------------------------- batch independence and stale state
def _mixed_batch(B):
    """spd, soft, infeasible and unbounded-LP problems of 9 variables and 7 rows in a shuffled order (the mix of
    tests/test_gpu_qp_dense.py)."""
    n, m = 9, 7
    probs = []
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
        probs.append(p)
    order = np.random.default_rng(2024).permutation(B)
    return [probs[i] for i in order], [int(i % 4) for i in order]


def test_mixed_batch_and_persistent_workgroups(torch_mod, setup, monkeypatch):
    """One workgroup per CU and more than three problems per workgroup, warm and cold instances alternating: what the warm
    start installs (working set, flags, factors) must not reach the next problem of the workgroup.  Every cold instance
    equals its result in an all-cold launch, every warm one its result in an all-warm launch, bit for bit."""
    monkeypatch.setenv("EEPACC_QP_WGS_PER_CU", "1")
    grid = torch_mod.cuda.get_device_properties(0).multi_processor_count
    B = 3 * grid + 5
    probs, kinds = _mixed_batch(B)
    eng = _engine(setup)
    cold = _dual(eng, probs)
    assert ((cold["status"] == 0) == (np.array(kinds) < 2)).all()
    assert cold["iters"][cold["status"] == 0].max() > 0
    ws0 = (cold["ws_a"], cold["ws_x"])
    warm = _dual(eng, probs, ws0=ws0)
    is_warm = (np.arange(B) % 2 == 0)
    mixed = _dual(eng, probs, ws0=(ws0[0] * is_warm[:, None].astype(np.int8), ws0[1] * is_warm[:, None].astype(np.int8)))
    for k in cold:
        np.testing.assert_array_equal(mixed[k][~is_warm], cold[k][~is_warm], err_msg="cold " + k)
        np.testing.assert_array_equal(mixed[k][is_warm], warm[k][is_warm], err_msg="warm " + k)
    solved = cold["status"] == 0
    assert (warm["status"] == cold["status"]).all()
    assert (warm["iters"][solved] <= cold["iters"][solved]).all()
    used = solved & is_warm & (cold["iters"] > 0)
    assert (mixed["iters"][used] < cold["iters"][used]).any(), "no warm instance of the mixed launch saved an iteration"
    print("mixed launch: %d of %d warm instances with cold iters > 0 need fewer iterations, %d need none"
          % ((mixed["iters"][used] < cold["iters"][used]).sum(), used.sum(), (mixed["iters"][used] == 0).sum()))
    for i in np.random.default_rng(11).choice(np.nonzero(solved & is_warm)[0], 12, replace=False):
        _check_duals("mixed[%d]" % i, probs[i], mixed, i)
    failed = ~solved
    assert np.isnan(mixed["lam_a"][failed]).all() and np.isnan(mixed["lam_x"][failed]).all()
    assert (mixed["ws_a"][failed] == 0).all() and (mixed["ws_x"][failed] == 0).all()


# ------------------------------------------------------------------------------------------------------------ edges
def _raw(eng, torch, p, drop=None):
    """The entry point through ctypes for one problem, with the output named `drop` passed as NULL."""
    H, g, A, lba, uba, lbx, ubx = p
    n, m = H.shape[0], A.shape[0]
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v), dtype=torch.float64, device=eng.device)
    ins = [dev(H), dev(g), dev(A.T), dev(lba), dev(uba), dev(lbx), dev(ubx)]
    outs = dict(x=torch.empty(n, dtype=torch.float64, device=eng.device), cost=torch.empty(1, dtype=torch.float64, device=eng.device),
                status=torch.empty(1, dtype=torch.int32, device=eng.device),
                lam_a=torch.empty(m, dtype=torch.float64, device=eng.device), lam_x=torch.empty(n, dtype=torch.float64, device=eng.device),
                ws_a=torch.empty(m, dtype=torch.int8, device=eng.device), ws_x=torch.empty(n, dtype=torch.int8, device=eng.device),
                iters=torch.empty(1, dtype=torch.int32, device=eng.device))
    ptr = lambda k: None if k == drop else outs[k].data_ptr()
    rc = eng.lib.eepacc_qp_solve_batched_dual(eng.h, 1, n, m, *[t.data_ptr() for t in ins], None, None, None,
                                              *[ptr(k) for k in ("x", "cost", "status", "lam_a", "lam_x", "ws_a", "ws_x", "iters")],
                                              eng._stream())
    assert rc == 0, eng.lib.eepacc_last_error()
    eng.synchronize()
    return {k: v.cpu().numpy() for k, v in outs.items() if k != drop}


def test_edges(torch_mod, setup):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    eng = _engine(setup)
    # nC = 0 with a box
    for n in (1, 6, 70):
        p = Q.spd(n, 0, seed=1)
        o = _dual(eng, [p])
        assert o["lam_a"].shape == (1, 0) and o["ws_a"].shape == (1, 0)
        _check_duals("box-%d" % n, p, o, 0, "spd")
    # no bounds at all: a linear solve, every multiplier zero
    H, g = Q.spd(6, 4, seed=2)[:2]
    A = Q.spd(6, 4, seed=2)[2]
    o = _dual(eng, [(H, g, A, None, None, None, None)])
    assert o["status"][0] == 0 and o["iters"][0] == 0
    for k in ("lam_a", "lam_x", "ws_a", "ws_x"):
        assert (o[k] == 0).all(), k
    assert np.abs(H @ o["x"][0] + g).max() <= 64 * EPS * np.linalg.cond(H) * max(1.0, np.abs(g).max())
    # each output that may be NULL, in turn: the others do not change
    p = Q.spd(9, 16, seed=3)
    full = _raw(eng, torch_mod, p)
    assert full["status"][0] == 0
    for drop in ("cost", "status", "lam_a", "lam_x", "ws_a", "ws_x", "iters"):
        part = _raw(eng, torch_mod, p, drop)
        for k in part:
            np.testing.assert_array_equal(part[k], full[k], err_msg="%s without %s" % (k, drop))
    # B = 0
    r = eng.qp_solve_batched_dual(np.zeros((0, 4, 4)), np.zeros((0, 4)), np.zeros((0, 4, 4)))
    assert r.x.shape == (0, 4) and r.lam_a.shape == (0, 4) and r.ws_x.shape == (0, 4) and r.iters.shape == (0,)
    # the refusals of eepacc_qp_solve_batched, under the new name
    good = _dual(eng, [p])

    def still_works():
        again = _dual(eng, [p])
        for k in good:
            np.testing.assert_array_equal(again[k], good[k])

    with pytest.raises(EepaccError, match=NAME + ": nV/nC above EEPACC_QP_MAX_NV/NC"):
        eng.qp_solve_batched_dual(np.eye(385)[None], np.zeros((1, 385)), np.zeros((1, 1, 385)))
    still_works()
    with pytest.raises(EepaccError, match=NAME + ": nV/nC above EEPACC_QP_MAX_NV/NC"):
        eng.qp_solve_batched_dual(np.eye(4)[None], np.zeros((1, 4)), np.zeros((1, 2049, 4)))
    still_works()
    with pytest.raises(EepaccError, match=NAME + ": bad sizes"):
        eng.qp_solve_batched_dual(np.zeros((1, 0, 0)), np.zeros((1, 0)), np.zeros((1, 0, 0)))
    still_works()
    rc = eng.lib.eepacc_qp_solve_batched_dual(eng.h, 1, 4, 4, *([None] * 8), None, None, *([None] * 8), eng._stream())
    assert rc == -1 and eng.lib.eepacc_last_error().decode() == NAME + ": NULL buffer"
    still_works()


def test_class_handle_is_refused(torch_mod, setup):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, EepaccError
    eng = Engine.from_classes([setup[0], setup[0]], [setup[1], setup[1]], device=0, max_batch=8)
    with pytest.raises(EepaccError, match=NAME + ": a handle of eepacc_create_classes runs ABMPC only"):
        eng.qp_solve_batched_dual(np.eye(4)[None], np.zeros((1, 4)), np.zeros((1, 1, 4)))
