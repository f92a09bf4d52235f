"""The optimality certificate of tests/qp_cert.py has teeth and the case table of tests/test_gpu_qp_dense.py is sound:
the CPU oracle solves every problem of the table (status 0) to a point the certificate accepts at pviol <= 1e-14,
stat <= 1e-13; three corrupted solutions are rejected; refined_solution agrees with the oracle within qp_cert.D_REF.
Runs without a GPU."""
import numpy as np
import pytest

import qp_cert as Q
from conftest import make_case

PVIOL_MAX, STAT_MAX = 1e-14, 1e-13
REJECT = 1e-8


@pytest.fixture(scope="module")
def orc():
    from oracle.loader import Oracle
    OPT, V, _, _ = make_case("ABO", 20)
    return Oracle(OPT, V)


@pytest.mark.parametrize("cid", list(Q.CASES))
def test_oracle_solves_table_case_and_certificate_accepts(cid, orc):
    fam, probs = Q.make_case(cid)
    sols = Q.solve_all(orc.qp_solve, probs)
    for i, (p, (x, cost, st)) in enumerate(zip(probs, sols)):
        assert st["status"] == 0, (cid, i, st)
        c = Q.certificate(*p, x)
        print("%s[%d] pviol %.2e stat %.2e active %d" % (cid, i, c["pviol"], c["stat"], len(c["active"])))
        assert c["pviol"] <= PVIOL_MAX and c["stat"] <= STAT_MAX, (cid, i, c["pviol"], c["stat"])
        if fam in Q.D_REF:
            xs, _ = Q.refined_solution(*p, x)
            d = np.abs(x - xs).max() / max(1.0, np.abs(xs).max())
            print("%s[%d] |x_oracle - x*| %.2e" % (cid, i, d))
            assert d <= Q.D_REF[fam], (cid, i, d)
            cs = Q.certificate(*p, xs)
            assert cs["pviol"] <= PVIOL_MAX and cs["stat"] <= STAT_MAX, (cid, i, cs["pviol"], cs["stat"])


def _drop_one_active(p, c):
    """The problem without the active one-sided constraint of the largest multiplier."""
    H, g, A, lba, uba, lbx, ubx = [np.array(a, copy=True) for a in p]
    kind, i, sgn = c["active"][int(np.argmax(c["lam"]))]
    lo, hi = (lba, uba) if kind == 0 else (lbx, ubx)
    if lo[i] == hi[i]:                     # an equality: both sides go
        lo[i], hi[i] = -np.inf, np.inf
    elif sgn > 0:
        lo[i] = -np.inf
    else:
        hi[i] = np.inf
    return H, g, A, lba, uba, lbx, ubx


@pytest.mark.parametrize("cid", ["spd-9x16", "spd-65x130", "soft-20+43-10-lbx-w1", "soft-20+44-10-row-w10000", "indef-70x40-0.05"])
def test_certificate_rejects_corrupted_solutions(cid, orc):
    fam, probs = Q.make_case(cid)
    p = probs[0]
    H, g, A, lba, uba, lbx, ubx = p
    n = H.shape[0]
    x, _, st = orc.qp_solve(*p)
    assert st["status"] == 0
    c = Q.certificate(*p, x)
    assert c["pviol"] <= PVIOL_MAX and c["stat"] <= STAT_MAX
    assert c["lam"].max() > 0.0
    # a free variable moved by 1e-6: no bound within reach, curvature along e_j
    bound_vars = {i for kind, i, _ in c["active"] if kind == 1}
    free = [j for j in range(n) if j not in bound_vars and abs(H[j, j]) > 0.0]
    assert free
    xb = x.copy(); xb[free[0]] += 1e-6
    cb = Q.certificate(*p, xb)
    assert max(cb["stat"], cb["pviol"]) >= REJECT, (cb["stat"], cb["pviol"])
    # the solution of the same problem with one active bound removed
    p2 = _drop_one_active(p, c)
    x2, _, st2 = orc.qp_solve(*p2)
    assert st2["status"] == 0
    c2 = Q.certificate(*p2, x2)
    assert c2["pviol"] <= PVIOL_MAX and c2["stat"] <= STAT_MAX          # right for its own problem
    cw = Q.certificate(*p, x2)
    assert max(cw["stat"], cw["pviol"]) >= REJECT, (cw["stat"], cw["pviol"])
    # a wrong vertex: every boxed variable on the bound opposite to the sign the gradient asks for
    xv = x.copy()
    grad = np.asarray(c["grad"], dtype=np.float64)
    for j in range(n):
        if np.isfinite(lbx[j]) and np.isfinite(ubx[j]):
            xv[j] = lbx[j] if grad[j] < 0.0 else ubx[j]
    cv = Q.certificate(*p, xv)
    assert max(cv["stat"], cv["pviol"]) >= REJECT, (cv["stat"], cv["pviol"])


def test_soft_working_sets_cross_every_carry_slot(orc):
    """The soft cases end with working sets beyond 64, 128, 192, 256 and 320 rows (one carry[] slot of gi_drop per 64)."""
    want = {"soft-20+44-10-lbx-w10000": 64, "soft-40+88-30-lbx-w10000": 128, "soft-60+196-40-lbx-w1": 192,
            "soft-60+196-40-lbx-w10000": 256, "soft-128+256-100-lbx-w1": 320}
    for cid, least in want.items():
        assert max(orc.qp_solve(*p)[2]["n_active"] for p in Q.make_case(cid)[1]) >= least, cid


def test_random_psd_and_lp_are_not_all_solved(orc):
    """The no-false-success inputs of the GPU test: random rank-deficient PSD / pure LP problems without the soft
    structure, on some of which the oracle itself gives up (status 1).  Wherever it reports 0 the certificate holds."""
    gave_up = 0
    for n, m, rank in Q.PSD_LP_SHAPES:
        probs = [Q.psd_lp(n, m, rank, s) for s in range(Q.NPROB)]
        for p, (x, _, st) in zip(probs, Q.solve_all(orc.qp_solve, probs)):
            if st["status"] != 0:
                gave_up += 1
                continue
            c = Q.certificate(*p, x)
            assert c["pviol"] <= PVIOL_MAX and c["stat"] <= STAT_MAX, (n, m, rank, c["pviol"], c["stat"])
    assert gave_up > 0
