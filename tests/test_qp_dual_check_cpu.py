"""tests/qp_dual_check.py pins the sign convention of the dense QP operator's multipliers (CasADi's: Hs x + g + A'lam_a +
lam_x = 0, lam <= 0 on a lower side, >= 0 on an upper side) without a GPU: multipliers built from the non-negative
least-squares certificate of tests/qp_cert.py at the CPU oracle's x are accepted on four small table cases, and each of
three corruptions is rejected -- a flipped sign, a multiplier moved to an inactive row, a ws entry on an absent bound."""
import numpy as np
import pytest

import qp_cert as Q
import qp_dual_check as D
from conftest import make_case

R_MAX = 1e-13          # the bound tests/test_qp_cert_cpu.py holds the certificate's stat to
REJECT = 1e-8

CASES = ["spd-3x5", "spd-9x16", "soft-20+43-10-lbx-w10000", "soft-20+43-10-row-w1"]      # each has absent bounds


@pytest.fixture(scope="module")
def orc():
    from oracle.loader import Oracle
    OPT, V, _, _ = make_case("ABO", 20)
    return Oracle(OPT, V)


def _accepted(orc, cid, i):
    p = Q.make_case(cid)[1][i]
    x, _, st = orc.qp_solve(*p)
    assert st["status"] == 0
    c = Q.certificate(*p, x)
    return p, x, c, D.from_certificate(p, c)


@pytest.mark.parametrize("cid", CASES)
def test_checker_accepts_certificate_multipliers(cid, orc):
    for i in range(Q.NPROB):
        p, x, c, (la, lx, wa, wx) = _accepted(orc, cid, i)
        d = D.dual_check(p, x, la, lx, wa, wx)
        print("%s[%d] r %.2e (certificate stat %.2e) held %d" % (cid, i, d["r"], c["stat"], (wa != 0).sum() + (wx != 0).sum()))
        assert not d["sign"] and not d["comp"], (d["sign"], d["comp"])
        assert d["r"] <= R_MAX, d["r"]
        N, mu_c, mu = D.net_multipliers(p, c, la, lx)
        assert np.array_equal(mu, mu_c)
        assert np.abs(np.asarray(c["grad"], dtype=np.float64) - N @ mu).max() <= R_MAX * max(1.0, np.abs(c["grad"]).max(), np.abs(p[1]).max())


@pytest.mark.parametrize("cid", CASES)
def test_checker_rejects_corruptions(cid, orc):
    p, x, c, (la, lx, wa, wx) = _accepted(orc, cid, 0)
    m = len(la)
    lam = np.concatenate([la, lx]); ws = np.concatenate([wa, wx])
    k = int(np.argmax(np.abs(lam)))
    assert lam[k] != 0.0
    split = lambda v: (v[:m], v[m:])
    # a flipped sign: the wrong side of zero for its ws entry, and stationarity off by twice the multiplier
    bad = lam.copy(); bad[k] = -bad[k]
    d = D.dual_check(p, x, *split(bad), wa, wx)
    assert any(s[:2] == ((0, k) if k < m else (1, k - m)) for s in d["sign"]) and d["r"] >= REJECT, (d["sign"], d["r"])
    # the same multiplier on a row or variable outside the working set
    idle = [j for j in range(len(ws)) if ws[j] == 0]
    assert idle
    bad = lam.copy(); bad[idle[0]] = bad[k]; bad[k] = 0.0
    d = D.dual_check(p, x, *split(bad), wa, wx)
    assert any("outside the working set" in s[2] for s in d["sign"]) and d["r"] >= REJECT, (d["sign"], d["r"])
    # a ws entry on a side without a bound
    lo = np.concatenate([Q._full(p[3], m, -np.inf), Q._full(p[5], len(lx), -np.inf)])
    hi = np.concatenate([Q._full(p[4], m, np.inf), Q._full(p[6], len(lx), np.inf)])
    absent = [(j, -1) for j in idle if not np.isfinite(lo[j])] + [(j, 1) for j in idle if not np.isfinite(hi[j])]
    assert absent, cid
    j, side = absent[0]
    wb = ws.copy(); wb[j] = side
    d = D.dual_check(p, x, la, lx, *split(wb))
    assert any("no finite bound" in s[2] for s in d["comp"]), d["comp"]
    # and one on a bound x is not at
    far = [j for j in idle if np.isfinite(lo[j]) and np.isfinite(hi[j])]
    if far:
        wb = ws.copy(); wb[far[0]] = -1
        assert any("not at the bound" in s[2] for s in D.dual_check(p, x, la, lx, *split(wb))["comp"])
