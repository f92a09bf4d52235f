"""Checker for the multipliers and the working set of  min 1/2 x'Hx + g'x  s.t.  lba <= Ax <= uba, lbx <= x <= ubx  in
CasADi's convention (the lam_a, lam_x outputs of conic):

    Hs x + g + A' lam_a + lam_x = 0,  Hs = (H + H')/2;   lam <= 0 where the lower side holds, lam >= 0 where the upper
    side holds, lam = 0 elsewhere;   ws = -1 / +1 / 0 names the side a row or variable is held at.

Plain numpy in numpy.longdouble, built on tests/qp_cert.py: nothing of the product is used here.
"""
import numpy as np

import qp_cert as Q

LD = Q.LD


def _problem(p):
    H, g, A, lba, uba, lbx, ubx = p
    H = np.asarray(H, dtype=np.float64); n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n); m = A.shape[0]
    return (H, np.asarray(g, dtype=np.float64), A, Q._full(lba, m, -np.inf), Q._full(uba, m, np.inf),
            Q._full(lbx, n, -np.inf), Q._full(ubx, n, np.inf))


def dual_check(p, x, lam_a, lam_x, ws_a, ws_x):
    """r = ||Hs x + g + A' lam_a + lam_x||_inf / max(1, ||g||_inf, ||lam||_inf);
    sign = the entries whose multiplier contradicts ws: (kind, index, why), kind 0 = row of A, 1 = variable;
    comp = the non-zero ws entries without a finite bound on that side, or with x further than
           qp_cert.ACTIVE_TOL (1 + |bound|) from it: (kind, index, why)."""
    H, g, A, lba, uba, lbx, ubx = _problem(p)
    n, m = H.shape[0], A.shape[0]
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    la = np.asarray(lam_a, dtype=np.float64).reshape(m); lx = np.asarray(lam_x, dtype=np.float64).reshape(n)
    wa = np.asarray(ws_a).reshape(m).astype(int); wx = np.asarray(ws_x).reshape(n).astype(int)
    Hs = 0.5 * (H.astype(LD) + H.astype(LD).T)
    res = Hs @ xl + g.astype(LD) + lx.astype(LD)
    if m:
        res = res + A.astype(LD).T @ la.astype(LD)
    lam = np.concatenate([la, lx])
    den = max(1.0, np.abs(g).max(initial=0.0), np.abs(lam).max(initial=0.0))
    r = float(np.abs(res).max(initial=0.0) / den)
    ax = A.astype(LD) @ xl if m else np.zeros(0, dtype=LD)
    sign, comp = [], []
    for kind, l, w, lo, hi, val in ((0, la, wa, lba, uba, ax), (1, lx, wx, lbx, ubx, xl)):
        for i in range(len(l)):
            if w[i] == -1 and l[i] > 0.0:
                sign.append((kind, i, "lam > 0 on a lower side"))
            elif w[i] == 1 and l[i] < 0.0:
                sign.append((kind, i, "lam < 0 on an upper side"))
            elif w[i] == 0 and l[i] != 0.0:
                sign.append((kind, i, "lam != 0 outside the working set"))
            elif w[i] not in (-1, 0, 1):
                sign.append((kind, i, "ws is none of -1, 0, +1"))
            if w[i] in (-1, 1):
                b = lo[i] if w[i] == -1 else hi[i]
                if not np.isfinite(b):
                    comp.append((kind, i, "working-set side has no finite bound"))
                elif abs(val[i] - LD(b)) > Q.ACTIVE_TOL * (1.0 + abs(b)):
                    comp.append((kind, i, "x is not at the bound: %.3e" % float(abs(val[i] - LD(b)))))
    return dict(r=r, sign=sign, comp=comp, res=res)


def from_certificate(p, c):
    """(lam_a, lam_x, ws_a, ws_x) in CasADi's convention from qp_cert.certificate(...)'s "active" / "lam": the
    certificate writes grad = sum lam_c sgn_c n_c with lam_c >= 0 over the sides sgn_c (row or variable) >= sgn_c bound,
    so the multiplier of that row or variable is -sgn_c lam_c.  Where both sides of an equality are listed the entry is
    their sum and ws names the side that carries it (the lower one if neither does)."""
    H, g, A, lba, uba, lbx, ubx = _problem(p)
    n, m = H.shape[0], A.shape[0]
    lam = (np.zeros(m), np.zeros(n))
    ws = (np.zeros(m, dtype=np.int8), np.zeros(n, dtype=np.int8))
    for (kind, i, sgn), l in zip(c["active"], c["lam"]):
        lam[kind][i] += -sgn * l
    for kind, i, sgn in c["active"]:
        v = lam[kind][i]
        ws[kind][i] = -1 if v < 0.0 else 1 if v > 0.0 else (ws[kind][i] if ws[kind][i] != 0 else (-1 if sgn > 0 else 1))
    return lam[0], lam[1], ws[0], ws[1]


def net_multipliers(p, c, lam_a, lam_x):
    """The certificate's rows and variables c["active"] with the two sides of an equality merged: (N, mu_cert, mu) with
    N the n x k matrix of their normals (unsigned), mu_cert = sum over the listed sides of sgn lam_c, and mu = -lam the
    same quantity from multipliers in CasADi's convention, so that  Hs x + g = N mu  is what both claim."""
    H, g, A, lba, uba, lbx, ubx = _problem(p)
    n = H.shape[0]
    ids, mu_c = [], []
    for (kind, i, sgn), l in zip(c["active"], c["lam"]):
        if (kind, i) not in ids:
            ids.append((kind, i)); mu_c.append(0.0)
        mu_c[ids.index((kind, i))] += sgn * l
    N = np.zeros((n, len(ids)))
    mu = np.zeros(len(ids))
    for k, (kind, i) in enumerate(ids):
        if kind == 0:
            N[:, k] = A[i]; mu[k] = -lam_a[i]
        else:
            N[i, k] = 1.0; mu[k] = -lam_x[i]
    return N, np.array(mu_c), mu
