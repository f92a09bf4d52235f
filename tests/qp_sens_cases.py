"""Problems, directions and steps shared by tests/test_qp_sens_cpu.py and tests/test_gpu_qp_kkt.py: the small cases of
tests/qp_cert.py (all three problems of each), four data directions per problem and one finite-difference step per case.

Directions (seeded per case, problem and kind; every array scaled to inf-norm 1, so a step moves each datum by at most h):
    "g"       dg dense;
    "bounds"  dlba, duba, dlbx, dubx dense (an equality lba == uba moves as one: duba = dlba there, or the perturbed
              problem would be infeasible); only the held sides enter the derivative, the free sides move inside their
              margin;
    "H"       dH dense and not symmetric, restricted to the non-zero pattern of H + H' (a curvature-free slack stays
              curvature-free: with it the perturbed problem would be non-convex along that variable);
    "A"       dA dense, zeros of A included.
Step: the margin test of strict complementarity asks min(|lam| over held entries, slack over free sides) > 10 h scale,
scale = the largest magnitude in (1, H, g, A, finite bounds).  Measured margins (smallest over the case's problems, on the
CPU): spd-3x5 5.6e-2, spd-9x16 7.7e-3, spd-65x130 2.0e-3, soft-20+43-10-lbx-w10000 2.9e-3 at scale 1e4,
soft-20+43-10-row-w1 6.0e-3, indef-12x9-0.05 1.8e-4.  h = 1e-6 leaves a factor >= 4 everywhere but on the w = 1e4 case,
which gets h = 1e-8 (10 h scale = 1e-3).  That is STEP, the step along g and the bounds, where the solution on a fixed
working set is linear in the step and a central difference has no truncation error.  Along H and A it has one,
h^2 |x'''| / 6, while the rounding of x(+-h) enters the quotient as (e+ + e-) / 2h: step(cid, kind) takes STEP / 10 there, which
cuts the share of the truncation in the quotient's error a thousandfold (it is of the order of a per cent of the
rounding share at STEP on the worst problem) and lets the tests compare against the rounding allowance alone.
"""
import numpy as np

import qp_cert as Q
import qp_dual_check as D

CASES = ["spd-3x5", "spd-9x16", "spd-65x130", "soft-20+43-10-lbx-w10000", "soft-20+43-10-row-w1", "indef-12x9-0.05"]
STEP = {cid: 1e-6 for cid in CASES}
STEP["soft-20+43-10-lbx-w10000"] = 1e-8
KINDS = ["g", "bounds", "H", "A"]


def step(cid, kind):
    """The finite-difference step of case cid along a direction of the given kind."""
    return STEP[cid] / 10.0 if kind in ("H", "A") else STEP[cid]

DATA = ("H", "g", "A", "lba", "uba", "lbx", "ubx")


def problem(p):
    """The seven arrays of a problem with every bound array present (+-inf = absent)."""
    return D._problem(p)


def data_scale(p):
    H, g, A, lba, uba, lbx, ubx = problem(p)
    fin = [np.abs(b[np.isfinite(b)]).max(initial=0.0) for b in (lba, uba, lbx, ubx)]
    return max(1.0, np.abs(H).max(), np.abs(g).max(), np.abs(A).max(initial=0.0), *fin)


def _unit(v):
    m = np.abs(v).max(initial=0.0)
    return v / m if m > 0.0 else v


def direction(cid, i, kind, p):
    """dict of the data directions (keys of DATA) of one kind for problem i of case cid."""
    H, g, A, lba, uba, lbx, ubx = problem(p)
    rng = np.random.default_rng([CASES.index(cid), i, KINDS.index(kind), 2718])
    if kind == "g":
        return dict(g=_unit(rng.standard_normal(g.shape)))
    if kind == "bounds":
        d = dict(lba=_unit(rng.standard_normal(lba.shape)), uba=_unit(rng.standard_normal(uba.shape)),
                 lbx=_unit(rng.standard_normal(lbx.shape)), ubx=_unit(rng.standard_normal(ubx.shape)))
        d["uba"] = np.where(lba == uba, d["lba"], d["uba"])
        d["ubx"] = np.where(lbx == ubx, d["lbx"], d["ubx"])
        return d
    if kind == "H":
        return dict(H=_unit(rng.standard_normal(H.shape) * ((H != 0.0) | (H.T != 0.0))))
    return dict(A=_unit(rng.standard_normal(A.shape)))


def perturbed(p, d, t):
    """The problem with its data moved by t along d."""
    arrs = dict(zip(DATA, problem(p)))
    return tuple(arrs[k] + t * d[k] if k in d else arrs[k] for k in DATA)


def effective_direction(p_plus, p_minus, d, h):
    """The direction two solves at +-h actually took: data + h d is rounded to float64, so (data(+h) - data(-h)) / 2h
    differs from d by up to eps |data| / h (4e-10 at h = 1e-6), more than the rounding allowance of the quotient leaves
    room for; the difference of the two neighbouring arrays is exact.  For H it is the difference of the symmetrised
    Hs = 0.5 (H + H') as every solver here forms it in float64: that sum rounds too, differently at +h and -h.
    An absent bound stays absent (0)."""
    out = {}
    for k in d:
        a, b = p_plus[DATA.index(k)], p_minus[DATA.index(k)]
        if k == "H":
            a, b = 0.5 * (a + a.T), 0.5 * (b + b.T)
        q = (a - b) / (2.0 * h)
        out[k] = np.where(np.isfinite(q), q, 0.0)
    return out


def margin(p, x, lam_a, lam_x, ws_a, ws_x):
    """Strict complementarity of (x, lam, ws): the smaller of min |lam| over the held entries and the smallest slack
    over the finite sides that are not held (both sides of a held equality are held)."""
    H, g, A, lba, uba, lbx, ubx = problem(p)
    x = np.asarray(x, dtype=np.float64)
    out = np.inf
    for val, lo, hi, w, lam in ((A @ x, lba, uba, np.asarray(ws_a), lam_a), (x, lbx, ubx, np.asarray(ws_x), lam_x)):
        held = w != 0
        out = min(out, np.abs(np.asarray(lam)[held]).min(initial=np.inf))
        eq = held & (lo == hi)
        lo_free = np.isfinite(lo) & (w != -1) & ~eq
        hi_free = np.isfinite(hi) & (w != 1) & ~eq
        out = min(out, (val - lo)[lo_free].min(initial=np.inf), (hi - val)[hi_free].min(initial=np.inf))
    return float(out)


def cpu_solution(solve, p):
    """The CPU solver of the sensitivity tests: `solve` (the oracle's qp_solve) for a first x, qp_cert.refined_solution
    for x*, and the multipliers and working set of qp_cert.certificate at x* in CasADi's convention.
    Returns dict(x, lam_a, lam_x, ws_a, ws_x, x_ld), x_ld the refined solution before its rounding to float64."""
    x0, _, st = solve(*p)
    assert st["status"] == 0
    x, x_ld = Q.refined_solution(*p, x0)
    c = Q.certificate(*p, x)
    la, lx, wa, wx = D.from_certificate(p, c)
    # a side the certificate lists with multiplier zero is not part of the working set
    wa = np.where(la == 0.0, 0, wa).astype(np.int8); wx = np.where(lx == 0.0, 0, wx).astype(np.int8)
    return dict(x=x, lam_a=la, lam_x=lx, ws_a=wa, ws_x=wx, x_ld=x_ld)
