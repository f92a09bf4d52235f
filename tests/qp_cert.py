"""Solver-independent optimality certificate for  min 1/2 x'Hx + g'x  s.t.  lba <= Ax <= uba, lbx <= x <= ubx,
a long-double refined solution for the strictly convex case, and the seeded problem families the dense QP operator
is tested on.  Plain numpy/scipy: nothing of the oracle or of the product is used here.

certificate():  pviol = worst violation of a finite bound, relative to 1 + |bound|;
                stat  = min_{lam >= 0} ||Hs x + g - N' lam||_2 / max(1, ||g||_inf, ||Hs x + g||_inf), N the signed normals
                of the one-sided constraints within 1e-8 (1 + |bound|) of their bound (non-negative least squares).
pviol ~ 0 and stat ~ 0 prove optimality of x for a convex problem and a first-order KKT point otherwise, whatever
produced x.  All values are evaluated in numpy.longdouble.
"""
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import scipy.linalg
from scipy.optimize import nnls

LD = np.longdouble
ACTIVE_TOL = 1e-8


def _full(v, n, fill):
    return np.full(n, fill) if v is None else np.asarray(v, dtype=np.float64).reshape(n)


def one_sided(A, lba, uba, lbx, ubx, vals_rows, vals_x):
    """The finite one-sided constraints  sgn * value >= sgn * bound  as (kind, index, sgn, bound, value) arrays:
    kind 0 = row of A, 1 = variable."""
    out = []
    for kind, lo, hi, vals in ((0, lba, uba, vals_rows), (1, lbx, ubx, vals_x)):
        for sgn, b in ((1.0, lo), (-1.0, hi)):
            idx = np.nonzero(np.isfinite(b))[0]
            for i in idx:
                out.append((kind, int(i), sgn, float(b[i]), vals[i]))
    return out


def certificate(H, g, A, lba, uba, lbx, ubx, x):
    H = np.asarray(H, dtype=np.float64); n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n); m = A.shape[0]
    lba, uba = _full(lba, m, -np.inf), _full(uba, m, np.inf)
    lbx, ubx = _full(lbx, n, -np.inf), _full(ubx, n, np.inf)
    xl = np.asarray(x, dtype=np.float64).astype(LD)
    Hs = 0.5 * (H.astype(LD) + H.astype(LD).T)
    grad = Hs @ xl + np.asarray(g, dtype=np.float64).astype(LD)
    ax = A.astype(LD) @ xl if m else np.zeros(0, dtype=LD)
    pviol = LD(0.0)
    cols, ids = [], []
    for kind, i, sgn, b, v in one_sided(A, lba, uba, lbx, ubx, ax, xl):
        slack = sgn * (v - LD(b))                     # >= 0 when the side holds
        scale = LD(1.0) + abs(LD(b))
        pviol = max(pviol, -slack / scale)
        if abs(slack) <= ACTIVE_TOL * scale:
            if kind == 0:
                nrm = sgn * A[i]
            else:
                nrm = np.zeros(n); nrm[i] = sgn
            cols.append(nrm); ids.append((kind, i, sgn))
    den = max(LD(1.0), np.abs(np.asarray(g, dtype=np.float64)).max(initial=0.0), np.abs(grad).max(initial=0.0))
    lam = np.zeros(len(cols))
    res = grad
    if cols:
        N = np.stack(cols, axis=1)                    # n x k
        cn = np.linalg.norm(N, axis=0)
        cn[cn == 0.0] = 1.0
        gscale = float(np.abs(grad).max())
        if gscale > 0.0:
            y, _ = nnls(N / cn, np.asarray(grad / gscale, dtype=np.float64), maxiter=30 * max(N.shape))
            lam = y * gscale / cn
        res = grad - N.astype(LD) @ lam.astype(LD)
    stat = np.sqrt((res * res).sum()) / den
    return dict(pviol=float(pviol), stat=float(stat), active=ids, lam=lam, grad=grad)


def refined_solution(H, g, A, lba, uba, lbx, ubx, x):
    """x* of a problem whose Hessian is positive definite on the null space of the active normals: the active set
    with lam > 0 of certificate(x), the equality-constrained KKT system solved by a float64 LU and refined with
    long-double residuals until the correction stalls."""
    H = np.asarray(H, dtype=np.float64); n = H.shape[0]
    A = np.asarray(A, dtype=np.float64).reshape(-1, n)
    c = certificate(H, g, A, lba, uba, lbx, ubx, x)
    rows, rhs = [], []
    m = A.shape[0]
    lo = (_full(lba, m, -np.inf), _full(lbx, n, -np.inf)); hi = (_full(uba, m, np.inf), _full(ubx, n, np.inf))
    for (kind, i, sgn), lam in zip(c["active"], c["lam"]):
        if lam <= 0.0:
            continue
        if kind == 0:
            rows.append(A[i])
        else:
            e = np.zeros(n); e[i] = 1.0
            rows.append(e)
        rhs.append(lo[kind][i] if sgn > 0 else hi[kind][i])
    k = len(rows)
    Hs = 0.5 * (H + H.T)
    K = np.zeros((n + k, n + k))
    K[:n, :n] = Hs
    if k:
        Nm = np.stack(rows)
        K[n:, :n] = Nm; K[:n, n:] = Nm.T
    b = np.concatenate([-np.asarray(g, dtype=np.float64), np.asarray(rhs, dtype=np.float64)]).astype(LD)
    Kl = K.astype(LD)
    lu = scipy.linalg.lu_factor(K)
    z = np.zeros(n + k, dtype=LD)
    last = np.inf
    for _ in range(40):
        r = b - Kl @ z
        dz = scipy.linalg.lu_solve(lu, np.asarray(r, dtype=np.float64))
        step = float(np.abs(dz).max(initial=0.0))
        if not step < 0.5 * last:                     # the correction no longer shrinks
            break
        z = z + dz.astype(LD)
        last = step
    return np.asarray(z[:n], dtype=np.float64), z[:n]


# ------------------------------------------------------------------------------------------------ problem families
def spd(n, m, seed=0, absent=True):
    rng = np.random.default_rng([n, m, seed])
    M = rng.standard_normal((n, n))
    H = M @ M.T / n + 0.1 * np.eye(n)
    g = rng.standard_normal(n)
    A = rng.standard_normal((m, n))
    lba = -rng.uniform(0.1, 1.0, m); uba = rng.uniform(0.1, 1.0, m)
    if absent:
        lba[::3] = -np.inf; uba[1::3] = np.inf
    xe = rng.uniform(-0.03, 0.03, n)
    if m >= 6:
        for k in range(min(m // 6, n // 3)):          # two-sided rows 2, 5, 8, ... become equalities
            i = 2 + 3 * k
            lba[i] = uba[i] = A[i] @ xe
    lbx = -rng.uniform(0.05, 0.5, n); ubx = rng.uniform(0.05, 0.5, n)
    return H, g, A, lba, uba, lbx, ubx


def soft(n1, ns, mh, slack_as_row, w, seed=0):
    """The MPC shape: n1 curved variables, ns curvature-free slacks of cost w, ns soft rows a'x1 - s_i <= b_i whose
    x1 part ends after (i % n1) + 1 columns, mh dense two-sided hard rows, s >= 0 as lbx or as rows 2 s_i >= 0."""
    rng = np.random.default_rng([n1, ns, mh, seed])
    n = n1 + ns
    M = rng.standard_normal((n1, n1))
    H = np.zeros((n, n)); H[:n1, :n1] = M @ M.T / n1 + 0.05 * np.eye(n1)
    g = np.concatenate([rng.standard_normal(n1), np.full(ns, float(w))])
    m = ns + mh + (ns if slack_as_row else 0)
    A = np.zeros((m, n)); lba = np.full(m, -np.inf); uba = np.full(m, np.inf)
    for i in range(ns):
        k = (i % n1) + 1
        A[i, :k] = rng.standard_normal(k)
        A[i, n1 + i] = -1.0
    uba[:ns] = rng.uniform(-0.2, 0.3, ns)
    A[ns:ns + mh, :n1] = rng.standard_normal((mh, n1))
    lba[ns:ns + mh] = -rng.uniform(0.5, 2.0, mh); uba[ns:ns + mh] = rng.uniform(0.5, 2.0, mh)
    lbx = np.concatenate([-np.ones(n1), np.zeros(ns)]); ubx = np.concatenate([np.ones(n1), np.full(ns, np.inf)])
    if slack_as_row:
        lbx[n1:] = -np.inf
        for i in range(ns):
            A[ns + mh + i, n1 + i] = 2.0
        lba[ns + mh:] = 0.0
    return H, g, A, lba, uba, lbx, ubx


def indef(n, m, neg, seed=0):
    H, g, A, lba, uba, lbx, ubx = spd(n, m, seed, absent=False)
    lam, V = np.linalg.eigh(H)
    lam[:3] = -neg * lam[-1]
    H = (V * lam) @ V.T
    return 0.5 * (H + H.T), g, A, lba, uba, lbx, ubx


def psd_lp(n, m, rank, seed=0):
    """Rank-deficient PSD (rank > 0) or pure LP (rank 0) without the soft structure: the proximal rounds of the
    method run out on many of them (status 1), which is what the no-false-success test wants."""
    H, g, A, lba, uba, lbx, ubx = spd(n, m, seed)
    rng = np.random.default_rng([n, m, rank, seed, 7])
    M = rng.standard_normal((n, rank))
    return M @ M.T / max(n, 1), g, A, lba, uba, lbx, ubx


SPD_SHAPES = [(1, 0), (2, 1), (3, 5), (4, 4), (5, 3), (7, 8), (8, 7), (9, 16), (63, 40), (64, 64), (65, 130), (130, 513),
              (255, 300), (256, 257), (257, 100), (384, 2048)]
SOFT_SHAPES = [(4, 3, 2), (20, 43, 10), (20, 44, 10), (40, 88, 30), (60, 196, 40), (100, 157, 60), (128, 256, 100)]
INDEF_SHAPES = [(12, 9), (70, 40), (130, 90), (260, 100)]
INDEF_NEG = [1e-3, 0.05]
PSD_LP_SHAPES = [(64, 64, 20), (130, 513, 0), (255, 300, 100)]
NPROB = 3                                             # problems (seeds) per case = batch of one launch


def _cases():
    C = {}
    for n, m in SPD_SHAPES:
        C["spd-%dx%d" % (n, m)] = ("spd", spd, (n, m))
    for n1, ns, mh in SOFT_SHAPES:
        for as_row in (False, True):
            for w in (1.0, 1e4):
                C["soft-%d+%d-%d-%s-w%g" % (n1, ns, mh, "row" if as_row else "lbx", w)] = ("soft", soft, (n1, ns, mh, as_row, w))
    for n, m in INDEF_SHAPES:
        for neg in INDEF_NEG:
            C["indef-%dx%d-%g" % (n, m, neg)] = ("indef", indef, (n, m, neg))
    return C


CASES = _cases()                                      # case id -> (family, generator, arguments): one shape, one launch


def make_case(cid):
    """(family, [NPROB problems of that shape])"""
    fam, gen, args = CASES[cid]
    return fam, [gen(*args, seed=s) for s in range(NPROB)]


def solve_all(solve, problems, workers=8):
    """[solve(*p) for p in problems] on a few threads (a ctypes solver releases the GIL)."""
    with ThreadPoolExecutor(max_workers=workers) as ex:
        return list(ex.map(lambda p: solve(*p), problems))


# Largest distance ||x_oracle - x*||_inf / max(1, ||x*||_inf) between the CPU oracle and refined_solution over the case
# table (tests/test_qp_cert_cpu.py asserts it): the yardstick of the kernel's distance to x*.
D_REF = {"spd": 2.8e-17, "soft": 2.8e-17}
