"""The shared wave and working-set linear algebra and the shared steps of a dual pass (csrc/eepacc_wave.h, eepacc_units.h,
eepacc_schur.h, eepacc_dual_step.h) called directly
on the GPU through tests/kernels/linalg_harness.hip and compared with plain numpy / mpmath references.

The closed-loop tests cannot see an error in these functions: solve_qp falls back to a full schur_invert when an updated
P misses its rows, rebuilds after six updates, and refines whatever P produced.  Here every primitive stands alone.

Exact checks use integer-valued inputs (every sum is exact) and compare bit for bit.

Floating-point checks of the inversions and updates follow one rule, per case:
    err_gpu = max |P_gpu - P_ref|,  err_cpu = the same for a float64 numpy restatement of the same sweep order,
    err_gpu <= max(8 err_cpu, 64 eps max |P_ref|).
P_ref is the mpmath inverse (34 digits).  The factor 8 covers FMA contraction and the different summation order across
lanes.  The products are held to the standard dot-product bound n eps (|A| |y|), which needs no measurement.

Matrix families: "spd" random symmetric positive definite, condition 1e2..1e3; "solver" S = diag(s) (C He C' / n + D)
diag(s) with the row scales s spread so that the diagonal of S spans 1e-2..1e7 like the ORIG weights (condition 1e9..1e10).

Largest err_gpu / err_cpu seen on an MI355X per primitive (the bound allows 8):
    he_invert_full 2.6, schur_invert 1.4, schur_remove 2.2, update chain 1.8, schur_insert 6.9 (at m = 2, where both errors
    are below one ulp of max |P_ref|, a hundredth of the floor; 1.0 wherever the error is above the floor).
    No err_gpu exceeded 1.2 times the floor 64 eps max |P_ref|.  test_print_ratios prints the figures of a run.

Working sets above 64 rows: the primitives handle one row per lane.  Measured before the contract was narrowed, with
the scratch column filled with NaN: schur_invert at m = 65 and m = 66 (MMAX = 66, a matrix of condition 316 that inverts
to 1.3e-15 at m = 64) read the NaN of rows 64 and 65, which are never loaded into the scratch column, left 129 and 260
NaN entries in P and stopped with status 65; without the NaN it would have used whatever the scratch held.
eepacc_schur.h now states m <= 64 and both solvers refuse a larger working set through schur_capacity<MMAX>()
(test_capacity_above_64_rows_is_refused); 65 and 66 are therefore not in the sweeps below.
"""
import functools

import mpmath
import numpy as np
import pytest

import linalg_harness as lh

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
mpmath.mp.dps = 34
LD = np.longdouble


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return lh.load(str(tmp_path_factory.mktemp("linalg_harness")))


# ---------------------------------------------------------------------------------------------- references
def tril_pack(A, mmax):
    """packed lower triangle (row-major) of A in a table of capacity mmax, the rest zero"""
    m = A.shape[0]
    out = np.zeros(mmax * (mmax + 1) // 2)
    out[:m * (m + 1) // 2] = A[np.tril_indices(m)]
    return out


def tril_unpack(P, m):
    A = np.zeros((m, m), dtype=P.dtype)
    A[np.tril_indices(m)] = P[:m * (m + 1) // 2]
    return A + np.tril(A, -1).T


def _spd(n, seed, lo, hi):
    rng = np.random.default_rng(seed)
    Q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    A = (Q * np.logspace(lo, hi, n)) @ Q.T
    return (A + A.T) / 2


@functools.lru_cache(maxsize=None)
def matrix(family, n):
    """float64 symmetric positive definite test matrix (the exact input of every implementation)"""
    if family == "spd":
        return _spd(n, 1000 + n, 0.0, 2.5)
    rng = np.random.default_rng(2000 + n)
    nv = n + 2
    He = _spd(nv, 3000 + n, 0.0, 1.0)
    C = rng.standard_normal((n, nv))
    S0 = C @ He @ C.T / nv + np.diag(rng.uniform(0.3, 1.0, n))
    s = rng.permutation(np.logspace(-1.0, 3.5, n)) if n > 1 else np.array([1e3])
    S = S0 * np.outer(s, s)
    return (S + S.T) / 2


def to_obj(A):
    return np.array([[mpmath.mpf(float(x)) for x in row] for row in A], dtype=object)


def to_ld(A):
    """mpf array -> longdouble (hi + lo of two doubles: exact to the longdouble precision)"""
    hi = np.array([[float(x) for x in row] for row in A])
    lo = np.array([[float(x - mpmath.mpf(float(x))) for x in row] for row in A])
    return hi.astype(LD) + lo.astype(LD)


def mp_inverse(A):
    return np.array(mpmath.inverse(mpmath.matrix(A.tolist())).tolist(), dtype=object)


@functools.lru_cache(maxsize=None)
def ref_inverse(family, n):
    """mpmath inverse of matrix(family, n), as an array of mpf"""
    return mp_inverse(matrix(family, n))


def ref_without(family, n, p):
    """mpmath inverse of matrix(family, n) with row and column p deleted: the exact downdate of the full inverse at 34
    digits (test_reference_downdate_is_an_inverse checks it against a direct inverse)"""
    P = ref_inverse(family, n)
    o = [i for i in range(n) if i != p]
    return P[np.ix_(o, o)] - np.outer(P[o, p], P[o, p]) / P[p, p]


def sweep_invert_np(S):
    """float64 restatement of schur_invert: symmetric sweeps over the lower triangle in the kernel's order, then the sign
    flip.  Returns the inverse, or 1 + k for a pivot that is not positive relative to its original diagonal."""
    A = S.copy()
    m = A.shape[0]
    sv = np.abs(np.diag(A)).copy()
    for k in range(m):
        d = A[k, k]
        if not d > 1e-12 * sv[k]:
            return 1 + k
        inv = 1.0 / d
        c = A[:, k].copy()
        cl = c * inv
        B = A - np.outer(c, cl)          # entry (r, cc): P - colk[r] * (colk[cc] * inv)
        B[:, k] = cl
        B[k, :] = cl
        B[k, k] = -inv
        A = np.tril(B) + np.tril(B, -1).T
    return -A


def sweep_full_np(Hm):
    """float64 restatement of he_invert_full: -H^-1, or None on a non-positive pivot"""
    A = Hm.copy()
    for k in range(A.shape[0]):
        d = A[k, k]
        if not d > 0.0:
            return None
        inv = 1.0 / d
        c = A[k, :].copy()
        f = c * inv
        B = A - np.outer(c, f)           # entry (i, j): old - colk[i] * (colk[j] * inv)
        B[:, k] = c * inv
        B[k, :] = f
        B[k, k] = -inv
        A = B
    return A


def insert_np(Pold, rv, p, iz):
    """float64 restatement of schur_insert"""
    m = Pold.shape[0] + 1
    o = [i for i in range(m) if i != p]
    Pn = np.zeros((m, m))
    Pn[np.ix_(o, o)] = Pold + np.outer(rv, rv) * iz
    Pn[o, p] = Pn[p, o] = -rv * iz
    Pn[p, p] = iz
    return Pn


def remove_np(Pm, p):
    """float64 restatement of schur_remove"""
    m = Pm.shape[0]
    o = [i for i in range(m) if i != p]
    c = Pm[:, p]
    ip = 1.0 / c[p]
    return Pm[np.ix_(o, o)] - np.outer(c[o], c[o]) * ip


RATIOS = {}


def check_against_reference(primitive, case, P_gpu, P_cpu, P_ref):
    """the tolerance rule of the module docstring; prints every figure before it asserts"""
    ref = to_ld(P_ref)
    err_gpu = float(np.abs(P_gpu.astype(LD) - ref).max())
    err_cpu = float(np.abs(P_cpu.astype(LD) - ref).max())
    floor = 64 * EPS * float(np.abs(ref).max())
    ratio = err_gpu / err_cpu if err_cpu > 0 else (0.0 if err_gpu == 0 else np.inf)
    RATIOS[primitive] = max(RATIOS.get(primitive, 0.0), ratio)
    print("%-14s %-28s err_gpu %.3e err_cpu %.3e ratio %.3g floor %.3e max|ref| %.3e"
          % (primitive, case, err_gpu, err_cpu, ratio, floor, float(np.abs(ref).max())))
    assert np.isfinite(P_gpu).all(), (primitive, case)
    assert err_gpu <= max(8 * err_cpu, floor), (primitive, case, err_gpu, err_cpu, floor)


FAMILIES = ("spd", "solver")
SCHUR_SIZES = (1, 2, 10, 11, 12, 32, 34, 63, 64)       # 11: the first triangle that spans two 64-entry chunks
MMAXES = (32, 34, 66)


def positions(m):
    return sorted({0, m // 2, m - 1})


def test_reference_downdate_is_an_inverse():
    for fam in FAMILIES:
        for p in positions(12):
            o = [i for i in range(12) if i != p]
            direct = mp_inverse(matrix(fam, 12)[np.ix_(o, o)])
            d = np.abs(ref_without(fam, 12, p) - direct).max() / np.abs(direct).max()
            assert d < mpmath.mpf(10) ** -20, (fam, p, d)


# ---------------------------------------------------------------------------------------------- eepacc_wave.h, exact
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def scan_inputs():
    lanes = np.arange(64)
    rng = np.random.default_rng(7)
    X = [lanes + 1.0, 64.0 - lanes, rng.integers(-2 ** 20, 2 ** 20, 64).astype(float),
         np.where(lanes < 32, 2.0 ** lanes, 0.0), np.where(lanes >= 32, 2.0 ** (lanes - 32), 0.0), 2.0 ** (lanes // 2)]
    X += [np.eye(64)[l] for l in range(64)]              # one lane set: a wrong row mask or bcast step shows at its lane
    return np.array(X)


def test_scans_and_sums_exact(H):
    X = scan_inputs()
    inc = np.cumsum(X, axis=1)
    exc = inc - X
    for wpb in (2, 3):
        np.testing.assert_array_equal(H.wave("scan_incl", X, wpb=wpb)[0], inc)
        np.testing.assert_array_equal(H.wave("scan_excl", X, wpb=wpb)[0], exc)
        np.testing.assert_array_equal(H.wave("wave_sum", X, wpb=wpb)[0], np.repeat(inc[:, 63:], 64, 1))
    for l in (15, 16, 31, 32, 47, 48, 63):               # the lanes where a 16-lane row or a 32-lane half ends / begins
        got = H.wave("scan_incl", np.eye(64)[l])[0][0]
        np.testing.assert_array_equal(got, (np.arange(64) >= l).astype(float), err_msg="lane %d" % l)
    prev = np.concatenate([np.zeros((len(X), 1)), X[:, :-1]], axis=1)
    nxt = np.concatenate([X[:, 1:], np.zeros((len(X), 1))], axis=1)
    np.testing.assert_array_equal(H.wave("lane_prev", X)[0], prev)
    np.testing.assert_array_equal(H.wave("lane_next", X)[0], nxt)


def test_scan_prod_excl_exact(H):
    lanes = np.arange(64)
    rng = np.random.default_rng(8)
    X = [np.full(64, 2.0), 2.0 ** ((lanes % 3) - 1.0), 2.0 ** rng.integers(-4, 5, 64).astype(float), np.full(64, 0.5)]
    X += [np.where(lanes == l, 2.0, 1.0) for l in range(64)]
    X = np.array(X)
    inc = np.cumprod(X, axis=1)                          # powers of two: exact
    exc = np.concatenate([np.ones((len(X), 1)), inc[:, :-1]], axis=1)
    for wpb in (2, 3):
        np.testing.assert_array_equal(H.wave("scan_prod_excl", X, wpb=wpb)[0], exc)


def test_argmax_and_broadcasts_exact(H):
    lanes = np.arange(64)
    rng = np.random.default_rng(9)
    base = rng.permutation(64).astype(float)             # distinct values 0..63
    X, want = [], []
    for l in (0, 15, 16, 31, 32, 63):                    # a unique maximum
        x = base.copy(); x[l] = 100.0
        X.append(x); want.append((100.0, l))
    for tie in ((15, 16), (31, 32), (0, 63), (16, 48), (47, 48, 63)):      # ties: the lowest lane wins
        x = base.copy(); x[list(tie)] = 100.0
        X.append(x); want.append((100.0, tie[0]))
    X.append(np.full(64, 3.0)); want.append((3.0, 0))                      # all lanes equal
    X.append(-(lanes + 1.0)); want.append((-1.0, 0))                       # all lanes negative
    x = -(base + 1.0) * 4.0; x[40] = -0.5
    X.append(x); want.append((-0.5, 40))
    X = np.array(X)
    payload = np.tile(1000 + 7 * lanes, (len(X), 1))
    for wpb in (2, 3):
        v, p = H.wave("wave_argmax", X, payload, wpb=wpb)
        np.testing.assert_array_equal(v, np.repeat(np.array([w[0] for w in want])[:, None], 64, 1))
        np.testing.assert_array_equal(p, np.repeat(np.array([1000 + 7 * w[1] for w in want])[:, None], 64, 1))
        np.testing.assert_array_equal(H.wave("wave_max", X, wpb=wpb)[0], v)
        v, p = H.wave("wave_argmin", -X, payload, wpb=wpb)
        np.testing.assert_array_equal(v, np.repeat(np.array([-w[0] for w in want])[:, None], 64, 1))
        np.testing.assert_array_equal(p, np.repeat(np.array([1000 + 7 * w[1] for w in want])[:, None], 64, 1))
    # broadcasts: arbitrary bit patterns in both halves of the double, negative integers
    Y = rng.standard_normal((3, 64)) * 10.0 ** rng.integers(-30, 30, (3, 64))
    pi = rng.integers(-2 ** 31, 2 ** 31, (3, 64)).astype(np.int32)
    src = np.array([0, 63, 17])
    v, _ = H.wave("bcast", Y, pi, src)
    np.testing.assert_array_equal(bits(v), bits(np.repeat(Y[np.arange(3), src][:, None], 64, 1)))
    _, p = H.wave("bcast_i", Y, pi, src)
    np.testing.assert_array_equal(p, np.repeat(pi[np.arange(3), src][:, None], 64, 1))


# ---------------------------------------------------------------------------------------------- eepacc_units.h, exact
def test_index_tables_exact(H):
    i, j = np.meshgrid(np.arange(66), np.arange(66), indexing="ij")
    a, b = np.maximum(i, j), np.minimum(i, j)
    np.testing.assert_array_equal(H.pidx(66), a * (a + 1) // 2 + b)
    for mmax in MMAXES:
        r, c = np.tril_indices(mmax)
        want = ((r << 8) | c).astype(np.uint16)
        for wpb in (2, 3):
            tab = H.rc_table(mmax, nblocks=2, wpb=wpb)
            for w in range(tab.shape[0]):                # every wave of every block sees the whole table
                np.testing.assert_array_equal(tab[w], want, err_msg="MMAX %d wave %d" % (mmax, w))


def test_shift_codes_exact(H):
    rng = np.random.default_rng(10)
    Ns = np.array([1, 2, 32, 63, 64])
    code = rng.integers(0, 2 ** 63, (len(Ns), 64), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (len(Ns), 64), dtype=np.uint64)
    want = code.copy()
    for q, N in enumerate(Ns):
        want[q, :N - 1] = code[q, 1:N]
    for wpb in (2, 3):
        np.testing.assert_array_equal(H.shift_codes(code, Ns, wpb=wpb), want)


# ---------------------------------------------------------------------------------------------- He
HE_LAYOUTS = ((32, False), (32, True), (64, False), (64, True))


def he_sizes(ns):
    return (1, 2, ns - 1, ns) + ((33,) if ns == 64 else ())


def he_table(A, ns, packed):
    """the ns x ns zero-padded table of the symmetric A, full or packed lower triangle"""
    T = np.zeros((ns, ns))
    T[:A.shape[0], :A.shape[0]] = A
    return T[np.tril_indices(ns)] if packed else T.ravel()


def int_sym(rng, n, lim=8):
    A = rng.integers(-lim, lim + 1, (n, n)).astype(float)
    return np.tril(A) + np.tril(A, -1).T


@pytest.mark.parametrize("ns,packed", HE_LAYOUTS)
def test_he_products_exact(H, ns, packed):
    rng = np.random.default_rng(11 + ns + packed)
    Ns = he_sizes(ns)
    tabs, y0, y1, want0, want1 = [], [], [], [], []
    for N in Ns:
        A = int_sym(rng, N)
        a, b = rng.integers(-8, 9, ns).astype(float), rng.integers(-8, 9, ns).astype(float)   # non-zero beyond N: the padding is zero
        tabs.append(he_table(A, ns, packed)); y0.append(a); y1.append(b)
        want0.append(np.concatenate([A @ a[:N], np.zeros(64 - N)])); want1.append(np.concatenate([A @ b[:N], np.zeros(64 - N)]))
    # a table whose padding is not zero, vectors that are: lanes >= N must still return exactly 0
    for N in (2, ns - 1):
        A = int_sym(rng, ns)
        a, b = np.zeros(ns), np.zeros(ns)
        a[:N], b[:N] = rng.integers(-8, 9, N), rng.integers(-8, 9, N)
        tabs.append(he_table(A, ns, packed)); y0.append(a); y1.append(b)
        want0.append(np.concatenate([(A @ a)[:N], np.zeros(64 - N)])); want1.append(np.concatenate([(A @ b)[:N], np.zeros(64 - N)]))
    Nq = list(Ns) + [2, ns - 1]
    for wpb in (2, 3):
        o0, _, _ = H.he(lh.HE_MUL, ns, packed, tabs, y0, None, Nq, wpb=wpb)
        np.testing.assert_array_equal(o0, np.array(want0))
        o0, o1, _ = H.he(lh.HE_MUL2, ns, packed, tabs, y0, y1, Nq, wpb=wpb)
        np.testing.assert_array_equal(o0, np.array(want0))
        np.testing.assert_array_equal(o1, np.array(want1))


@pytest.mark.parametrize("ns", (32, 64))
def test_he_products_float(H, ns):
    """random reals against the longdouble product, bound NS eps (|He| |y|) per component; the packed and the full layout
    agree bit for bit on the same symmetric matrix"""
    rng = np.random.default_rng(12 + ns)
    Ns = he_sizes(ns)
    out = {}
    A, a, b = [], [], []
    for N in Ns:
        M = np.zeros((ns, ns)); M[:N, :N] = _spd(N, 50 + N, -1.0, 2.0) * rng.choice([-1.0, 1.0], (N, N))
        M = np.tril(M) + np.tril(M, -1).T
        A.append(M); y = np.zeros((2, ns)); y[:, :N] = rng.standard_normal((2, N)) * 10.0 ** rng.integers(-3, 4, (2, N))
        a.append(y[0]); b.append(y[1])
    for packed in (False, True):
        tabs = [he_table(M, ns, packed) for M in A]
        o0, _, _ = H.he(lh.HE_MUL, ns, packed, tabs, a, None, Ns)
        p0, p1, _ = H.he(lh.HE_MUL2, ns, packed, tabs, a, b, Ns)
        out[packed] = (o0, p0, p1)
        for q, N in enumerate(Ns):
            Ml = A[q].astype(LD)
            for name, got, y in (("he_mul", o0[q], a[q]), ("he_mul2.0", p0[q], a[q]), ("he_mul2.1", p1[q], b[q])):
                ref = Ml @ y.astype(LD)
                bound = ns * EPS * (np.abs(A[q]) @ np.abs(y))
                err = np.abs(got[:ns].astype(LD) - ref).astype(float)
                print("%-10s NS %d packed %d N %2d  max err / bound %.3g" % (name, ns, packed, N, (err[:N] / bound[:N]).max()))
                assert (err[:N] <= bound[:N]).all(), (name, ns, packed, N)
                assert (got[N:] == 0.0).all(), (name, ns, packed, N)
    for x, y in zip(out[False], out[True]):
        np.testing.assert_array_equal(bits(x), bits(y))


@pytest.mark.parametrize("ns,packed", HE_LAYOUTS)
def test_he_sub_outer_exact(H, ns, packed):
    rng = np.random.default_rng(13 + ns + packed)
    tabs, yv, yj, want, Ns = [], [], [], [], []
    for N in he_sizes(ns) + (ns,):
        full_vec = len(Ns) == len(he_sizes(ns))           # last case: the vector is non-zero over all NS entries
        A = np.zeros((ns, ns)); A[:N, :N] = int_sym(rng, N)
        if full_vec:
            A = int_sym(rng, ns)
        v = np.zeros(ns); v[:N] = rng.integers(-8, 9, N)
        if full_vec:
            v = rng.integers(1, 9, ns).astype(float)
        kappa = float(rng.integers(1, 5))
        tabs.append(he_table(A, ns, packed)); yv.append(v); yj.append(kappa * v); Ns.append(N)
        want.append(A - np.outer(v, kappa * v))
    if not packed:                                        # the full table is a plain outer-product update, symmetric or not
        A = int_sym(rng, ns); v = rng.integers(-8, 9, ns).astype(float); w = rng.integers(-8, 9, ns).astype(float)
        tabs.append(A.ravel()); yv.append(v); yj.append(w); Ns.append(ns); want.append(A - np.outer(v, w))
    for wpb in (2, 3):
        _, _, Ho = H.he(lh.HE_SUB_OUTER, ns, packed, tabs, yv, yj, Ns, wpb=wpb)
        for q, W in enumerate(want):
            got = tril_unpack(Ho[q], ns) if packed else Ho[q].reshape(ns, ns)
            np.testing.assert_array_equal(got, W, err_msg="case %d" % q)      # padding included: zero stays zero
            if np.array_equal(W, W.T):
                np.testing.assert_array_equal(got, got.T)


def he_invert_cases(ns):
    return [(fam, N) for fam in FAMILIES for N in ((1, 2, 31, 32) if ns == 32 else (33, 63, 64))]


@pytest.mark.parametrize("ns", (32, 64))
def test_he_invert_full(H, ns):
    cases = he_invert_cases(ns)
    tabs = []
    for fam, N in cases:
        T = np.zeros((ns, ns)); T[:N, :N] = matrix(fam, N)
        tabs.append(T)
    out, ret = H.he_invert(ns, tabs, [N for _, N in cases], wpb=2)
    assert (ret == 0).all()
    for q, (fam, N) in enumerate(cases):
        pad = out[q].copy(); pad[:N, :N] = 0.0
        assert (pad == 0.0).all(), (fam, N)               # he_mul sums over all NS rows: the padding must stay exactly zero
        check_against_reference("he_invert_full", "NS %d %s N %d" % (ns, fam, N), -out[q][:N, :N],
                                -sweep_full_np(matrix(fam, N)), ref_inverse(fam, N))


@pytest.mark.parametrize("ns", (32, 64))
def test_he_invert_full_bad_pivots(H, ns):
    N = ns - 1
    A = matrix("spd", N)
    indef = A.copy(); indef[5, 5] = -indef[5, 5]
    late = A.copy(); late[N - 1, N - 1] = 1e-9            # not positive definite: only the last pivot turns negative
    nan = A.copy(); nan[3, 3] = np.nan
    tabs = []
    for M in (indef, late, np.zeros((N, N)), nan, A):
        T = np.zeros((ns, ns)); T[:N, :N] = M
        tabs.append(T)
    assert sweep_full_np(late) is None
    _, ret = H.he_invert(ns, tabs, [N] * 5, wpb=3)
    for q in range(4):
        assert (ret[q] != 0).all(), q                     # every lane reports it, and the call returned (no hang)
    assert (ret[4] == 0).all()


# ---------------------------------------------------------------------------------------------- P
def schur_problems(mmax):
    return [(fam, m) for fam in FAMILIES for m in SCHUR_SIZES if m <= lh_capacity(mmax)]


def lh_capacity(mmax):
    return min(mmax, 64)


@pytest.mark.parametrize("mmax", MMAXES)
def test_schur_invert(H, mmax):
    cases = schur_problems(mmax)
    P, ret, sv, _ = H.schur(lh.S_INVERT, mmax, [tril_pack(matrix(f, m), mmax) for f, m in cases], [m for _, m in cases])
    assert (ret == 0).all()
    for q, (fam, m) in enumerate(cases):
        np.testing.assert_array_equal(sv[q, :m], np.abs(np.diag(matrix(fam, m))))
        check_against_reference("schur_invert", "MMAX %d %s m %d" % (mmax, fam, m), tril_unpack(P[q], m),
                                sweep_invert_np(matrix(fam, m)), ref_inverse(fam, m))


def test_schur_invert_singular(H):
    """an exactly singular S (a duplicated row) and a relative pivot below 1e-12 return 1 + k for the right k"""
    cases = []
    for m, i, j in ((12, 3, 7), (40, 5, 39), (64, 0, 63)):
        S = matrix("spd", m).copy()
        S[j, :] = S[i, :]; S[:, j] = S[:, i]; S[j, j] = S[i, i]
        cases.append((S, 1 + j))
    for m, j, piv, want in ((12, 6, 1e-7, 7), (34, 33, 1e-7, 34), (12, 6, 1e-4, 0)):      # pivot piv^2 relative to a diagonal of about 1
        rng = np.random.default_rng(60 + m)
        L = np.eye(m) + 0.3 * np.tril(rng.standard_normal((m, m)), -1) / np.sqrt(m)
        L[j, j] = piv
        S = L @ L.T
        cases.append(((S + S.T) / 2, want))
    for S, want in cases:
        got = sweep_invert_np(S)
        assert (got == want) if want else not isinstance(got, int)         # the float64 restatement agrees on k
    _, ret, _, _ = H.schur(lh.S_INVERT, 66, [tril_pack(S, 66) for S, _ in cases], [S.shape[0] for S, _ in cases])
    for q, (_, want) in enumerate(cases):
        assert (ret[q] == want).all(), (q, ret[q][0], want)


def update_cases(mmax):
    return [(fam, m, p) for fam, m in schur_problems(mmax) if m >= 2 for p in positions(m)]


@pytest.mark.parametrize("mmax", MMAXES)
def test_schur_insert(H, mmax):
    """new size m: P of the old list (the reference inverse without row p), rv = P sv and the pivot as the solver computes
    them, against the reference inverse of the bordered S"""
    cases = update_cases(mmax)
    Ps, ms, ps, rvs, izs, cpu = [], [], [], [], [], []
    for fam, m, p in cases:
        S = matrix(fam, m)
        o = [i for i in range(m) if i != p]
        Pold = ref_without(fam, m, p).astype(float)
        sv = S[o, p]
        rv = Pold @ sv
        iz = 1.0 / (S[p, p] - sv @ rv)
        Ps.append(tril_pack(Pold, mmax)); ms.append(m); ps.append(p); izs.append(iz)
        rvs.append(np.concatenate([rv, np.zeros(mmax - m + 1)])); cpu.append(insert_np(Pold, rv, p, iz))
    P, _, _, _ = H.schur(lh.S_INSERT, mmax, Ps, ms, pos=ps, vec=rvs, piv=izs)
    for q, (fam, m, p) in enumerate(cases):
        check_against_reference("schur_insert", "MMAX %d %s m %d p %d" % (mmax, fam, m, p), tril_unpack(P[q], m), cpu[q],
                                ref_inverse(fam, m))


@pytest.mark.parametrize("mmax", MMAXES)
def test_schur_remove(H, mmax):
    """old size m: the row at p leaves, against the reference inverse of S without that row and column"""
    cases = update_cases(mmax)
    Ps, cpu = [], []
    for fam, m, p in cases:
        Pm = ref_inverse(fam, m).astype(float)
        Ps.append(tril_pack(Pm, mmax)); cpu.append(remove_np(Pm, p))
    P, _, _, m_out = H.schur(lh.S_REMOVE, mmax, Ps, [m for _, m, _ in cases], pos=[p for _, _, p in cases])
    for q, (fam, m, p) in enumerate(cases):
        assert m_out[q] == m - 1
        check_against_reference("schur_remove", "MMAX %d %s m_old %d p %d" % (mmax, fam, m, p), tril_unpack(P[q], m - 1),
                                cpu[q], ref_without(fam, m, p))


@pytest.mark.parametrize("mmax,m0", ((34, 20), (66, 60)))
def test_update_chain(H, mmax, m0):
    """what solve_qp relies on: schur_invert, then six mixed inserts and removes (the longest run it allows) at random
    positions, against the fresh inverse of the final S"""
    kinds = (1, 1, 2, 1, 2, 1)
    Ps, pos, vec, piv, cpu, final = [], [], [], [], [], []
    for fam in FAMILIES:
        rng = np.random.default_rng(70 + m0)
        pool = matrix(fam, m0 + 4)
        order = list(rng.permutation(m0 + 4))
        lst, spare = order[:m0], order[m0:]
        Pc = sweep_invert_np(pool[np.ix_(lst, lst)])
        Ps.append(tril_pack(pool[np.ix_(lst, lst)], mmax))
        pq, vq, zq = [], [], []
        for k in kinds:
            if k == 1:
                g, p = spare.pop(), int(rng.integers(0, len(lst) + 1))
                sv = pool[lst, g]
                rv = Pc @ sv
                Pc = insert_np(Pc, rv, p, 1.0 / (pool[g, g] - sv @ rv))
                vq.append(np.concatenate([sv, np.zeros(mmax - len(lst))])); zq.append(pool[g, g])
                lst.insert(p, g)
            else:
                p = int(rng.integers(0, len(lst)))
                Pc = remove_np(Pc, p)
                vq.append(np.zeros(mmax)); zq.append(0.0)
                lst.pop(p)
            pq.append(p)
        pos.append(pq); vec.append(vq); piv.append(zq); cpu.append(Pc); final.append(list(lst))
    P, ret, _, m_out = H.schur(lh.S_CHAIN, mmax, Ps, [m0] * len(FAMILIES), kind=[kinds] * len(FAMILIES), pos=pos, vec=vec,
                               piv=piv, wpb=2)
    assert (ret == 0).all()
    for q, fam in enumerate(FAMILIES):
        m = len(final[q])
        assert m_out[q] == m == m0 + 2
        ref = mp_inverse(matrix(fam, m0 + 4)[np.ix_(final[q], final[q])])
        check_against_reference("update_chain", "MMAX %d %s m0 %d" % (mmax, fam, m0), tril_unpack(P[q], m), cpu[q], ref)


@pytest.mark.parametrize("mmax,ns,m", ((32, 32, 1), (34, 32, 34), (66, 64, 64)))
def test_solve_multipliers(H, mmax, ns, m):
    """lam = -P (d + C h) against mpmath.  Bound per row i, from the rounding of the m-term fma chain and of the four-term
    row value sv_j = d_j + sum of terms (T_j = sum of their magnitudes):  eps sum_j |P_ij| ((m + 1) |sv_j| + 6 T_j)."""
    N = ns
    mp = mpmath.mpf
    P_all, img_all, rows_all, wk_all, want, bound = [], [], [], [], [], []
    for fam in FAMILIES:
        rng = np.random.default_rng(80 + m)
        Pm = ref_inverse(fam, m).astype(float)
        img = rng.standard_normal((3, ns + 1)) * 10.0 ** rng.integers(-2, 3, (3, ns + 1))
        rows = np.zeros((5, mmax)); rows[:, :m] = rng.standard_normal((5, m)) * 10.0 ** rng.integers(-2, 3, (5, m))
        wk = np.zeros(mmax, dtype=np.int32); wk[:m] = rng.integers(0, N + 1, m)
        wk[0] = 0; wk[m - 1] = N                          # the first stage has no previous input, the terminal stage no own input
        sv, T = [], []
        for i in range(m):
            k = int(wk[i])
            terms = [mp(rows[0, i]) * mp(img[1, k]), mp(rows[1, i]) * mp(img[2, k])]
            if k < N:
                terms.append(mp(rows[2, i]) * mp(img[0, k]))
            if k > 0:
                terms.append(mp(rows[3, i]) * mp(img[0, k - 1]))
            sv.append(mp(rows[4, i]) + sum(terms)); T.append(abs(mp(rows[4, i])) + sum(abs(t) for t in terms))
        Po = to_obj(Pm)
        want.append(np.array([-sum(Po[i, j] * sv[j] for j in range(m)) for i in range(m)], dtype=object))
        w = np.array([float((m + 1) * abs(sv[j]) + 6 * T[j]) for j in range(m)])
        bound.append(EPS * (np.abs(Pm) @ w))
        P_all.append(tril_pack(Pm, mmax)); img_all.append(img); rows_all.append(rows); wk_all.append(wk)
    lam, sv_gpu = H.multipliers(mmax, ns, P_all, img_all, rows_all, wk_all, [m] * 2, [N] * 2)
    for q, fam in enumerate(FAMILIES):
        err = np.array([float(abs(mp(float(lam[q, i])) - want[q][i])) for i in range(m)])
        print("solve_multipliers MMAX %d %s m %d  max err / bound %.3g" % (mmax, fam, m, (err / bound[q]).max()))
        assert np.isfinite(lam[q, :m]).all()
        assert (err <= bound[q]).all(), (fam, m)
        assert np.isnan(lam[q, m:]).all() and np.isnan(sv_gpu[q, m:]).all()      # nothing written past the working set


def test_capacity_above_64_rows_is_refused(H):
    """m = 65 and 66 fit the tables of the long-horizon kernels (MMAX = 66) but not the one-row-per-lane linear algebra:
    rebuild_and_factor refuses m > schur_capacity<MMAX>() (tests/test_linalg_harness_cpu.py checks that both solvers use
    it as their guard), and the harness refuses to run the primitives there."""
    assert H.schur_capacity(32) == 32 and H.schur_capacity(34) == 34 and H.schur_capacity(66) == 64
    for m in (65, 66):
        assert m > H.schur_capacity(66)
        with pytest.raises(lh.HarnessError):
            H.schur(lh.S_INVERT, 66, [tril_pack(matrix("spd", 64), 66)], [m])


# ---------------------------------------------------------------------------------------------- eepacc_dual_step.h
# Not covered: the candidate bookkeeping of the ratio test (EEPACC_CAND, t1n / t1d, the final division and wave_argmin).  It
# stays written out, twice, in the two solve_qp (shared, it changed the register spills of every solver kernel:
# profiles/dual_step_codegen.txt), so there is no routine to call and only the event-code format is tested here.
# step_rates is called under `if (m > 0)`, as the solvers call it.
# One problem per wave, 1..4 waves per block; the float64 restatements (linalg_harness.py, checked against dense algebra in
# test_linalg_harness_cpu.py) are written in the kernel's order.  Integer-valued data make every sum exact in any order.
WPBS = (1, 2, 3, 4)


def same_bits(got, want, msg):
    np.testing.assert_array_equal(got, want, err_msg=msg)
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=msg)       # NaN poison and the sign of a zero too


@pytest.mark.parametrize("mmax,ns", lh.DUAL_SIZES)
def test_scatter_rows_exact(H, mmax, ns):
    M, cases = lh.scatter_rows_cases(H.dual_mem, mmax, ns)
    want = [lh.scatter_rows_np(r, m, N, r["rv" if x else "lam"], sign) for r, (N, m, x, sign, _) in zip(M, cases)]
    for wpb in WPBS:
        out, _, _ = H.dual(lh.D_SCATTER_ROWS, mmax, ns, M, [c[1] for c in cases], [c[0] for c in cases],
                           x=[c[2] for c in cases], scale=[c[3] for c in cases], wpb=wpb)
        for q, c in enumerate(cases):
            for name, w in zip(("ws", "wv", "wa"), want[q]):
                same_bits(out[name][q], w, "%s case %s wpb %d" % (name, c, wpb))
            if c[1] == 0:
                for name in ("ws", "wv", "wa"):
                    same_bits(out[name][q], M[name][q], "untouched %s" % name)


@pytest.mark.parametrize("mmax,ns", lh.DUAL_SIZES)
def test_scatter_row_exact(H, mmax, ns):
    M, cases = lh.scatter_row_cases(H.dual_mem, mmax, ns)
    want = [lh.scatter_row_np(r, kq, N, scale, *row[:4]) for r, (N, kq, scale, row) in zip(M, cases)]
    for wpb in WPBS:
        out, _, _ = H.dual(lh.D_SCATTER_ROW, mmax, ns, M, 0, [c[0] for c in cases], kq=[c[1] for c in cases],
                           scale=[c[2] for c in cases], row=[c[3] for c in cases], wpb=wpb)
        for q, c in enumerate(cases):
            for name, w in zip(("ws", "wv", "wa"), want[q]):
                same_bits(out[name][q], w, "%s case %s wpb %d" % (name, c, wpb))


@pytest.mark.parametrize("mmax,ns", lh.DUAL_SIZES)
def test_row_value_exact(H, mmax, ns):
    M, cases = lh.row_value_cases(H.dual_mem, mmax, ns)
    want = np.array([lh.row_value_np(row, kq, N, r["av"], r["shv"], r["vhv"]) for r, (N, kq, row) in zip(M, cases)])
    for wpb in WPBS:
        _, got, _ = H.dual(lh.D_ROW_VALUE, mmax, ns, M, 0, [c[0] for c in cases], kq=[c[1] for c in cases],
                           row=[c[2] for c in cases], wpb=wpb)
        np.testing.assert_array_equal(got, np.repeat(want[:, None], 64, 1))


@pytest.mark.parametrize("mmax,ns", lh.DUAL_SIZES)
def test_step_rates_exact(H, mmax, ns):
    M, cases = lh.step_rates_int_cases(H.dual_mem, mmax, ns)
    want = [lh.step_rates_np(r, m, N) for r, (N, m) in zip(M, cases)]
    for wpb in WPBS:
        out, sr, _ = H.dual(lh.D_STEP_RATES, mmax, ns, M, [c[1] for c in cases], [c[0] for c in cases], wpb=wpb)
        for q, (N, m) in enumerate(cases):
            sv, rv, s = want[q]
            np.testing.assert_array_equal(sr[q], np.full(64, s), err_msg=str((N, m)))
            np.testing.assert_array_equal(out["sv"][q, :m], sv)
            np.testing.assert_array_equal(out["rv"][q, :m], rv)
            assert np.isnan(out["sv"][q, m:]).all() and np.isnan(out["rv"][q, m:]).all()      # m = 0: both stay poisoned
            if m == 0:
                assert (bits(sr[q]) == 0).all()


@pytest.mark.parametrize("mmax,ns,m", ((32, 32, 1), (34, 32, 34), (66, 64, 64)))
def test_step_rates_float(H, mmax, ns, m):
    """rv = P sv and sr = sv' rv on random data against mpmath, by the rule of the module docstring"""
    N = ns
    mp = mpmath.mpf
    M = H.dual_mem(mmax, ns, len(FAMILIES))
    for r, fam in zip(M, FAMILIES):
        rng = np.random.default_rng(90 + m)
        r["P"][:] = tril_pack(ref_inverse(fam, m).astype(float), mmax)
        r["ub"][:], r["sub"][:], r["vub"][:] = rng.standard_normal((3, ns + 1)) * 10.0 ** rng.integers(-2, 3, (3, ns + 1))
        for name in ("e_al", "e_be", "e_ga", "e_de"):
            r[name][:m] = rng.standard_normal(m) * 10.0 ** rng.integers(-2, 3, m)
        r["w_k"][:m] = rng.integers(0, N + 1, m)
        r["w_k"][0], r["w_k"][m - 1] = 0, N
    out, sr, _ = H.dual(lh.D_STEP_RATES, mmax, ns, M, m, N)
    for q, fam in enumerate(FAMILIES):
        r = M[q]
        sv = []
        for i in range(m):
            k = int(r["w_k"][i])
            x = mp(r["e_al"][i]) * mp(r["sub"][k]) + mp(r["e_be"][i]) * mp(r["vub"][k])
            x += mp(r["e_ga"][i]) * mp(r["ub"][k]) if k < N else 0
            x += mp(r["e_de"][i]) * mp(r["ub"][k - 1]) if k > 0 else 0
            sv.append(x)
        Po = to_obj(unpack_full(r["P"], m))
        rv = [sum(Po[i, j] * sv[j] for j in range(m)) for i in range(m)]
        s = sum(a * b for a, b in zip(sv, rv))
        sv_c, rv_c, s_c = lh.step_rates_np(r, m, N)
        check_against_reference("step_rates.rv", "MMAX %d %s m %d" % (mmax, fam, m), out["rv"][q, :m][None, :], rv_c[None, :],
                                np.array([rv], dtype=object))
        check_against_reference("step_rates.sr", "MMAX %d %s m %d" % (mmax, fam, m), sr[q][None, :1], np.array([[s_c]]),
                                np.array([[s]], dtype=object))
        assert (bits(sr[q]) == bits(sr[q])[0]).all()


def unpack_full(P, m):
    return tril_unpack(P, m)


@pytest.mark.parametrize("mmax,ns", lh.DUAL_SIZES)
def test_refine_rounds(H, mmax, ns):
    M, cases = lh.refine_cases(H.dual_mem, mmax, ns)
    for wpb in WPBS:
        out, rel0, calls = H.dual(lh.D_REFINE, mmax, ns, M, [c[1] for c in cases], [c[0] for c in cases],
                                  x=[c[3] for c in cases], scale=[c[4] for c in cases], wpb=wpb)
        for q, (N, m, kind, mr, tol) in enumerate(cases):
            msg = "MMAX %d case %s wpb %d" % (mmax, cases[q], wpb)
            r = M[q].copy()
            rel0_np, calls_np = lh.refine_rounds_np(r, m, N, mr, tol)
            assert (calls[q] == calls_np).all(), msg
            assert (bits(rel0[q]) == bits(rel0[q])[0]).all(), msg
            after = out[q].copy()
            res = lh.rows_dot_np(after, m, N, after["av"], after["shv"], after["vhv"]) - after["e_d"][:m]
            rel_after = float(np.max(np.abs(res) / (1.0 + np.abs(after["e_d"][:m]))))
            if kind == "exact":
                assert calls_np == 1 and (rel0[q] == 0.0).all(), msg
                same_bits(out["lam"][q], M["lam"][q], msg)                     # no correction
            elif kind == "one_round":
                assert calls_np == 2 and rel_after <= tol < rel0[q][0], msg
            elif kind == "no_rounds":
                assert calls_np == 1 and (rel0[q] == 0.0).all(), msg
                same_bits(out["lam"][q], M["lam"][q], msg)
            else:
                assert calls_np == 1 + mr and rel_after > tol, msg
            # rel0: a maximum of |four-term sums| / (1 + |d|); each sum rounds within 6 eps of its terms' magnitudes
            T = np.abs(M["e_d"][q][:m]) + 4 * 150.0 * 1.5 * 3.0
            assert abs(rel0[q][0] - rel0_np) <= 6 * EPS * float(np.max(T / (1.0 + np.abs(M["e_d"][q][:m])))), msg


def test_event_codes_and_tolerance_exact(H):
    packs, tols = lh.pack_cases(), lh.tolerance_cases()
    code, _ = H.step_scalars(packs, np.zeros(len(packs)))
    for (kind, lane, t), got in zip(packs, code):
        assert tuple(got) == (lh.pack_np(kind, lane, t), kind, lane, t)
    _, tol = H.step_scalars(tols, np.full(len(tols), 1e-11))
    want = np.array([lh.viol_tolerance_np(1e-11, it, N) for it, N, _ in tols])
    np.testing.assert_array_equal(bits(tol), bits(want))
    assert sorted(set(want)) == [1e-11, 1e-11 * 10.0, 1e-11 * 100.0, 1e-11 * 1000.0]


def test_print_ratios():
    print("largest err_gpu / err_cpu per primitive:", {k: "%.3g" % v for k, v in sorted(RATIOS.items())})
