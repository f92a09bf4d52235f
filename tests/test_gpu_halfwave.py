"""The functions that put lanes 32-63 of a wave to work at NS = 32 (csrc/eepacc_wave.h scan_excl_half, eepacc_schur.h
he_sub_outer_halves / he_mul_halves, eepacc_ab_cols.h ab_schur_columns4), called directly on the GPU through
tests/kernels/halfwave_harness.hip.

Bit-for-bit checks: scan_excl_half against numpy on integer-valued input, he_sub_outer_halves against he_sub_outer, the
four-column build of S against the two-column loop it replaces (kept in the harness), he_mul_halves on small integers.

Floating-point checks use the dot-product bound of test_gpu_linalg.test_he_products_float, NS eps (|He| |y|), against a
long-double reference; nothing in it is measured.

Convention of the S check: he_mul's product is out_k = sum_i He[i][k] y[i], so column j is u_j = He' c_j and
P[pidx(i, j)] = c_i' He' c_j.  The tables of the test are not symmetric, so an entry built from the wrong pair of rows,
the wrong half of the wave or with rows and columns exchanged differs from the reference by much more than the bound."""
import numpy as np
import pytest

import halfwave_harness as hw

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
LD = np.longdouble
NS, MMAX = hw.NS, hw.MMAX
SIZES = (1, 2, 16, 17, 31, 32)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return hw.load(str(tmp_path_factory.mktemp("halfwave_harness")))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---------------------------------------------------------------------------------------------- scan_excl_half
def excl_halves(x):
    out = np.zeros_like(x)
    for h in (0, 32):
        out[:, h + 1:h + 32] = np.cumsum(x[:, h:h + 31], axis=1)
    return out


def test_scan_excl_half_exact(H):
    rng = np.random.default_rng(1)
    x = rng.integers(-1000, 1000, (7, 64)).astype(np.float64)
    x[0] = 1.0
    x[1] = np.arange(64)
    assert np.array_equal(H.scan_excl_half(x), excl_halves(x))


def test_scan_excl_half_does_not_cross_lane_32(H):
    rng = np.random.default_rng(2)
    x = np.zeros((4, 64))
    x[0, :32] = rng.integers(1, 1000, 32)
    x[1, 32:] = rng.integers(1, 1000, 32)
    x[2, 31] = 7.0
    x[3, 32] = 7.0
    out = H.scan_excl_half(x)
    assert np.array_equal(out, excl_halves(x))
    assert not out[0, 32:].any() and not out[1, :32].any() and not out[2].any()
    assert np.array_equal(out[3, 33:], np.full(31, 7.0)) and not out[3, :33].any()


# ---------------------------------------------------------------------------------------------- He
def he_inputs(seed, integer):
    """one problem per N of SIZES: full table with non-zero padding, yv zero beyond N as the solvers leave it"""
    rng = np.random.default_rng(seed)
    n = len(SIZES)
    if integer:
        Hm = rng.integers(-9, 10, (n, NS, NS)).astype(np.float64)
        y = rng.integers(-9, 10, (n, NS)).astype(np.float64)
        yj = rng.integers(-9, 10, (n, NS)).astype(np.float64)
    else:
        Hm = rng.standard_normal((n, NS, NS)) * np.exp(rng.uniform(-3, 3, (n, NS, NS)))
        y = rng.standard_normal((n, NS))
        yj = rng.standard_normal((n, NS))
    for q, N in enumerate(SIZES):
        y[q, N:] = 0.0
    return Hm, y, yj, np.array(SIZES)


def test_he_sub_outer_halves_bit_equal(H):
    Hm, y, yj, N = he_inputs(3, False)
    y = np.random.default_rng(4).standard_normal(y.shape)          # every row of the table is updated, padding included
    _, new = H.he(hw.HW_SUB_OUTER, Hm, y, yj, N)
    _, old = H.he(hw.HW_SUB_OUTER_REF, Hm, y, yj, N)
    assert np.array_equal(bits(new), bits(old))
    ref = Hm - y[:, :, None] * yj[:, None, :]
    assert np.abs(new.reshape(ref.shape) - ref).max() <= 4 * EPS * np.abs(ref).max()


def test_he_mul_halves_exact_on_integers(H):
    Hm, y, _, N = he_inputs(5, True)
    o, _ = H.he(hw.HW_MUL, Hm, y, None, N)
    for q, n in enumerate(SIZES):
        ref = np.zeros(64)
        ref[:n] = (Hm[q].T @ y[q])[:n]
        assert np.array_equal(o[q], ref), n


def test_he_mul_halves_float(H):
    Hm, y, _, N = he_inputs(6, False)
    o, _ = H.he(hw.HW_MUL, Hm, y, None, N)
    for q, n in enumerate(SIZES):
        ref = Hm[q].T.astype(LD) @ y[q].astype(LD)
        bound = NS * EPS * (np.abs(Hm[q]).T @ np.abs(y[q]))
        err = np.abs(o[q, :n].astype(LD) - ref[:n]).astype(np.float64)
        print("he_mul_halves N %2d max err / bound %.3g" % (n, (err / bound[:n]).max()))
        assert (err <= bound[:n]).all(), n
        # lanes >= N, both halves: exactly zero although the table's padding is not
        assert np.array_equal(bits(o[q, n:]), np.zeros(64 - n, dtype=np.uint64)), n


# ---------------------------------------------------------------------------------------------- columns of S
COLUMN_CASES = [(32, m) for m in (1, 2, 3, 4, 5, 7, 8, 33)] + [(5, m) for m in (1, 4, 6)] + [(31, 33), (30, 26)]
ROTATIONS = 4


def column_problems():
    """Per (N, m): ROTATIONS problems whose row lists start at a different place of the pattern of stages 0, N - 1, N, 1
    (with a non-zero e_de), so that every m meets every one of them; the rest of a list is random stages.  T_k in
    {1/4, 1/2, 1}: tau = cumsum(T) is exact, which makes the condensed rows the adjoint of the trajectory scans."""
    rng = np.random.default_rng(7)
    probs = []
    for N, m in COLUMN_CASES:
        for rot in range(ROTATIONS):
            T = rng.choice([0.25, 0.5, 1.0], NS)
            tau = np.concatenate([[0.0], np.cumsum(T)])
            He = rng.standard_normal((NS, NS))                  # not symmetric; padding beyond N is not zero either
            pattern = [0, N - 1, N, min(1, N)]
            stages = [pattern[(rot + i) % 4] if i < 4 else int(rng.integers(0, N + 1)) for i in range(m)]
            rows = np.zeros((4, MMAX))
            rows[:, :m] = rng.standard_normal((4, m))
            w_k = np.zeros(MMAX, dtype=np.int32)
            w_k[:m] = stages
            probs.append(dict(N=N, m=m, T=T, tau=tau, He=He, rows=rows, w_k=w_k))
    return probs


@pytest.fixture(scope="module")
def columns(H):
    probs = column_problems()
    args = [np.stack([p[k] for p in probs]) for k in ("He", "T", "tau", "rows", "w_k")]
    args += [np.array([p["m"] for p in probs]), np.array([p["N"] for p in probs])]
    return probs, H.columns(0, *args), H.columns(1, *args)


def test_columns4_bit_equal_to_two_column_loop(columns):
    probs, two, four = columns
    for q, p in enumerate(probs):
        nnz = p["m"] * (p["m"] + 1) // 2
        assert np.isfinite(two[q, :nnz]).all(), (p["N"], p["m"])
        assert np.array_equal(bits(four[q, :nnz]), bits(two[q, :nnz])), (p["N"], p["m"], q % ROTATIONS)
        assert np.isnan(four[q, nnz:]).all(), (p["N"], p["m"])      # nothing written beyond the triangle of m rows


def normal_ld(p, i):
    """(c_i, sum of the absolute terms of c_i) in the a-space of the horizon, long double"""
    N, k = p["N"], int(p["w_k"][i])
    T, tau = p["T"].astype(LD), p["tau"].astype(LD)
    al, be, ga, de = (LD(x) for x in p["rows"][:, i])
    c, a = np.zeros(N, dtype=LD), np.zeros(N, dtype=LD)
    for j in range(N):
        if j < k:
            lever = LD(0.5) * T[j] + tau[k] - tau[j + 1]
            c[j] = T[j] * (be + al * lever)
            a[j] = T[j] * (abs(be) + abs(al) * lever)
        if j == k:
            c[j] += ga; a[j] += abs(ga)
        if j == k - 1:
            c[j] += de; a[j] += abs(de)
    return c, a


def test_columns4_against_long_double(columns):
    probs, _, four = columns
    worst = 0.0
    for q, p in enumerate(probs):
        N, m = p["N"], p["m"]
        Ht = p["He"][:N, :N].T.astype(LD)
        C, A = zip(*[normal_ld(p, i) for i in range(m)])
        C, A = np.stack(C), np.stack(A)
        S = C @ Ht @ C.T
        bound = NS * EPS * (A @ np.abs(Ht) @ A.T)
        for i in range(m):
            for j in range(i + 1):
                err = float(abs(LD(four[q, i * (i + 1) // 2 + j]) - S[i, j]))
                worst = max(worst, err / float(bound[i, j]))
                assert err <= float(bound[i, j]), (N, m, i, j, err, float(bound[i, j]))
    print("ab_schur_columns4: largest err / bound %.3g" % worst)
