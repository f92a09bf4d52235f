"""Build helper and ctypes front end of tests/kernels/linalg_harness.hip, the device harness that calls the functions
of csrc/eepacc_wave.h, eepacc_units.h, eepacc_schur.h and eepacc_dual_step.h directly (tests/test_gpu_linalg.py).

The harness is compiled with hipcc and build.BASE_FLAGS into a directory the caller names (a pytest temporary
directory), rebuilt when its source or one of the headers is newer, and loaded with ctypes; nothing of it goes
into libeepacc.so.  EEPACC_LINALG_CSRC points the build at another copy of csrc/ (an edited header under test)."""
from __future__ import annotations

import contextlib
import ctypes
import faulthandler
import os
import subprocess

import numpy as np

from eepacc_mpc_casadi_matlab_amd import build as eb

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "kernels", "linalg_harness.hip")
HEADERS = ("eepacc_wave.h", "eepacc_units.h", "eepacc_schur.h", "eepacc_dual_step.h")
SYMBOLS = ("lh_wave", "lh_pidx", "lh_rc_table", "lh_shift_codes", "lh_he", "lh_he_invert", "lh_schur",
           "lh_multipliers", "lh_schur_capacity", "lh_dual_mem_size", "lh_dual", "lh_step_scalars")
COMPILE_TIMEOUT_S = 600
CALL_TIMEOUT_S = 60          # a harness call is a few tiny launches; one that takes this long hangs

WAVE_OPS = {n: i for i, n in enumerate(("scan_incl", "scan_excl", "wave_sum", "scan_prod_excl", "lane_prev", "lane_next",
                                        "wave_max", "wave_argmax", "wave_argmin", "bcast", "bcast_i"))}
HE_MUL, HE_MUL2, HE_SUB_OUTER = 0, 1, 2
S_INVERT, S_INSERT, S_REMOVE, S_CHAIN = 0, 1, 2, 3
CHAIN_OPS = 6
D_SCATTER_ROWS, D_SCATTER_ROW, D_ROW_VALUE, D_STEP_RATES, D_REFINE = 0, 1, 2, 3, 4
NO_EVENT = 0x7fffffff
MAP_ROWS = ("s0", "cs", "v0", "cv", "a0", "ca", "cb")      # the affine map of the harness's recompute (D_REFINE)


def dual_mem_dtype(mmax, ns):
    """one record = DualMem<mmax, ns> of the harness (C layout)"""
    d = [("P", "f8", (mmax * (mmax + 1) // 2,)), ("av", "f8", (ns,))]
    d += [(n, "f8", (ns + 1,)) for n in ("shv", "vhv", "ub", "sub", "vub", "ws", "wv", "wa")]
    d += [(n, "f8", (mmax,)) for n in ("e_al", "e_be", "e_ga", "e_de", "e_d", "lam", "sv", "rv")]
    d += [("map", "f8", (len(MAP_ROWS), ns + 1)), ("w_k", "i4", (mmax,))]
    return np.dtype(d, align=True)


def csrc_dir() -> str:
    return os.environ.get("EEPACC_LINALG_CSRC") or eb.CSRC


def inputs() -> list[str]:
    return [SOURCE] + [os.path.join(csrc_dir(), h) for h in HEADERS]


def is_stale(lib: str) -> bool:
    return not os.path.exists(lib) or any(os.path.getmtime(p) > os.path.getmtime(lib) for p in inputs())


def compile_harness(out_dir: str) -> str:
    """libeepacc_linalg_harness.so in out_dir, for gfx950 (cross-compiles without a GPU)."""
    lib = os.path.join(out_dir, "libeepacc_linalg_harness.so")
    if is_stale(lib):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc] + eb.BASE_FLAGS + ["-shared", "-I", csrc_dir(), "-x", "hip", SOURCE, "-o", lib]
        subprocess.run(cmd, check=True, timeout=COMPILE_TIMEOUT_S)
    return lib


class HarnessError(RuntimeError):
    pass


@contextlib.contextmanager
def deadline(seconds: int = CALL_TIMEOUT_S):
    """Ends the process (with a traceback) if the block does not return in time: a hung kernel must not hold the GPU."""
    faulthandler.dump_traceback_later(seconds, exit=True)
    try:
        yield
    finally:
        faulthandler.cancel_dump_traceback_later()


def _arg(a):
    if a is None:
        return ctypes.c_void_p(None)
    if isinstance(a, np.ndarray):
        assert a.flags["C_CONTIGUOUS"]
        return a.ctypes.data_as(ctypes.c_void_p)
    if isinstance(a, (int, np.integer)):
        return ctypes.c_int(int(a))
    raise TypeError(type(a))


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


class Harness:
    """numpy in, numpy out; one problem per wave, `wpb` waves per block."""

    def __init__(self, lib: str):
        self.lib = ctypes.CDLL(lib)
        for s in SYMBOLS:
            getattr(self.lib, s).restype = ctypes.c_int

    def call(self, name, *args):
        with deadline():
            rc = getattr(self.lib, name)(*[_arg(a) for a in args])
        if rc != 0:
            raise HarnessError("%s returned %d" % (name, rc))

    # ---- eepacc_wave.h
    def wave(self, op, x, payload=None, src=None, wpb=3):
        x = _f64(x).reshape(-1, 64)
        n = x.shape[0]
        pi = _i32(np.zeros((n, 64)) if payload is None else payload).reshape(n, 64)
        src = _i32(np.zeros(n) if src is None else src).reshape(n)
        od, oi = np.full((n, 64), np.nan), np.full((n, 64), -1, dtype=np.int32)
        self.call("lh_wave", WAVE_OPS[op], x, pi, src, od, oi, n, wpb)
        return od, oi

    # ---- eepacc_units.h
    def pidx(self, n):
        out = np.full((n, n), -1, dtype=np.int32)
        self.call("lh_pidx", n, out)
        return out

    def rc_table(self, mmax, nblocks=2, wpb=3):
        out = np.zeros((nblocks * wpb, mmax * (mmax + 1) // 2), dtype=np.uint16)
        self.call("lh_rc_table", mmax, out, nblocks, wpb)
        return out

    def shift_codes(self, code, N, wpb=3):
        code = np.ascontiguousarray(code, dtype=np.uint64).reshape(-1, 64)
        n = code.shape[0]
        out = np.zeros_like(code)
        self.call("lh_shift_codes", code, _i32(N).reshape(n), out, n, wpb)
        return out

    # ---- He
    @staticmethod
    def he_size(ns, packed):
        return ns * (ns + 1) // 2 if packed else ns * ns

    def he(self, op, ns, packed, H, y0, y1, N, wpb=3):
        """H [n][he_size], y0 / y1 [n][ns], N [n] -> (o0 [n][64], o1 [n][64], Hout [n][he_size])"""
        H = _f64(H).reshape(-1, self.he_size(ns, packed))
        n = H.shape[0]
        y0 = _f64(y0).reshape(n, ns)
        y1 = _f64(np.zeros((n, ns)) if y1 is None else y1).reshape(n, ns)
        o0, o1, Ho = np.full((n, 64), np.nan), np.full((n, 64), np.nan), np.full_like(H, np.nan)
        self.call("lh_he", op, ns, int(packed), H, y0, y1, _i32(N).reshape(n), o0, o1, Ho, n, wpb)
        return o0, o1, Ho

    def he_invert(self, ns, H, N, wpb=2):
        H = _f64(H).reshape(-1, ns, ns).copy()
        n = H.shape[0]
        ret = np.full((n, 64), -1, dtype=np.int32)
        self.call("lh_he_invert", ns, H, _i32(N).reshape(n), ret, n, wpb)
        return H, ret

    # ---- P
    def schur(self, op, mmax, P, m, kind=None, pos=None, vec=None, piv=None, wpb=3):
        """P [n][mmax (mmax + 1) / 2] -> (P, ret [n][64], sv [n][mmax], m_out [n])"""
        P = _f64(P).reshape(-1, mmax * (mmax + 1) // 2).copy()
        n = P.shape[0]
        per = CHAIN_OPS if op == S_CHAIN else 1
        m = _i32(m).reshape(n)
        kind = None if kind is None else _i32(kind).reshape(n, per)
        pos = None if pos is None else _i32(pos).reshape(n, per)
        vec = None if vec is None else _f64(vec).reshape(n, per, mmax)
        piv = None if piv is None else _f64(piv).reshape(n, per)
        ret, sv = np.full((n, 64), -1, dtype=np.int32), np.full((n, mmax), np.nan)
        m_out = np.full(n, -1, dtype=np.int32)
        self.call("lh_schur", op, mmax, P, m, kind, pos, vec, piv, ret, sv, m_out, n, wpb)
        return P, ret, sv, m_out

    def multipliers(self, mmax, ns, P, img, rows, w_k, m, N, wpb=2):
        P = _f64(P).reshape(-1, mmax * (mmax + 1) // 2)
        n = P.shape[0]
        lam, sv = np.full((n, mmax), np.nan), np.full((n, mmax), np.nan)
        self.call("lh_multipliers", mmax, ns, P, _f64(img).reshape(n, 3, ns + 1), _f64(rows).reshape(n, 5, mmax),
                  _i32(w_k).reshape(n, mmax), _i32(m).reshape(n), _i32(N).reshape(n), lam, sv, n, wpb)
        return lam, sv

    # ---- eepacc_dual_step.h
    def dual_mem(self, mmax, ns, n, fill=np.nan):
        """n records of the per-wave struct, every double `fill` (NaN: a routine that reads what it was not given shows)"""
        dt = dual_mem_dtype(mmax, ns)
        with deadline():
            assert int(self.lib.lh_dual_mem_size(ctypes.c_int(mmax), ctypes.c_int(ns))) == dt.itemsize
        M = np.zeros(n, dtype=dt)
        for name in dt.names:
            if name != "w_k":
                M[name] = fill
        return M

    def dual(self, op, mmax, ns, M, m, N, kq=None, x=None, scale=None, row=None, wpb=2):
        """M: records of dual_mem (not modified); row [n][5] = al, be, ga, de, d -> (M after the call, ret [n][64], calls [n][64])"""
        M = M.copy()
        n = M.shape[0]
        ipar = np.zeros((n, 4), dtype=np.int32)
        ipar[:, 0], ipar[:, 1] = m, N
        ipar[:, 2] = 0 if kq is None else kq
        ipar[:, 3] = 0 if x is None else x
        par = np.zeros((n, 6))
        par[:, 0] = 0.0 if scale is None else scale
        if row is not None:
            par[:, 1:] = _f64(row).reshape(n, 5)
        od, oi = np.full((n, 64), np.nan), np.full((n, 64), -1, dtype=np.int32)
        self.call("lh_dual", op, mmax, ns, M, par, ipar, od, oi, n, wpb)
        return M, od, oi

    def step_scalars(self, triples, tol0):
        """triples [n][3] -> (EvCode::pack(a, b, c) and its kind / lane / type [n][4], viol_tolerance(tol0, a, b) [n])"""
        triples = _i32(triples).reshape(-1, 3)
        n = triples.shape[0]
        code, tol = np.full((n, 4), -1, dtype=np.int32), np.full(n, np.nan)
        self.call("lh_step_scalars", triples, _f64(tol0).reshape(n), code, tol, n)
        return code, tol

    def schur_capacity(self, mmax):
        with deadline():
            return int(self.lib.lh_schur_capacity(ctypes.c_int(mmax)))


def load(out_dir: str) -> Harness:
    return Harness(compile_harness(out_dir))


# ---------------------------------------------------------------------------------------------- eepacc_dual_step.h
# float64 restatements in the kernel's order (a record r of dual_mem; they return what the routine leaves behind)
def scatter_rows_np(r, m, N, vec, sign):
    ws, wv, wa = r["ws"].copy(), r["wv"].copy(), r["wa"].copy()
    for i in range(m):
        k, l = int(r["w_k"][i]), sign * vec[i]
        ws[k] += l * r["e_al"][i]
        wv[k] += l * r["e_be"][i]
        if k < N and r["e_ga"][i] != 0.0:
            wa[k] += l * r["e_ga"][i]
        if k > 0 and r["e_de"][i] != 0.0:
            wa[k - 1] += l * r["e_de"][i]
    return ws, wv, wa


def scatter_row_np(r, kq, N, scale, al, be, ga, de):
    ws, wv, wa = r["ws"].copy(), r["wv"].copy(), r["wa"].copy()
    ws[kq] += scale * al
    wv[kq] += scale * be
    if kq < N and ga != 0.0:
        wa[kq] += scale * ga
    if kq > 0 and de != 0.0:
        wa[kq - 1] += scale * de
    return ws, wv, wa


def row_value_np(row, kq, N, a, s, v):
    al, be, ga, de, d = row
    x = al * s[kq] + be * v[kq] - d
    if kq < N:
        x += ga * a[kq]
    if kq > 0:
        x += de * a[kq - 1]
    return x


def rows_dot_np(r, m, N, x, sx, vx):
    out = np.zeros(m)
    for i in range(m):
        out[i] = row_value_np((r["e_al"][i], r["e_be"][i], r["e_ga"][i], r["e_de"][i], 0.0), int(r["w_k"][i]), N, x, sx, vx)
    return out


def unpack_sym(P, m):
    A = np.zeros((m, m), dtype=P.dtype)
    A[np.tril_indices(m)] = P[:m * (m + 1) // 2]
    return A + np.tril(A, -1).T


def step_rates_np(r, m, N):
    """(sv, rv, sr); the sum over the lanes in the order of wave_sum's scan is any order on exact data"""
    if m == 0:
        return np.zeros(0), np.zeros(0), 0.0
    sv = rows_dot_np(r, m, N, r["ub"], r["sub"], r["vub"])
    P = unpack_sym(r["P"], m)
    rv = np.zeros(m)
    for i in range(m):
        acc = 0.0
        for j in range(m):
            acc = P[i, j] * sv[j] + acc
        rv[i] = acc
    return sv, rv, float(np.sum(sv * rv))


def recompute_np(r, m, N):
    """the harness's affine map lam -> (av, shv, vhv), in place"""
    mp = dict(zip(MAP_ROWS, r["map"]))
    lam = np.concatenate([r["lam"][:m], np.zeros(len(mp["s0"]) + 1 - m)])
    k = np.arange(N + 1)
    r["shv"][:N + 1] = mp["s0"][k] + mp["cs"][k] * lam[k]
    r["vhv"][:N + 1] = mp["v0"][k] + mp["cv"][k] * lam[k]
    k = np.arange(N)
    r["av"][:N] = mp["a0"][k] + mp["ca"][k] * lam[k] + mp["cb"][k] * lam[k + 1]


def refine_rounds_np(r, m, N, max_rounds, res_tol):
    """(rel0, calls); r is updated like the kernel's struct"""
    calls = 1
    recompute_np(r, m, N)
    if m == 0:
        return 0.0, calls
    rel0 = 0.0
    P = unpack_sym(r["P"], m)
    for rnd in range(max_rounds):
        res = rows_dot_np(r, m, N, r["av"], r["shv"], r["vhv"]) - r["e_d"][:m]
        rel = float(np.max(np.abs(res) / (1.0 + np.abs(r["e_d"][:m]))))
        r["sv"][:m] = res
        if rnd == 0:
            rel0 = rel
        if not rel > res_tol:
            break
        r["lam"][:m] += P @ res
        recompute_np(r, m, N)
        calls += 1
    return rel0, calls


def refine_matrix(r, m, N):
    """the working-set residual of the harness's map as G lam + c - d (rows at stages 0..m-1): dense G and c"""
    mp = dict(zip(MAP_ROWS, r["map"]))
    G, c = np.zeros((m, m)), np.zeros(m)
    for i in range(m):
        G[i, i] = r["e_al"][i] * mp["cs"][i] + r["e_be"][i] * mp["cv"][i]
        c[i] = r["e_al"][i] * mp["s0"][i] + r["e_be"][i] * mp["v0"][i]
        if i < N:
            G[i, i] += r["e_ga"][i] * mp["ca"][i]
            c[i] += r["e_ga"][i] * mp["a0"][i]
            if i + 1 < m:
                G[i, i + 1] = r["e_ga"][i] * mp["cb"][i]
        if i > 0:
            G[i, i - 1] = r["e_de"][i] * mp["ca"][i - 1]
            G[i, i] += r["e_de"][i] * mp["cb"][i - 1]
            c[i] += r["e_de"][i] * mp["a0"][i - 1]
    return G, c


def viol_tolerance_np(tol0, iters, N):
    e = 3 * N + 30
    return tol0 * (1.0 if iters < e else (10.0 if iters < 2 * e else (100.0 if iters < 3 * e else 1000.0)))


def pack_np(kind, lane, t):
    return (kind << 16) | (lane << 5) | t


# ---- cases: (records, m, N, ...) per table size; integer-valued unless said otherwise
DUAL_SIZES = ((34, 32), (32, 32), (66, 64))


def capacity(mmax):
    return min(mmax, 64)


def stage_counts(ns):
    return (1, 2, ns - 1, ns)


def _int_rows(rng, r, m, N, zero_frac=0.3):
    """m integer rows at random stages; the first at stage 0, the last at stage N, three on one stage; some ga / de zero"""
    wk = rng.integers(0, N + 1, m)
    if m >= 1:
        wk[0] = 0
    if m >= 2:
        wk[m - 1] = N
    if m >= 5:
        wk[1:4] = min(1, N)
    r["w_k"][:m] = wk
    for name in ("e_al", "e_be", "e_ga", "e_de", "e_d"):
        r[name][:m] = rng.integers(1, 5, m) * rng.choice([-1.0, 1.0], m)
    for name in ("e_ga", "e_de"):
        r[name][:m] = np.where(rng.random(m) < zero_frac, 0.0, r[name][:m])


def scatter_rows_cases(harness_mem, mmax, ns, seed=101):
    """records with ws | wv | wa filled: integers, or -0.0 in wa (an add of +0.0 that should have been skipped flips its sign)"""
    rng = np.random.default_rng(seed + mmax)
    cases = [(N, m, x, sign, negzero) for N in stage_counts(ns) for m in sorted({0, 1, 7, min(capacity(mmax), 3 * (N + 1)), capacity(mmax)})
             for x, sign, negzero in ((0, 1.0, True), (1, -1.0, False))]
    M = harness_mem(mmax, ns, len(cases))
    for r, (N, m, x, sign, negzero) in zip(M, cases):
        _int_rows(rng, r, m, N)
        r["rv" if x else "lam"][:m] = rng.integers(1, 6, m) * (1.0 if negzero else rng.choice([-1.0, 1.0], m))
        for name in ("ws", "wv", "wa"):
            r[name][:] = rng.integers(-9, 10, ns + 1)
        if negzero:
            r["wa"][:] = -0.0
    return M, cases


def scatter_row_cases(harness_mem, mmax, ns, seed=102):
    rng = np.random.default_rng(seed + mmax)
    cases = []
    for N in stage_counts(ns):
        for kq in sorted({0, N // 2, N}):
            for ga, de in ((2.0, -3.0), (0.0, 0.0), (0.0, 5.0), (-1.0, 0.0)):
                cases.append((N, kq, float(rng.integers(1, 7)) * (-1.0 if ga < 0 else 1.0), (float(rng.integers(-4, 5)), float(rng.integers(-4, 5)), ga, de, 0.0)))
    M = harness_mem(mmax, ns, len(cases))
    for r in M:
        r["ws"][:], r["wv"][:], r["wa"][:] = rng.integers(-9, 10, ns + 1), rng.integers(-9, 10, ns + 1), -0.0
    return M, cases


def row_value_cases(harness_mem, mmax, ns, seed=103):
    rng = np.random.default_rng(seed + mmax)
    cases = [(N, kq, tuple(float(v) for v in rng.integers(1, 6, 5) * rng.choice([-1, 1], 5)))
             for N in stage_counts(ns) for kq in sorted({0, 1, N // 2, N - 1, N})]
    M = harness_mem(mmax, ns, len(cases))
    for r in M:
        r["av"][:] = rng.integers(-9, 10, ns)
        r["shv"][:], r["vhv"][:] = rng.integers(-9, 10, ns + 1), rng.integers(-9, 10, ns + 1)
    return M, cases


def step_rates_int_cases(harness_mem, mmax, ns, seed=104):
    rng = np.random.default_rng(seed + mmax)
    cases = [(N, m) for N in stage_counts(ns) for m in sorted({0, 1, 2, min(capacity(mmax), N + 1), capacity(mmax)})]
    M = harness_mem(mmax, ns, len(cases))
    for r, (N, m) in zip(M, cases):
        _int_rows(rng, r, m, N)
        A = rng.integers(-3, 4, (m, m)).astype(float)
        A = np.tril(A) + np.tril(A, -1).T
        r["P"][:m * (m + 1) // 2] = A[np.tril_indices(m)]
        r["ub"][:], r["sub"][:], r["vub"][:] = (rng.integers(-5, 6, ns + 1) for _ in range(3))
    return M, cases


def refine_cases(harness_mem, mmax, ns, seed=105):
    """(records, cases); case = (N, m, kind, max_rounds, res_tol), kind: exact | one_round | no_rounds | half"""
    rng = np.random.default_rng(seed + mmax)
    sizes = sorted({(1, 1), (2, 2), (2, 3), (ns - 1, min(ns, capacity(mmax))), (ns, min(ns + 1, capacity(mmax)))})
    cases = [(N, m, kind, mr, tol) for N, m in sizes
             for kind, mr, tol in (("exact", 3, 1e-11), ("one_round", 3, 1e-11), ("no_rounds", 0, 1e-11), ("half", 4, 1e-11))]
    M = harness_mem(mmax, ns, len(cases))
    for r, (N, m, kind, mr, tol) in zip(M, cases):
        integer = kind == "exact"
        draw = (lambda n: rng.integers(1, 4, n) * rng.choice([-1.0, 1.0], n)) if integer else (lambda n: rng.uniform(0.5, 1.5, n) * rng.choice([-1.0, 1.0], n))
        r["w_k"][:m] = np.arange(m)
        for name in ("e_al", "e_be", "e_ga", "e_de"):
            r[name][:m] = draw(m)
        mp = {n: draw(ns + 1) for n in MAP_ROWS}
        if not integer:
            mp["cs"][:m] = 100.0 * np.sign(r["e_al"][:m]) * np.abs(mp["cs"][:m])      # G_ii >= 25 - 11.25, off the diagonal <= 2.25
            ga, de_next = np.ones(ns + 1), np.zeros(ns + 1)
            ga[:m] = r["e_ga"][:m]
            de_next[:m - 1] = r["e_de"][1:m]
            mp["cb"] = de_next * mp["ca"] / ga                                 # G symmetric, as P is
        r["map"][:] = np.array([mp[n] for n in MAP_ROWS])
        lam = draw(m)
        G, c = refine_matrix(r, m, N)
        r["e_d"][:m] = G @ lam + c                                             # lam solves the rows (exactly on integers)
        if kind != "exact":
            G = (G + G.T) / 2
            Pm = -np.linalg.inv(G) * (0.5 if kind == "half" else 1.0)
            r["P"][:m * (m + 1) // 2] = ((Pm + Pm.T) / 2)[np.tril_indices(m)]
            lam = lam * (1.0 + 1e-3 * rng.uniform(0.5, 1.0, m))
        r["lam"][:m] = lam
    return M, cases


def tolerance_cases():
    return [(it, N, 0) for N in (1, 32, 63) for e in (3 * N + 30,) for it in (e - 1, e, 2 * e - 1, 2 * e, 3 * e - 1, 3 * e)]


def pack_cases():
    return [(kind, lane, t) for kind in range(1, 6) for lane in (0, 63) for t in (0, 31)]
