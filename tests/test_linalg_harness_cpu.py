"""Without a GPU: the device harness of the shared headers (tests/kernels/linalg_harness.hip) cross-compiles for gfx950,
so a header change that breaks it is seen here; and the solvers guard their working set with the capacity the harness
tests."""
import ctypes
import os
import re

import numpy as np

import linalg_harness as lh
from eepacc_mpc_casadi_matlab_amd import build as eb


def test_harness_cross_compiles_for_gfx950(tmp_path):
    assert "--offload-arch=gfx950" in eb.BASE_FLAGS
    lib = lh.compile_harness(str(tmp_path))
    assert os.path.getsize(lib) > 0 and not lh.is_stale(lib)
    t = os.path.getmtime(lib)
    assert lh.compile_harness(str(tmp_path)) == lib and os.path.getmtime(lib) == t      # up to date: not rebuilt
    os.utime(lib, (t - 10 ** 9, t - 10 ** 9))                                             # older than its inputs
    assert lh.is_stale(lib)
    dll = ctypes.CDLL(lib)
    for s in lh.SYMBOLS:
        assert hasattr(dll, s), s
    dll.lh_schur_capacity.restype = ctypes.c_int
    assert [dll.lh_schur_capacity(ctypes.c_int(m)) for m in (32, 34, 66)] == [32, 34, 64]


def test_solvers_guard_the_working_set_with_schur_capacity():
    """rebuild_and_factor of both solvers refuses m > schur_capacity<MMAX>() (one row per lane, eepacc_schur.h) through
    its overflow path, not only m > MMAX"""
    for name in ("eepacc_ab_impl.inc", "eepacc_fbs.hip"):
        with open(os.path.join(eb.CSRC, name)) as f:
            src = f.read()
        body = src[src.index("int rebuild_and_factor("):]
        body = body[:body.index("rc_table<MMAX>()")]
        assert re.search(r"if \(m > schur_capacity<MMAX>\(\)\) return -2;", body), name
        assert "m > MMAX" not in body, name


# ---------------------------------------------------------------------------------------------- eepacc_dual_step.h
# The float64 restatements the GPU tests compare with (linalg_harness.py, written in the kernels' order) against plain dense
# algebra on the very inputs of those tests.
def cpu_mem(mmax, ns, n, fill=np.nan):
    M = np.zeros(n, dtype=lh.dual_mem_dtype(mmax, ns))
    for name in M.dtype.names:
        if name != "w_k":
            M[name] = fill
    return M


def row_matrix(r, m, N, ns):
    """C with  C [a | s | v] = the rows' values: columns a_0..a_{ns-1}, s_0..s_ns, v_0..v_ns"""
    C = np.zeros((m, 3 * ns + 2))
    for i in range(m):
        k = int(r["w_k"][i])
        C[i, ns + k], C[i, 2 * ns + 1 + k] = r["e_al"][i], r["e_be"][i]
        if k < N:
            C[i, k] += r["e_ga"][i]
        if k > 0:
            C[i, k - 1] += r["e_de"][i]
    return C


def test_record_layout_is_the_c_layout():
    for mmax, ns in lh.DUAL_SIZES:
        dt = lh.dual_mem_dtype(mmax, ns)
        doubles = mmax * (mmax + 1) // 2 + ns + 8 * (ns + 1) + 8 * mmax + len(lh.MAP_ROWS) * (ns + 1)
        assert dt.fields["P"][1] == 0 and dt.fields["w_k"][1] == 8 * doubles
        assert dt.itemsize == 8 * doubles + 4 * mmax + (4 * mmax) % 8      # padded to the alignment of a double


def test_scatter_restatements_agree_with_dense_algebra():
    for mmax, ns in lh.DUAL_SIZES:
        M, cases = lh.scatter_rows_cases(cpu_mem, mmax, ns)
        assert {c[1] for c in cases} >= {0, 1, lh.capacity(mmax)} and {c[0] for c in cases} >= {1, 2, ns - 1}
        for r, (N, m, x, sign, _) in zip(M, cases):
            vec = r["rv" if x else "lam"]
            ws, wv, wa = lh.scatter_rows_np(r, m, N, vec, sign)
            got = np.concatenate([wa, ws, wv])
            add = row_matrix(r, m, N, ns).T @ (sign * vec[:m])
            want = np.concatenate([r["wa"], r["ws"], r["wv"]]) + np.concatenate([add[:ns], [0.0], add[ns:]])
            np.testing.assert_array_equal(got, want)
        M, cases = lh.scatter_row_cases(cpu_mem, mmax, ns)
        assert {c[1] for c in cases} >= {0} and any(c[1] == c[0] for c in cases)
        for r, (N, kq, scale, row) in zip(M, cases):
            one = cpu_mem(mmax, ns, 1)[0]
            one["w_k"][0] = kq
            one["e_al"][0], one["e_be"][0], one["e_ga"][0], one["e_de"][0] = row[:4]
            add = row_matrix(one, 1, N, ns).T @ np.array([scale])
            ws, wv, wa = lh.scatter_row_np(r, kq, N, scale, *row[:4])
            np.testing.assert_array_equal(np.concatenate([wa, ws, wv]),
                                          np.concatenate([r["wa"], r["ws"], r["wv"]]) + np.concatenate([add[:ns], [0.0], add[ns:]]))


def test_row_value_and_step_rates_restatements_agree_with_dense_algebra():
    for mmax, ns in lh.DUAL_SIZES:
        M, cases = lh.row_value_cases(cpu_mem, mmax, ns)
        for r, (N, kq, row) in zip(M, cases):
            one = cpu_mem(mmax, ns, 1)[0]
            one["w_k"][0] = kq
            one["e_al"][0], one["e_be"][0], one["e_ga"][0], one["e_de"][0] = row[:4]
            x = np.concatenate([r["av"], r["shv"], r["vhv"]])
            assert lh.row_value_np(row, kq, N, r["av"], r["shv"], r["vhv"]) == (row_matrix(one, 1, N, ns) @ x)[0] - row[4]
        M, cases = lh.step_rates_int_cases(cpu_mem, mmax, ns)
        for r, (N, m) in zip(M, cases):
            sv, rv, sr = lh.step_rates_np(r, m, N)
            if m == 0:
                assert sr == 0.0
                continue
            x = np.concatenate([r["ub"][:ns], r["sub"], r["vub"]])
            sv_d = row_matrix(r, m, N, ns) @ x
            P = lh.unpack_sym(r["P"], m)
            np.testing.assert_array_equal(sv, sv_d)
            np.testing.assert_array_equal(rv, P @ sv_d)
            assert sr == sv_d @ P @ sv_d


def test_refine_restatement_agrees_with_the_closed_form():
    for mmax, ns in lh.DUAL_SIZES:
        M, cases = lh.refine_cases(cpu_mem, mmax, ns)
        assert {c[2] for c in cases} == {"exact", "one_round", "no_rounds", "half"}
        for r0, (N, m, kind, mr, tol) in zip(M, cases):
            r = r0.copy()
            G, c = lh.refine_matrix(r, m, N)
            res0 = G @ r["lam"][:m] + c - r["e_d"][:m]
            want0 = float(np.max(np.abs(res0) / (1.0 + np.abs(r["e_d"][:m]))))
            rel0, calls = lh.refine_rounds_np(r, m, N, mr, tol)
            assert calls == {"exact": 1, "one_round": 2, "no_rounds": 1, "half": 1 + mr}[kind], (mmax, N, m, kind)
            if kind == "exact":
                assert rel0 == 0.0 == want0
            elif kind == "no_rounds":
                assert rel0 == 0.0 and want0 > tol
            else:
                assert abs(rel0 - want0) <= 1e-12 * want0 and want0 > tol
                if kind == "half":                       # P = -G^-1 / 2: every round halves the residual
                    res = G @ r["lam"][:m] + c - r["e_d"][:m]
                    np.testing.assert_allclose(res, res0 * 0.5 ** mr, rtol=1e-6, atol=1e-12)


def test_tolerance_and_event_code_restatements():
    for it, N, _ in lh.tolerance_cases():
        assert lh.viol_tolerance_np(1e-11, it, N) == 1e-11 * 10.0 ** min(3, it // (3 * N + 30))
    for kind, lane, t in lh.pack_cases():
        ev = lh.pack_np(kind, lane, t)
        assert (ev >> 16, (ev >> 5) & 63, ev & 31) == (kind, lane, t) and ev != lh.NO_EVENT
