"""Without a GPU: the device harness of the shared headers (tests/kernels/linalg_harness.hip) cross-compiles for gfx950,
so a header change that breaks it is seen here; and the solvers guard their working set with the capacity the harness
tests."""
import ctypes
import os
import re

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
