"""Build helper and ctypes front end of tests/kernels/linalg_harness.hip, the device harness that calls the functions
of csrc/eepacc_wave.h, eepacc_units.h and eepacc_schur.h directly (tests/test_gpu_linalg.py).

The harness is compiled with hipcc and build.BASE_FLAGS into a directory the caller names (a pytest temporary
directory), rebuilt when its source or one of the three headers is newer, and loaded with ctypes; nothing of it goes
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
HEADERS = ("eepacc_wave.h", "eepacc_units.h", "eepacc_schur.h")
SYMBOLS = ("lh_wave", "lh_pidx", "lh_rc_table", "lh_shift_codes", "lh_he", "lh_he_invert", "lh_schur",
           "lh_multipliers", "lh_schur_capacity")
COMPILE_TIMEOUT_S = 600
CALL_TIMEOUT_S = 60          # a harness call is a few tiny launches; one that takes this long hangs

WAVE_OPS = {n: i for i, n in enumerate(("scan_incl", "scan_excl", "wave_sum", "scan_prod_excl", "lane_prev", "lane_next",
                                        "wave_max", "wave_argmax", "wave_argmin", "bcast", "bcast_i"))}
HE_MUL, HE_MUL2, HE_SUB_OUTER = 0, 1, 2
S_INVERT, S_INSERT, S_REMOVE, S_CHAIN = 0, 1, 2, 3
CHAIN_OPS = 6


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

    def schur_capacity(self, mmax):
        with deadline():
            return int(self.lib.lh_schur_capacity(ctypes.c_int(mmax)))


def load(out_dir: str) -> Harness:
    return Harness(compile_harness(out_dir))
