"""Build helper and ctypes front end of tests/kernels/halfwave_harness.hip, the device harness of the functions that
use both 32-lane halves of a wave at NS = 32 (tests/test_gpu_halfwave.py).  Built and loaded the way
tests/linalg_harness.py builds its harness: hipcc with build.BASE_FLAGS into a directory the caller names, ctypes, and
its deadline() around every call."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

import linalg_harness as lh
from eepacc_mpc_casadi_matlab_amd import build as eb

SOURCE = os.path.join(lh.HERE, "kernels", "halfwave_harness.hip")
HEADERS = ("eepacc_wave.h", "eepacc_units.h", "eepacc_schur.h", "eepacc_ab_cols.h")
SYMBOLS = ("hw_scan_excl_half", "hw_he", "hw_columns")
NS, MMAX = 32, 34
PS = MMAX * (MMAX + 1) // 2
HW_MUL, HW_SUB_OUTER, HW_SUB_OUTER_REF = 0, 1, 2


def compile_harness(out_dir: str) -> str:
    """libeepacc_halfwave_harness.so in out_dir, for gfx950 (cross-compiles without a GPU)."""
    lib = os.path.join(out_dir, "libeepacc_halfwave_harness.so")
    inputs = [SOURCE] + [os.path.join(lh.csrc_dir(), h) for h in HEADERS]
    if not os.path.exists(lib) or any(os.path.getmtime(p) > os.path.getmtime(lib) for p in inputs):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc] + eb.BASE_FLAGS + ["-shared", "-I", lh.csrc_dir(), "-x", "hip", SOURCE, "-o", lib]
        subprocess.run(cmd, check=True, timeout=lh.COMPILE_TIMEOUT_S)
    return lib


class Harness:
    """numpy in, numpy out; one problem per wave, `wpb` waves per block."""

    def __init__(self, lib: str):
        self.lib = ctypes.CDLL(lib)
        for s in SYMBOLS:
            getattr(self.lib, s).restype = ctypes.c_int

    def call(self, name, *args):
        with lh.deadline():
            rc = getattr(self.lib, name)(*[lh._arg(a) for a in args])
        if rc != 0:
            raise lh.HarnessError("%s returned %d" % (name, rc))

    def scan_excl_half(self, x, wpb=3):
        x = lh._f64(x).reshape(-1, 64)
        out = np.full_like(x, np.nan)
        self.call("hw_scan_excl_half", x, out, x.shape[0], wpb)
        return out

    def he(self, op, H, y0, y1, N, wpb=3):
        """H [n][NS * NS], y0 / y1 [n][NS], N [n] -> (o0 [n][64], Hout [n][NS * NS])"""
        H = lh._f64(H).reshape(-1, NS * NS)
        n = H.shape[0]
        y0 = lh._f64(y0).reshape(n, NS)
        y1 = lh._f64(np.zeros((n, NS)) if y1 is None else y1).reshape(n, NS)
        o0, Ho = np.full((n, 64), np.nan), np.full_like(H, np.nan)
        self.call("hw_he", op, H, y0, y1, lh._i32(N).reshape(n), o0, Ho, n, wpb)
        return o0, Ho

    def columns(self, four, He, Tvec, tau, rows, w_k, m, N, wpb=2):
        """He [n][NS * NS], Tvec [n][NS], tau [n][NS + 1], rows [n][4][MMAX], w_k [n][MMAX], m / N [n] -> P [n][PS]"""
        He = lh._f64(He).reshape(-1, NS * NS)
        n = He.shape[0]
        P = np.full((n, PS), np.nan)
        self.call("hw_columns", int(four), He, lh._f64(Tvec).reshape(n, NS), lh._f64(tau).reshape(n, NS + 1),
                  lh._f64(rows).reshape(n, 4, MMAX), lh._i32(w_k).reshape(n, MMAX), lh._i32(m).reshape(n),
                  lh._i32(N).reshape(n), P, n, wpb)
        return P


def load(out_dir: str) -> Harness:
    return Harness(compile_harness(out_dir))
