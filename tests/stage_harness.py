"""Build helper and ctypes front end of tests/kernels/stage_harness.hip, the device harness that calls the per-stage
functions of csrc/eepacc_stage.h directly (tests/test_gpu_stage.py).

The harness is compiled with hipcc and build.BASE_FLAGS into a directory the caller names (a pytest temporary directory),
rebuilt when its source, eepacc_stage.h or eepacc_device.h is newer, and loaded with ctypes; nothing of it goes into
libeepacc.so.  EEPACC_STAGE_CSRC points the build at another copy of csrc/ (an edited header under test).

The DevCfg a call takes is the byte image of the product's own settings translation (cfg_harness.Built.cfg, made on the host
from a reference-style OPT dict); it is copied to the device unchanged."""
from __future__ import annotations

import ctypes
import os
import subprocess

import numpy as np

from eepacc_mpc_casadi_matlab_amd import build as eb
from linalg_harness import HarnessError, deadline

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "kernels", "stage_harness.hip")
HEADERS = ("eepacc_stage.h", "eepacc_device.h")
SYMBOLS = ("sh_estimate", "sh_route_bounds", "sh_interp_pwa", "sh_plant", "sh_sizeof_devcfg")
COMPILE_TIMEOUT_S = 600
ROUTE_OUTPUTS = ("v_lim", "v_curv", "v_stop", "v_TL", "a_min", "a_max", "j_min", "j_max")


def csrc_dir() -> str:
    return os.environ.get("EEPACC_STAGE_CSRC") or eb.CSRC


def inputs() -> list[str]:
    return [SOURCE] + [os.path.join(csrc_dir(), h) for h in HEADERS]


def is_stale(lib: str) -> bool:
    return not os.path.exists(lib) or any(os.path.getmtime(p) > os.path.getmtime(lib) for p in inputs())


def compile_harness(out_dir: str) -> str:
    """libeepacc_stage_harness.so in out_dir, for gfx950 (cross-compiles without a GPU)."""
    lib = os.path.join(out_dir, "libeepacc_stage_harness.so")
    if is_stale(lib):
        hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
        cmd = [hipcc] + eb.BASE_FLAGS + ["-shared", "-I", csrc_dir(), "-x", "hip", SOURCE, "-o", lib]
        subprocess.run(cmd, check=True, timeout=COMPILE_TIMEOUT_S)
    return lib


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64).ravel()


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32).ravel()


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class Harness:
    """numpy in, numpy out; one problem per thread."""

    def __init__(self, lib: str):
        self.lib = ctypes.CDLL(lib)
        for s in SYMBOLS:
            getattr(self.lib, s).restype = ctypes.c_int

    def call(self, name, *args):
        with deadline():
            rc = getattr(self.lib, name)(*args)
        if rc != 0:
            raise HarnessError("%s returned %d" % (name, rc))

    def sizeof_devcfg(self) -> int:
        with deadline():
            return int(self.lib.sh_sizeof_devcfg())

    @staticmethod
    def _cfg(cfg):
        cfg = np.ascontiguousarray(cfg, dtype=np.uint8)
        return cfg, _p(cfg), ctypes.c_int(cfg.size)

    def estimate(self, cfg, mode, tConstACC, s0, v0, a0, lane):
        """estimate_traj (modes 0 and 1) for every problem -> s_est [n], v_est [n]"""
        s0 = _f64(s0)
        n = s0.size
        b = lambda a, conv: conv(np.broadcast_to(a, (n,)))
        mode, lane, tc, v0, a0 = b(mode, _i32), b(lane, _i32), b(tConstACC, _f64), b(v0, _f64), b(a0, _f64)
        keep, cp, cn = self._cfg(cfg)
        s_est, v_est = np.full(n, np.nan), np.full(n, np.nan)
        self.call("sh_estimate", cp, cn, _p(mode), _p(tc), _p(s0), _p(v0), _p(a0), _p(lane), _p(s_est), _p(v_est), ctypes.c_int(n))
        return s_est, v_est

    def route_bounds(self, cfg, s_est, v_est, t0, i):
        """route_bounds for every problem -> dict of the eight outputs, each [n]"""
        s_est = _f64(s_est)
        n = s_est.size
        v_est, t0, i = _f64(np.broadcast_to(v_est, (n,))), _f64(np.broadcast_to(t0, (n,))), _i32(np.broadcast_to(i, (n,)))
        keep, cp, cn = self._cfg(cfg)
        out = np.full((8, n), np.nan)
        self.call("sh_route_bounds", cp, cn, _p(s_est), _p(v_est), _p(t0), _p(i), _p(out), ctypes.c_int(n))
        return dict(zip(ROUTE_OUTPUTS, out))

    def interp_pwa(self, d, doms, vals):
        d, doms, vals = _f64(d), _f64(doms), _f64(vals)
        assert doms.size == vals.size
        out = np.full(d.size, np.nan)
        self.call("sh_interp_pwa", _p(d), _p(doms), _p(vals), ctypes.c_int(doms.size), _p(out), ctypes.c_int(d.size))
        return out

    def plant(self, cfg, s, v, u):
        """plant_rk4 for every problem (u = Fm + Fb) -> s1 [n], v1 [n]"""
        s, v, u = _f64(s), _f64(v), _f64(u)
        assert s.size == v.size == u.size
        keep, cp, cn = self._cfg(cfg)
        s1, v1 = np.full(s.size, np.nan), np.full(s.size, np.nan)
        self.call("sh_plant", cp, cn, _p(s), _p(v), _p(u), _p(s1), _p(v1), ctypes.c_int(s.size))
        return s1, v1


def load(out_dir: str) -> Harness:
    return Harness(compile_harness(out_dir))
