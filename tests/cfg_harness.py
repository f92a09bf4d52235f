"""Build helper and ctypes front end of tests/kernels/cfg_harness.cpp, the host harness that calls the settings translation
of csrc/eepacc_cfg.cpp directly (tests/test_cfg_cpu.py).

The harness and eepacc_cfg.cpp are compiled with plain g++ (no ROCm include path) into a directory the caller names (a pytest
temporary directory) and loaded with ctypes; nothing of it goes into libeepacc.so and nothing touches a device."""
from __future__ import annotations

import ctypes as C
import hashlib
import os
import subprocess

import numpy as np

from eepacc_mpc_casadi_matlab_amd import build as eb
from eepacc_mpc_casadi_matlab_amd._abi import SettingsHolder, SettingsPOD, Vehicle, make_vehicle

HERE = os.path.dirname(os.path.abspath(__file__))
SOURCE = os.path.join(HERE, "kernels", "cfg_harness.cpp")
UNIT = os.path.join(eb.CSRC, "eepacc_cfg.cpp")
GXX_FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-Werror", "-O2", "-fPIC"]
COMPILE_TIMEOUT_S = 300
MAX_N = 63


def gxx() -> str:
    return os.environ.get("CXX", "g++")


def compile_harness(out_dir: str) -> str:
    lib = os.path.join(out_dir, "libeepacc_cfg_harness.so")
    cmd = [gxx()] + GXX_FLAGS + ["-shared", "-I", eb.CSRC, SOURCE, UNIT, "-o", lib]
    subprocess.run(cmd, check=True, timeout=COMPILE_TIMEOUT_S)
    return lib


class Built:
    """What the translation returned for one settings / vehicle pair."""

    def __init__(self, h, rc, msg, cfg, hinv, kpi, follow):
        self._h, self.rc, self.msg, self.cfg, self.kpi, self.follow = h, rc, msg, cfg, kpi, follow
        self.N = int(self.field("N")[0]) if rc == 0 else 0
        self.Hinv = hinv[:self.N * self.N].reshape(self.N, self.N).copy()

    def field(self, name, dtype=None):
        """A field of DevCfg as an array; dtype defaults to int32 for 4-byte elements and float64 otherwise."""
        off, nbytes = self._h.field(name)
        if dtype is None:
            dtype = np.int32 if name in self._h.INT_FIELDS else np.float64
        return np.frombuffer(self.cfg, dtype=dtype, count=nbytes // np.dtype(dtype).itemsize, offset=off)

    def digests(self):
        sha = lambda b: hashlib.sha256(bytes(b)).hexdigest()
        return {"DevCfg": sha(self.cfg), "Hinv": sha(self.Hinv.tobytes()), "KpiCfg": sha(self.kpi), "FollowCfg": sha(self.follow)}


class Harness:
    INT_FIELDS = ("N", "const_T", "const_slope", "mb_any", "max_iter", "bl_mode", "mb_lead", "mb_end", "mb_maxlen", "fb_row0",
                  "mb_mask", "N_integratePlant", "n_TL")

    def __init__(self, lib: str):
        self.lib = C.CDLL(lib)
        self.lib.ch_last_error.restype = C.c_char_p
        self.lib.ch_build.restype = C.c_int
        self.lib.ch_build.argtypes = [C.POINTER(SettingsPOD), C.POINTER(Vehicle), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        self.lib.ch_field.argtypes = [C.c_char_p, C.POINTER(C.c_int), C.POINTER(C.c_int)]
        s = [C.c_int() for _ in range(3)]
        self.lib.ch_sizes(*[C.byref(x) for x in s])
        self.sizeof_devcfg, self.sizeof_kpi, self.sizeof_follow = (x.value for x in s)

    def field(self, name):
        off, nbytes = C.c_int(), C.c_int()
        if self.lib.ch_field(name.encode(), C.byref(off), C.byref(nbytes)) != 0:
            raise KeyError(name)
        return off.value, nbytes.value

    def build_pod(self, pod: SettingsPOD, veh: Vehicle) -> Built:
        cfg = np.full(self.sizeof_devcfg, 0xAB, dtype=np.uint8)        # the translation must zero it itself
        kpi, follow = np.zeros(self.sizeof_kpi, dtype=np.uint8), np.zeros(self.sizeof_follow, dtype=np.uint8)
        hinv = np.zeros(MAX_N * MAX_N)
        rc = self.lib.ch_build(C.byref(pod), C.byref(veh), cfg.ctypes.data, hinv.ctypes.data, kpi.ctypes.data, follow.ctypes.data)
        return Built(self, rc, self.lib.ch_last_error().decode(), cfg, hinv, kpi, follow)

    def build(self, OPT, V, mutate=None) -> Built:
        """mutate(pod, veh, holder) edits the PODs after the holder has filled them (what SettingsHolder itself would refuse)."""
        holder, veh = SettingsHolder(OPT), make_vehicle(V)
        if mutate is not None:
            mutate(holder.pod, veh, holder)
        return self.build_pod(holder.pod, veh)


def load(out_dir: str) -> Harness:
    return Harness(compile_harness(out_dir))
