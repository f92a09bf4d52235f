"""What eepacc_classes_build_qp / _qp_size / _qp_rows need that can be checked without a GPU.

b1  The host row catalogue of csrc/eepacc_cfg.cpp (classes_qp_num_rows, classes_qp_max_rows, classes_qp_rows), which the entry
    eepacc_classes_qp_rows and the launcher share, through tests/kernels/classes_rows_harness.cpp built with plain g++: the
    per-class counts, the padding, the order of eepacc_ab_qp_rows / eepacc_bl_qp_rows for a one-class handle (against the
    restatements tests/ab_cert_cases.py::row_map and tests/bl_qp_ref.py::rows_of), cls out of range.
b2  The same functions as a program of its own under AddressSanitizer and UndefinedBehaviorSanitizer
    (tests/kernels/classes_rows_sanitize_main.cpp); nothing is loaded into Python under a sanitizer.
b3  _abi.py declares the three entries with the header's parameter lists, the built library exports them, and the two new
    kernel units cross-compile for gfx950 without scratch.
b4  Python-side argument errors of Engine.classes_build_qp and the row selection of qp_sens.ab_lead_gradient on a class engine.
"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import ab_cert_cases as T
import bl_qp_ref as blr
import cfg_harness
from eepacc_mpc_casadi_matlab_amd import _abi, engine, qp_sens
from eepacc_mpc_casadi_matlab_amd import build as eb

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
NAMES = ("eepacc_classes_qp_size", "eepacc_classes_qp_rows", "eepacc_classes_build_qp")
i32p = C.POINTER(C.c_int32)


# ------------------------------------------------------------------------------------------------ b1
class Rows:
    def __init__(self, lib):
        self.lib = C.CDLL(lib)
        self.lib.cr_last_error.restype = C.c_char_p
        self.lib.cr_num_rows.argtypes = [C.c_int, i32p, i32p, i32p, C.c_int]
        self.lib.cr_max_rows.argtypes = [C.c_int, i32p, i32p, i32p]
        self.lib.cr_rows.argtypes = [C.c_int, i32p, i32p, i32p, C.c_int, i32p, i32p]
        self.lib.cr_of_devcfg.argtypes = [C.c_int, C.c_int, C.c_int, i32p]

    @staticmethod
    def _pack(classes):
        a = [np.ascontiguousarray([c[j] for c in classes], dtype=np.int32) for j in range(3)]
        return a, [x.ctypes.data_as(i32p) for x in a]

    def num_rows(self, classes, cls):
        keep, p = self._pack(classes)
        return self.lib.cr_num_rows(len(classes), *p, cls)

    def max_rows(self, classes):
        keep, p = self._pack(classes)
        return self.lib.cr_max_rows(len(classes), *p)

    def rows(self, classes, cls, nC=None):
        keep, p = self._pack(classes)
        nC = self.max_rows(classes) if nC is None else nC
        stage, typ = np.full(nC + 1, 77, dtype=np.int32), np.full(nC + 1, 77, dtype=np.int32)      # one guard entry each
        rc = self.lib.cr_rows(len(classes), *p, cls, stage.ctypes.data_as(i32p), typ.ctypes.data_as(i32p))
        assert stage[nC] == 77 and typ[nC] == 77
        return rc, self.lib.cr_last_error().decode(), stage[:nC], typ[:nC]


@pytest.fixture(scope="module")
def rows(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("classes_rows"))
    lib = os.path.join(out, "libeepacc_classes_rows_harness.so")
    cmd = [cfg_harness.gxx()] + cfg_harness.GXX_FLAGS + ["-shared", "-I", eb.CSRC, os.path.join(HERE, "kernels", "classes_rows_harness.cpp"),
                                                         cfg_harness.UNIT, "-o", lib]
    subprocess.run(cmd, check=True, timeout=cfg_harness.COMPILE_TIMEOUT_S)
    return Rows(lib)


@pytest.mark.parametrize("N", [2, 3, 20, 33, 63])
def test_counts_per_class(rows, N):
    ab = [(N, 0, 0), (N, 0, 1), (N, 0, 0)]
    assert [rows.num_rows(ab, c) for c in range(3)] == [14 * N + 2, 18 * N + 2, 14 * N + 2]
    assert rows.max_rows(ab) == 18 * N + 2 and rows.max_rows(ab[:1]) == 14 * N + 2 and rows.max_rows(ab[::2]) == 14 * N + 2
    bl, tv = [(N, 1, 0), (N, 1, 1)], [(N, 2, 1), (N, 2, 0)]               # the baseline rows do not depend on ab_route_rows
    assert [rows.num_rows(bl, c) for c in range(2)] == [13 * N + 2] * 2 and rows.max_rows(bl) == 13 * N + 2
    assert [rows.num_rows(tv, c) for c in range(2)] == [11 * N] * 2 and rows.max_rows(tv) == 11 * N


def test_what_the_catalogue_reads_of_a_devcfg(rows):
    out = np.zeros(3, dtype=np.int32)
    rows.lib.cr_of_devcfg(33, 2, 1, out.ctypes.data_as(i32p))
    assert list(out) == [33, 2, 1]


@pytest.mark.parametrize("N", [2, 20, 63])
def test_padding(rows, N):
    classes = [(N, 0, 0), (N, 0, 1)]
    nC, own = 18 * N + 2, 14 * N + 2
    rc, _, stage, typ = rows.rows(classes, 0)
    assert rc == 0 and stage.size == nC
    assert (stage[own:] == -1).all() and (typ[own:] == -1).all() and (stage[:own] >= 0).all() and (typ[:own] >= 0).all()
    assert list(stage[own - 2:own]) == [N, N] and [_abi.AB_ROW_TYPES[t] for t in typ[own - 2:own]] == ["safe1", "safe2"]
    rc, _, stage, typ = rows.rows(classes, 1)
    assert rc == 0 and (stage >= 0).all() and (typ >= 0).all()          # the largest class has no padding
    # the rows of the small class are those of the large one without the four speed caps, in the same order
    caps = np.isin(typ, [_abi.AB_ROW[n] for n in ("v_lim", "v_curv", "v_stop", "v_tl")])
    assert caps.sum() == 4 * N
    _, _, s0, t0 = rows.rows(classes, 0)
    assert np.array_equal(s0[:own], stage[~caps]) and np.array_equal(t0[:own], typ[~caps])


@pytest.mark.parametrize("tree", ["ABO", "ORIG"])
@pytest.mark.parametrize("N", [2, 3, 20, 63])
def test_one_class_handle_has_the_order_of_ab_qp_rows(rows, tree, N):
    stage, names = T.row_map(tree, N)
    rc, _, got_s, got_t = rows.rows([(N, 0, int(tree == "ORIG"))], 0)
    assert rc == 0 and got_s.size == len(stage)
    assert np.array_equal(got_s, np.asarray(stage)) and [_abi.AB_ROW_TYPES[t] for t in got_t] == list(names)
    assert _abi.AB_ROW["blocked"] not in got_t                          # class handles have no move blocking


@pytest.mark.parametrize("tv", [False, True])
@pytest.mark.parametrize("N", [2, 20, 63])
def test_one_class_handle_has_the_order_of_bl_qp_rows(rows, tv, N):
    stage, typ = blr.rows_of(N, tv)
    rc, _, got_s, got_t = rows.rows([(N, 2 if tv else 1, 0)], 0)
    assert rc == 0 and np.array_equal(got_s, np.asarray(stage)) and np.array_equal(got_t, np.asarray(typ))


def test_cls_out_of_range(rows):
    classes = [(20, 0, 0), (20, 0, 1)]
    for cls in (-1, 2, 4096):
        rc, msg, stage, typ = rows.rows(classes, cls, nC=4)
        assert rc == -1 and msg == "eepacc_classes_qp_rows: cls = %d is outside [0, 2)" % cls
        assert (stage == 77).all() and (typ == 77).all()                # nothing written


# ------------------------------------------------------------------------------------------------ b2
def test_sanitized_host_program(tmp_path):
    exe = str(tmp_path / "classes_rows_sanitize")
    cmd = [cfg_harness.gxx(), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",        # the runtimes in the program itself: nothing to order or preload
           "-I", eb.CSRC, os.path.join(HERE, "kernels", "classes_rows_sanitize_main.cpp"), cfg_harness.UNIT, "-o", exe]
    subprocess.run(cmd, check=True, timeout=cfg_harness.COMPILE_TIMEOUT_S)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)


# ------------------------------------------------------------------------------------------------ b3
def _prototype(name):
    m = re.search(r"\bint\s+%s\s*\(([^;]*?)\)\s*;" % name, HDR)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype(param):
    typ = re.sub(r"\s*[A-Za-z_0-9]+$", "", param).replace("const ", "").replace(" ", "")
    return {"int": C.c_int, "int*": C.POINTER(C.c_int), "int32_t*": C.POINTER(C.c_int32), "double*": C.c_void_p,
            "void*": C.c_void_p, "eepacc_handle*": C.c_void_p}[typ]


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_argtypes(name):
    params = _prototype(name)
    got = _abi.CLASSES_BUILD_ARGTYPES[name]
    assert len(got) == len(params), (name, params)
    for p, g in zip(params, got):
        w = _ctype(p)
        assert w is g or w == g, (name, p, w, g)
    assert name in engine.ABI_SYMBOLS


def test_build_prototype_is_that_of_ab_build_qp_est():
    assert [p for p in _prototype("eepacc_classes_build_qp")] == _prototype("eepacc_ab_build_qp_est")
    assert _abi.CLASSES_BUILD_ARGTYPES["eepacc_classes_build_qp"] == _abi.AB_EST_ARGTYPES["eepacc_ab_build_qp_est"]
    assert _prototype("eepacc_classes_qp_size") == _prototype("eepacc_ab_qp_size")
    assert _prototype("eepacc_classes_qp_rows") == ["const eepacc_handle* h", "int cls", "int32_t* stage", "int32_t* type"]


def test_symbols_of_the_built_library():
    lib = C.CDLL(eb.build())
    for name in NAMES:
        assert hasattr(lib, name), name
    loaded = engine.load_library()
    for name in NAMES:
        assert getattr(loaded, name).argtypes == _abi.CLASSES_BUILD_ARGTYPES[name]


@pytest.mark.parametrize("unit,kernel", [("eepacc_ab_build_cls.hip", "k_ab_build_cls"), ("eepacc_bl_qp_cls.hip", "k_bl_qp_cls")])
def test_kernel_units_cross_compile_for_gfx950(tmp_path, unit, kernel):
    assert unit in eb.SOURCES
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = str(tmp_path / (unit + ".o"))
    cmd = [hipcc] + eb.BASE_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", os.path.join(eb.CSRC, unit), "-o", obj,
                                     '-DEEPACC_BUILD_FLAGS=""', "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(obj) > 0
    assert kernel in r.stderr                                           # the kernel is in the object
    assert len(re.findall(r"Function Name: ", r.stderr)) == 1          # one kernel per translation unit
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    print(re.findall(r"remark:\s+(.*?) \[-Rpass", r.stderr))
    assert m and int(m.group(1)) == 0                                   # a writer: no scratch, as the plain builders


# ------------------------------------------------------------------------------------------------ b4
def _bare_engine(N):
    """An Engine without a handle: the argument checks come before any use of the library or a device."""
    import torch
    e = engine.Engine.__new__(engine.Engine)
    e.torch, e.N, e.h = torch, N, None
    return e


def test_python_side_argument_errors():
    N, B = 20, 3
    e = _bare_engine(N)
    z = np.zeros(B); good = np.zeros((N + 1, B))
    with pytest.raises(ValueError, match="s_est and v_est"):
        e.classes_build_qp(z, z, z, z, z, z, z, s_est=good)
    with pytest.raises(ValueError, match="s_est and v_est"):
        e.classes_build_qp(z, z, z, z, v_est=good)
    with pytest.raises(ValueError, match=r"s_tv_est has shape \(20, 3\)"):
        e.classes_build_qp(z, z, z, z, z, z, z, s_tv_est=np.zeros((N, B)))


def test_lead_gradient_reads_every_instance_through_its_own_catalogue(monkeypatch):
    """ab_lead_gradient on a class engine: instance i is summed over the lead rows of class_of[i]'s catalogue; padding rows
    (type -1) and the rows of another class's layout contribute nothing.  The adjoint solve is replaced by a given dL/duba."""
    import torch
    N = 3
    cat = {0: T.row_map("ABO", N), 1: T.row_map("ORIG", N)}
    nC = len(cat[1][0])

    def catalogue(c):
        stage = np.full(nC, -1, dtype=np.int32); typ = np.full(nC, -1, dtype=np.int32)
        stage[:len(cat[c][0])] = cat[c][0]
        typ[:len(cat[c][0])] = [_abi.AB_ROW[n] for n in cat[c][1]]
        return stage, typ
    e = _bare_engine(N)
    e.class_of = np.array([1, 0, 0, 1], dtype=np.int32)
    e.classes_qp_rows = catalogue
    g_uba = torch.arange(4 * nC, dtype=torch.float64).reshape(4, nC) + 1.0
    monkeypatch.setattr(qp_sens, "qp_vjp", lambda eng, sol, H, A, gx: dict(uba=g_uba))

    class Q:
        H = torch.zeros(4, 5 * N, 5 * N); A = None
    got = qp_sens.ab_lead_gradient(e, Q, None, None, None).numpy()
    assert got.shape == (4, N + 1)
    for i, c in enumerate(e.class_of):
        stage, typ = catalogue(c)
        want = np.zeros(N + 1)
        for r in range(nC):
            if typ[r] in (_abi.AB_ROW["safe1"], _abi.AB_ROW["safe2"], _abi.AB_ROW["hwp"]):
                want[min(stage[r], N - 1)] += g_uba[i, r].item()
        assert np.array_equal(got[i], want), i
        assert got[i, N] == 0.0
    # an instance of the small class: what stands in its padding rows is not read
    pad = g_uba.clone(); pad[1, len(cat[0][0]):] = 1e9
    monkeypatch.setattr(qp_sens, "qp_vjp", lambda eng, sol, H, A, gx: dict(uba=pad))
    assert np.array_equal(qp_sens.ab_lead_gradient(e, Q, None, None, None).numpy()[1], got[1])
    # baseline classes are refused
    class Qbl:
        H = torch.zeros(4, 2 * N, 2 * N); A = None
    with pytest.raises(ValueError, match="ABMPC"):
        qp_sens.ab_lead_gradient(e, Qbl, None, None, None)
