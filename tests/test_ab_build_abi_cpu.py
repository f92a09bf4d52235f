"""The C prototypes of the entry points that build the condensed QP of an ABMPC step (include/eepacc.h) against their
ctypes mirror in _abi.py, and the header's row-type enum against AB_ROW_TYPES.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from eepacc_mpc_casadi_matlab_amd import _abi, engine
from eepacc_mpc_casadi_matlab_amd import build as eb

HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
NAMES = ["eepacc_ab_qp_size", "eepacc_ab_qp_rows", "eepacc_ab_build_qp"]


def _ctype(decl):
    """ctypes type of one parameter declaration as the mirror writes it."""
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    typ = re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", decl).replace(" ", "")      # drop the parameter's name
    table = {"int": C.c_int, "int*": C.POINTER(C.c_int), "int32_t*": C.POINTER(C.c_int32),
             "double*": C.c_void_p,             # device arrays travel as addresses (tensor.data_ptr())
             "void*": C.c_void_p, "eepacc_handle*": C.c_void_p}
    return table[typ]


def _prototype(name):
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, HDR, re.M)
    assert m, name
    return [p.strip() for p in " ".join(m.group(1).split()).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_argtypes(name):
    params = _prototype(name)
    want = [_ctype(p) for p in params]
    got = _abi.AB_BUILD_ARGTYPES[name]
    assert len(got) == len(want), (name, params)
    for p, w, g in zip(params, want, got):
        assert w is g or w == g, (name, p, w, g)
    assert name in engine.ABI_SYMBOLS


def test_prototypes_as_the_issue_states_them():
    assert [len(_prototype(n)) for n in NAMES] == [3, 3, 15]
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in _prototype("eepacc_ab_build_qp")]
    assert names == ["h", "B", "s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev", "H", "g", "A", "lba", "uba", "stream"]
    # inputs are const, outputs are not
    for p in _prototype("eepacc_ab_build_qp")[2:9]:
        assert p.startswith("const double*"), p
    for p in _prototype("eepacc_ab_build_qp")[9:14]:
        assert p.startswith("double*"), p


def test_row_types_match_the_header_enum():
    m = re.search(r"enum\s*\{\s*EEPACC_AB_ROW_S = 0,(.*?)EEPACC_AB_ROW_N\s*\}", HDR, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", "EEPACC_AB_ROW_S," + m.group(1), flags=re.S)
    names = [x.strip() for x in body.split(",") if x.strip()]
    assert all(n.startswith("EEPACC_AB_ROW_") and "=" not in n for n in names)
    assert [n[len("EEPACC_AB_ROW_"):].lower() for n in names] == _abi.AB_ROW_TYPES
    assert _abi.AB_ROW == {n: i for i, n in enumerate(_abi.AB_ROW_TYPES)}
    # the row types the issue names: bounds on s, v and the four slacks, blocked move, a and j limits, the four ORIG speed
    # caps, speed incentive, the two safe distances, headway policy
    assert len(_abi.AB_ROW_TYPES) == 19


def test_library_exports_and_refuses_a_null_handle():
    from eepacc_mpc_casadi_matlab_amd import build as eb
    eb.build()
    lib = engine.load_library()
    for n in NAMES:
        assert hasattr(lib, n) and getattr(lib, n).argtypes == _abi.AB_BUILD_ARGTYPES[n]
    a, b = C.c_int(), C.c_int()
    assert lib.eepacc_ab_qp_size(None, C.byref(a), C.byref(b)) == -1
    assert lib.eepacc_last_error().decode() == "eepacc_ab_qp_size: NULL handle"
    assert lib.eepacc_ab_build_qp(None, 1, *([None] * 12), None) == -1
    assert lib.eepacc_last_error().decode() == "eepacc_ab_build_qp: NULL handle"


def test_kernel_file_cross_compiles_for_gfx950(tmp_path):
    """As the FB and BL builders' CPU tests do for their units: the unit compiles for the device on its own, the kernel is in
    the object and keeps nothing in scratch."""
    assert "eepacc_ab_build.hip" in eb.SOURCES
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = str(tmp_path / "eepacc_ab_build.o")
    cmd = [hipcc] + eb.BASE_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", os.path.join(eb.CSRC, "eepacc_ab_build.hip"), "-o", obj,
                                     '-DEEPACC_BUILD_FLAGS=""', "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(obj) > 0
    assert "k_ab_build" in r.stderr                                     # the kernel is in the object
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    print(re.findall(r"remark:\s+(.*?) \[-Rpass", r.stderr))
    assert m and int(m.group(1)) == 0
