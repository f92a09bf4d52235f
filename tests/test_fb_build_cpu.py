"""eepacc_fb_build_qp without a GPU: the new kernel file compiles for gfx950 with the project's flags, the ctypes mirror
agrees with include/eepacc.h (prototypes and the EEPACC_FB_ROW_* enum), and the header points to the entry instead of
saying that the FBMPC problem is not built."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT
from eepacc_mpc_casadi_matlab_amd import _abi, engine
from eepacc_mpc_casadi_matlab_amd import build as eb

HDR = open(os.path.join(ROOT, "include", "eepacc.h")).read()
NAMES = ["eepacc_fb_qp_size", "eepacc_fb_qp_rows", "eepacc_fb_build_qp"]


def test_kernel_file_cross_compiles_for_gfx950(tmp_path):
    assert "eepacc_fb_qp.hip" in eb.SOURCES
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    obj = str(tmp_path / "eepacc_fb_qp.o")
    cmd = [hipcc] + eb.BASE_FLAGS + ["-x", "hip", "--cuda-device-only", "-c", os.path.join(eb.CSRC, "eepacc_fb_qp.hip"), "-o", obj,
                                     '-DEEPACC_BUILD_FLAGS=""', "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(obj) > 0
    assert "k_fb_qp" in r.stderr                                        # the kernel is in the object
    m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)
    print(re.findall(r"remark:\s+(.*?) \[-Rpass", r.stderr))
    assert m and int(m.group(1)) == 0                                   # the issue's aim: no scratch


def _prototype(name):
    m = re.search(r"^int\s+%s\s*\(([^;]*)\);" % name, HDR, re.M)
    assert m, name
    return [p.strip() for p in " ".join(m.group(1).split()).split(",")]


def _ctype(decl):
    decl = re.sub(r"\bconst\b", " ", decl).strip()
    typ = re.sub(r"\s*[A-Za-z_][A-Za-z_0-9]*$", "", decl).replace(" ", "")
    return {"int": C.c_int, "int*": C.POINTER(C.c_int), "int32_t*": C.POINTER(C.c_int32), "double*": C.c_void_p,
            "void*": C.c_void_p, "eepacc_handle*": C.c_void_p}[typ]


@pytest.mark.parametrize("name", NAMES)
def test_prototype_matches_argtypes(name):
    params = _prototype(name)
    got = _abi.FB_BUILD_ARGTYPES[name]
    assert len(got) == len(params), (name, params)
    for p, g in zip(params, got):
        w = _ctype(p)
        assert w is g or w == g, (name, p, w, g)
    assert name in engine.ABI_SYMBOLS


def test_build_prototype_as_the_issue_states_it():
    params = _prototype("eepacc_fb_build_qp")
    names = [re.search(r"([A-Za-z_0-9]+)$", p).group(1) for p in params]
    assert names == ["h", "B", "s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev", "A22", "D2",
                     "H", "g", "A", "lba", "uba", "A22_used", "D2_used", "stream"]
    for p in params[2:11]:
        assert p.startswith("const double*"), p
    for p in params[11:18]:
        assert p.startswith("double*"), p


def test_row_types_match_the_header_enum():
    m = re.search(r"enum\s*\{\s*EEPACC_FB_ROW_S = 0,(.*?)EEPACC_FB_ROW_N\s*\}", HDR, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", "EEPACC_FB_ROW_S," + m.group(1), flags=re.S)
    names = [x.strip() for x in body.split(",") if x.strip()]
    assert all(n.startswith("EEPACC_FB_ROW_") and "=" not in n for n in names)
    assert [n[len("EEPACC_FB_ROW_"):].lower() for n in names] == _abi.FB_ROW_TYPES
    assert _abi.FB_ROW == {n: i for i, n in enumerate(_abi.FB_ROW_TYPES)}
    # 26 rows every stage has (CreateQP_FB.m:311-473) and the two blocked-move rows
    assert len(_abi.FB_ROW_TYPES) == 28
    assert _abi.FB_ROW_TYPES[8:10] == ["blocked_fm", "blocked_fb"]
    # every entry of the enum cites its lines of CreateQP_FB.m, on its own line or on that of the group it belongs to
    cited = re.findall(r":(\d+)-(\d+)", m.group(1))
    for lines in ("311-342", "346-356", "359-366", "369-377", "380-387", "390-397", "400-418", "421-442", "445-448", "451-458",
                  "461-473"):
        assert tuple(lines.split("-")) in cited, lines


def test_header_no_longer_says_not_built():
    assert "Not built: the FBMPC problem" not in HDR
    assert not re.search(r"Not built:[^.]*FBMPC problem", HDR)
    ab = HDR[HDR.index("The condensed QP of one ABMPC step as data"):HDR.index("int  eepacc_ab_qp_size")]
    assert "eepacc_fb_build_qp" in ab                                  # the AB comment points to the new entry
