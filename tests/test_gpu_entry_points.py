"""Contract of the C-ABI entry points that the shared host bodies of eepacc_capi.cpp and engine.py carry: host path equals
device path, which entry point runs on which kind of handle (with the refusal texts), argument checks, the resume rules,
and that a handle gives back all of its device memory.  Shapes are where dispatch and copy paths differ: N = 6 with B = 3
(small kernels, a partly filled block of four waves), N = 33 with B = 4 (large kernels of three waves per block, a second
partly filled block), 3 closed-loop steps."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import make_case, ROOT
from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV

pytestmark = pytest.mark.gpu

N_STEPS = 3


def _engine(kind, N, max_batch=4):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    OPT, V, *_ = make_case("ABO", N)
    OPT["TV_N_hor"] = N
    OPT = {"bl": Settings_BL, "tv": Settings_TV}.get(kind, dict)(OPT)
    return Engine(OPT, V, device=0, max_batch=max_batch)


def _scenario(B, lead_trace, n_steps=N_STEPS):
    sc = make_s2(B, n_steps, lead_trace["V_TO_2Hz"])
    return (sc["s0"], sc["v0"], sc["a_minus1"]), (sc["s_tv"], sc["v_tv"])


def _run(eng, kind, ins, lead, host=False, **kw):
    """run_<kind>mpc or its _host form with the arguments that controller takes."""
    fn = getattr(eng, "run_%smpc%s" % (kind, "_host" if host else ""))
    return fn(*ins, lead[0].shape[0], **kw) if kind == "tv" else fn(*ins, *lead, **kw)


def _np(pair):
    return tuple(x if isinstance(x, np.ndarray) else x.cpu().numpy() for x in pair)


@pytest.mark.parametrize("kind,N,B", [("ab", 6, 3), ("bl", 6, 3), ("fb", 6, 3), ("tv", 6, 3), ("ab", 33, 4), ("tv", 33, 4)])
def test_host_path_equals_device_path(kind, N, B, lead_trace):
    import torch
    eng = _engine(kind, N)
    ins, lead = _scenario(B, lead_trace)
    th, sh = _run(eng, kind, ins, lead, host=True)
    dev = lambda xs: [torch.as_tensor(x, device="cuda") for x in xs]
    td, sd = _np(_run(eng, kind, dev(ins), dev(lead)))
    eng.synchronize()
    assert (sd == 0).all() and (sh == 0).all(), (sd, sh)       # the comparison must not pass on failed solves
    assert sh.tobytes() == sd.tobytes()
    assert th.tobytes() == td.tobytes()


@pytest.mark.parametrize("kind", ["ab", "tv"])
def test_resume_equals_one_launch(kind, lead_trace):
    eng = _engine(kind, 6)
    ins, lead = _scenario(3, lead_trace)
    t1, s1 = _np(_run(eng, kind, ins, lead))
    assert (s1 == 0).all()
    ta, sa = _np(_run(eng, kind, ins, [x[:2] for x in lead]))
    tb, sb = _np(_run(eng, kind, ins, [x[2:] for x in lead], resume=True))
    eng.synchronize()
    assert np.concatenate([ta, tb]).tobytes() == t1.tobytes()
    assert np.concatenate([sa, sb]).tobytes() == s1.tobytes()


@pytest.mark.parametrize("kind", ["ab", "tv"])
def test_resume_with_another_batch_is_refused_until_reset(kind, lead_trace):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    eng = _engine(kind, 6)
    ins, lead = _scenario(3, lead_trace)
    _run(eng, kind, ins, lead)
    ins2, lead2 = _scenario(2, lead_trace)
    with pytest.raises(EepaccError, match="eepacc_run_%smpc: B changed while resuming; call eepacc_reset first" % ("tv" if kind == "tv" else "ab")):
        _run(eng, kind, ins2, lead2, resume=True)
    eng.reset()
    _, st = _np(_run(eng, kind, ins2, lead2, resume=True))
    eng.synchronize()
    assert (st == 0).all()


def test_fbmpc_runs_after_step_once_reset(lead_trace):
    eng = _engine("fb", 6)
    ins, lead = _scenario(3, lead_trace)
    z = np.zeros(3)
    eng.fb_step(ins[0], ins[1], z, z, z, z, z, lead[0][0], lead[1][0], z)
    eng.reset()
    _, st = _np(_run(eng, "fb", ins, lead, resume=True))
    eng.synchronize()
    assert (st == 0).all()


# Refusal texts of eepacc_capi.cpp by the bl_mode the handle was created with (None: the call runs).  eepacc_bl_step and
# eepacc_run_blmpc* check for a baseline handle first; the *_host wrappers of ABMPC / FBMPC refuse through the device entry
# point they call.
_TV_HANDLE = "%s: this handle was created with bl_mode = 2 (RunOpt_TVMPC); use eepacc_tv_step / eepacc_run_tvmpc"
_NOT_BL = "this handle was not created with bl_mode = 1 (RunOpt_BLMPC)"
_NOT_TV = "this handle was not created with bl_mode = 2 (RunOpt_TVMPC)"
ENTRY_TABLE = {
    "ab_step":        (None, None, _TV_HANDLE % "eepacc_ab_step"),
    "bl_step":        (_NOT_BL, None, _NOT_BL),
    "tv_step":        (_NOT_TV, _NOT_TV, None),
    "fb_step":        (None, None, _TV_HANDLE % "eepacc_fb_step"),
    "run_abmpc":      (None, None, _TV_HANDLE % "eepacc_run_abmpc"),
    "run_blmpc":      (_NOT_BL, None, _NOT_BL),
    "run_tvmpc":      (_NOT_TV, _NOT_TV, None),
    "run_fbmpc":      (None, None, _TV_HANDLE % "eepacc_run_fbmpc"),
    "run_abmpc_host": (None, None, _TV_HANDLE % "eepacc_run_abmpc"),
    "run_blmpc_host": (_NOT_BL, None, _NOT_BL),
    "run_tvmpc_host": (_NOT_TV, _NOT_TV, None),
    "run_fbmpc_host": (None, None, _TV_HANDLE % "eepacc_run_fbmpc"),
}


@pytest.mark.parametrize("bl_mode", [0, 1, 2])
def test_every_entry_point_on_every_kind_of_handle(bl_mode, lead_trace):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    eng = _engine(["ab", "bl", "tv"][bl_mode], 6)
    ins, lead = _scenario(3, lead_trace)
    z = np.zeros(3)
    step_in = (ins[0], ins[1], z, z)                     # s, v, a_prev, t0
    step_lead = (lead[0][0], lead[1][0], z)
    calls = {
        "ab_step": lambda: eng.ab_step(*step_in, *step_lead),
        "bl_step": lambda: eng._step(eng.lib.eepacc_bl_step, step_in + step_lead, True),
        "tv_step": lambda: eng.tv_step(*step_in),
        "fb_step": lambda: eng.fb_step(ins[0], ins[1], z, z, z, z, z, *step_lead),
    }
    for kind in ("ab", "bl", "tv", "fb"):
        for host in (False, True):
            calls["run_%smpc%s" % (kind, "_host" if host else "")] = lambda kind=kind, host=host: _run(eng, kind, ins, lead, host=host)
    assert set(calls) == set(ENTRY_TABLE)
    for name, call in calls.items():
        eng.reset()
        refusal = ENTRY_TABLE[name][bl_mode]
        if refusal is None:
            call()
            eng.synchronize()
        else:
            with pytest.raises(EepaccError) as ei:
                call()
            assert refusal in str(ei.value), (name, str(ei.value))


EINVAL = -1


def test_argument_checks_through_ctypes(lead_trace):
    import torch
    B = 3
    buf = torch.zeros(64 * B, dtype=torch.float64, device="cuda")
    st = torch.zeros(8 * B, dtype=torch.int32, device="cuda")
    d, s = buf.data_ptr(), st.data_ptr()
    for kind, step, n_in in (("ab", "eepacc_ab_step", 7), ("tv", "eepacc_tv_step", 4), ("fb", "eepacc_fb_step", 10)):
        eng = _engine(kind, 6)
        lib, h = eng.lib, eng.h
        err = lambda: lib.eepacc_last_error().decode()
        stepf, run = getattr(lib, step), getattr(lib, "eepacc_run_%smpc" % kind)
        n_run = 3 if kind == "tv" else 5
        # a NULL required buffer: every input in turn, then out and status (s_pred / v_pred may be NULL)
        for i in range(n_in + 4):
            if kind == "fb" and i in (2, 4, 5) or i in (n_in + 1, n_in + 2):
                continue                                  # v_prev, Fm_prev, Fb_prev are accepted and unused
            a = [d] * n_in + [d, None, None, s]
            a[i] = None
            assert stepf(h, B, *a, None) == EINVAL and err() == step + ": NULL buffer", (step, i, err())
        for i in range(n_run + 2):
            a = [d] * n_run + [d, s]
            a[i] = None
            assert run(h, B, 1, *a, None) == EINVAL and err() == "eepacc_run_%smpc: NULL buffer" % kind, (kind, i, err())
        # B above max_batch (4), and B = 0, which returns before it looks at a buffer
        assert stepf(h, 5, *([d] * n_in), d, None, None, s, None) == EINVAL and err() == "B exceeds max_batch of the handle"
        assert run(h, 5, 1, *([d] * n_run), d, s, None) == EINVAL and err().endswith("bad B / n_steps")
        assert stepf(h, 0, *([None] * (n_in + 4)), None) == 0
        assert run(h, 0, 1, *([None] * (n_run + 2)), None) == 0
        eng.synchronize()
    # a baseline handle by name reports as the ABMPC entry point it stands for
    eng = _engine("bl", 6)
    assert eng.lib.eepacc_bl_step(eng.h, B, *([d] * 6), None, d, None, None, s, None) == EINVAL
    assert eng.lib.eepacc_last_error().decode() == "eepacc_ab_step: NULL buffer"
    assert (st == 0).all() and (buf == 0).all()           # nothing was launched


_CHILD = r"""
import ctypes as C, os, sys
import numpy as np, torch
sys.path.insert(0, os.path.join(sys.argv[1], "tests")); sys.path.insert(0, sys.argv[1])
from conftest import make_case
from eepacc_mpc_casadi_matlab_amd.engine import Engine, load_library
from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV
lib = load_library()
def used():
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free
def cycle(i):
    OPT, V, *_ = make_case("ABO", 6)
    OPT["TV_N_hor"] = 6
    if i % 3 == 1:
        OPT["fuel_map"] = "ICE"                           # ab_fuel_term = 2: the handle owns the base-inverse scratch
    elif i % 3 == 0:
        OPT = (dict, Settings_BL, Settings_TV)[i // 3 % 3](OPT)
    eng = Engine(OPT, V, device=0, max_batch=4096)        # most buffers of the handle above the allocation granule
    if i % 3 == 2:                                        # FBMPC handle, stepped once through the dense path
        z = np.zeros(3)
        eng.fb_step(z, z, z, z, z, z, z, z + 30.0, z, z)
        eng.synchronize()
    lib.eepacc_destroy(eng.h); eng.h = None
for i in range(3):                                        # code objects, the caching allocator: in place before the baseline
    cycle(i)
torch.cuda.empty_cache()
# what one hipMalloc of 1 byte costs: allocate until the device figure moves
lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]; lib.hipFree.argtypes = [C.c_void_p]
u0, ptrs, granule = used(), [], 0
while granule == 0 and len(ptrs) < 8192:
    p = C.c_void_p(); assert lib.hipMalloc(C.byref(p), 1) == 0
    ptrs.append(p); granule = used() - u0
for p in ptrs:
    assert lib.hipFree(p) == 0
start = used()
for i in range(20):
    cycle(i)
torch.cuda.empty_cache()
print("MEM", granule, start, used())
"""


def test_create_destroy_returns_device_memory():
    env = dict(os.environ, EEPACC_FB_DENSE="1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    granule, start, end = (int(x) for x in [l for l in r.stdout.splitlines() if l.startswith("MEM")][-1].split()[1:])
    print("granule %d B, in use before %d B, after 20 handles %d B" % (granule, start, end))
    assert granule > 0
    assert abs(end - start) <= granule, (granule, start, end)
