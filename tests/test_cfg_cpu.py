"""The settings translation of csrc/eepacc_cfg.cpp (validation, move-blocking maps, condensed Hessian and its inverse, the
key-figure tables), called on the host through tests/cfg_harness.py: no GPU, no libeepacc.so except where a test compares
the two."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import cfg_harness
from conftest import make_case, GOLDEN_AB_ICEMAP
from eepacc_mpc_casadi_matlab_amd import build as eb
from eepacc_mpc_casadi_matlab_amd import engine
from eepacc_mpc_casadi_matlab_amd._abi import SettingsHolder, make_vehicle
from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL, Settings_TV

HERE = os.path.dirname(os.path.abspath(__file__))
EINVAL, ENOTSUP = -1, -4
MB20 = [0, 1, 0, 0, 1, 1, 0, 0, 0, 1, 0, 1, 1, 1, 0, 0, 1, 0, 0, 1]


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    with pytest.MonkeyPatch.context() as mp:
        for name in ("EEPACC_DEBUG_BL_MAX_ITER", "EEPACC_DEBUG_BL_EPS"):       # debug overrides that build_cfg reads
            mp.delenv(name, raising=False)
        yield cfg_harness.load(str(tmp_path_factory.mktemp("cfg_harness")))


def cases():
    """name -> (OPT, V): the settings whose translation is pinned byte for byte (tests/cfg_digests.json)."""
    orig, Vo, *_ = make_case("ORIG", 20)
    abo, V, *_ = make_case("ABO", 20)
    ice = make_case("ABO", 20, **GOLDEN_AB_ICEMAP)[0]
    tvec = 0.5 + 0.05 * np.arange(20)
    tvec[7] = 0.3
    return {
        "orig20": (orig, Vo),
        "abo20": (abo, V),
        "abo20_mb": (dict(abo, Mb=np.array(MB20, dtype=np.int32)), V),
        "abo20_ice": (ice, V),
        "abo20_ice_mb": (dict(ice, Mb=np.array(MB20, dtype=np.int32)), V),
        "bl_quadratic": (Settings_BL(dict(abo, W_BL=np.array([1e2, 3.0, 10.0, 1e7]))), V),
        "bl_lp": (Settings_BL(abo), V),
        "tv": (Settings_TV(abo), V),
        "abo20_tvec": (dict(abo, Tvec=tvec), V),
        "abo20_est2": (dict(abo, paramEstSetting=2), V),
        "abo2": (make_case("ABO", 2)[0], V),
        "abo63": (make_case("ABO", 63)[0], V),
    }


@pytest.fixture(scope="module")
def built(H):
    out = {}
    for name, (OPT, V) in cases().items():
        out[name] = H.build(OPT, V)
        assert out[name].rc == 0, (name, out[name].msg)
    return out


def test_bytes_unchanged(H, built):
    """DevCfg (zeroed first, device pointers null), Hinv, KpiCfg and FollowCfg of every case hash to what the translation
    produced while it was part of eepacc_capi.cpp (digests recorded there, before the move)."""
    with open(os.path.join(HERE, "cfg_digests.json")) as f:
        want = json.load(f)
    assert want["sizeof"] == {"DevCfg": H.sizeof_devcfg, "KpiCfg": H.sizeof_kpi, "FollowCfg": H.sizeof_follow}
    assert sorted(want["cases"]) == sorted(built)
    for name, b in built.items():
        for ptr in ("Hinv", "pred", "hb"):
            assert not b.field(ptr, np.uint64)[0], (name, ptr)
        assert b.digests() == want["cases"][name], name


def _hessian(OPT, V):
    """The a-space Hessian from its definition: H = 2 cq Sv'Sv + (2 w_a + bl_eps) I + 2 w_j D' diag(1 / T^2) D with the
    speed map Sv (v_k = v_0 + sum_{i<k} T_i a_i, k = 1 .. N-1) and the first difference D; with Mb folded as E'HE on the
    block leaders, identity on the other stages."""
    N, T = int(OPT["N_hor"]), np.asarray(OPT["Tvec"], dtype=np.float64)
    bl_eps = 0.0
    if OPT.get("bl_mode", 0):
        cq, w_a, w_j = 0.0, float(OPT["W_BL"][1]), float(OPT["W_BL"][2])
        if w_a == 0.0 and w_j == 0.0:
            bl_eps = 0.1
    else:
        W = np.asarray(OPT["W_AB"], dtype=np.float64)
        w_FC, w_a, w_j = (W[0], W[1], W[2]) if W.size == 7 else (0.0, W[0], W[1])
        cq = 0.0 if OPT.get("fuel_map", "EFF") == "ICE" else w_FC * V["p01"] * V["F2"]
    Sv = np.zeros((N, N))
    for k in range(1, N):
        Sv[k, :k] = T[:k]
    D = np.eye(N) - np.eye(N, k=-1)
    Hm = 2.0 * cq * Sv.T @ Sv + (2.0 * w_a + bl_eps) * np.eye(N) + 2.0 * w_j * D.T @ np.diag(1.0 / T ** 2) @ D
    Mb = np.asarray(OPT.get("Mb", np.zeros(N)), dtype=int)
    if Mb.any():
        lead = [k for k in range(N)]
        for k in range(1, N):
            if Mb[k]:
                lead[k] = lead[k - 1]
        E = np.zeros((N, N))
        E[np.arange(N), lead] = 1.0
        Hm = E.T @ Hm @ E
        for k in range(N):
            if lead[k] != k:
                Hm[k, k] = 1.0
    return Hm


def _residual(Hm, X):
    """max |H X - I|, the product formed in extended precision so that the figure is the error of X and not that of the
    product: in double, rounding the N-term sums adds the same noise to either inverse and can decide the comparison."""
    R = Hm.astype(np.longdouble) @ X.astype(np.longdouble) - np.eye(Hm.shape[0], dtype=np.longdouble)
    return float(np.abs(R).max())


# Room over "no larger than numpy's" that a case gets.  The residual is measured on the test's H, assembled in double; the
# code assembles the same entries in long double and inverts that matrix.  With the uniform T = 0.5 every T_i T_j and 1 / T^2
# is exact, so both inverses are of one matrix.  With the non-uniform grid each entry of the test's H carries several double
# roundings (T_i T_j, the N-term sums of Sv'Sv, 1 / T_k^2) that numpy's inverse follows and the code's cannot: on top of the
# u max(|H| |Hinv|) of rounding the exact inverse to double comes a second term |dH| |Hinv| of the same size.  Measured there:
# 3.366e-16 against numpy's 2.991e-16, with u max(|H| |Hinv|) = 7.7e-16.
HINV_ROOM = {"abo20_tvec": 2.0}


@pytest.mark.parametrize("name", ["orig20", "abo20", "abo20_mb", "abo20_tvec", "bl_lp", "abo2", "abo63"])
def test_hinv_against_independent_assembly(built, name):
    """Hinv is exactly symmetric and inverts the independently assembled H no worse than numpy's double-precision inverse
    of the same matrix: both are inverses rounded to double, and Hinv is computed in extended precision."""
    OPT, V = cases()[name]
    Hinv = built[name].Hinv
    assert np.array_equal(Hinv, Hinv.T)
    Hm = _hessian(OPT, V)
    ours, numpys = _residual(Hm, Hinv), _residual(Hm, np.linalg.inv(Hm))
    print("%s: max|H Hinv - I| = %.3e, numpy.linalg.inv: %.3e" % (name, ours, numpys))
    assert ours <= HINV_ROOM.get(name, 1.0) * numpys, "%s: max|H Hinv - I| = %.3e, numpy.linalg.inv: %.3e" % (name, ours, numpys)


def test_move_blocking_maps_by_hand(H):
    OPT, V, *_ = make_case("ABO", 6)
    b = H.build(dict(OPT, Mb=np.array([0, 1, 1, 0, 0, 1], dtype=np.int32)), V)
    assert b.rc == 0, b.msg
    assert b.field("mb_any")[0] == 1
    assert b.field("mb_lead")[:7].tolist() == [0, 0, 0, 3, 4, 4, 6]
    assert b.field("mb_end")[:7].tolist() == [2, 1, 2, 3, 5, 5, 6]
    assert b.field("mb_maxlen")[0] == 3
    assert b.field("mb_mask")[:7].tolist() == [0, 1, 1, 0, 0, 1, 0]
    assert b.field("fb_row0")[:7].tolist() == [0, 26, 54, 82, 108, 134, 162]


@pytest.mark.parametrize("null_mb", [False, True])
def test_no_move_blocking_and_time_grid(H, null_mb):
    N = 9
    OPT, V, *_ = make_case("ABO", N)
    T = np.array([0.5, 0.25, 0.1, 0.7, 0.3, 0.9, 1.1, 0.2, 0.6])
    OPT = dict(OPT, Tvec=T, Mb=np.zeros(N, dtype=np.int32))
    b = H.build(OPT, V, (lambda pod, veh, holder: setattr(pod, "Mb", type(pod.Mb)())) if null_mb else None)
    assert b.rc == 0, b.msg
    assert b.field("mb_any")[0] == 0 and b.field("mb_maxlen")[0] == 1
    assert b.field("mb_lead")[:N + 1].tolist() == list(range(N + 1))
    assert b.field("mb_end")[:N + 1].tolist() == list(range(N + 1))
    assert b.field("mb_mask")[:N + 1].tolist() == [0] * (N + 1)
    assert b.field("fb_row0")[:N + 1].tolist() == [26 * k for k in range(N + 1)]
    tau = [0.0]
    for t in T:
        tau.append(tau[-1] + float(t))
    assert b.field("tau")[:N + 1].tolist() == tau
    assert b.field("Tvec")[:N].tolist() == T.tolist()
    assert b.field("const_T")[0] == 0 and b.field("const_slope")[0] == 1
    u = H.build(dict(OPT, Tvec=0.25 * np.ones(N), s_slope=np.array([0.0, 500.0]), slope=np.array([0.0, 0.02])), V)
    assert u.rc == 0, u.msg
    assert u.field("const_T")[0] == 1 and u.field("const_slope")[0] == 0


def _refusals():
    """(id, base settings, changes to OPT, to V, to the POD after packing (None: a null pointer), code, text): one row per
    refusal of build_cfg, written from the text of eepacc_capi.cpp before the move."""
    tv_T = 0.5 * np.ones(20)
    tv_T[3] = 1.0
    T0 = 0.5 * np.ones(20)
    T0[11] = 0.0
    sizes = "route table sizes out of range"
    return [
        ("N_hor_1", "abo", {}, {}, {"N_hor": 1}, EINVAL, "N_hor must be in [2, 63]"),
        ("N_hor_64", "abo", {}, {}, {"N_hor": 64}, EINVAL, "N_hor must be in [2, 63]"),
        ("Tvec_null", "abo", {}, {}, {"Tvec": None}, EINVAL, "Tvec is NULL"),
        ("Tvec_zero_entry", "abo", {"Tvec": T0}, {}, {}, EINVAL, "Tvec entries must be positive"),
        ("solverToUse_2", "abo", {"solverToUse": 2}, {}, {}, ENOTSUP, "solverToUse == 2 (HPIPM formulation, ABO/Settings.m:114) is not built"),
        ("paramEstSetting_3", "abo", {"paramEstSetting": 3}, {}, {}, EINVAL, "paramEstSetting must be 0, 1 or 2"),
        ("TVestSetting_2", "abo", {"TVestSetting": 2}, {}, {}, EINVAL, "TVestSetting must be 0 or 1"),
        ("n_speedLim_65", "abo", {}, {}, {"n_speedLim": 65}, EINVAL, sizes),
        ("n_speedLim_0", "abo", {}, {}, {"n_speedLim": 0}, EINVAL, sizes),
        ("n_curv_65", "abo", {}, {}, {"n_curv": 65}, EINVAL, sizes),
        ("n_slope_65", "abo", {}, {}, {"n_slope": 65}, EINVAL, sizes),
        ("n_stop_17", "abo", {}, {}, {"n_stop": 17}, EINVAL, sizes),
        ("n_TL_9", "abo", {}, {}, {"n_TL": 9}, EINVAL, sizes),
        ("N_integratePlant_0", "abo", {"N_integratePlant": 0}, {}, {}, EINVAL, "N_integratePlant < 1"),
        ("ab_fuel_term_3", "abo", {}, {}, {"ab_fuel_term": 3}, EINVAL, "ab_fuel_term must be 0, 1 or 2"),
        ("ice_tau_fd_0", "ice", {}, {"tau_fd": 0.0}, {}, EINVAL, "ab_fuel_term == 2 needs V.tau_fd, V.eta_drive, V.R_w > 0"),
        ("ice_gear_ratio_0", "ice", {}, {"tau_gb": np.array([4.714, 3.314, 0.0, 1.667, 1.285, 1, 0.839, 0.667])}, {}, EINVAL,
         "ab_fuel_term == 2 needs positive gear ratios V.tau_gb"),
        ("ice_upSpd_descending", "ice", {}, {"upSpd": np.array([4.0, 6.0, 8.0, 7.0, 14.0, 18.0, 22.0])}, {}, EINVAL, "V.upSpd must ascend"),
        ("Mb0_1", "abo", {"Mb": [1, 0] * 10}, {}, {}, EINVAL, "Mb[0] must be 0 (the first stage has no predecessor in the horizon)"),
        ("Mb_entry_2", "abo", {"Mb": [0, 0, 2] + [0] * 17}, {}, {}, EINVAL, "Mb entries must be 0 or 1"),
        ("bl_mode_3", "abo", {"bl_mode": 3}, {}, {}, EINVAL, "bl_mode must be 0, 1 (RunOpt_BLMPC) or 2 (RunOpt_TVMPC)"),
        ("bl_with_Mb", "bl", {"Mb": [0, 1] * 10}, {}, {}, ENOTSUP, "the baseline controller has no move blocking (RunOpt_BLMPC.m)"),
        ("tv_nonuniform_Tvec", "tv", {"Tvec": tv_T}, {}, {}, EINVAL, "bl_mode = 2: Tvec must be uniform (TV_Ts, CreateQP_TV.m:29)"),
        ("W_BL_negative", "bl", {"W_BL": np.array([1e2, -1.0, 0.0, 1e7])}, {}, {}, EINVAL, "W_BL weights must be non-negative (w_f positive)"),
        ("bl_limit_0", "bl", {"BL_j_LimLowVel": 0.0}, {}, {}, EINVAL, "baseline acceleration / jerk limits must be positive"),
        ("w_a_0", "abo", {"W_AB": np.array([1.0, 0.0, 1.0, 1.0, 1.0, 1.0, 1.0])}, {}, {}, EINVAL,
         "W_AB weights must be positive (w_a, w_h) / non-negative"),
        # w_FC is the one weight without a sign check: a negative one makes 2 cq Sv'Sv outweigh 2 w_a I
        ("hessian_not_spd", "abo", {"W_AB": np.array([-1e6, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0])}, {}, {}, EINVAL,
         "condensed Hessian is not positive definite"),
    ]


REFUSALS = _refusals()
ALSO_THROUGH_THE_LIBRARY = ("N_hor_64", "ice_gear_ratio_0", "bl_with_Mb", "hessian_not_spd")


def _packed(row):
    _, base, d_opt, d_veh, d_pod, _, _ = row
    abo, V, *_ = make_case("ABO", 20)
    OPT = {"abo": abo, "ice": dict(abo, **GOLDEN_AB_ICEMAP), "bl": Settings_BL(abo), "tv": Settings_TV(abo)}[base]
    holder, veh = SettingsHolder(dict(OPT, **d_opt)), make_vehicle(dict(V, **d_veh))
    for key, val in d_pod.items():
        setattr(holder.pod, key, type(getattr(holder.pod, key))() if val is None else val)
    return holder, veh


@pytest.mark.parametrize("row", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_every_refusal(H, row):
    """Every `return fail(...)` of build_cfg, with its code and text.  The last row reaches the positive-definiteness check
    of the inverse through a negative w_FC."""
    holder, veh = _packed(row)
    b = H.build_pod(holder.pod, veh)
    assert b.rc == row[5] and row[6] in b.msg, (b.rc, b.msg)


@pytest.mark.parametrize("name", ALSO_THROUGH_THE_LIBRARY)
def test_refusal_through_the_library(H, name):
    """eepacc_create refuses before it touches a device, with the code and the whole message of the harness."""
    eb.build()
    lib = engine.load_library()
    row = [r for r in REFUSALS if r[0] == name][0]
    holder, veh = _packed(row)
    b = H.build_pod(holder.pod, veh)
    h = C.c_void_p()
    rc = lib.eepacc_create(C.byref(h), C.byref(holder.pod), C.byref(veh), 0, 16)
    assert not h.value
    assert (rc, lib.eepacc_last_error().decode()) == (b.rc, b.msg) and rc == row[5]


def test_sanitized_host_program(tmp_path):
    """tests/kernels/cfg_sanitize_main.cpp calls the three builders at the edges of the fixed arrays (N = 63 with every stage
    but the first blocked, full route tables, ICE map) and with each table one entry too long, as a program of its own under
    AddressSanitizer and UndefinedBehaviorSanitizer."""
    exe = str(tmp_path / "cfg_sanitize")
    cmd = [cfg_harness.gxx(), "-std=c++17", "-Wall", "-Wextra", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan",        # the runtimes in the program itself: nothing to order or preload
           "-I", eb.CSRC, os.path.join(HERE, "kernels", "cfg_sanitize_main.cpp"), cfg_harness.UNIT, "-o", exe]
    subprocess.run(cmd, check=True, timeout=cfg_harness.COMPILE_TIMEOUT_S)
    env = {k: v for k, v in os.environ.items() if k not in ("EEPACC_DEBUG_BL_MAX_ITER", "EEPACC_DEBUG_BL_EPS")}
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stderr == "", (r.returncode, r.stdout, r.stderr)
