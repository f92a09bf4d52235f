"""ctypes mirror of include/eepacc.h (struct layouts and enum values only)."""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict

import numpy as np

c_double_p = C.POINTER(C.c_double)
c_int32_p = C.POINTER(C.c_int32)

EEPACC_MAX_HORIZON = 63
EEPACC_MAX_CLASSES = 4096

OUT_FIELDS = ["s", "v", "Fm", "Fb", "a", "xi_v", "xi_h", "xi_s", "xi_f", "cost", "DistHor", "a_qp"]
OUT_N = len(OUT_FIELDS)
OUT = {name: i for i, name in enumerate(OUT_FIELDS)}

# enum EEPACC_KPI_*: rows of the table of eepacc_kpis, raw SI units
KPI_FIELDS = ["bad_exits", "distance_m", "energy_J", "cutoff_index", "reached", "vlim_err", "energy_cutoff_J", "time_cutoff_s",
              "a_max", "a_min", "a_rms", "j_max", "j_min", "j_rms", "fuel_kg", "FE_L_per_100km"]
KPI_N = len(KPI_FIELDS)
KPI = {name: i for i, name in enumerate(KPI_FIELDS)}
KPI_WAVES = 16        # EEPACC_KPI_WAVES
KPI_MIN_SLICE = 8     # EEPACC_KPI_MIN_SLICE

# enum EEPACC_FKPI_*: rows of the table of eepacc_follow_kpis, raw SI units, and the values of its `weights` argument
FKPI_FIELDS = ["lead_samples", "h_min_m", "h_min_index", "thw_min_s", "margin_min_m", "margin_viol_steps", "ttc_min_s", "xi_h_max",
               "cost_P", "cost_a", "cost_j", "cost_xi_v", "cost_xi_h", "cost_xi_s", "cost_xi_f"]
FKPI_N = len(FKPI_FIELDS)
FKPI = {name: i for i, name in enumerate(FKPI_FIELDS)}
FKPI_WEIGHTS = {"ab": 0, "fb": 1, "none": 2}      # EEPACC_FKPI_W_AB, _W_FB, _W_NONE

# enum EEPACC_RKPI_*: rows of the table of eepacc_route_kpis, raw SI units; enum EEPACC_RLIM_*: the caps of its `limits`
RKPI_FIELDS = ["vlim_excess_max", "vlim_excess_index", "vlim_viol_steps", "vcurv_excess_max", "vcurv_viol_steps",
               "vstop_excess_max", "vstop_viol_steps", "vtl_excess_max", "vtl_viol_steps", "stops_passed", "stop_cross_v_max",
               "tl_passed", "red_crossings", "red_crossings_possible", "red_cross_first_index",
               "a_over_max", "a_under_max", "j_over_max", "j_under_max", "comfort_viol_steps", "v_min"]
RKPI_N = len(RKPI_FIELDS)
RKPI = {name: i for i, name in enumerate(RKPI_FIELDS)}
RLIM_FIELDS = ["v_lim", "v_curv", "v_stop", "v_tl"]
RLIM_N = len(RLIM_FIELDS)
RLIM = {name: i for i, name in enumerate(RLIM_FIELDS)}
# eepacc_route_kpis(h, B, n_steps, t_start, tol_host, traj, status, rkpi, limits, stream); device arrays travel as addresses
ROUTE_KPIS_ARGTYPES = [C.c_void_p, C.c_int, C.c_int, C.c_double, c_double_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]

# enum EEPACC_AB_ROW_*: the row types of eepacc_ab_qp_rows, ascending in the order of the rows within a stage
AB_ROW_TYPES = ["s", "v", "xi_v", "xi_h", "xi_s", "xi_f", "blocked", "a_max", "a_min", "j_max", "j_min",
                "v_lim", "v_curv", "v_stop", "v_tl", "v_inc", "safe1", "safe2", "hwp"]
AB_ROW = {name: i for i, name in enumerate(AB_ROW_TYPES)}

# argument types of the entry points that build the condensed QP of an ABMPC step; device arrays travel as addresses
AB_BUILD_ARGTYPES = {
    "eepacc_ab_qp_size": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "eepacc_ab_qp_rows": [C.c_void_p, c_int32_p, c_int32_p],
    "eepacc_ab_build_qp": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 5 + [C.c_void_p],
}

# the entry points that take the horizon guesses s_est, v_est, s_tv_est (each may be None) after the seven step inputs, and
# the closed loop that reads the lead's guess from the lead trace (B, n_steps, n_lead)
AB_EST_ARGTYPES = {
    "eepacc_ab_step_est": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 3 + [C.c_void_p] * 4 + [C.c_void_p],
    "eepacc_ab_build_qp_est": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 3 + [C.c_void_p] * 5 + [C.c_void_p],
    "eepacc_run_abmpc_preview": [C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p] * 2 + [C.c_void_p],
}
# the baseline controller's counterparts (a handle with bl_mode = 1): arguments and order are those of the AB entries
BL_EST_ARGTYPES = {name.replace("eepacc_ab_", "eepacc_bl_").replace("abmpc", "blmpc"): list(argtypes)
                   for name, argtypes in AB_EST_ARGTYPES.items()}
# the step and the closed loop of the two on a handle with settings classes (eepacc_create_classes, eepacc_create_classes_bl
# with bl_mode = 1): arguments and order are those of eepacc_ab_step_est and eepacc_run_abmpc_preview
CLASSES_EST_ARGTYPES = {
    "eepacc_classes_step_est": list(AB_EST_ARGTYPES["eepacc_ab_step_est"]),
    "eepacc_run_classes_preview": list(AB_EST_ARGTYPES["eepacc_run_abmpc_preview"]),
}

# the condensed QP of a step as data on a handle with settings classes: size and rows as the ab_ / bl_ entries (the rows of one
# class, cls, padded with -1 to the handle's nC), the build with the arguments of eepacc_ab_build_qp_est
CLASSES_BUILD_ARGTYPES = {
    "eepacc_classes_qp_size": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "eepacc_classes_qp_rows": [C.c_void_p, C.c_int, c_int32_p, c_int32_p],
    "eepacc_classes_build_qp": list(AB_EST_ARGTYPES["eepacc_ab_build_qp_est"]),
}

# enum EEPACC_FB_ROW_*: the row types of eepacc_fb_qp_rows, ascending in the order of the rows within a stage
FB_ROW_TYPES = ["s", "v", "fm", "fb", "xi_v", "xi_h", "xi_s", "xi_f", "blocked_fm", "blocked_fb", "tm_min", "tm_max",
                "axle_min", "axle_max", "fric_max", "fric_min", "a_max", "a_min", "j_max", "j_min",
                "v_lim", "v_curv", "v_stop", "v_tl", "v_inc", "safe1", "safe2", "hwp"]
FB_ROW = {name: i for i, name in enumerate(FB_ROW_TYPES)}

# the same for an FBMPC step: the seven inputs, the model A22, D2 (or None), the five outputs, A22_used, D2_used (or None)
FB_BUILD_ARGTYPES = {
    "eepacc_fb_qp_size": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "eepacc_fb_qp_rows": [C.c_void_p, c_int32_p, c_int32_p],
    "eepacc_fb_build_qp": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 2 + [C.c_void_p] * 5 + [C.c_void_p] * 2 + [C.c_void_p],
}

# FBMPC with the horizon guesses supplied: the ten inputs of eepacc_fb_step, then s_est, v_est, s_tv_est (each may be None), then its
# outputs; the build with the three guesses before the model; the closed loop with B, n_steps, n_lead
FB_EST_ARGTYPES = {
    "eepacc_fb_step_est": [C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_void_p] * 3 + [C.c_void_p] * 4 + [C.c_void_p],
    "eepacc_fb_build_qp_est": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 3 + [C.c_void_p] * 2 + [C.c_void_p] * 5 + [C.c_void_p] * 2 + [C.c_void_p],
    "eepacc_run_fbmpc_preview": list(AB_EST_ARGTYPES["eepacc_run_abmpc_preview"]),
}

# FBMPC on a handle with settings classes (eepacc_create_classes): arguments and order are those of eepacc_fb_step (ten
# inputs, four outputs) and eepacc_run_fbmpc (B, n_steps, five inputs, two outputs)
CLASSES_FB_ARGTYPES = {
    "eepacc_classes_fb_step": [C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_void_p] * 4 + [C.c_void_p],
    "eepacc_run_classes_fbmpc": [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_void_p] * 2 + [C.c_void_p],
}

# enum EEPACC_BL_ROW_*: the row types of eepacc_bl_qp_rows, ascending in the order of the rows within a stage (a handle created
# with bl_mode = 2 has none of the two safe-distance types)
BL_ROW_TYPES = ["s", "v", "xi_f", "a_min", "a_max", "j_min", "j_max", "v_lim", "v_curv", "v_stop", "v_tl", "safe1", "safe2"]
BL_ROW = {name: i for i, name in enumerate(BL_ROW_TYPES)}

# the same for a BLMPC / TVMPC step: the seven inputs (the three lead arrays may be None with bl_mode = 2), the five outputs
BL_BUILD_ARGTYPES = {
    "eepacc_bl_qp_size": [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_int)],
    "eepacc_bl_qp_rows": [C.c_void_p, c_int32_p, c_int32_p],
    "eepacc_bl_build_qp": [C.c_void_p, C.c_int] + [C.c_void_p] * 7 + [C.c_void_p] * 5 + [C.c_void_p],
}

_VEH_FIELDS = ["m", "A_f", "c_d", "L", "h_g", "WD_s_F", "L_f", "L_r", "F0", "F1", "F2",
               "p00", "p10", "p01", "P_m_max", "T_m_max", "omega_m_r", "omega_m_max",
               "c_r", "R_w", "beta_gb", "beta_fd", "phi", "v_max", "eta_TF",
               "lambda", "mu", "rho_a", "g", "zeta_a",
               "k00", "k10", "k01", "tau_fd", "eta_drive"]
_VEH_OPTIONAL = {"k00": 0.0, "k10": 0.0, "k01": 0.0, "tau_fd": 1.0, "eta_drive": 1.0}


class Vehicle(C.Structure):
    _fields_ = ([(("lambda_" if f == "lambda" else f), C.c_double) for f in _VEH_FIELDS]
                + [("upSpd", C.c_double * 7), ("tau_gb", C.c_double * 8)])


class SettingsPOD(C.Structure):
    _fields_ = [
        ("N_hor", C.c_int32),
        ("Tvec", c_double_p),
        ("Mb", c_int32_p),
        ("W_AB", C.c_double * 7),
        ("W_FB", C.c_double * 7),
        ("ab_fuel_term", C.c_int32),
        ("ab_route_rows", C.c_int32),
        ("tau_min", C.c_double), ("h_min", C.c_double), ("s_goal", C.c_double),
        ("paramEstSetting", C.c_int32), ("TVestSetting", C.c_int32),
        ("tConstACC_ego", C.c_double), ("tConstACC_tar", C.c_double),
        ("N_integratePlant", C.c_int32),
        ("solverToUse", C.c_int32),
        ("FBuseTaylor", C.c_int32),
        ("b_quadr", C.c_double * 6),
        ("b_fifthOrder", C.c_double * 21),
        ("n_speedLim", C.c_int32), ("s_speedLim", c_double_p), ("v_speedLim", c_double_p),
        ("n_curv", C.c_int32), ("s_curv", c_double_p), ("curvature", c_double_p),
        ("n_slope", C.c_int32), ("s_slope", c_double_p), ("slope", c_double_p),
        ("n_stop", C.c_int32), ("stopLoc", c_double_p),
        ("n_TL", C.c_int32), ("TLLoc", c_double_p),
        ("stopRefDist", C.c_double), ("stopRefVelSlope", C.c_double), ("stopVel", C.c_double),
        ("TLstopVel", C.c_double), ("TLStopRegionSize", C.c_double), ("alpha_TTL", C.c_double),
        ("bl_mode", C.c_int32), ("bl_prox_iter", C.c_int32),
        ("W_BL", C.c_double * 4),
        ("BL_a_LimLowVel", C.c_double), ("BL_a_LimHighVel", C.c_double),
        ("BL_j_LimLowVel", C.c_double), ("BL_j_LimHighVel", C.c_double),
        ("bl_lp_eps", C.c_double),
        ("state_bound_tol", C.c_double),
    ]


def make_vehicle(V: Dict[str, float]) -> Vehicle:
    v = Vehicle()
    for f in _VEH_FIELDS:
        setattr(v, "lambda_" if f == "lambda" else f, float(V[f] if f not in _VEH_OPTIONAL else V.get(f, _VEH_OPTIONAL[f])))
    up = np.asarray(V.get("upSpd", np.full(7, 1e9)), dtype=np.float64).ravel()
    gb = np.asarray(V.get("tau_gb", np.ones(8)), dtype=np.float64).ravel()
    if up.size != 7 or gb.size != 8:
        raise ValueError("upSpd needs 7 and tau_gb 8 entries (SetVehicleParameters.m:96-98)")
    for i in range(7):
        v.upSpd[i] = float(up[i])
    for i in range(8):
        v.tau_gb[i] = float(gb[i])
    return v


class SettingsHolder:
    """Owns the numpy buffers the POD points into."""

    def __init__(self, OPT: Dict[str, Any]):
        self._keep = []
        self.pod = SettingsPOD()
        p = self.pod
        N = int(OPT["N_hor"])
        if N > EEPACC_MAX_HORIZON:
            raise ValueError(f"N_hor {N} exceeds EEPACC_MAX_HORIZON {EEPACC_MAX_HORIZON}")
        p.N_hor = N
        p.Tvec = self._dptr(OPT["Tvec"], N)
        mb = np.ascontiguousarray(OPT.get("Mb", np.zeros(N)), dtype=np.int32)
        self._keep.append(mb)
        p.Mb = mb.ctypes.data_as(c_int32_p)
        W_AB = np.asarray(OPT["W_AB"], dtype=np.float64).ravel()
        if W_AB.size == 7:
            p.ab_fuel_term = 2 if OPT.get("fuel_map", "EFF") == "ICE" else 1     # CreateQP_AB.m:154-166
            wab = W_AB
        elif W_AB.size == 6:       # ORIG/Settings.m:48-62: no w_FC entry
            p.ab_fuel_term = 0
            wab = np.concatenate([[0.0], W_AB])
        else:
            raise ValueError("W_AB must have 6 (ORIG) or 7 (ABO) entries")
        for i in range(7):
            p.W_AB[i] = float(wab[i])
            p.W_FB[i] = float(np.asarray(OPT["W_FB"]).ravel()[i])
        p.ab_route_rows = int(OPT.get("ab_route_rows", 1 if OPT.get("tree", "ABO") == "ORIG" else 0))
        p.tau_min = float(OPT["tau_min"]); p.h_min = float(OPT["h_min"]); p.s_goal = float(OPT["s_goal"])
        p.paramEstSetting = int(OPT["paramEstSetting"]); p.TVestSetting = int(OPT["TVestSetting"])
        p.tConstACC_ego = float(OPT["tConstACC_ego"]); p.tConstACC_tar = float(OPT["tConstACC_tar"])
        p.N_integratePlant = int(OPT["N_integratePlant"])
        p.solverToUse = int(OPT["solverToUse"])
        p.FBuseTaylor = int(bool(OPT["FBuseTaylor"]))
        for i in range(6):
            p.b_quadr[i] = float(OPT["b_quadr"][i])
        for i in range(21):
            p.b_fifthOrder[i] = float(OPT["b_fifthOrder"][i])
        p.n_speedLim = len(OPT["s_speedLim"])
        p.s_speedLim = self._dptr(OPT["s_speedLim"]); p.v_speedLim = self._dptr(OPT["v_speedLim"])
        p.n_curv = len(OPT["s_curv"])
        p.s_curv = self._dptr(OPT["s_curv"]); p.curvature = self._dptr(OPT["curvature"])
        p.n_slope = len(OPT["s_slope"])
        p.s_slope = self._dptr(OPT["s_slope"]); p.slope = self._dptr(OPT["slope"])
        stop = np.asarray(OPT.get("stopLoc", []), dtype=np.float64).ravel()
        p.n_stop = stop.size
        p.stopLoc = self._dptr(stop) if stop.size else c_double_p()
        TL = np.asarray(OPT.get("TLLoc", np.zeros((0, 4))), dtype=np.float64).reshape(-1, 4)
        p.n_TL = TL.shape[0]
        p.TLLoc = self._dptr(TL) if TL.size else c_double_p()
        p.stopRefDist = float(OPT["stopRefDist"]); p.stopRefVelSlope = float(OPT["stopRefVelSlope"])
        p.stopVel = float(OPT["stopVel"]); p.TLstopVel = float(OPT["TLstopVel"])
        p.TLStopRegionSize = float(OPT["TLStopRegionSize"]); p.alpha_TTL = float(OPT["alpha_TTL"])
        # baseline controller (RunOpt_BLMPC): settings.Settings_BL() fills these
        p.state_bound_tol = float(OPT.get("state_bound_tol", 0.0))
        p.bl_mode = int(OPT.get("bl_mode", 0))
        if p.bl_mode:
            for i in range(4):
                p.W_BL[i] = float(np.asarray(OPT["W_BL"]).ravel()[i])
            p.BL_a_LimLowVel = float(OPT["BL_a_LimLowVel"]); p.BL_a_LimHighVel = float(OPT["BL_a_LimHighVel"])
            p.BL_j_LimLowVel = float(OPT["BL_j_LimLowVel"]); p.BL_j_LimHighVel = float(OPT["BL_j_LimHighVel"])
            p.bl_lp_eps = float(OPT.get("bl_lp_eps", 0.0))
            p.bl_prox_iter = int(OPT.get("bl_prox_iter", 0))

    def _dptr(self, arr, n=None):
        a = np.ascontiguousarray(arr, dtype=np.float64).ravel()
        if n is not None and a.size != n:
            raise ValueError(f"expected {n} entries, got {a.size}")
        self._keep.append(a)
        return a.ctypes.data_as(c_double_p)


def pack_classes(OPT_list, V_list):
    """The S[n_classes], V[n_classes] arrays of eepacc_create_classes.  Returns (holders, S, V): the holders own the buffers
    the entries of S point into and must outlive the call."""
    holders = [SettingsHolder(o) for o in OPT_list]
    S = (SettingsPOD * len(holders))(*[h.pod for h in holders])
    V = (Vehicle * len(V_list))(*[make_vehicle(v) for v in V_list])
    return holders, S, V


def as_dptr(a: np.ndarray):
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_double_p)


def as_iptr(a: np.ndarray):
    assert a.dtype == np.int32 and a.flags["C_CONTIGUOUS"]
    return a.ctypes.data_as(c_int32_p)
