"""Synthetic scenario generators shared by the tests and bench.py.

S2 "closed-loop scenarios": instance i starts at (s, v) = (0, U(0,10)); its lead vehicle follows
the 2 Hz TO01_EAD speed trace circularly shifted by (13 i) mod 870 samples and scaled by
U(0.8, 1.2), starting U(6, 40) m ahead; lead distance is the forward-Euler integral of the speed
as in ABO/Run_DrivingCycle.m:37-47.  Deterministic (numpy Generator, seed 1234 + rank).
"""
from __future__ import annotations

import numpy as np


def make_s2(B: int, n_steps: int, V_TO_2Hz: np.ndarray, Ts: float = 0.5, seed: int = 1234,
            first_instance: int = 0):
    # one stream per quantity, so that instance i gets the same draw whatever the shard size
    total = first_instance + B
    v0_all = np.random.default_rng([seed, 0]).uniform(0.0, 10.0, total)
    scale_all = np.random.default_rng([seed, 1]).uniform(0.8, 1.2, total)
    gap_all = np.random.default_rng([seed, 2]).uniform(6.0, 40.0, total)
    idx = np.arange(first_instance, total)
    v0, scale, gap = v0_all[idx], scale_all[idx], gap_all[idx]
    base = np.where(np.asarray(V_TO_2Hz, dtype=np.float64) < 0.1, 0.0, V_TO_2Hz)   # Run_DrivingCycle.m:17
    L = base.size
    k = np.arange(n_steps)[:, None]
    shift = ((idx * 13) % L)[None, :]
    v_tv = base[(k + shift) % L] * scale[None, :]
    v_tv[0, :] = 0.0                                   # the reference's trace starts at standstill
    s_tv = gap[None, :] + Ts * np.cumsum(v_tv, axis=0)
    s_tv[0, :] = gap
    return dict(s0=np.zeros(B), v0=v0, a_minus1=np.zeros(B), s_tv=np.ascontiguousarray(s_tv),
                v_tv=np.ascontiguousarray(v_tv))


def make_s1(B: int, golden: dict, s_tv: np.ndarray, v_tv: np.ndarray, Ts: float = 0.5, seed: int = 1234):
    """S1 "open-loop step batch": instance i takes the golden state of step (7 i) mod 871 and
    perturbs speed by U(-0.5,0.5) m/s and gap by U(-2,2) m."""
    rng = np.random.default_rng(seed)
    n = golden["s_opt"].size
    k = (np.arange(B) * 7) % n
    dv = rng.uniform(-0.5, 0.5, B)
    dgap = rng.uniform(-2.0, 2.0, B)
    s = golden["s_opt"][k].copy()
    v = np.maximum(golden["v_opt"][k] + dv, 0.0)
    vprev = golden["v_opt"][np.maximum(k - 1, 0)]
    a_prev = np.where(k > 0, (golden["v_opt"][k] - vprev) / Ts, 0.0)
    vtv = np.where(k > 0, v_tv[k], 0.0)
    vtv_prev = np.where(k > 1, v_tv[np.maximum(k - 1, 0)], 0.0)
    return dict(s=s, v=v, a_prev=a_prev, t0=k * Ts, s_tv=s_tv[k] + dgap, v_tv=vtv,
                a_tv_prev=np.where(k > 0, (vtv - vtv_prev) / Ts, 0.0), k=k)


def make_use_case_mix(cases, per_case: int, tree: str, N_hor: int, n_steps=None, argonne_lead=None, controller: str = "ab"):
    """Several GetUseCase scenarios as the settings classes of one launch (Engine.from_classes): class k is cases[k], every
    class has per_case instances, interleaved (class_of = 0, 1, 2, ..., 0, 1, 2, ...).  Each instance starts from its use
    case's own s_init, v_init, a_minus1 and follows its use case's lead: the recorded one of 8 and 9 (argonne_lead =
    (t, v_mph), the two columns of the measurement file), the cut-in of 10, none otherwise (s_tv = inf, v_tv = 0,
    Main.m:77-80).  n_steps defaults to the shortest simulated time of the chosen cases (t_sim / Ts + 1).
    controller "ab": OPT holds the settings themselves (ABMPC); "bl": settings.Settings_BL of every case, the classes of a
    baseline engine.

    Returns a dict: OPT (settings per class), V (vehicle per class), class_of [B], s0, v0, a_minus1 [B],
    s_tv, v_tv [n_steps][B], n_steps, and TV: settings.Settings_TV per class (the classes of the engine that generates a lead
    along every route, engine.generate_lead_and_run_mix) with the class's TVlength, TVinitDist, TVinitVel; None for a class
    whose TV_Ts differs from its Tvec[0], which has no such view."""
    from .settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV, default_opt
    if controller not in ("ab", "bl"):
        raise ValueError("controller must be 'ab' or 'bl'")
    cases = [int(c) for c in cases]
    if not cases or per_case < 1:
        raise ValueError("make_use_case_mix needs at least one use case and per_case >= 1")
    OPTs, Vs = [], []
    for c in cases:
        o = default_opt(); o["useCaseNum"] = c
        if argonne_lead is not None:
            o["argonne_lead"] = argonne_lead
        OPTs.append(Settings(o, tree=tree, N_hor=N_hor))
        Vs.append(SetVehicleParameters(tree))
    full = [int(round(o["t_sim"] / o["Tvec"][0])) + 1 for o in OPTs]
    if n_steps is None:
        n_steps = min(full)
    n_steps = int(n_steps)
    if n_steps < 1 or n_steps > min(full):
        raise ValueError("n_steps must be in [1, %d], the shortest simulated time of the chosen cases" % min(full))
    K, B = len(cases), len(cases) * int(per_case)
    class_of = (np.arange(B) % K).astype(np.int32)
    s_tv = np.full((n_steps, B), np.inf)
    v_tv = np.zeros((n_steps, B))
    for k, (c, o) in enumerate(zip(cases, OPTs)):
        if c in (8, 9, 10):
            s_tv[:, class_of == k] = np.asarray(o["s_tv"], dtype=np.float64)[:n_steps, None]
            v_tv[:, class_of == k] = np.asarray(o["v_tv"], dtype=np.float64)[:n_steps, None]
    pick = lambda key: np.array([float(OPTs[k][key]) for k in class_of])
    TV = [Settings_TV(o) if float(o["TV_Ts"]) == float(np.asarray(o["Tvec"]).ravel()[0]) else None for o in OPTs]
    return dict(OPT=[Settings_BL(o) for o in OPTs] if controller == "bl" else OPTs, V=Vs, class_of=class_of, s0=pick("s_init"),
                v0=pick("v_init"), a_minus1=pick("a_minus1"), s_tv=s_tv, v_tv=v_tv, n_steps=n_steps, TV=TV)


def preview_tables(Tvec):
    """(idx, frac), [N] each: where stage k of a horizon looks into a trace sampled every Tvec[0], counted in rows from the
    step's own.  p = tau_k / Tvec[0] with tau_k = sum_{i<k} Tvec[i], in numpy.longdouble; idx = floor(p), frac = p - idx,
    snapped to 0 below 1e-9 and to the next index above 1 - 1e-9 (a stage that falls on a sample up to rounding, as with
    Tvec[k] / Ts a whole number and Ts = 0.3, reads that sample)."""
    LD = np.longdouble
    T = np.asarray(Tvec, dtype=np.float64).reshape(-1)
    idx = np.zeros(T.size, dtype=np.int32); frac = np.zeros(T.size)
    tau = LD(0.0)
    for k in range(T.size):
        p = tau / LD(T[0])
        i = np.floor(p); f = p - i
        if f < LD("1e-9"):
            f = LD(0.0)
        elif f > LD(1.0) - LD("1e-9"):
            i += 1; f = LD(0.0)
        idx[k] = int(i); frac[k] = float(f)
        tau = tau + LD(T[k])
    return idx, frac


def lead_preview(s_tv, v_tv, r, Tvec):
    """The lead's horizon guess s_tv_est [N+1, B] of the step at row r of the traces s_tv, v_tv [n_lead, B], read from the
    traces themselves: the specification of what eepacc_run_abmpc_preview hands its steps (Engine.ab_step_est takes the
    result as s_tv_est).  Stage k looks tau_k ahead, at row r + idx[k] + frac[k] (preview_tables): the sample itself where
    frac is 0 (so +inf, no lead, stays +inf), else (1 - frac) s_tv[i] + frac s_tv[i + 1], and past the last row
    s_tv[-1] + v_tv[-1] (tau_k - (n_lead - 1 - r) Tvec[0]).  Row N is not read by the step and is left at the value of
    row N - 1."""
    s_tv = np.asarray(s_tv, dtype=np.float64); v_tv = np.asarray(v_tv, dtype=np.float64)
    if s_tv.ndim == 1:
        s_tv = s_tv[:, None]; v_tv = v_tv[:, None]
    T = np.asarray(Tvec, dtype=np.float64).reshape(-1)
    N, last = T.size, s_tv.shape[0] - 1
    idx, frac = preview_tables(T)
    tau = np.concatenate([[0.0], np.cumsum(T)])                    # running double sum, as the settings translation keeps it
    out = np.empty((N + 1, s_tv.shape[1]))
    for k in range(N):
        i, f = int(r) + int(idx[k]), float(frac[k])
        if i < last or (i == last and f == 0.0):
            out[k] = s_tv[i] if f == 0.0 else (1.0 - f) * s_tv[i] + f * s_tv[i + 1]
        else:
            out[k] = s_tv[last] + v_tv[last] * (tau[k] - float(last - int(r)) * T[0])
    out[N] = out[N - 1]
    return out
