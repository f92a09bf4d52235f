"""Inputs of tests/test_gpu_classes_fb.py and tests/test_classes_fb_cpu.py: the settings classes of the FBMPC mixed launches and
their scenarios.  No GPU is needed to make them.

classes(N): four classes of the ORIG tree that differ in what FBMPC reads
  0  use case 5 (traffic lights)
  1  use case 7 (stop sign and a slope table), W_FB scaled entry by entry
  2  use case 6 (curve), FBuseTaylor = 0, the vehicle 350 kg heavier
  3  use case 3 (speed-limit step), estimator modes 0 / 0, another driveline (phi, eta_TF)
classes(N, pe2=True) gives class 1 paramEstSetting = 2 (the shifted previous solution) on top.
scenario(B, n_steps, K): interleaved map 0, 1, .., K-1, 0, 1, ..; leads of scenarios.make_s2 (the recorded trace, shifted and scaled per
instance) at gaps from tight following to far ahead, and no lead at all (s_tv = +inf, v_tv = 0) for every fifth instance.

oracle_classes(), oracle_scenario(): the mix that is compared with the oracle (N = 20, B = 6, 30 steps).  The classes above are
compared with the plain engine of their class, bit for bit, and that is what carries the class binding.  The oracle is a
reference for the structured FBMPC kernels at the bars of tests/test_gpu_fb.py only on the settings that file compares: the
default route of a tree with S2 leads, in the estimator modes.  On routes with features it is not one: where a slope table
varies the kernels interpolate the slope and the reference and the oracle use slope(1), and no test
compares the plain engine with the oracle on a GetUseCase route.  So the three classes are those of
tests/test_gpu_fb.py::test_fb_estimator_modes and its neighbours, the ABO tree's settings with the estimators in modes 1 / 1 (as
they are), 0 / 0 and paramEstSetting = 2, and the scenario is that test's (make_s2 with seed 5: close following at + 15 m,
following at + 40 m, far ahead at + 500 m), its three instances and the next three of the same stream, with the classes
rotated against the three gaps (class_of = 0, 1, 2, 1, 2, 0).
"""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W_FB_SCALE = np.array([1.0, 3.0, 0.5, 2.0, 1.0, 1.0, 1.0])
ORACLE_MIX = dict(N=20, B=6, n_steps=30, K=3)


def use_case(case, N, **kw):
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, default_opt
    o = default_opt(); o["useCaseNum"] = case
    OPT = Settings(o, tree="ORIG", N_hor=N)
    OPT.update(kw)
    return OPT


def classes(N, pe2=False):
    from eepacc_mpc_casadi_matlab_amd.settings import SetVehicleParameters
    V = SetVehicleParameters("ORIG")
    o1 = use_case(7, N)
    o1["W_FB"] = np.asarray(o1["W_FB"], dtype=np.float64) * W_FB_SCALE
    if pe2:
        o1["paramEstSetting"] = 2
    OPTs = [use_case(5, N), o1, use_case(6, N, FBuseTaylor=False), use_case(3, N, paramEstSetting=0, TVestSetting=0)]
    Vs = [V, V, dict(V, m=V["m"] + 350.0), dict(V, phi=1.1 * V["phi"], eta_TF=0.9)]
    return OPTs, Vs


def scenario(B, n_steps, K, seed=21):
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    lead = np.load(os.path.join(GOLDEN, "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    sc = make_s2(B, n_steps, lead, seed=seed)
    sc["s_tv"] = np.ascontiguousarray(sc["s_tv"] + np.resize(np.array([30.0, 60.0, 0.0, 150.0, 25.0, 80.0, 400.0]), B)[None, :])
    free = np.arange(B) % 5 == 2
    sc["s_tv"][:, free] = np.inf
    sc["v_tv"][:, free] = 0.0
    sc["class_of"] = (np.arange(B) % K).astype(np.int32)
    return sc


def oracle_classes():
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters
    V = SetVehicleParameters("ABO")
    OPTs = []
    for est in ({}, dict(paramEstSetting=0, TVestSetting=0), dict(paramEstSetting=2)):
        OPT = Settings(tree="ABO", N_hor=ORACLE_MIX["N"])
        OPT.update(est)
        OPTs.append(OPT)
    return OPTs, [V, V, V]


def oracle_scenario():
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    B = ORACLE_MIX["B"]
    lead = np.load(os.path.join(GOLDEN, "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    sc = make_s2(B, ORACLE_MIX["n_steps"], lead, seed=5)
    sc["s_tv"] = np.ascontiguousarray(sc["s_tv"] + np.resize(np.array([15.0, 40.0, 500.0]), B)[None, :])
    i = np.arange(B)
    sc["class_of"] = ((i + i // 3) % 3).astype(np.int32)
    return sc


def step_inputs(B, seed=5):
    """Three consecutive fb_step calls on inputs that differ from call to call (the second and third find the codes of another
    problem): tuples in the order of eepacc_fb_step's ten inputs."""
    rng = np.random.default_rng(seed)
    calls = []
    for k in range(3):
        s = rng.uniform(0.0, 250.0, B)
        v = rng.uniform(2.0, 14.0, B)
        gap = rng.uniform(8.0, 120.0, B)
        s_tv = s + gap
        v_tv = rng.uniform(0.0, 15.0, B)
        free = np.arange(B) % 5 == 3
        s_tv[free] = np.inf; v_tv[free] = 0.0
        z = np.zeros(B)
        calls.append((s, v, z.copy(), rng.uniform(-0.5, 0.5, B), z.copy(), z.copy(), np.full(B, 0.5 * k), s_tv, v_tv,
                      np.where(free, 0.0, rng.uniform(-0.3, 0.3, B))))
    return calls
