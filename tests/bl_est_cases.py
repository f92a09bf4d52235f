"""Inputs of tests/test_bl_est_cpu.py and tests/test_gpu_bl_est.py: the baseline controller's entry points that take the horizon
guesses s_est, v_est, s_tv_est from the caller (eepacc_bl_step_est, eepacc_bl_build_qp_est, eepacc_run_blmpc_preview).

Per configuration (both trees at N = 2, 3, 20, 33, 63) the step inputs are six states: the five of tests/bl_qp_ref.py
(standstill, the two knots of the comfort limits, a braking state, a close lead at speed) and a follower at 8 m/s.  The
supplied guesses are seeded random arrays that no estimator mode produces, of the kind tests/ab_est_cases.py makes: an ego speed
that wanders (kept >= 0, positions ordered, unrelated to the constant-speed guess), a lead that speeds up over the first half of
the horizon and brakes over the second (its acceleration reverses inside the horizon; it never falls behind the constant-speed
guess, so the hard terminal rows stay feasible), instance 4 with +inf from the middle of the horizon on and instance 5 with +inf
throughout.  Row 0 of s_est, v_est is the measurement, as the reference passes it.

oracle_problems() is the reference for the built problem: orc_create_qp_bl on the same arrays and the literal condensing of
orc_transform_to_dense, as the oracle's own step does after its estimators (n_u = 2)."""
import ctypes as C
import functools

import numpy as np

import bl_qp_ref as blr
from eepacc_mpc_casadi_matlab_amd._abi import SettingsPOD, Vehicle, c_double_p, as_dptr

CONFIGS = {"%s%d" % (t.lower(), N): (t, N) for N in (2, 3, 20, 33, 63) for t in ("ABO", "ORIG")}
STEP_CONFIGS = tuple(c for c, (_, N) in CONFIGS.items() if N in (3, 20, 33, 63))      # the step against the built problem
SEED = 20262
B = 6
MAX_LEFT_OUT = 1                         # of a configuration's six instances, and only where the oracle's own solve fails
STATES = list(blr.STATES) + [(50.0, 8.0, 0.0, 3.0, 75.0, 8.0, 0.0)]
INS = blr.KEYS


@functools.lru_cache(maxsize=None)
def settings(cfg):
    tree, N = CONFIGS[cfg]
    return blr._bl_case(N, tree)


@functools.lru_cache(maxsize=None)
def inputs(cfg):
    """-> columns (INS -> [B]) of the configuration, the same for every one; no user writes to them"""
    return {n: np.array([st[j] for st in STATES]) for j, n in enumerate(INS)}


def take(cols, idx):
    return {n: np.ascontiguousarray(cols[n][idx]) for n in INS}


@functools.lru_cache(maxsize=None)
def supplied(cfg):
    """-> s_est, v_est, s_tv_est, each [N+1, B] (read-only)"""
    tree, N = CONFIGS[cfg]
    BL, _ = settings(cfg)
    Tv = np.asarray(BL["Tvec"], dtype=np.float64)
    cols = inputs(cfg)
    rng = np.random.default_rng([SEED, N, int(tree == "ORIG")])
    s_est = np.empty((N + 1, B)); v_est = np.empty((N + 1, B)); s_tv_est = np.empty((N + 1, B))
    s_est[0], v_est[0], s_tv_est[0] = cols["s"], cols["v"], cols["s_tv"]
    a_ego = rng.uniform(-1.5, 1.5, (N, B))
    a_lead = rng.uniform(0.3, 1.2, B) * min(1.0, 5.0 / Tv.sum())     # the lead gains at most 3 m/s
    v_lead = cols["v_tv"].copy()
    for k in range(N):
        v_est[k + 1] = np.maximum(v_est[k] + Tv[k] * a_ego[k], 0.0)
        s_est[k + 1] = s_est[k] + Tv[k] * v_est[k]
        s_tv_est[k + 1] = s_tv_est[k] + Tv[k] * v_lead
        v_lead = v_lead + Tv[k] * (a_lead if 2 * k < N else -a_lead)
    s_tv_est[N // 2:, B - 2] = np.inf
    s_tv_est[:, B - 1] = np.inf
    for a in (s_est, v_est, s_tv_est):
        a.setflags(write=False)
    return s_est, v_est, s_tv_est


def device_arrays(cfg, idx=None):
    """the supplied arrays of a configuration as the device gets them: row N of s_tv_est is NaN (it is not read)"""
    se, ve, st = supplied(cfg)
    st = st.copy(); st[-1] = np.nan
    if idx is not None:
        se, ve, st = se[:, idx], ve[:, idx], st[:, idx]
    return dict(s_est=np.ascontiguousarray(se), v_est=np.ascontiguousarray(ve), s_tv_est=np.ascontiguousarray(st))


class DenseOracle:
    """orc_create_qp_bl + orc_transform_to_dense of the CPU oracle on supplied horizon guesses"""

    def __init__(self, BL, V):
        from oracle import Oracle
        self.orc = Oracle(BL, V)
        L = self.orc.lib
        S, Vp = C.POINTER(SettingsPOD), C.POINTER(Vehicle)
        L.orc_create_qp_bl.restype = None
        L.orc_create_qp_bl.argtypes = [S, Vp, C.c_double, C.c_double] + [c_double_p] * 3 + [C.c_double, C.c_double] + [c_double_p] * 5
        L.orc_transform_to_dense.restype = None
        L.orc_transform_to_dense.argtypes = [C.c_int] * 3 + [c_double_p] * 8 + [C.c_double, C.c_double] + [c_double_p] * 7

    def dense(self, s, v, a_prev, t0, s_est, v_est, s_tv_est):
        """-> dict H [nV, nV], c [nV], G [nC, nV], lb, ub [nC] of one instance; the guesses are [N+1]"""
        o = self.orc
        N, nu, nx = o.N, 2, 2
        nz, nV, nC = N * (nx + nu) + nx, N * nu, o.nC("ab")
        f = lambda a: np.ascontiguousarray(a, dtype=np.float64)
        se, ve, st = f(s_est), f(v_est), f(s_tv_est)
        Hs, cs, Gs, glb, gub = np.zeros((nz, nz)), np.zeros(nz), np.zeros((nC, nz)), np.zeros(nC), np.zeros(nC)
        o.lib.orc_create_qp_bl(C.byref(o.S), C.byref(o.V), float(s), float(v), as_dptr(se), as_dptr(ve), as_dptr(st), float(t0),
                               float(a_prev), as_dptr(Hs), as_dptr(cs), as_dptr(Gs), as_dptr(glb), as_dptr(gub))
        Tv = np.asarray(o.OPT["Tvec"], dtype=np.float64)
        A = np.zeros((N, 4)); Bm = np.zeros((N, 2 * nu)); Dm = np.zeros((N, 2))          # RunOpt_BLMPC.m: A_k, B_k, D_k
        A[:, 0] = 1.0; A[:, 1] = Tv; A[:, 3] = 1.0
        Bm[:, 0] = 0.5 * Tv * Tv; Bm[:, nu] = Tv
        Hd, cd, Gd, lbd, ubd = np.zeros((nV, nV)), np.zeros(nV), np.zeros((nC, nV)), np.zeros(nC), np.zeros(nC)
        Psi, d = np.zeros((nz, nV)), np.zeros(nz)
        o.lib.orc_transform_to_dense(N, nu, nC, as_dptr(A), as_dptr(Bm), as_dptr(Dm), as_dptr(Hs), as_dptr(cs), as_dptr(Gs),
                                     as_dptr(glb), as_dptr(gub), float(s), float(v), as_dptr(Hd), as_dptr(cd), as_dptr(Gd),
                                     as_dptr(lbd), as_dptr(ubd), as_dptr(Psi), as_dptr(d))
        return dict(H=Hd, c=cd, G=Gd, lb=lbd, ub=ubd)


@functools.lru_cache(maxsize=None)
def oracle_problems(cfg):
    """The oracle's dense problem of every instance of a configuration on the supplied guesses (computed once)"""
    BL, V = settings(cfg)
    D = DenseOracle(BL, V)
    cols = inputs(cfg)
    se, ve, st = supplied(cfg)
    st = st.copy(); st[-1] = st[-2]                  # row N is not read by the reference either; any finite-or-not value does
    return D, [D.dense(cols["s"][i], cols["v"][i], cols["a_prev"][i], cols["t0"][i], se[:, i], ve[:, i], st[:, i])
               for i in range(B)]


def objective(H, g, x):
    return float(0.5 * x @ H @ x + g @ x)


def braking_lead(n_rows, nB, Ts):
    """a lead that brakes to a stop and pulls away again, one phase shift per instance (tests/test_gpu_ab_est.py)"""
    t = Ts * np.arange(n_rows)[:, None] + 1.5 * np.arange(nB)[None, :]
    v = np.clip(np.minimum(10.0 - 2.0 * (t - 6.0), 1.5 * (t - 16.0)), 0.0, 10.0)
    v = np.where(t < 6.0, 10.0, np.maximum(v, 0.0))
    s = 25.0 + Ts * np.concatenate([np.zeros((1, nB)), np.cumsum(v[:-1], axis=0)])
    return np.ascontiguousarray(s), np.ascontiguousarray(v)
