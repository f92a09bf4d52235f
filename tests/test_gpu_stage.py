"""The per-stage device functions of csrc/eepacc_stage.h (trajectory estimator, route and comfort bounds, PWA interpolation,
RK4 plant), called one at a time through tests/kernels/stage_harness.hip and compared with the plain-Python restatement of the
reference's .m files (tests/stage_ref.py) on inputs that sit on the branch edges (tests/stage_cases.py; which edges, and that
the tables still hold them, is asserted without a GPU by tests/test_stage_ref_cpu.py).

The DevCfg of every call is what the product's settings translation makes of the reference-style OPT dict (cfg_harness), so
tau, const_T, const_slope, vcurv_tab, bl_mode and the bl_* limits are the product's.  Every test is one tiny launch of at most
a few thousand threads, one thread per problem.

    timeout 600 python -m pytest -m gpu tests/test_gpu_stage.py
"""
import numpy as np
import pytest

import cfg_harness
import stage_cases as sc
import stage_harness as sh

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps
PLANT_ROOM = 8          # the device may be this many times as far from the 50-digit scheme as the fp64 reference is


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    return sh.load(str(tmp_path_factory.mktemp("stage_harness")))


@pytest.fixture(scope="module")
def CH(tmp_path_factory):
    return cfg_harness.load(str(tmp_path_factory.mktemp("cfg_harness")))


def _cfg(CH, OPT, V):
    b = CH.build(OPT, V)
    assert b.rc == 0, b.msg
    return b.cfg


def _check(name, got, want, tol):
    """|got - want| <= tol per problem (tol 0: bit-equal, the sign of a zero included); prints the figure first"""
    got, want, tol = np.asarray(got), np.asarray(want), np.broadcast_to(tol, np.shape(want))
    assert not np.isnan(got).any(), name
    err = np.abs(got - want)
    over = err > tol
    exact = tol == 0
    bits = exact & (got.view(np.uint64) != want.view(np.uint64))
    print("%s: %d problems, %d bit-equal by demand, largest error %.3e, largest error / tolerance %.3f"
          % (name, got.size, int(exact.sum()), err.max(), (err[~exact] / tol[~exact]).max() if (~exact).any() else 0.0))
    bad = np.where(over | bits)[0]
    assert bad.size == 0, "%s: %d problems differ, first %s: got %r, reference %r, tolerance %.3e" % (
        name, bad.size, bad[:8], got[bad[:8]], want[bad[:8]], tol[bad[0]])


def test_sizeof_devcfg(H, CH):
    assert H.sizeof_devcfg() == CH.sizeof_devcfg


# ---------------------------------------------------------------------------------------------- route_bounds
def _ulp4(*terms):
    """4 ulp of the largest term of an a * b + c or a one-division expression (the device may contract to an fma)"""
    return 4 * np.spacing(np.max(np.abs(np.array(np.broadcast_arrays(*terms))), axis=0))


def _route_tolerances(OPT, MPCtype, s, v, ref):
    """Per output and problem: 0 where the reference's value is a table value or a constant, else 4 ulp of the largest term"""
    c_stop, c_TL = float(OPT["stopVel"]), float(OPT["TLstopVel"])
    tol = {k: np.zeros(len(s)) for k in ref}
    m = ref["v_stop"] != 1e5
    tol["v_stop"][m] = _ulp4(ref["v_stop"] - c_stop, c_stop)[m]
    m = (ref["v_TL"] != 1e5) & (ref["v_TL"] != c_TL)
    tol["v_TL"][m] = _ulp4(ref["v_TL"] - c_TL, c_TL)[m]
    m = (v >= 5) & (v < 20)                                           # the affine middle piece of the comfort limits
    if MPCtype == 0:                                                  # EstimateRouteAndComfortBounds.m:163-166
        terms = dict(a_min=(5.5, v / 10), a_max=(14 / 3, 2 * v / 15), j_min=(35 / 6, v / 6), j_max=(35 / 6, v / 6))
    else:                                                             # :180-183, :197-200
        p = "BL" if MPCtype == 1 else "TV"
        aLo, aHi, jLo, jHi = (float(OPT[p + k]) for k in ("_a_LimLowVel", "_a_LimHighVel", "_j_LimLowVel", "_j_LimHighVel"))
        ta, tj = ((4 * aLo - aHi) / 3, (aHi - aLo) / 15 * v), ((4 * jLo - jHi) / 3, (jHi - jLo) / 15 * v)
        terms = dict(a_min=ta, a_max=ta, j_min=tj, j_max=tj)
    for k, t in terms.items():
        tol[k][m] = _ulp4(*t)[m]
    return tol


@pytest.mark.parametrize("MPCtype", sc.MPC_TYPES)
@pytest.mark.parametrize("name", sorted(sc.ROUTE_VARIANTS))
def test_route_bounds(H, CH, name, MPCtype):
    """Speed-limit and curve tables on, beside, below and beyond every knot (one, two and five knots), stops and traffic
    lights on every distance and phase edge (two in range, a cycle that wraps, times before the light's offset, a cycle of
    length zero, the stage entering as (i + 1) Tvec[i] with a variable Tvec), comfort limits at 5 and 20 and their
    neighbours, for bl_mode 0 / 1 / 2 and both trees' settings.  Table values and constants bit-equal, a * b + c and
    one-division outputs within 4 ulp of their largest term."""
    OPT, V, s, v, t0, i = sc.route_case(name, MPCtype)
    ref = sc.route_reference(OPT, MPCtype, s, v, t0, i)
    got = H.route_bounds(_cfg(CH, OPT, V), s, v, t0, i)
    tol = _route_tolerances(OPT, MPCtype, s, v, ref)
    assert sorted(got) == sorted(ref) == sorted(sh.ROUTE_OUTPUTS)
    failures = []
    for k in sh.ROUTE_OUTPUTS:
        try:
            _check("%s MPCtype %d %s" % (name, MPCtype, k), got[k], ref[k], tol[k])
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- estimate_traj
@pytest.mark.parametrize("name", sorted(sc.ESTIMATE_VARIANTS))
def test_estimate_traj(H, CH, name):
    """Modes 0 and 1 at every lane 0 .. N and three lanes beyond N (clamped to N), for the ego and the target vehicle's
    tConstACC: whole and fractional tConstACC / Ts, tConstACC < 2 Ts, a speed that reaches exactly 0 (kept by the strict >),
    stays clamped or decelerates again when a shorter step follows, uniform, non-monotone and geometric Tvec, the
    constant-velocity tail against the reference's repeated adds.  Bit-equal where every sum is exact (dyadic inputs), else
    within N eps max(1, |value|): one rounding per stage in the reference against one product on the device."""
    OPT, V, exact, runs, run, lane = sc.estimate_case(name)
    N = int(OPT["N_hor"])
    s_ref, v_ref = sc.estimate_reference(OPT, runs, run, lane)
    col = lambda k: np.array([runs[q][k] for q in run])
    s_got, v_got = H.estimate(_cfg(CH, OPT, V), col(1).astype(np.int32), col(2), col(3), col(4), col(5), lane)
    failures = []
    for nm, got, want in (("s_est", s_got, s_ref), ("v_est", v_got, v_ref)):
        tol = 0.0 if exact else N * EPS * np.maximum(1.0, np.abs(want))
        try:
            _check("%s %s" % (name, nm), got, want, tol)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, "\n".join(failures)


# ---------------------------------------------------------------------------------------------- interp_pwa
@pytest.mark.parametrize("name", sorted(sc.INTERP_TABLES))
def test_interp_pwa(H, name):
    """Below, on, beside and above every knot and inside every segment; one, two and five knots, a flat segment, a first knot
    that is not 0, infinite arguments.  Inside a segment within 2 ulp of the larger neighbouring value.  On a knot and outside
    the table bit-equal: the interpolation factor is exactly 0 or 1 there, its product with the difference of the values is
    exact, so an fma rounds as the product and the sum do (and on the right end of a segment the formula of InterpPWA.m:22-23
    does not always return the table value: the tables hold such segments)."""
    doms, vals, d, exp, tol = sc.interp_case(name)
    _check(name, H.interp_pwa(d, doms, vals), exp, tol)


# ---------------------------------------------------------------------------------------------- plant_rk4
@pytest.fixture(scope="module")
def plant_yardstick():
    """The fp64 reference's own largest distance to the 50-digit run of the same scheme, over all the variants' inputs"""
    return max(sc.plant_distance(*sc.plant_references(name)) for name in sc.PLANT_VARIANTS)


@pytest.mark.parametrize("name", sorted(sc.PLANT_VARIANTS))
def test_plant_rk4(H, CH, plant_yardstick, name):
    """Flat road (const_slope) and a sloped table with starts whose RK stages straddle a knot, forces from -1e4 N to full
    drive, standstill with braking (no clamp: the speed goes negative), s near 0 and near 1e4 m, N_integratePlant 1 and 10,
    both vehicles, against stage_ref.plant_rk4(mp=True), the same scheme at 50 digits.

    Distances are relative to max(1, |value|), the largest over s and v and all problems.  The fp64 reference is 5.49e-16
    from the 50-digit run (test_stage_ref_cpu.test_plant_fp64_against_mpmath); the device is allowed 8 times that, 4.39e-15,
    for fma contraction and the device sin / cos.  Measured on the device (MI355X): abo_sloped_m10 5.49e-16, orig_sloped_m1
    4.45e-16, abo_flat_m1 3.47e-16, orig_flat_m10 4.21e-16, so 5.49e-16 over all, the reference's own distance."""
    OPT, V, s, v, u = sc.plant_case(name)
    f0, f1, ref = sc.plant_references(name)
    s1, v1 = H.plant(_cfg(CH, OPT, V), s, v, u)
    assert not np.isnan(s1).any() and not np.isnan(v1).any()
    dist = sc.plant_distance(s1, v1, ref)
    print("%s: device against mpmath %.3e, fp64 reference against mpmath %.3e (this variant %.3e), allowed %.3e"
          % (name, dist, plant_yardstick, sc.plant_distance(f0, f1, ref), PLANT_ROOM * plant_yardstick))
    assert dist <= PLANT_ROOM * plant_yardstick
