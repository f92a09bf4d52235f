"""eepacc_route_kpis / Engine.route_kpis: the route-compliance key figures (speed limit, curve speed, stop profile, red lights:
ABO/Main.m:374-433, :486-534; comfort envelope: EstimateRouteAndComfortBounds.m:154-189) reduced on the device from synthetic
trajectories, against report.route_table / report.route_limits, the specification (tests/test_route_table_cpu.py checks that
one by hand, against a plain loop and against the planner's own look-up).

Bar: np.array_equal, for every field and for `limits`.  Every figure is a maximum, a minimum, a count or an index of values
that are each rounded once, and the kernel's unit is compiled with contraction off: there is nothing to tolerate.

Shapes.  n_steps: 1, 2, 7 and 8 are one slice of one wave (8 fills it), 9 is the first two-slice case, 128 fills all sixteen
waves at the minimum slice length L = 8, at 129 the slices grow to 9 with a last one that is empty, at 130 it is partial.
B: 1, 63 and 64 are one workgroup, 65 and 130 have a part-filled last one.  What is planted on the edges: synthetic()."""
import numpy as np
import pytest

from eepacc_mpc_casadi_matlab_amd import report
from eepacc_mpc_casadi_matlab_amd._abi import KPI_MIN_SLICE, KPI_WAVES, OUT, OUT_N, RKPI, RKPI_FIELDS, RKPI_N, RLIM, RLIM_N

pytestmark = pytest.mark.gpu

INF = np.inf
EINVAL = "libeepacc error -1"
KINDS = 6
TS = 0.5
T_START = 3.5                      # light A (offset 5 s) turns red exactly at t_3
TOL = (0.25, 0.125, 0.5)
STOPS = [200.0, 520.0]
LIGHTS = [[330.0, 5.0, 20.0, 25.0],        # A: red on [5, 25) + 45 i
          [515.0, 1000.0, 10.0, 10.0],     # B: every sample lies before its offset (negative argument of mod)
          [525.0, 30.0, 0.0, 0.0],         # C: a cycle of length 0, mod returns its argument: red before t = 30, green from there
          [600.0, 0.0, 15.0, 15.0]]


def slice_len(n):
    return max(KPI_MIN_SLICE, -(-n // KPI_WAVES))


def settings(tree, which):
    """Full settings of a tree with a route that has every feature ("full"), none ("bare": one-knot tables, no stops, no
    lights), or the full one on a handle of the baseline controller ("bl")."""
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, default_opt
    OPT = default_opt()
    if which == "bare":
        OPT.update(slopes=np.zeros((0, 3)), speedLimZones=np.array([[60.0, 0.0]]), curves=np.zeros((0, 3)), stopLoc=np.zeros(0),
                   TLLoc=np.zeros((0, 4)))
    else:
        OPT.update(slopes=np.array([[3.0, 40, 160]]), speedLimZones=np.array([[50.0, 0.0], [30.0, 150.0], [70.0, 400.0]]),
                   curves=np.array([[-1 / 25.0, 90, 120], [1 / 60.0, 250, 300]]), stopLoc=np.array(STOPS), TLLoc=np.array(LIGHTS))
    OPT = Settings(OPT, tree=tree, N_hor=20)
    if which == "bare":                                              # GenerateUseCase brackets a zone with knots: one knot each here
        OPT.update(s_speedLim=OPT["s_speedLim"][:1], v_speedLim=OPT["v_speedLim"][:1], s_curv=OPT["s_curv"][:1], curvature=OPT["curvature"][:1])
    return (Settings_BL(OPT) if which == "bl" else OPT), SetVehicleParameters(tree)


CASES = [("ABO", "full"), ("ORIG", "full"), ("ABO", "bare"), ("ORIG", "bare"), ("ORIG", "bl")]


@pytest.fixture(scope="module")
def engines():
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    out = {}
    for tree, which in CASES:
        OPT, V = settings(tree, which)
        out[tree, which] = (Engine(OPT, V, device=0, max_batch=256), OPT, int(OPT.get("bl_mode", 0)))
    return out


def synthetic(n, B, OPT, seed=0):
    """A seeded trajectory [n, OUT_N, B] over the route of settings("...", "full") and, per instance, what was planted.  With
    L = slice_len(n), instance b has, by b % 6 (where n allows it):
      0  the stop line at 200 m crossed on the first step of slice 1 (k = L; n <= L: at k = 1), arriving exactly on it
      1  two lights and a stop (515, 520, 525 m) crossed in the last step
      2  a sample exactly on a light, the next one beyond it: `<` on the left, nothing is crossed (odd b // 6: the stop line
         at 200 m crossed at k = 1 instead)
      3  the largest excess over the speed limit twice, on the last step of slice 0 and the first of slice 1 (n <= L: first
         and last step): VLIM_EXCESS_INDEX is the earlier one
      4  NaN and -0.0 in v, v on 5 and 20, s on speed-limit and curve knots and one ulp either side
      5  s at exactly stopRefDist and TLStopRegionSize in front of light A while it is red (odd b // 6: light A crossed in
         the step to k = 3, green at t_2, red exactly from t_3: possible, not certain)
    Every row the operator does not read is random too; v and a are multiples of 1/8."""
    rng = np.random.default_rng(1000 * n + B + seed)
    L = slice_len(n)
    traj = rng.uniform(-1.0, 1.0, (n, OUT_N, B))
    s = np.cumsum(rng.integers(0, max(2, 5600 // n), (n, B)), axis=0) / 8.0 - 5.0
    v = rng.integers(-4, 280, (n, B)) / 8.0
    a = rng.integers(-48, 41, (n, B)) / 8.0
    knots = np.concatenate([OPT["s_speedLim"], OPT["s_curv"]])
    planted = []
    for b in range(B):
        kind, odd = b % KINDS, (b // KINDS) % 2
        what = {"kind": kind}
        if kind == 0 and n >= 2:
            k = L if n > L else 1
            s[k - 1, b], s[k, b] = STOPS[0] - 0.5, STOPS[0]
            v[k - 1, b], v[k, b] = 3.0, 2.0
            what.update(stops_min=1.0, cross_v_min=2.0)
        elif kind == 1 and n >= 2:
            s[n - 2, b], s[n - 1, b] = 510.0, 530.0
            what.update(stops_min=1.0, lights_min=2.0)
        elif kind == 2 and n >= 2:
            s[:, b] = np.linspace(0.0, 100.0, n)
            s[0, b], s[1, b] = (STOPS[0] - 0.5, STOPS[0]) if odd else (LIGHTS[0][0], LIGHTS[0][0] + 1.0)
            what.update(stops_passed=float(odd), tl_passed=0.0)
        elif kind == 3:
            ka, kb = (L - 1, L) if n > L else (0, n - 1)
            s[:, b] = np.linspace(10.0, 140.0, n) if n > 1 else 10.0
            v[:, b] = np.minimum(v[:, b], 10.0)
            v[ka, b] = v[kb, b] = 40.0
            what.update(vlim_excess_index=float(ka), vlim_excess_max=40.0 - float(OPT["v_speedLim"][1]))
        elif kind == 4:
            for k in rng.choice(n, size=min(n, 9), replace=False):
                m = knots[rng.integers(knots.size)]
                s[k, b] = (m, np.nextafter(m, INF), np.nextafter(m, -INF))[rng.integers(3)]
            for k, x in zip(rng.permutation(n)[:4], (5.0, 20.0, -0.0, np.nan)):
                v[k, b] = x
        elif kind == 5 and n >= 5:
            if odd:
                s[2, b], s[3, b] = LIGHTS[0][0] - 0.5, LIGHTS[0][0]
                what.update(possible_min=1.0)
            else:
                s[3, b], s[4, b] = LIGHTS[0][0] - OPT["stopRefDist"], LIGHTS[0][0] - OPT["TLStopRegionSize"]
        planted.append(what)
    traj[:, OUT["s"]] = s
    traj[:, OUT["v"]] = v
    traj[:, OUT["a"]] = a
    return traj, np.zeros((n, B), dtype=np.int32), planted


def spec(traj, OPT, bl_mode, t_start=T_START, tol=TOL):
    s, v, a = [traj[:, OUT[k]] for k in ("s", "v", "a")]
    return report.route_table(s, v, a, TS, t_start, tol, OPT, bl_mode), report.route_limits(s, TS, t_start, OPT)


def assert_equal(got, ref, what):
    for name in RKPI_FIELDS:
        assert np.array_equal(got[RKPI[name]], ref[RKPI[name]]), (what, name, got[RKPI[name]], ref[RKPI[name]])
    assert not np.isnan(got).any()


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 2, 7, 8, 9, 128, 129, 130])
def test_synthetic_against_the_specification(engines, n, B):
    t = engines["ABO", "full"][0].torch
    traj, status, planted = synthetic(n, B, engines["ABO", "full"][1])
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status)]
    for case in CASES:
        eng, OPT, bl_mode = engines[case]
        ref, ref_lim = spec(traj, OPT, bl_mode)
        if case == ("ABO", "full"):                                  # the placement is what the docstring says
            for b, what in enumerate(planted):
                r = {k: ref[i, b] for k, i in RKPI.items()}
                for name, want in what.items():
                    ok = {"kind": True, "stops_min": r["stops_passed"] >= want, "lights_min": r["tl_passed"] >= want,
                          "cross_v_min": r["stop_cross_v_max"] >= want, "possible_min": r["red_crossings_possible"] >= want
                          and r["red_crossings_possible"] > r["red_crossings"]}.get(name)
                    assert ok if ok is not None else r[name] == want, (b, what, name, r)
            if n >= 5:
                k3 = ref_lim[3, RLIM["v_tl"]]
                assert (k3[[b for b in range(B) if b % KINDS == 5 and (b // KINDS) % 2 == 0]] == 1e5).all()      # exactly stopRefDist away
        got, lim = eng.route_kpis(*dev, t_start=T_START, tol=TOL, want_limits=True)
        assert got.shape == (RKPI_N, B) and lim.shape == (n, RLIM_N, B) and got.is_cuda and lim.is_cuda
        got, lim = got.cpu().numpy(), lim.cpu().numpy()
        assert_equal(got, ref, "n=%d B=%d %s" % (n, B, case))
        assert np.array_equal(lim, ref_lim), ("limits", n, B, case, np.argwhere(lim != ref_lim)[:4])
        alone = eng.route_kpis(*dev, t_start=T_START, tol=TOL).cpu().numpy()           # limits = NULL: the same table
        assert np.array_equal(alone, got, equal_nan=True)
        if n == 1:
            assert (got[[RKPI["j_over_max"], RKPI["j_under_max"]]] == -INF).all() and (got[RKPI["stops_passed"]] == 0.0).all()
        if case[1] == "bare":
            assert (got[RKPI["vtl_excess_max"]] == -INF).all() and (got[RKPI["tl_passed"]] == 0.0).all() and (lim[:, RLIM["v_stop"]] == 1e5).all()


def test_t_start_and_tolerances_reach_the_kernel(engines):
    eng, OPT, bl_mode = engines["ORIG", "full"]
    traj, status, _ = synthetic(130, 65, OPT, seed=6)
    tables = []
    for t_start, tol in ((0.0, (0.0, 0.0, 0.0)), (0.0, TOL), (17.5, TOL), (1e6 + 0.1, (3.0, 1.0, 2.0))):
        ref, ref_lim = spec(traj, OPT, bl_mode, t_start, tol)
        got, lim = [x.cpu().numpy() for x in eng.route_kpis(traj, status, t_start=t_start, tol=tol, want_limits=True)]
        assert_equal(got, ref, (t_start, tol))
        assert np.array_equal(lim, ref_lim)
        tables.append(got)
    assert not np.array_equal(tables[0], tables[1]) and not np.array_equal(tables[1], tables[2])


def test_two_calls_agree_bit_for_bit(engines):
    eng, OPT, _ = engines["ABO", "full"]
    traj, status, _ = synthetic(130, 130, OPT, seed=1)
    t = eng.torch
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status)]
    a = [x.cpu().numpy() for x in eng.route_kpis(*dev, t_start=T_START, tol=TOL, want_limits=True)]
    b = [x.cpu().numpy() for x in eng.route_kpis(*dev, t_start=T_START, tol=TOL, want_limits=True)]
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and not np.isnan(a[0]).any()


@pytest.mark.parametrize("n", [9, 129])
def test_a_column_does_not_depend_on_its_place_or_on_B(engines, n):
    """The same instances at other positions of another B: every column of the table and of limits, bit for bit."""
    eng, OPT, _ = engines["ORIG", "full"]
    traj, status, _ = synthetic(n, 130, OPT, seed=2)
    kw = dict(t_start=T_START, tol=TOL, want_limits=True)
    whole, wl = [x.cpu().numpy() for x in eng.route_kpis(traj, status, **kw)]
    cols = np.random.default_rng(5).permutation(130)[:65]
    part, pl = [x.cpu().numpy() for x in eng.route_kpis(np.ascontiguousarray(traj[:, :, cols]), np.ascontiguousarray(status[:, cols]), **kw)]
    assert np.array_equal(part, whole[:, cols]) and np.array_equal(pl, wl[:, :, cols])
    one, ol = [x.cpu().numpy() for x in eng.route_kpis(np.ascontiguousarray(traj[:, :, 77:78]), status[:, 77:78].copy(), **kw)]
    assert np.array_equal(one[:, 0], whole[:, 77]) and np.array_equal(ol[:, :, 0], wl[:, :, 77])


def test_rows_that_are_not_read(engines):
    """Only s, v and a are read; status is not read either."""
    eng, OPT, _ = engines["ABO", "full"]
    traj, status, _ = synthetic(129, 65, OPT, seed=3)
    a = eng.route_kpis(traj, status, t_start=T_START, tol=TOL).cpu().numpy()
    traj[:, [r for r in range(OUT_N) if r not in (OUT["s"], OUT["v"], OUT["a"])]] = np.nan
    assert np.array_equal(a, eng.route_kpis(traj, status + 7, t_start=T_START, tol=TOL).cpu().numpy())


def test_class_handle_synthetic(engines):
    """Three classes (the full route of ORIG, the bare one, the full one with other stop / light constants), two instances
    each, interleaved: every column equals that of an ordinary handle of its class, and the specification with the class's
    settings, bit for bit; before eepacc_set_classes, and with a map for another B, the call is refused."""
    from test_gpu_classes import _mixed, _single
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    full, V = settings("ORIG", "full")
    OPTs = [full, settings("ORIG", "bare")[0], dict(full, stopRefDist=60.0, stopVel=0.5, TLstopVel=0.25, TLStopRegionSize=5.0, stopRefVelSlope=0.75)]
    traj, status, _ = synthetic(129, 6, full, seed=4)
    class_of = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    ce = _mixed(OPTs, [V] * 3, max_batch=8)
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_route_kpis: eepacc_set_classes has not been called"):
        ce.route_kpis(traj, status)
    ce.set_classes([0, 1, 2, 0])
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_route_kpis: B = 6 differs"):
        ce.route_kpis(traj, status)
    ce.set_classes(class_of)
    got, lim = [x.cpu().numpy() for x in ce.route_kpis(traj, status, t_start=T_START, tol=TOL, want_limits=True)]
    for k, OPT in enumerate(OPTs):
        idx = np.nonzero(class_of == k)[0]
        sub = [np.ascontiguousarray(x[..., idx]) for x in (traj, status)]
        alone, al = [x.cpu().numpy() for x in _single(OPT, V, max_batch=8).route_kpis(*sub, t_start=T_START, tol=TOL, want_limits=True)]
        assert np.array_equal(alone, got[:, idx]) and np.array_equal(al, lim[:, :, idx]), k
        ref, ref_lim = spec(sub[0], OPT, 0)
        assert_equal(got[:, idx], ref, "class %d" % k)
        assert np.array_equal(lim[:, :, idx], ref_lim)
    v_stop = lim[:, RLIM["v_stop"]]                                                      # the classes do differ
    assert (v_stop[:, class_of == 1] == 1e5).all() and (v_stop[:, class_of != 1] < 1e5).all()
    assert not np.array_equal(spec(traj[:, :, :1], OPTs[0], 0)[1], spec(traj[:, :, :1], OPTs[2], 0)[1])
    S = report.summarise_table(got, class_of)
    assert S["mean"].shape == (3, RKPI_N) and (S["count"] == 2).all() and not np.isnan(S["mean"]).any()


def test_refusals(engines):
    import ctypes as C
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    eng, OPT, bl_mode = engines["ABO", "full"]
    lib, t = eng.lib, eng.torch
    traj, status, _ = synthetic(5, 4, OPT)
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status)]
    rkpi = t.empty((RKPI_N, 4), dtype=t.float64, device="cuda")
    tol3 = lambda *x: (C.c_double * 3)(*x)
    names = ("tol", "traj", "status", "rkpi", "limits")
    args = dict(tol=tol3(*TOL), traj=dev[0].data_ptr(), status=dev[1].data_ptr(), rkpi=rkpi.data_ptr(), limits=None)

    def call(B=4, n=5, t_start=T_START, **kw):
        rc = lib.eepacc_route_kpis(eng.h, B, n, t_start, *[dict(args, **kw)[k] for k in names], None)
        return rc, lib.eepacc_last_error().decode()
    for name, text in (("tol", "tol_host"), ("traj", "traj"), ("status", "status"), ("rkpi", "rkpi")):
        rc, msg = call(**{name: None})
        assert rc == -1 and "eepacc_route_kpis: %s is NULL" % text in msg, msg
    for bad in (0, -3):
        rc, msg = call(n=bad)
        assert rc == -1 and "eepacc_route_kpis: n_steps = %d" % bad in msg, msg
    rc, msg = call(B=257)
    assert rc == -1 and "B = 257" in msg and "max_batch" in msg, msg
    rc, msg = call(B=-1)
    assert rc == -1 and "B = -1" in msg, msg
    for i, name in enumerate(("v_tol", "a_tol", "j_tol")):
        for bad in (-0.5, INF, np.nan):
            x = list(TOL); x[i] = bad
            rc, msg = call(tol=tol3(*x))
            assert rc == -1 and "tol_host[%d] (%s)" % (i, name) in msg, msg
    for bad in (INF, np.nan):
        rc, msg = call(t_start=bad)
        assert rc == -1 and "eepacc_route_kpis: t_start" in msg, msg
    assert call(B=0)[0] == 0
    assert call()[0] == 0
    with pytest.raises(ValueError):
        eng.route_kpis(dev[0], dev[1][:4])
    with pytest.raises(ValueError):
        eng.route_kpis(*dev, tol=(0.0, 0.0))
    with pytest.raises(EepaccError, match=EINVAL + ".*v_tol"):
        eng.route_kpis(*dev, tol=(-1.0, 0.0, 0.0))
    eng.synchronize()
    assert_equal(rkpi.cpu().numpy(), spec(traj, OPT, bl_mode)[0], "raw call")
