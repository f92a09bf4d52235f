"""eepacc_kpis / Engine.kpis: the per-instance key figures (ABO/Main.m:131-263, ABO/Custom_plots.m:73-107) reduced on the
device, against report.kpi_table, its specification in numpy.

Tolerances are those of tests/test_report_table_cpu.py (its docstring has the reasoning): integer-valued fields, minima,
maxima and copied samples equal; a summed figure within 4 n u sum|terms| (u = 2^-53), a root mean square within 4 n u rms,
the speed-limit error within 4 n u (|vlim| + |v|), FE within the fuel's relative bar.  The two energies are also held
against E of eepacc_postprocess on the same trajectory, within 8 n u Ts sum|P_k| over the samples summed.

The synthetic shapes walk the kernel's paths: n_steps around the slice length L = KPI_MIN_SLICE (one slice, exactly one,
two), W L + 1 (the first length at which the slices grow beyond L), 871 (the headline), and B below, at and above a
workgroup's 64 instances and several workgroups.  Crossings lie in the first slice, in the last, on and next to every
kind of slice boundary, and nowhere."""
import ctypes as C

import numpy as np
import pytest

from conftest import make_case
from eepacc_mpc_casadi_matlab_amd import report
from eepacc_mpc_casadi_matlab_amd._abi import KPI, KPI_N, KPI_WAVES, KPI_MIN_SLICE, OUT, OUT_N

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
L, W = KPI_MIN_SLICE, KPI_WAVES
EINVAL = "libeepacc error -1"
EXACT = ("bad_exits", "distance_m", "cutoff_index", "reached", "time_cutoff_s", "a_max", "a_min", "j_max", "j_min")
CUT = 5000.0


def slice_len(n):
    return max(L, -(-n // W))


@pytest.fixture(scope="module")
def case():
    OPT, V, _, _ = make_case("ABO", 20)
    return OPT, V


@pytest.fixture(scope="module")
def eng(case):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(case[0], case[1], device=0, max_batch=256)


def crossing_indices(n):
    """Where the synthetic instances cross the cut-off: first slice, last slice, on and beside slice boundaries; None: nowhere."""
    Ls = slice_len(n)
    nS = -(-n // Ls)
    cand = {1, 2, 3, Ls - 1, Ls, Ls + 1, 2 * Ls, (nS - 1) * Ls - 1, (nS - 1) * Ls, (nS - 1) * Ls + 1, n - 2, n - 1}
    return sorted(i for i in cand if 1 <= i <= n - 1) + [None]


def synthetic(n, B, seed=0):
    """A seeded trajectory [n, OUT_N, B] and status [n, B]: s non-decreasing and placed so that instance b crosses CUT at
    crossing_indices(n)[(b + n) % len] (or stays below it), a random, a few bad exits; the rows the operator does not
    read are random too."""
    rng = np.random.default_rng(1000 * n + B + seed)
    traj = rng.uniform(-1.0, 1.0, (n, OUT_N, B))
    c = np.cumsum(rng.uniform(1.0, 6.0, (n, B)), axis=0)
    cand = crossing_indices(n)
    where = [cand[(b + n) % len(cand)] for b in range(B)]
    for b, i in enumerate(where):
        c[:, b] += (CUT - c[-1, b] - 10.0) if i is None else (CUT - 0.5 * (c[i - 1, b] + c[i, b]))
    traj[:, OUT["s"]] = c
    traj[:, OUT["v"]] = rng.uniform(0.0, 25.0, (n, B))
    traj[:, OUT["Fm"]] = rng.uniform(-3000.0, 5000.0, (n, B))
    traj[:, OUT["a"]] = rng.uniform(-3.0, 2.0, (n, B))
    status = np.zeros((n, B), dtype=np.int32)
    bad = rng.random((n, B)) < 0.03
    status[bad] = rng.choice([1, 3], size=int(bad.sum()))
    return traj, status, where


def spec_table(OPT, V, traj, status, cut):
    return report.kpi_table(traj[:, OUT["s"]], traj[:, OUT["v"]], traj[:, OUT["Fm"]], traj[:, OUT["a"]], status, OPT["Tvec"][0], cut,
                            OPT["s_speedLim"], OPT["v_speedLim"], OPT["b_fifthOrder"], V["phi"], V)


def assert_table(got, ref, OPT, V, traj, cut, what):
    """got against the specification's table ref, field by field, with the module's tolerances; prints the worst ratio."""
    n, _, B = traj.shape
    Ts = float(OPT["Tvec"][0])
    cols = np.arange(B)
    for name in EXACT:
        assert np.array_equal(got[KPI[name]], ref[KPI[name]]), (what, name, got[KPI[name]], ref[KPI[name]])
    v = traj[:, OUT["v"]]
    absP = Ts * np.abs(report.power_surface(OPT["b_fifthOrder"], traj[:, OUT["Fm"]], 30.0 / np.pi * v * V["phi"]))
    k2 = np.maximum(ref[KPI["cutoff_index"]].astype(int) - 2, 0)
    vk = np.abs(v[k2, cols])
    vlim = np.abs(ref[KPI["vlim_err"]] + v[k2, cols])
    bars = {"energy_J": absP.sum(axis=0), "energy_cutoff_J": np.cumsum(absP, axis=0)[k2, cols], "vlim_err": vlim + vk,
            "a_rms": ref[KPI["a_rms"]], "j_rms": ref[KPI["j_rms"]], "fuel_kg": ref[KPI["fuel_kg"]], "FE_L_per_100km": ref[KPI["FE_L_per_100km"]]}
    worst = {}
    for name, terms in bars.items():
        d = np.abs(got[KPI[name]] - ref[KPI[name]])
        bar = 4 * n * U * terms
        worst[name] = float(np.max(d / np.where(bar > 0, bar, 1.0)))
        assert (d <= bar).all(), (what, name, int(np.argmax(d - bar)), float(np.max(d - bar)), worst[name])
    print(what, "largest difference / bar:", {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("B", [1, 63, 65, 200])
@pytest.mark.parametrize("n", [1, 2, 3, L - 1, L, L + 1, W * L + 1, 871])
def test_synthetic_against_the_specification(eng, case, n, B):
    OPT, V = case
    traj, status, where = synthetic(n, B)
    ref = spec_table(OPT, V, traj, status, CUT)
    # the placement is what the docstring says
    want = np.array([n - 1 if i is None else i for i in where])
    assert np.array_equal(ref[KPI["cutoff_index"]], want) and np.array_equal(ref[KPI["reached"]], [i is not None and n > 1 for i in where])
    t = eng.torch
    d_traj = t.as_tensor(traj, device="cuda")
    got = eng.kpis(d_traj, t.as_tensor(status, device="cuda"), CUT)
    assert got.shape == (KPI_N, B) and got.is_cuda
    got = got.cpu().numpy()
    assert_table(got, ref, OPT, V, traj, CUT, "n=%d B=%d" % (n, B))


@pytest.mark.parametrize("B", [1, 63, 65, 200])
@pytest.mark.parametrize("n", [1, 2, 3, L - 1, L, L + 1, W * L + 1, 871])
def test_energies_against_postprocess(eng, case, n, B):
    """ENERGY_J and ENERGY_CUTOFF_J against E of eepacc_postprocess on the same trajectory, bar 8 n u Ts sum|P_k| over the
    samples summed.  k_kpis states with explicit fused multiply-adds the roundings of k_postprocess's compiled polynomial
    (csrc/eepacc_power.h), so the two differ by summation order only, and not at all where one sample is summed."""
    OPT, V = case
    traj, status, where = synthetic(n, B)
    ref = spec_table(OPT, V, traj, status, CUT)
    t = eng.torch
    d_traj = t.as_tensor(traj, device="cuda")
    got = eng.kpis(d_traj, t.as_tensor(status, device="cuda"), CUT).cpu().numpy()
    _, _, P, E = [x.cpu().numpy() for x in eng.postprocess(d_traj)]
    Ts, cols = float(OPT["Tvec"][0]), np.arange(B)
    k2 = np.maximum(ref[KPI["cutoff_index"]].astype(int) - 2, 0)
    cumP = Ts * np.cumsum(np.abs(P), axis=0)
    for name, e, terms in (("energy_J", E[-1], cumP[-1]), ("energy_cutoff_J", E[k2, cols], cumP[k2, cols])):
        d, bar = np.abs(got[KPI[name]] - e), 8 * n * U * terms
        print("n=%d B=%d %s against eepacc_postprocess: largest difference / bar %.4f" % (n, B, name, float(np.max(d / bar))))
        assert (d <= bar).all(), (name, n, B, int(np.argmax(d / bar)), float(np.max(d / bar)))
    if n == 1:
        assert np.array_equal(got[KPI["energy_J"]], E[0]) and np.array_equal(E[0], ref[KPI["energy_J"]])


def test_two_calls_agree_bit_for_bit(eng):
    traj, status, _ = synthetic(871, 200, seed=1)
    t = eng.torch
    d_traj, d_status = t.as_tensor(traj, device="cuda"), t.as_tensor(status, device="cuda")
    a = eng.kpis(d_traj, d_status, CUT).cpu().numpy()
    b = eng.kpis(d_traj, d_status, CUT).cpu().numpy()
    assert np.isfinite(a).all() and np.array_equal(a, b)


def test_rows_that_are_not_read(eng):
    traj, status, _ = synthetic(W * L + 1, 65, seed=2)
    t = eng.torch
    a = eng.kpis(t.as_tensor(traj, device="cuda"), t.as_tensor(status, device="cuda"), CUT).cpu().numpy()
    read = [OUT[k] for k in ("s", "v", "Fm", "a")]
    traj[:, [r for r in range(OUT_N) if r not in read]] = np.nan
    b = eng.kpis(t.as_tensor(traj, device="cuda"), t.as_tensor(status, device="cuda"), CUT).cpu().numpy()
    assert np.isfinite(b).all() and np.array_equal(a, b)


def test_real_run_of_a_class_handle(case, lead_trace):
    """Ten classes x two instances, interleaved, 80 steps of ABMPC in one launch, a cut-off per class: every instance's
    column against the specification with its class's constants, and bit for bit against an ordinary handle of the class."""
    from test_gpu_classes import classes_a, scenario, _mixed, _single
    OPTs, Vs = classes_a(20)
    sc = scenario(len(OPTs), 2, 80, lead_trace)
    eng = _mixed(OPTs, Vs)
    eng.set_classes(sc["class_of"])
    traj, status = eng.run_abmpc(sc["s0"], sc["v0"], sc["a_minus1"], sc["s_tv"], sc["v_tv"])
    cuts = np.linspace(40.0, 400.0, len(OPTs))
    got = eng.kpis(traj, status, cuts).cpu().numpy()
    tr, st = traj.cpu().numpy(), status.cpu().numpy()
    assert np.isfinite(got).all() and got.shape == (KPI_N, 20)
    assert 0 < got[KPI["reached"]].sum() < 20                       # both outcomes occur
    for k, (OPT, V) in enumerate(zip(OPTs, Vs)):
        idx = np.nonzero(sc["class_of"] == k)[0]
        sub = np.ascontiguousarray(tr[:, :, idx])
        ref = spec_table(OPT, V, sub, st[:, idx], cuts[k])
        assert_table(got[:, idx], ref, OPT, V, sub, cuts[k], "class %d" % k)
        one = _single(OPT, V)
        alone = one.kpis(sub, np.ascontiguousarray(st[:, idx]), cuts[k]).cpu().numpy()
        assert np.array_equal(alone, got[:, idx]), (k, np.abs(alone - got[:, idx]).max(axis=1))
    S = report.summarise_table(got, sc["class_of"])
    assert S["mean"].shape == (len(OPTs), KPI_N) and (S["count"] == 2).all()
    assert len(report.format_report("ABMPC", report.table_to_reports(got)[3], dict(OPTs[3], cutOffDist=cuts[3]))) > 100


@pytest.mark.parametrize("kind", ["bl", "fb"])
def test_other_controllers(case, lead_trace, kind):
    """The operator is not ABMPC-only: a BLMPC and an FBMPC handle at B = 4."""
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    S = Settings_BL(OPT) if kind == "bl" else OPT
    e = Engine(S, V, device=0, max_batch=4)
    n, B = (40, 4) if kind == "bl" else (10, 4)
    stv = np.repeat(s_tv[:n, None], B, 1) + np.array([0.0, 20.0, 100.0, 1e4]); vtv = np.repeat(v_tv[:n, None], B, 1)
    run = e.run_blmpc if kind == "bl" else e.run_fbmpc
    traj, status = run(np.zeros(B), np.array([0.0, 3.0, 6.0, 9.0]), np.zeros(B), stv, vtv)
    cut = 15.0
    got = e.kpis(traj, status, cut).cpu().numpy()
    tr = traj.cpu().numpy()
    assert np.isfinite(got).all() and 0 < got[KPI["reached"]].sum()
    assert_table(got, spec_table(S, V, tr, status.cpu().numpy(), cut), S, V, tr, cut, kind)


def test_refusals(eng, case, lead_trace):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    from test_gpu_classes import classes_a, scenario, _mixed
    lib, t = eng.lib, eng.torch
    traj, status, _ = synthetic(5, 4)
    d_traj, d_status = t.as_tensor(traj, device="cuda"), t.as_tensor(status, device="cuda")
    kpi = t.empty((KPI_N, 4), dtype=t.float64, device="cuda")
    cut = (C.c_double * 1)(CUT)
    args = dict(traj=d_traj.data_ptr(), status=d_status.data_ptr(), cutoff_dist_host=cut, kpi=kpi.data_ptr())
    call = lambda B=4, n=5, **kw: lib.eepacc_kpis(eng.h, B, n, *[dict(args, **kw)[k] for k in ("traj", "status", "cutoff_dist_host", "kpi")], None)
    for name in args:
        assert call(**{name: None}) == -1 and ("eepacc_kpis: %s is NULL" % name).encode() in lib.eepacc_last_error()
    assert call(n=0) == -1 and b"n_steps" in lib.eepacc_last_error()
    assert call(n=-3) == -1 and b"n_steps" in lib.eepacc_last_error()
    assert call(B=257) == -1 and b"max_batch" in lib.eepacc_last_error() and b"B = 257" in lib.eepacc_last_error()
    assert call(B=0) == 0
    assert call() == 0
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(EepaccError, match=EINVAL + r".*cutoff_dist_host\[0\] is not finite"):
            eng.kpis(d_traj, d_status, bad)
    with pytest.raises(ValueError):
        eng.kpis(d_traj, d_status, [1.0, 2.0])                     # one class: one cut-off
    # a class handle: the map must be set, and for this B
    OPTs, Vs = classes_a(20)
    ce = _mixed(OPTs[:3], Vs[:3], max_batch=8)
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_kpis: eepacc_set_classes has not been called"):
        ce.kpis(d_traj, d_status, CUT)
    ce.set_classes([0, 1, 2, 0, 1, 2])
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_kpis: B = 4 differs"):
        ce.kpis(d_traj, d_status, CUT)
    with pytest.raises(EepaccError, match=EINVAL + r".*cutoff_dist_host\[2\] is not finite"):
        ce.kpis(d_traj, d_status, [1.0, 2.0, np.nan])
    ce.set_classes([2, 1, 0, 2])
    assert np.isfinite(ce.kpis(d_traj, d_status, [CUT, CUT + 1.0, CUT + 2.0]).cpu().numpy()).all()
    eng.synchronize()


def test_no_effect_on_a_resumed_run(case, lead_trace):
    """kpis between two chunks of a closed loop: the resumed chunk is bit for bit what it is without the call."""
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    B, n1, n2 = 5, 30, 20
    stv = np.repeat(s_tv[:n1 + n2, None], B, 1) + np.linspace(0.0, 80.0, B); vtv = np.repeat(v_tv[:n1 + n2, None], B, 1)
    z, v0 = np.zeros(B), np.linspace(0.0, 8.0, B)
    e = Engine(OPT, V, device=0, max_batch=8)
    outs = []
    for with_kpis in (False, True):
        head, hst = e.run_abmpc(z, v0, z, stv[:n1], vtv[:n1])
        if with_kpis:
            k = e.kpis(head, hst, 100.0)
            assert np.isfinite(k.cpu().numpy()).all()
        tail, tst = e.run_abmpc(z, v0, z, stv[n1:], vtv[n1:], resume=True)
        e.synchronize()
        outs.append((head.cpu().numpy(), hst.cpu().numpy(), tail.cpu().numpy(), tst.cpu().numpy()))
    for a, b in zip(*outs):
        assert np.array_equal(a, b)
    assert np.abs(outs[0][2][0, OUT["s"]] - outs[0][0][-1, OUT["s"]]).max() < 20.0      # the tail continues the head
