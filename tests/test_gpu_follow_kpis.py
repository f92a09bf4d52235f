"""eepacc_follow_kpis / Engine.follow_kpis: the vehicle-following and cost key figures (ABO/Main.m:679-771,
RunOpt_ABMPC.m:382-404, RunOpt_FBMPC.m:373-397) reduced on the device, against report.follow_table, its specification.

Bars (tests/test_follow_table_cpu.py has the reasoning): the counts, the index, the four minima and the maximum equal the
specification's bit for bit; a cost within 4 n u |w| sum|terms|, u = 2^-53, the specification adding in the order of k and
the device slice by slice.

The synthetic shapes walk the kernel's paths.  n_steps: 1, 2, 3 and 8 are one slice of one wave (8 fills it), 9 is the
first two-slice case, 128 fills all sixteen waves at the minimum slice length L = 8, at 129 the slices grow to 9, 130.
B: 1, 63 and 64 are one workgroup (part-filled, part-filled, full), 65 and 130 have a part-filled last one.  The planted
features sit on slice boundaries (synthetic()).  Gaps and positions are multiples of 1/8 m, so that planted equal gaps are
equal in floating point."""
import ctypes as C

import numpy as np
import pytest

from conftest import GOLDEN_AB_VARIANTS, make_case
from eepacc_mpc_casadi_matlab_amd import report
from eepacc_mpc_casadi_matlab_amd._abi import FKPI, FKPI_FIELDS, FKPI_N, KPI_WAVES, KPI_MIN_SLICE, OUT, OUT_N

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
INF = np.inf
EINVAL = "libeepacc error -1"
EXACT = FKPI_FIELDS[:FKPI["cost_P"]]
COSTS = FKPI_FIELDS[FKPI["cost_P"]:]
READ = ("s", "v", "Fm", "a", "xi_v", "xi_h", "xi_s", "xi_f")
KINDS = 6


def slice_len(n):
    return max(KPI_MIN_SLICE, -(-n // KPI_WAVES))


@pytest.fixture(scope="module")
def case():
    # seven distinct W_AB entries (a weight set of the saved solutions): a shifted or permuted weight shows
    OPT, V, _, _ = make_case("ABO", 20, W_AB=np.array(GOLDEN_AB_VARIANTS["abo_abmpc_fcopt"]))
    return OPT, V


@pytest.fixture(scope="module")
def eng(case):
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    return Engine(case[0], case[1], device=0, max_batch=256)


def synthetic(n, B, seed=0):
    """A seeded trajectory [n, OUT_N, B], lead traces [n, B] and, per instance, what was planted.  With L = slice_len(n) and
    nS slices, instance b has, by b % 6:
      0  the smallest gap (1 m) on the last step of slice 0 and again on the first step of slice 1 (n <= L: on the first and
         the last step): H_MIN_INDEX is the earlier one
      1  a lead on the last step only
      2  a lead that is faster than the ego except at one sample of the last slice (its first step, or the last step of all)
      3  no lead before k = L, one from there on (n <= L: none at all)
      4  a lead with gaps in it (inf, one NaN)
      5  a lead throughout
    Every row the operator does not read is random too."""
    rng = np.random.default_rng(1000 * n + B + seed)
    L = slice_len(n)
    nS = -(-n // L)
    traj = rng.uniform(-1.0, 1.0, (n, OUT_N, B))
    s = np.cumsum(rng.integers(4, 24, (n, B)), axis=0) / 4.0
    v = rng.integers(0, 200, (n, B)) / 8.0
    v[rng.random((n, B)) < 0.05] = 0.0
    s_tv = s + rng.integers(80, 480, (n, B)) / 8.0
    v_tv = v + rng.uniform(-3.0, 3.0, (n, B))
    planted = []
    for b in range(B):
        kind = b % KINDS
        what = {"kind": kind}
        if kind == 0:
            ka, kb = (L - 1, L) if n > L else (0, n - 1)
            s_tv[ka, b] = s[ka, b] + 1.0; s_tv[kb, b] = s[kb, b] + 1.0
            what.update(h_min_m=1.0, h_min_index=float(ka))
        elif kind == 1:
            s_tv[:n - 1, b] = INF
            what.update(lead_samples=1.0, h_min_index=float(n - 1))
        elif kind == 2:
            kc = n - 1 if (b // KINDS) % 2 else (nS - 1) * L
            v_tv[:, b] = v[:, b] + 1.0
            v[kc, b] = 10.0; v_tv[kc, b] = 8.0
            what.update(ttc_min_s=(s_tv[kc, b] - s[kc, b]) / 2.0)
        elif kind == 3:
            s_tv[:L, b] = INF
            what.update(lead_samples=float(max(n - L, 0)))
        elif kind == 4:
            s_tv[rng.random(n) < 0.25, b] = INF
            s_tv[rng.integers(0, n), b] = np.nan
        planted.append(what)
    traj[:, OUT["s"]] = s
    traj[:, OUT["v"]] = v
    traj[:, OUT["Fm"]] = rng.uniform(-3000.0, 5000.0, (n, B))
    traj[:, OUT["a"]] = rng.uniform(-3.0, 2.0, (n, B))
    for k in ("xi_v", "xi_h", "xi_s", "xi_f"):
        traj[:, OUT[k]] = np.where(rng.random((n, B)) < 0.5, rng.uniform(0.0, 2.0, (n, B)), 0.0)
    return traj, np.zeros((n, B), dtype=np.int32), np.ascontiguousarray(s_tv), np.ascontiguousarray(v_tv), planted


def spec_table(OPT, V, traj, s_tv, v_tv, weights):
    rows = [traj[:, OUT[k]] for k in READ]
    return report.follow_table(*rows, s_tv, v_tv, OPT["Tvec"][0], OPT["h_min"], OPT["tau_min"], report.follow_weights(OPT, weights),
                               OPT["b_fifthOrder"], V["phi"])


def assert_table(got, ref, OPT, V, traj, weights, what):
    """got against the specification's table ref, field by field, with the module's bars; prints the worst ratio."""
    n = traj.shape[0]
    for name in EXACT:
        assert np.array_equal(got[FKPI[name]], ref[FKPI[name]]), (what, name, got[FKPI[name]], ref[FKPI[name]])
    s, v, Fm, a, xi_v, xi_h, xi_s, xi_f = [traj[:n - 1, OUT[k]] for k in READ]
    W = report.follow_weights(OPT, weights)
    j = np.diff(traj[:, OUT["a"]], axis=0) / float(OPT["Tvec"][0])
    P = report.power_surface(OPT["b_fifthOrder"], Fm, 30.0 / np.pi * v * V["phi"]) if W[0] != 0.0 else np.zeros_like(v)
    worst = {}
    for w, name, terms in zip(W, COSTS, (P * P, a * a, j * j, xi_v, xi_h, xi_s, xi_f)):
        d = np.abs(got[FKPI[name]] - ref[FKPI[name]])
        bar = 4 * n * U * abs(w) * np.abs(terms).sum(axis=0)
        worst[name] = float(np.max(d / np.where(bar > 0, bar, 1.0)))
        assert (d <= bar).all(), (what, name, int(np.argmax(d - bar)), float(np.max(d - bar)), worst[name])
    print(what, "largest difference / bar:", {k: round(x, 4) for k, x in worst.items()})


@pytest.mark.parametrize("B", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("n", [1, 2, 3, 8, 9, 128, 129, 130])
def test_synthetic_against_the_specification(eng, case, n, B):
    OPT, V = case
    traj, status, s_tv, v_tv, planted = synthetic(n, B)
    t = eng.torch
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status, s_tv, v_tv)]
    for weights in ("ab", "fb", "none"):
        ref = spec_table(OPT, V, traj, s_tv, v_tv, weights)
        if weights == "ab":                                         # the placement is what the docstring says
            for b, what in enumerate(planted):
                for name, want in what.items():
                    assert name == "kind" or ref[FKPI[name], b] == want, (b, what, name, ref[FKPI[name], b])
        got = eng.follow_kpis(*dev, weights=weights)
        assert got.shape == (FKPI_N, B) and got.is_cuda
        got = got.cpu().numpy()
        assert_table(got, ref, OPT, V, traj, weights, "n=%d B=%d %s" % (n, B, weights))
        if n == 1:
            assert (got[FKPI["cost_P"]:] == 0.0).all()              # the sums of k = 1:N_sim are empty
        if weights != "fb":
            assert (got[FKPI["cost_P"]] == 0.0).all()
        elif n > 1:
            assert (got[FKPI["cost_P"]] > 0.0).all()


def test_two_calls_agree_bit_for_bit(eng):
    traj, status, s_tv, v_tv, _ = synthetic(130, 130, seed=1)
    t = eng.torch
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status, s_tv, v_tv)]
    a = eng.follow_kpis(*dev, weights="fb").cpu().numpy()
    b = eng.follow_kpis(*dev, weights="fb").cpu().numpy()
    assert not np.isnan(a).any() and np.array_equal(a, b)


@pytest.mark.parametrize("n", [9, 129])
def test_a_column_does_not_depend_on_its_place_or_on_B(eng, n):
    """The same instances at other positions of another B: every column, the sums included, bit for bit."""
    traj, status, s_tv, v_tv, _ = synthetic(n, 130, seed=2)
    t = eng.torch
    whole = eng.follow_kpis(traj, status, s_tv, v_tv, weights="fb").cpu().numpy()
    cols = np.random.default_rng(5).permutation(130)[:65]
    part = eng.follow_kpis(np.ascontiguousarray(traj[:, :, cols]), np.ascontiguousarray(status[:, cols]), np.ascontiguousarray(s_tv[:, cols]),
                           np.ascontiguousarray(v_tv[:, cols]), weights="fb").cpu().numpy()
    assert np.array_equal(part, whole[:, cols])
    one = eng.follow_kpis(np.ascontiguousarray(traj[:, :, 77:78]), status[:, 77:78].copy(), s_tv[:, 77:78].copy(), v_tv[:, 77:78].copy(),
                          weights="fb").cpu().numpy()
    assert np.array_equal(one[:, 0], whole[:, 77])


def test_rows_that_are_not_read(eng):
    """Fb, cost, DistHor and a_qp are never read, Fm only where COST_P has a weight."""
    traj, status, s_tv, v_tv, _ = synthetic(129, 65, seed=3)
    a = {w: eng.follow_kpis(traj, status, s_tv, v_tv, weights=w).cpu().numpy() for w in ("ab", "fb")}
    traj[:, [r for r in range(OUT_N) if r not in [OUT[k] for k in READ]]] = np.nan
    assert np.array_equal(a["fb"], eng.follow_kpis(traj, status, s_tv, v_tv, weights="fb").cpu().numpy())
    traj[:, OUT["Fm"]] = np.nan
    assert np.array_equal(a["ab"], eng.follow_kpis(traj, status, s_tv, v_tv, weights="ab").cpu().numpy())


@pytest.mark.parametrize("kind", ["ab", "fb", "bl"])
def test_real_run(case, lead_trace, kind):
    """One closed loop per weight set at the smallest real size (N = 20, B = 4, 40 steps, S2 leads from tight following
    to a far one): the table from the device traj against follow_table of the copied traj."""
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL
    OPT, V = case
    S = Settings_BL(OPT) if kind == "bl" else OPT
    weights = {"ab": "ab", "fb": "fb", "bl": "none"}[kind]
    e = Engine(S, V, device=0, max_batch=4)
    n, B = 40, 4
    sc = make_s2(B, n, lead_trace["V_TO_2Hz"], seed=11)
    s_tv = np.ascontiguousarray(sc["s_tv"] + np.array([5.0, 1e4, 60.0, 150.0])[None, :])
    run = {"ab": e.run_abmpc, "fb": e.run_fbmpc, "bl": e.run_blmpc}[kind]
    traj, status = run(sc["s0"], sc["v0"], sc["a_minus1"], s_tv, sc["v_tv"])
    got = e.follow_kpis(traj, status, s_tv, sc["v_tv"], weights=weights).cpu().numpy()
    tr = traj.cpu().numpy()
    assert np.isfinite(tr).all() and got.shape == (FKPI_N, B)
    assert (got[FKPI["lead_samples"]] == n).all() and (got[FKPI["h_min_m"]] < 1e5).all() and got[FKPI["h_min_m"], 1] > 5e3
    assert (got[FKPI["cost_a"]] > 0.0).all() and (got[FKPI["cost_P"]] > 0.0).all() == (kind == "fb")
    assert_table(got, spec_table(S, V, tr, s_tv, sc["v_tv"], weights), S, V, tr, weights, kind)


def _class_settings():
    OPT, V, _, _ = make_case("ORIG", 20)
    OPTs = [OPT,
            dict(OPT, h_min=3.5, tau_min=0.8, W_AB=OPT["W_AB"] * np.array([3.0, 0.5, 1.0, 2.0, 1.0, 1.0])),
            dict(OPT, h_min=1.0, tau_min=1.25, W_AB=OPT["W_AB"] * np.array([0.25, 2.0, 4.0, 0.5, 3.0, 1.0]))]
    return OPTs, [V] * 3


def test_class_handle():
    """Three classes that differ in h_min, tau_min and W_AB, two instances each, interleaved: every column equals that of
    an ordinary handle of its class bit for bit (and the specification with the class's constants: ORIG's six W_AB entries
    are stored behind a leading zero, the weights must be the user's W(1..5) all the same)."""
    from test_gpu_classes import _mixed, _single
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    OPTs, Vs = _class_settings()
    traj, status, s_tv, v_tv, _ = synthetic(129, 6, seed=4)
    class_of = np.array([0, 1, 2, 0, 1, 2], dtype=np.int32)
    ce = _mixed(OPTs, Vs, max_batch=8)
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_follow_kpis: eepacc_set_classes has not been called"):
        ce.follow_kpis(traj, status, s_tv, v_tv)
    ce.set_classes([0, 1, 2, 0])
    with pytest.raises(EepaccError, match=EINVAL + ".*eepacc_follow_kpis: B = 6 differs"):
        ce.follow_kpis(traj, status, s_tv, v_tv)
    ce.set_classes(class_of)
    for weights in ("ab", "fb", "none"):
        got = ce.follow_kpis(traj, status, s_tv, v_tv, weights=weights).cpu().numpy()
        for k, (OPT, V) in enumerate(zip(OPTs, Vs)):
            idx = np.nonzero(class_of == k)[0]
            sub = [np.ascontiguousarray(x[..., idx]) for x in (traj, status, s_tv, v_tv)]
            alone = _single(OPT, V, max_batch=8).follow_kpis(*sub, weights=weights).cpu().numpy()
            assert np.array_equal(alone, got[:, idx]), (weights, k, np.abs(alone - got[:, idx]).max(axis=1))
            assert_table(got[:, idx], spec_table(OPT, V, sub[0], sub[2], sub[3], weights), OPT, V, sub[0], weights, "class %d %s" % (k, weights))
    ab = ce.follow_kpis(traj, status, s_tv, v_tv, weights="ab").cpu().numpy()
    assert not np.array_equal(ab[FKPI["margin_min_m"], 0], ab[FKPI["margin_min_m"], 1])       # the classes do differ
    S = report.summarise_table(ab, class_of)
    assert S["mean"].shape == (3, FKPI_N) and (S["count"] == 2).all()


def test_refusals(eng):
    from eepacc_mpc_casadi_matlab_amd.engine import EepaccError
    lib, t = eng.lib, eng.torch
    traj, status, s_tv, v_tv, _ = synthetic(5, 4)
    dev = [t.as_tensor(x, device="cuda") for x in (traj, status, s_tv, v_tv)]
    fkpi = t.empty((FKPI_N, 4), dtype=t.float64, device="cuda")
    names = ("traj", "status", "s_tv", "v_tv", "fkpi")
    args = dict(zip(names, [x.data_ptr() for x in dev] + [fkpi.data_ptr()]))
    call = lambda B=4, n=5, weights=0, **kw: lib.eepacc_follow_kpis(eng.h, B, n, weights, *[dict(args, **kw)[k] for k in names], None)
    for name in names:
        assert call(**{name: None}) == -1 and ("eepacc_follow_kpis: %s is NULL" % name).encode() in lib.eepacc_last_error()
    assert call(n=0) == -1 and b"n_steps" in lib.eepacc_last_error()
    assert call(weights=3) == -1 and b"weights = 3" in lib.eepacc_last_error()
    assert call(B=257) == -1 and b"max_batch" in lib.eepacc_last_error() and b"B = 257" in lib.eepacc_last_error()
    assert call(B=-1) == -1 and b"B = -1" in lib.eepacc_last_error()
    assert call(B=0) == 0
    assert call() == 0
    with pytest.raises(ValueError):
        eng.follow_kpis(*dev, weights="bl")
    with pytest.raises(ValueError):
        eng.follow_kpis(dev[0], dev[1], dev[2][:4], dev[3])
    eng.synchronize()
    want = eng.follow_kpis(*dev).cpu().numpy()
    assert np.array_equal(fkpi.cpu().numpy(), want)
