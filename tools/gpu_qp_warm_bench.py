"""What the dual outputs of the dense QP operator cost and what its warm start gains, in ONE process: a sequence of --seq
problems of the reference's AB shape (100 variables, 282 rows; the dense QPs of saved closed-loop steps as
tests/test_gpu_fb.py builds them, --batch saved steps spread over the run), each with g perturbed from the one before (a
random walk of --g-rel per entry that keeps the signs) and every finite bound moved anew by up to --b-abs, at batch --batch.

  (a) eepacc_qp_solve_batched                      the operator without the dual outputs
  (b) eepacc_qp_solve_batched_dual, cold           (b)/(a): the price of multipliers and working set
  (c) eepacc_qp_solve_batched_dual, warm-started from the working set of the previous problem of the sequence
                                                   (c)/(b): the gain of the warm start

One sample of a side is the whole sequence (--seq launches, synchronised at its end); the sides alternate a, b, c, a, b, c
...; the figure is the median of --reps samples in ms per launch, the spread their (max - min) / median.

  python tools/gpu_qp_warm_bench.py --out profiles/qp_dual_bench.json
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--g-rel", type=float, default=0.01, help="relative perturbation of every entry of g per problem")
    ap.add_argument("--b-abs", type=float, default=1e-3, help="largest move of a finite bound per problem")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import bench
    from conftest import make_case, load_golden, golden_step_inputs
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from oracle.loader import Oracle

    B, T = a.batch, a.seq
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    G = load_golden("abo_abmpc")
    orc = Oracle(OPT, V)
    steps = np.linspace(0, 870, B).astype(int)
    base = [orc.ab_step(**golden_step_inputs(G, s_tv, v_tv, int(k)), want_dense=True) for k in steps]
    H = np.stack([p["H"] for p in base]); g0 = np.stack([p["c"] for p in base]); A = np.stack([p["G"] for p in base])
    lb0 = np.stack([p["lb"] for p in base]); ub0 = np.stack([p["ub"] for p in base])
    nV, nC = H.shape[1], A.shape[1]
    rng = np.random.default_rng(0)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    seq = []
    g = g0
    for t in range(T):
        lb, ub = lb0, ub0
        if t:
            # g: every entry scaled by 1 + g_rel N(0,1), a random walk that keeps the signs (a slack whose cost turned
            # negative would make the problem unbounded).  Bounds: each finite one moved outwards from the saved step's
            # by b_abs U(0,1), drawn anew for every problem, so they move both ways from one problem to the next and the
            # saved step's feasible set stays inside (rows moved freely make some of these problems infeasible).
            g = g * (1.0 + a.g_rel * rng.standard_normal(g.shape))
            lb = lb0 - a.b_abs * rng.uniform(0.0, 1.0, lb0.shape)
            ub = ub0 + a.b_abs * rng.uniform(0.0, 1.0, ub0.shape)
        seq.append((dev(g), dev(lb), dev(ub)))
    dH, dA = dev(H), dev(A)
    eng = Engine(OPT, V, device=0, max_batch=B)

    def side_a():
        st = []
        t0 = time.perf_counter()
        for g_, lb_, ub_ in seq:
            st.append(eng.qp_solve_batched(dH, g_, dA, lb_, ub_)[2])
        eng.synchronize()
        return time.perf_counter() - t0, st, None

    def side_dual(warm):
        st, it, ws0 = [], [], None
        t0 = time.perf_counter()
        for g_, lb_, ub_ in seq:
            r = eng.qp_solve_batched_dual(dH, g_, dA, lb_, ub_, ws0=ws0)
            st.append(r.status); it.append(r.iters)
            if warm:
                ws0 = (r.ws_a, r.ws_x)
        eng.synchronize()
        return time.perf_counter() - t0, st, it

    sides = (("a_primal", side_a), ("b_dual_cold", lambda: side_dual(False)), ("c_dual_warm", lambda: side_dual(True)))
    for _, fn in sides:
        fn()                                                 # untimed: first-launch costs
    times = {name: [] for name, _ in sides}
    last = {}
    for _ in range(a.reps):
        for name, fn in sides:
            dt, st, it = fn()
            times[name].append(1e3 * dt / T)
            last[name] = (st, it)
    rec = dict(batch=B, seq=T, reps=a.reps, nV=nV, nC=nC, g_rel=a.g_rel, b_abs=a.b_abs)
    for name, _ in sides:
        med = statistics.median(times[name])
        st, it = last[name]
        rec[name] = dict(median_ms_per_launch=med, spread=(max(times[name]) - min(times[name])) / med, all_ms=times[name],
                         failed=int(sum(int((s != 0).sum().item()) for s in st)))
        if it is not None:
            per = [float(x.double().mean().item()) for x in it]
            rec[name]["iters_mean_per_problem"] = per
            rec[name]["iters_mean_after_first"] = float(np.mean(per[1:])) if T > 1 else per[0]
    rec["dual_over_primal"] = rec["b_dual_cold"]["median_ms_per_launch"] / rec["a_primal"]["median_ms_per_launch"]
    rec["warm_over_cold"] = rec["c_dual_warm"]["median_ms_per_launch"] / rec["b_dual_cold"]["median_ms_per_launch"]
    rec["spread_max"] = max(rec[name]["spread"] for name, _ in sides)
    print(json.dumps(rec), flush=True)
    out = dict(source_hash=bench.source_hash(), device=torch.cuda.get_device_name(0), result=rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
