"""What a solve with the KKT matrix of the final working set costs next to the QP solve that produced it, in ONE process:
--batch problems of the reference's AB shape (100 variables, 282 rows; the dense QPs of saved closed-loop steps as
tests/test_gpu_fb.py builds them, spread over the run).

  (a) eepacc_qp_solve_batched_dual, cold                        the solve whose working set is differentiated
  (b) eepacc_qp_kkt_solve_batched, nR = 1                       one adjoint (qp_vjp) or one direction (qp_jvp)
  (c) eepacc_qp_kkt_solve_batched, nR = 8                       eight directions per launch

One sample is --launches launches of a side, synchronised at the end; the sides alternate a, b, c, a, b, c ...; the
figure is the median of --reps samples in ms per launch, the spread their (max - min) / median.  Written down: (b)/(a)
and (c)/(a).  No target is set.

  python tools/gpu_qp_kkt_bench.py --out profiles/qp_kkt_bench.json
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
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=5)
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

    B, T = a.batch, a.launches
    OPT, V, s_tv, v_tv = make_case("ABO", 20)
    G = load_golden("abo_abmpc")
    orc = Oracle(OPT, V)
    steps = np.linspace(0, 870, B).astype(int)
    base = [orc.ab_step(**golden_step_inputs(G, s_tv, v_tv, int(k)), want_dense=True) for k in steps]
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    H, g, A = (dev(np.stack([p[k] for p in base])) for k in ("H", "c", "G"))
    lb, ub = (dev(np.stack([p[k] for p in base])) for k in ("lb", "ub"))
    nV, nC = H.shape[1], A.shape[1]
    eng = Engine(OPT, V, device=0, max_batch=B)
    sol = eng.qp_solve_batched_dual(H, g, A, lb, ub)
    eng.synchronize()
    rng = np.random.default_rng(0)
    rhs = {nR: (dev(rng.standard_normal((B, nR, nV))), dev(rng.standard_normal((B, nR, nC))), dev(rng.standard_normal((B, nR, nV))))
           for nR in (1, 8)}

    def side_solve():
        t0 = time.perf_counter()
        for _ in range(T):
            st = eng.qp_solve_batched_dual(H, g, A, lb, ub).status
        eng.synchronize()
        return time.perf_counter() - t0, st

    def side_kkt(nR):
        t0 = time.perf_counter()
        for _ in range(T):
            st = eng.qp_kkt_solve(H, A, sol.ws_a, sol.ws_x, *rhs[nR])[3]
        eng.synchronize()
        return time.perf_counter() - t0, st

    sides = (("a_dual_cold", side_solve), ("b_kkt_nR1", lambda: side_kkt(1)), ("c_kkt_nR8", lambda: side_kkt(8)))
    for _, fn in sides:
        fn()                                                 # untimed: first-launch costs
    times = {name: [] for name, _ in sides}
    failed = {}
    for _ in range(a.reps):
        for name, fn in sides:
            dt, st = fn()
            times[name].append(1e3 * dt / T)
            failed[name] = int((st != 0).sum().item())
    rec = dict(batch=B, launches=T, reps=a.reps, nV=nV, nC=nC,
               held_mean=float(((sol.ws_a != 0).sum(1) + (sol.ws_x != 0).sum(1)).double().mean().item()))
    for name, _ in sides:
        med = statistics.median(times[name])
        rec[name] = dict(median_ms_per_launch=med, spread=(max(times[name]) - min(times[name])) / med, all_ms=times[name],
                         failed=failed[name])
    rec["kkt_nR1_over_cold"] = rec["b_kkt_nR1"]["median_ms_per_launch"] / rec["a_dual_cold"]["median_ms_per_launch"]
    rec["kkt_nR8_over_cold"] = rec["c_kkt_nR8"]["median_ms_per_launch"] / rec["a_dual_cold"]["median_ms_per_launch"]
    rec["nR8_over_nR1"] = rec["c_kkt_nR8"]["median_ms_per_launch"] / rec["b_kkt_nR1"]["median_ms_per_launch"]
    rec["spread_max"] = max(rec[name]["spread"] for name, _ in sides)
    print(json.dumps(rec), flush=True)
    out = dict(source_hash=bench.source_hash(), device=torch.cuda.get_device_name(0), result=rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
