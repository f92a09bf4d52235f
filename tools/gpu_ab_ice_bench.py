"""Closed-loop throughput of the ABMPC ICE-map fuel term (OPT["fuel_map"] = "ICE", the kernel variant `ice`) against the
efficiency map on the same launch, through bench.run_bench (same S2 scenarios, warm-up and timing as bench.py's
secondary abmpc_N60_b8192 entry).  Each figure is the median QP steps/s of --reps launches.

  python tools/gpu_ab_ice_bench.py                      # (i) N = 60 x 8192, (ii) reference mask N = 50 x 8192, (iii) N = 30 x 4096
  python tools/gpu_ab_ice_bench.py --tree DIR --only iii   # the same with the package of another checkout (e.g. the parent commit)

Prints one JSON line per figure and a summary line; --out FILE also writes them there.
"""
import argparse
import copy
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def reference_long_mask():
    """ABO/Settings.m:100 (commented alternative) expanded as Settings.m:243-250: N = 50, 25 blocked stages."""
    mb = []
    for n in [1] * 10 + [2] * 10 + [4] * 5:
        mb += [0] + [1] * (n - 1)
    return mb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(HERE), help="checkout whose package and bench.py are measured")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="i,ii,iii")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    tree = os.path.abspath(a.tree)
    sys.path[:0] = [tree, os.path.join(tree, "tests")]
    import numpy as np
    import bench
    from eepacc_mpc_casadi_matlab_amd.engine import Engine

    def factory(fuel_map, mb):
        def make_engine(OPT, V, dev, B):
            OPT = dict(OPT)
            OPT["fuel_map"] = fuel_map
            if mb is not None:
                OPT["Mb"] = np.array(mb, dtype=np.int32)
            return Engine(OPT, V, device=dev, max_batch=B)
        return make_engine

    mask = reference_long_mask()
    plan = {"i": [("ICE", None, 60, 8192), ("EFF", None, 60, 8192)],
            "ii": [("ICE", mask, len(mask), 8192), ("EFF", mask, len(mask), 8192)],
            "iii": [("ICE", None, 30, 4096)]}
    base = bench.resolve_defaults(bench.build_parser().parse_args(["--gpus", "1", "--steps", str(a.steps),
                                                                   "--warmup", str(a.warmup)]))
    results = []
    for key in [k.strip() for k in a.only.split(",") if k.strip()]:
        for fuel_map, mb, N, B in plan[key]:
            args = copy.copy(base)
            args.workload, args.horizon, args.batch, args.chunk = "abmpc", N, B, 0
            vals = []
            for _ in range(a.reps):
                r = bench.run_bench(args, make_engine=factory(fuel_map, mb))
                vals.append(r["value"])
            rec = dict(figure=key, fuel_map=fuel_map, N=N, batch=B, move_blocking=mb is not None, steps=a.steps,
                       warmup=a.warmup, reps=a.reps, median_qp_steps_per_s=statistics.median(vals), all=vals, tree=tree)
            results.append(rec)
            print(json.dumps(rec), flush=True)
    for key in ("i", "ii"):
        pair = {r["fuel_map"]: r["median_qp_steps_per_s"] for r in results if r["figure"] == key}
        if len(pair) == 2:
            print(json.dumps(dict(figure=key, ice_over_eff=pair["ICE"] / pair["EFF"])), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
