"""Closed-loop throughput of the target-vehicle MPC (RunOpt_TVMPC, a handle with bl_mode = 2, kernels `tvc`) next to the
baseline controller (RunOpt_BLMPC, bl_mode = 1, kernels `blc`) in ONE process: for each horizon a launch of --warmup steps,
then a resumed launch of --steps steps that is timed; the figure is the median QP steps/s of --reps such launches, the spread
their (max - min) / median.  N = 20 and 30 run the N <= 32 kernels, N = 40 the N <= 63 kernels.

  python tools/gpu_tv_bench.py --out profiles/tvmpc_bench.json

The TVMPC instances drive the route of the default settings (speed-limit zones, ABO/Settings.m:150-193) from spread-out
starts; the BLMPC instances follow the synthetic S2 lead scenarios of bench.py on the same route.
"""
import argparse
import glob
import hashlib
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def source_hash():
    h = hashlib.sha256()
    files = sorted(glob.glob(os.path.join(ROOT, "eepacc_mpc_casadi_matlab_amd", "csrc", "*")) +
                   glob.glob(os.path.join(ROOT, "eepacc_mpc_casadi_matlab_amd", "*.py")) + [os.path.join(ROOT, "include", "eepacc.h")])
    for f in files:
        if os.path.isfile(f):
            h.update(os.path.basename(f).encode()); h.update(open(f, "rb").read())
    return h.hexdigest()[:16]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizons", default="20,30,40")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV

    B, n_all = a.batch, a.warmup + a.steps
    lead = np.load(os.path.join(ROOT, "tests", "golden", "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    V = SetVehicleParameters("ABO")
    rng = np.random.default_rng(0)
    results = []
    for N in [int(x) for x in a.horizons.split(",")]:
        OPT = Settings(tree="ABO", N_hor=N)
        OPT["TV_N_hor"] = N
        sc = make_s2(B, n_all, lead)
        dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
        stv, vtv = dev(sc["s_tv"]), dev(sc["v_tv"])
        tv_s0, tv_v0 = rng.uniform(0.0, 1500.0, B), rng.uniform(0.0, 12.0, B)
        z = np.zeros(B)
        tv = Engine(Settings_TV(OPT), V, device=0, max_batch=B)
        bl = Engine(Settings_BL(OPT), V, device=0, max_batch=B)
        traj = torch.empty((a.steps, 12, B), dtype=torch.float64, device="cuda")
        stat = torch.empty((a.steps, B), dtype=torch.int32, device="cuda")

        def run_tv():
            tv.run_tvmpc(tv_s0, tv_v0, z, a.warmup)
            tv.synchronize()
            t0 = time.perf_counter()
            tv.run_tvmpc(tv_s0, tv_v0, z, a.steps, resume=True, out=(traj, stat))
            tv.synchronize()
            return time.perf_counter() - t0

        def run_bl():
            bl.run_blmpc(sc["s0"], sc["v0"], sc["a_minus1"], stv[:a.warmup], vtv[:a.warmup])
            bl.synchronize()
            t0 = time.perf_counter()
            bl.run_blmpc(sc["s0"], sc["v0"], sc["a_minus1"], stv[a.warmup:], vtv[a.warmup:], resume=True, out=(traj, stat))
            bl.synchronize()
            return time.perf_counter() - t0

        rec = dict(N=N, batch=B, steps=a.steps, warmup=a.warmup, reps=a.reps)
        for name, fn in (("tvmpc", run_tv), ("blmpc", run_bl)):
            fn()                                             # untimed: first-launch costs
            vals = [B * a.steps / fn() for _ in range(a.reps)]
            bad = int((stat != 0).sum().item())
            med = statistics.median(vals)
            rec[name] = dict(median_qp_steps_per_s=med, spread=(max(vals) - min(vals)) / med, all=vals, failed_steps_last_launch=bad,
                             iterations_per_step=float(np.mean((tv if name == "tvmpc" else bl).last_iterations(B))) / a.steps)
        rec["tvmpc_over_blmpc"] = rec["tvmpc"]["median_qp_steps_per_s"] / rec["blmpc"]["median_qp_steps_per_s"]
        results.append(rec)
        print(json.dumps(rec), flush=True)
        del tv, bl
    out = dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
