"""What supplied horizon guesses cost FBMPC: eepacc_fb_step_est with all three arrays against eepacc_fb_step, and
eepacc_run_fbmpc_preview against eepacc_run_fbmpc, in ONE process on one build (the method of tools/gpu_bl_est_bench.py): the
median of --reps samples taken alternately, the spread their (max - min) / median.

  python tools/gpu_fb_est_bench.py --out profiles/fb_est_bench.json

Shapes (--shapes N:batch): N = 20 and N = 30 at batch 4096, N = 60 at batch 1024, the S2 scenarios of bench.py, --steps steps
after --warmup.  The step pair solves the same problems (the supplied arrays are the estimators' own guesses, made on the host
from the states of the warmed-up loop; constant-speed estimators so that the host can state them exactly), so its ratio is the
cost of three coalesced loads per lane against the two estimators.  Every call of a sample moves the handle's step counter on,
on both sides alike.  The preview loop solves other problems than the estimator loop (it knows the lead's future): its ratio
describes the workload and carries no bar.  The steps with status != 0 of the last timed launch are counted for both loops: a
failed step can be a cheap one (a step decided infeasible before the solve runs none), so a differing share is part of the ratio.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(N, B, a):
    import numpy as np
    import torch
    from eepacc_mpc_casadi_matlab_amd._abi import OUT
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters

    n_all = a.warmup + a.steps
    lead = np.load(os.path.join(ROOT, "tests", "golden", "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    OPT = Settings(tree="ABO", N_hor=N)
    OPT.update(paramEstSetting=0, TVestSetting=0)             # constant-speed guesses: the host can state them exactly
    V = SetVehicleParameters("ABO")
    Tv = np.asarray(OPT["Tvec"], dtype=np.float64)
    sc = make_s2(B, n_all + N, lead)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    stv, vtv = dev(sc["s_tv"]), dev(sc["v_tv"])
    ins = (sc["s0"], sc["v0"], sc["a_minus1"])
    eng = Engine(OPT, V, device=0, max_batch=B)
    traj = torch.empty((a.steps, 12, B), dtype=torch.float64, device="cuda")
    stat = torch.empty((a.steps, B), dtype=torch.int32, device="cuda")

    failed = {}                                              # steps with status != 0 in the last timed launch of either loop

    def run_est():
        eng.run_fbmpc(*ins, stv[:a.warmup], vtv[:a.warmup])
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run_fbmpc(*ins, stv[a.warmup:n_all], vtv[a.warmup:n_all], resume=True, out=(traj, stat))
        eng.synchronize()
        dt = time.perf_counter() - t0
        failed["run_fbmpc"] = int((stat != 0).sum().item())
        return dt

    def run_preview():
        eng.run_fbmpc_preview(*ins, stv, vtv, n_steps=a.warmup)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run_fbmpc_preview(*ins, stv[a.warmup:], vtv[a.warmup:], n_steps=a.steps, resume=True, out=(traj, stat))
        eng.synchronize()
        dt = time.perf_counter() - t0
        failed["run_fbmpc_preview"] = int((stat != 0).sum().item())
        return dt

    # single steps from the state the warmed-up loop reached: the same inputs for both entry points
    wt, _ = eng.run_fbmpc(*ins, stv[:a.warmup], vtv[:a.warmup])
    last = wt[-1]
    s, v = last[OUT["s"]].clone(), last[OUT["v"]].clone()
    z = torch.zeros(B, dtype=torch.float64, device="cuda")
    t0v = torch.full((B,), a.warmup * float(Tv[0]), dtype=torch.float64, device="cuda")
    s_l, v_l = stv[a.warmup - 1].clone(), vtv[a.warmup - 1].clone()
    tau = dev(np.concatenate([[0.0], np.cumsum(Tv)]))[:, None]
    sup = dict(s_est=(s[None, :] + tau * v[None, :]).contiguous(), v_est=v[None, :].repeat(N + 1, 1).contiguous(),
               s_tv_est=(s_l[None, :] + tau * v_l[None, :]).contiguous())
    step_ins = (s, v, z, z, z, z, t0v, s_l, v_l, z)
    n_calls = 50

    def run_step(fn, **kw):
        eng.reset()
        fn(*step_ins, want_pred=False, **kw)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            fn(*step_ins, want_pred=False, **kw)
        eng.synchronize()
        return (time.perf_counter() - t0) / n_calls

    pairs = dict(loop=(("run_fbmpc", run_est), ("run_fbmpc_preview", run_preview)),
                 step=(("fb_step", lambda: run_step(eng.fb_step)), ("fb_step_est", lambda: run_step(eng.fb_step_est, **sup))))
    rec = dict(N=N, batch=B, steps=a.steps, warmup=a.warmup, reps=a.reps, step_calls_per_sample=n_calls)
    for kind, ((n0, f0), (n1, f1)) in pairs.items():
        eng.reset()
        f0(); f1()                                           # untimed: first-launch costs
        t = {n0: [], n1: []}
        for _ in range(a.reps):                              # alternating samples
            t[n0].append(f0()); t[n1].append(f1())
        for n in (n0, n1):
            med = statistics.median(t[n])
            rec[n] = dict(median_seconds=med, spread=(max(t[n]) - min(t[n])) / med, all=t[n])
        rec["%s_over_%s" % (n1, n0)] = rec[n1]["median_seconds"] / rec[n0]["median_seconds"]
        if kind == "loop":
            rec["failed_steps_last_launch"] = dict(failed, of=a.steps * B)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", nargs="+", default=["20:4096", "30:4096", "60:1024"], help="N:batch")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import torch
    from gpu_tv_bench import source_hash
    results = []
    for shape in a.shapes:
        N, B = (int(x) for x in shape.split(":"))
        rec = measure(N, B, a)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
