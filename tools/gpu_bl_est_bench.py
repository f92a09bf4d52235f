"""What supplied horizon guesses cost the baseline controller: eepacc_bl_step_est with all three arrays against eepacc_bl_step,
and eepacc_run_blmpc_preview against eepacc_run_blmpc, in ONE process (the method of tools/gpu_ab_est_bench.py): the median of
--reps samples taken alternately, the spread their (max - min) / median.

  python tools/gpu_bl_est_bench.py --out profiles/bl_est_bench.json

Shape: N = 20 and N = 30 (--N), batch 4096, the S2 scenarios of bench.py, --steps steps after --warmup.  The step pair solves the
same problems (the supplied arrays are the estimators' own guesses, made on the host from the states of the warmed-up loop), so
its ratio is the cost of the three uncoalesced loads per lane and step in the blest kernels.  The preview loop solves other
problems than the estimator loop (it knows the lead's future): its ratio describes the workload and carries no bar.
"""
import argparse
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def measure(N, a):
    import numpy as np
    import torch
    from eepacc_mpc_casadi_matlab_amd._abi import OUT
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL

    B, n_all = a.batch, a.warmup + a.steps
    lead = np.load(os.path.join(ROOT, "tests", "golden", "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    OPT = Settings(tree="ABO", N_hor=N)
    OPT["BL_N_hor"] = N
    BL = Settings_BL(OPT)
    BL.update(paramEstSetting=0, TVestSetting=0)              # constant-speed guesses: the host can state them exactly
    V = SetVehicleParameters("ABO")
    Tv = np.asarray(BL["Tvec"], dtype=np.float64)
    sc = make_s2(B, n_all + N, lead)
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    stv, vtv = dev(sc["s_tv"]), dev(sc["v_tv"])
    ins = (sc["s0"], sc["v0"], sc["a_minus1"])
    eng = Engine(BL, V, device=0, max_batch=B)
    traj = torch.empty((a.steps, 12, B), dtype=torch.float64, device="cuda")
    stat = torch.empty((a.steps, B), dtype=torch.int32, device="cuda")

    def run_est():
        eng.run_blmpc(*ins, stv[:a.warmup], vtv[:a.warmup])
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run_blmpc(*ins, stv[a.warmup:n_all], vtv[a.warmup:n_all], resume=True, out=(traj, stat))
        eng.synchronize()
        return time.perf_counter() - t0

    def run_preview():
        eng.run_blmpc_preview(*ins, stv, vtv, n_steps=a.warmup)
        eng.synchronize()
        t0 = time.perf_counter()
        eng.run_blmpc_preview(*ins, stv[a.warmup:], vtv[a.warmup:], n_steps=a.steps, resume=True, out=(traj, stat))
        eng.synchronize()
        return time.perf_counter() - t0

    # single steps from the state the warmed-up loop reached: the same inputs for both entry points
    wt, _ = eng.run_blmpc(*ins, stv[:a.warmup], vtv[:a.warmup])
    last = wt[-1]
    s, v = last[OUT["s"]].clone(), last[OUT["v"]].clone()
    z = torch.zeros(B, dtype=torch.float64, device="cuda")
    t0v = torch.full((B,), a.warmup * float(Tv[0]), dtype=torch.float64, device="cuda")
    s_l, v_l = stv[a.warmup - 1].clone(), vtv[a.warmup - 1].clone()
    tau = dev(np.concatenate([[0.0], np.cumsum(Tv)]))[:, None]
    sup = dict(s_est=(s[None, :] + tau * v[None, :]).contiguous(), v_est=v[None, :].repeat(N + 1, 1).contiguous(),
               s_tv_est=(s_l[None, :] + tau * v_l[None, :]).contiguous())
    step_ins = (s, v, z, t0v, s_l, v_l, z)
    n_calls = 50
    bl_step = lambda *x, want_pred=False: eng._step(eng.lib.eepacc_bl_step, x, want_pred)

    def run_step(fn, **kw):
        eng.reset()
        fn(*step_ins, want_pred=False, **kw)
        eng.synchronize()
        t0 = time.perf_counter()
        for _ in range(n_calls):
            fn(*step_ins, want_pred=False, **kw)
        eng.synchronize()
        return (time.perf_counter() - t0) / n_calls

    pairs = dict(loop=(("run_blmpc", run_est), ("run_blmpc_preview", run_preview)),
                 step=(("bl_step", lambda: run_step(bl_step)), ("bl_step_est", lambda: run_step(eng.bl_step_est, **sup))))
    rec = dict(N=N, batch=B, steps=a.steps, warmup=a.warmup, reps=a.reps, step_calls_per_sample=n_calls)
    for kind, ((n0, f0), (n1, f1)) in pairs.items():
        f0(); f1()                                           # untimed: first-launch costs
        t = {n0: [], n1: []}
        for _ in range(a.reps):                              # alternating samples
            t[n0].append(f0()); t[n1].append(f1())
        for n in (n0, n1):
            med = statistics.median(t[n])
            rec[n] = dict(median_seconds=med, spread=(max(t[n]) - min(t[n])) / med, all=t[n])
        rec["%s_over_%s" % (n1, n0)] = rec[n1]["median_seconds"] / rec[n0]["median_seconds"]
        if kind == "loop":
            rec["failed_steps_last_launch"] = int((stat != 0).sum().item())
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, nargs="+", default=[20, 30])
    ap.add_argument("--batch", type=int, default=4096)
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
    for N in a.N:
        rec = measure(N, a)
        print(json.dumps(rec), flush=True)
        results.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), results=results), f, indent=1)


if __name__ == "__main__":
    main()
