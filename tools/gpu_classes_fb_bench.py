"""What FBMPC on settings classes costs and gains, in ONE process (the method of tools/gpu_classes_est_bench.py): the two sides of a
comparison alternate, --reps times each; the figure is the median, the spread (max - min) / median of the same side.  The outputs
of the two sides are compared bit for bit before any timing, and the share of failed steps (status != 0) of each side's timed
launch is recorded, since the workloads differ.

(1) mixed:     the twelve GetUseCase scenarios of the ORIG tree, --batch instances in all, as ONE eepacc_run_classes_fbmpc launch
               on a class handle against the same instances as twelve eepacc_run_fbmpc launches on twelve ordinary handles,
               queued back to back on one stream.  A launch of --warmup steps, then a resumed launch of --steps steps that is timed.
(2) one class: bench.py's FBMPC workload (ABO tree, S2 leads) through eepacc_run_classes_fbmpc on a handle with n_classes = 1
               against eepacc_run_fbmpc on the ordinary handle at the same B: what the class map costs when nothing is mixed.
(3) step:      the same one class through eepacc_classes_fb_step against eepacc_fb_step, from the state a warmed-up loop reached.

All are ratios between entries of the same commit.  The twelve launches split the batch in twelve parts, so their launch geometry
differs from the mixed launch's and their outputs are compared per class only in (1)'s `outputs_bit_equal` after gathering.

  python tools/gpu_classes_fb_bench.py --out profiles/classes_fb_bench.json
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
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    from gpu_classes_bench import source_hash
    from eepacc_mpc_casadi_matlab_amd._abi import OUT
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2, make_use_case_mix
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    N, B, W, K = a.horizon, a.batch, a.warmup, a.steps
    golden = os.path.join(ROOT, "tests", "golden")
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    traj = torch.empty((K, 12, B), dtype=torch.float64, device="cuda")
    stat = torch.empty((K, B), dtype=torch.int32, device="cuda")

    def compare(name, sides, unit, work, rows=slice(None)):
        """sides: name -> function that returns the seconds of its timed window and leaves its outputs in traj, stat (rows: those it writes)."""
        outs = {}
        for s, fn in sides.items():                             # untimed: first-launch costs; keeps the outputs
            fn()
            outs[s] = (traj.clone(), stat.clone())
        (ta, sa), (tb, sb) = outs.values()
        same = lambda x, y: bool(torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)) and torch.equal(x.isnan(), y.isnan()))
        rec = dict(name=name, N=N, batch=B, steps=K, warmup=W, reps=a.reps, unit=unit,
                   outputs_bit_equal=same(ta, tb) and bool(torch.equal(sa, sb)))
        vals = {s: [] for s in sides}
        for _ in range(a.reps):
            for s, fn in sides.items():                         # alternating
                vals[s].append(work / fn())
        for (s, v), (_, so) in zip(vals.items(), outs.values()):
            med = statistics.median(v)
            rec[s] = dict(median=med, spread=(max(v) - min(v)) / med, all=v, failed_step_share=float((so[rows] != 0).float().mean().item()))
        a_, b_ = list(sides)
        rec[a_ + "_over_" + b_] = rec[a_]["median"] / rec[b_]["median"]
        print(json.dumps(rec), flush=True)
        return rec

    results = []

    # (1) the twelve use cases ------------------------------------------------------------------------------------------------
    rec = np.load(os.path.join(golden, "argonne_61505019_lead.npz"))
    cases = list(range(1, 13))
    mix = make_use_case_mix(cases, (B + 11) // 12, "ORIG", N, argonne_lead=(rec["t"], rec["v_mph"]))
    cls = mix["class_of"][:B]                                   # interleaved: 0, 1, ..., 11, 0, 1, ...
    frac = 0.5 + 0.5 * np.random.default_rng(0).uniform(size=B)
    v0 = mix["v0"][:B].copy()
    s_tv, v_tv = np.full((W + K, B), np.inf), np.zeros((W + K, B))
    for k, o in enumerate(mix["OPT"]):
        if cases[k] in (8, 9, 10):                              # the use case's lead, driving on at its last speed
            sl, vl = np.asarray(o["s_tv"], dtype=np.float64), np.asarray(o["v_tv"], dtype=np.float64)
            more = max(W + K - sl.size, 0)
            sl = np.concatenate([sl, sl[-1] + vl[-1] * float(o["Tvec"][0]) * np.arange(1, more + 1)])[:W + K]
            vl = np.concatenate([vl, np.full(more, vl[-1])])[:W + K]
            s_tv[:, cls == k], v_tv[:, cls == k] = sl[:, None], vl[:, None]
        else:
            v0[cls == k] = frac[cls == k] * float(o["v_speedLim"][0])
    s0, am1 = mix["s0"][:B], mix["a_minus1"][:B]
    stv, vtv = dev(s_tv), dev(v_tv)
    idx = [np.nonzero(cls == k)[0] for k in range(12)]
    whole = dict(s0=s0, v0=v0, am1=am1, stv=stv, vtv=vtv)
    mixed = Engine.from_classes(mix["OPT"], mix["V"], device=0, max_batch=B)
    mixed.set_classes(cls)
    singles = [Engine(o, v, device=0, max_batch=len(i)) for o, v, i in zip(mix["OPT"], mix["V"], idx)]
    part = [dict(s0=s0[i], v0=v0[i], am1=am1[i], stv=stv[:, i].contiguous(), vtv=vtv[:, i].contiguous(),
                 traj=torch.empty((K, 12, len(i)), dtype=torch.float64, device="cuda"),
                 stat=torch.empty((K, len(i)), dtype=torch.int32, device="cuda"), dev_idx=torch.as_tensor(i, device="cuda")) for i in idx]

    def launch(eng, entry, p, warm, out=None):
        rows = slice(0, W) if warm else slice(W, W + K)
        return getattr(eng, entry)(p["s0"], p["v0"], p["am1"], p["stv"][rows], p["vtv"][rows], resume=not warm, out=out)

    def closed_loop(eng, entry, p):
        def run():
            launch(eng, entry, p, True)
            eng.synchronize()
            t0 = time.perf_counter()
            launch(eng, entry, p, False, out=(traj, stat))
            eng.synchronize()
            return time.perf_counter() - t0
        return run

    def run_twelve():
        for e, p in zip(singles, part):
            launch(e, "run_fbmpc", p, True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e, p in zip(singles, part):                         # twelve launches back to back on one stream
            launch(e, "run_fbmpc", p, False, out=(p["traj"], p["stat"]))
        for e in singles:
            e.synchronize()
        dt = time.perf_counter() - t0
        for p in part:                                          # after the clock: gather for the comparison of the outputs
            traj[:, :, p["dev_idx"]] = p["traj"]; stat[:, p["dev_idx"]] = p["stat"]
        return dt

    results.append(compare("twelve_use_cases_fbmpc", dict(mixed_one_launch=closed_loop(mixed, "run_classes_fbmpc", whole),
                                                          twelve_launches=run_twelve), "QP steps/s", B * K))
    del mixed, singles, part

    # (2) one class through the class kernels, bench.py's FBMPC workload ----------------------------------------------------------
    lead = np.load(os.path.join(golden, "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    OPT, V = Settings(tree="ABO", N_hor=N), SetVehicleParameters("ABO")
    sc = make_s2(B, W + K, lead)
    p1 = dict(s0=sc["s0"], v0=sc["v0"], am1=sc["a_minus1"], stv=dev(sc["s_tv"]), vtv=dev(sc["v_tv"]))
    one = Engine.from_classes([OPT], [V], device=0, max_batch=B)
    one.set_classes(np.zeros(B, dtype=np.int32))
    plain = Engine(OPT, V, device=0, max_batch=B)
    results.append(compare("one_class_run_bench_workload", dict(run_classes_fbmpc=closed_loop(one, "run_classes_fbmpc", p1),
                                                                run_fbmpc=closed_loop(plain, "run_fbmpc", p1)), "QP steps/s", B * K))

    # (3) the step entry for the same class, from the state the warm-up loop reached --------------------------------------------------
    wt, _ = plain.run_fbmpc(sc["s0"], sc["v0"], sc["a_minus1"], p1["stv"][:W], p1["vtv"][:W])
    last = wt[-1]
    s, v = last[OUT["s"]].clone(), last[OUT["v"]].clone()
    z = torch.zeros(B, dtype=torch.float64, device="cuda")
    t0v = torch.full((B,), W * 0.5, dtype=torch.float64, device="cuda")
    step_ins = (s, v, z, z, z, z, t0v, p1["stv"][W - 1].clone(), p1["vtv"][W - 1].clone(), z)
    n_calls = 50

    def stepper(eng, fn):
        def run():
            eng.reset()
            out, _, _, st = fn(*step_ins, want_pred=False)
            eng.synchronize()
            t0 = time.perf_counter()
            for _ in range(n_calls):
                out, _, _, st = fn(*step_ins, want_pred=False)
            eng.synchronize()
            dt = time.perf_counter() - t0
            traj[0].copy_(out); stat[0].copy_(st)               # the last step's outputs, for the comparison of the two sides
            return dt
        return run

    traj.zero_(); stat.zero_()
    r = compare("one_class_step_bench_workload", dict(classes_fb_step=stepper(one, one.classes_fb_step),
                                                       fb_step=stepper(plain, plain.fb_step)), "QP steps/s", B * n_calls, rows=slice(0, 1))
    r["step_calls_per_sample"] = n_calls
    results.append(r)
    out = dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
