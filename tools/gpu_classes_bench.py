"""Closed-loop throughput of a handle with settings classes in ONE process: ABMPC (eepacc_create_classes, kernels `cls`,
--kind ab, the default), the baseline controller (eepacc_create_classes_bl with bl_mode = 1, kernels `blcls`, --kind bl) or the
target-vehicle controller (bl_mode = 2, kernels `tvcls`, --kind tv).

(1) mixed:     the twelve GetUseCase scenarios of the ORIG tree, --batch instances in all (341 or 342 per use case at 4096),
               as ONE launch on a class handle, against the same instances as twelve launches on twelve ordinary handles,
               queued back to back on one stream -- the only way to run them without classes.
(2) one class: bench.py's ABMPC workload (ABO tree, S2 leads) through the class kernels with n_classes = 1 against the
               ordinary handle: what binding the settings per work unit costs when nothing is mixed.

Every configuration runs a launch of --warmup steps, then a resumed launch of --steps steps that is timed (host clock
around launches that end in a device synchronise).  The two sides of a comparison alternate, --reps times each; the figure
is the median QP steps/s, the spread (max - min) / median of the same side.  The outputs of the two sides are compared bit
for bit before any timing.

  python tools/gpu_classes_bench.py --out profiles/classes_bench.json
  python tools/gpu_classes_bench.py --kind bl --out profiles/classes_bench.json      # adds the key "bl" to the file, "tv" likewise; a run keeps the other kinds

--kind bl runs Settings_BL of the same instances and workloads through run_blmpc (one class: `blcls` against `blc`); --kind tv
runs Settings_TV of them through run_tvmpc, which takes no lead (one class: `tvcls` against `tvc`), every vehicle starting at
its class's TVinitDist with the initial speeds described below.  A mixed launch counts as a gain only where it exceeds the
twelve launches by more than the spreads printed beside it; the one-class ratio is reported without a bar.

The use-case instances start from their use case's own initial state; without a lead of their own (all but 8, 9, 10)
they differ inside a use case by the initial speed, spread over 0.5 .. 1 of the use case's speed limit at s = 0.  The
window is longer than the shortest use case simulates: the routes' tables extend to 1e5 m, and a use case's own lead drives
on at its last speed.
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
    ap.add_argument("--horizon", type=int, default=30)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kind", choices=("ab", "bl", "tv"), default="ab")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from eepacc_mpc_casadi_matlab_amd.engine import Engine
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s2, make_use_case_mix
    from eepacc_mpc_casadi_matlab_amd.settings import Settings, SetVehicleParameters, Settings_BL, Settings_TV

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    N, B, W, K = a.horizon, a.batch, a.warmup, a.steps
    golden = os.path.join(ROOT, "tests", "golden")
    dev = lambda x: torch.as_tensor(np.ascontiguousarray(x), dtype=torch.float64, device="cuda")
    traj = torch.empty((K, 12, B), dtype=torch.float64, device="cuda")
    stat = torch.empty((K, B), dtype=torch.int32, device="cuda")

    def compare(name, sides, B_):
        """sides: name -> function that runs warm-up and timed window and returns the seconds of the window."""
        outs = {}
        for s, fn in sides.items():                             # untimed: first-launch costs; keeps the outputs
            fn()
            outs[s] = (traj.clone(), stat.clone())
        (ta, sa), (tb, sb) = outs.values()
        rec = dict(name=name, N=N, batch=B_, steps=K, warmup=W, reps=a.reps,
                   outputs_bit_equal=bool(torch.equal(ta, tb) and torch.equal(sa, sb)), failed_steps=int((sa != 0).sum().item()))
        vals = {s: [] for s in sides}
        for _ in range(a.reps):
            for s, fn in sides.items():                         # alternating
                vals[s].append(B_ * K / fn())
        for s, v in vals.items():
            med = statistics.median(v)
            rec[s] = dict(median_qp_steps_per_s=med, spread=(max(v) - min(v)) / med, all=v)
        a_, b_ = list(sides)
        rec[a_ + "_over_" + b_] = rec[a_]["median_qp_steps_per_s"] / rec[b_]["median_qp_steps_per_s"]
        print(json.dumps(rec), flush=True)
        return rec

    results = []

    def launch(eng, p, rows, resume, out=None):
        """One closed-loop launch of the controller of --kind over the rows of p's lead (tv: as many steps, no lead)."""
        if a.kind == "tv":
            return eng.run_tvmpc(p["s0"], p["v0"], p["am1"], rows.stop - rows.start, resume=resume, out=out)
        run = eng.run_blmpc if a.kind == "bl" else eng.run_abmpc
        return run(p["s0"], p["v0"], p["am1"], p["stv"][rows], p["vtv"][rows], resume=resume, out=out)

    # (1) the twelve use cases ------------------------------------------------------------------------------------------
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
    OPTs = {"ab": mix["OPT"], "bl": [Settings_BL(o) for o in mix["OPT"]], "tv": mix["TV"]}[a.kind]
    if a.kind == "tv":                                          # the generated vehicles: every one from its class's TVinitDist
        s0 = np.array([float(OPTs[k]["TVinitDist"]) for k in cls])
        v0 = 0.8 * frac * np.array([float(OPTs[k]["v_speedLim"][0]) for k in cls])
    stv, vtv = dev(s_tv), dev(v_tv)
    idx = [np.nonzero(cls == k)[0] for k in range(12)]
    mixed = Engine.from_classes(OPTs, mix["V"], device=0, max_batch=B)
    mixed.set_classes(cls)
    whole = dict(s0=s0, v0=v0, am1=am1, stv=stv, vtv=vtv)
    singles = [Engine(o, v, device=0, max_batch=len(i)) for o, v, i in zip(OPTs, mix["V"], idx)]
    part = [dict(s0=s0[i], v0=v0[i], am1=am1[i], stv=stv[:, i].contiguous(), vtv=vtv[:, i].contiguous(),
                 traj=torch.empty((K, 12, len(i)), dtype=torch.float64, device="cuda"),
                 stat=torch.empty((K, len(i)), dtype=torch.int32, device="cuda"), dev_idx=torch.as_tensor(i, device="cuda")) for i in idx]

    def run_mixed():
        launch(mixed, whole, slice(0, W), False)
        mixed.synchronize()
        t0 = time.perf_counter()
        launch(mixed, whole, slice(W, W + K), True, out=(traj, stat))
        mixed.synchronize()
        return time.perf_counter() - t0

    def run_twelve():
        for e, p in zip(singles, part):
            launch(e, p, slice(0, W), False)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for e, p in zip(singles, part):                         # twelve launches back to back on one stream
            launch(e, p, slice(W, W + K), True, out=(p["traj"], p["stat"]))
        for e in singles:
            e.synchronize()
        dt = time.perf_counter() - t0
        for p in part:                                          # after the clock: gather for the comparison of the outputs
            traj[:, :, p["dev_idx"]] = p["traj"]; stat[:, p["dev_idx"]] = p["stat"]
        return dt

    results.append(compare("twelve_use_cases", dict(mixed_one_launch=run_mixed, twelve_launches=run_twelve), B))
    del mixed, singles, part

    # (2) one class through the class kernels, bench.py's ABMPC workload (bl, tv: that controller's view of its settings) ------
    lead = np.load(os.path.join(golden, "lead_TO01_EAD.npz"))["V_TO_2Hz"]
    OPT, V = Settings(tree="ABO", N_hor=N), SetVehicleParameters("ABO")
    OPT = {"ab": lambda o: o, "bl": Settings_BL, "tv": Settings_TV}[a.kind](OPT)
    sc = make_s2(B, W + K, lead)
    stv, vtv = dev(sc["s_tv"]), dev(sc["v_tv"])
    whole = dict(s0=np.full(B, float(OPT["TVinitDist"])) if a.kind == "tv" else sc["s0"], v0=sc["v0"], am1=sc["a_minus1"], stv=stv, vtv=vtv)
    one = Engine.from_classes([OPT], [V], device=0, max_batch=B)
    one.set_classes(np.zeros(B, dtype=np.int32))
    plain = Engine(OPT, V, device=0, max_batch=B)

    def runner(eng):
        def run():
            launch(eng, whole, slice(0, W), False)
            eng.synchronize()
            t0 = time.perf_counter()
            launch(eng, whole, slice(W, W + K), True, out=(traj, stat))
            eng.synchronize()
            return time.perf_counter() - t0
        return run

    results.append(compare("one_class_bench_workload", dict(class_kernels=runner(one), ordinary_handle=runner(plain)), B))
    out = dict(source_hash=source_hash(), device=torch.cuda.get_device_name(0), results=results)
    # one file holds the three kinds: ABMPC at the top level, as before, the others under the keys "bl" and "tv"; a run
    # replaces its own kind and keeps what the file has of the others
    have = {}
    if a.out and os.path.exists(a.out):
        with open(a.out) as f:
            have = json.load(f)
    if a.kind == "ab":
        out.update({k: have[k] for k in ("bl", "tv") if k in have})
    else:
        have[a.kind] = out
        out = have
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
