"""What a key-figure table costs next to reading its input once, in ONE process: eepacc_kpis, eepacc_follow_kpis or
eepacc_route_kpis at the headline shape, 871 steps x 4096 instances, against a device-to-device copy of exactly the rows the
kernel reads (the rows of traj through torch.index_select into a preallocated buffer, status and the lead traces through
copy_).  The tables are readers: a few hundred bytes per instance go out, so the copy, which also writes what it reads, is a
generous yardstick.

  kpis    rows S, V, FM, A of traj and status
  follow  rows S, V, A, XI_V, XI_H, XI_S, XI_F of traj, s_tv and v_tv (weights "ab": FM is not read)
  route   rows S, V, A of traj, without the per-sample limits; a second figure with them (written, not read, by the kernel)

The trajectory is synthetic (a monotone drive over the route of the ABO settings, random speeds, forces and slacks): the
kernels' work does not depend on the values except through the number of route features, which is that of the settings.  A
time is the median of --reps single launches between two HIP events, the two sides alternating, after one untimed launch of
each; the spread is (max - min) / median of the same launches.  Written down: both times, the bytes and kernel / copy.  No
assertion.  The result is merged into the JSON file under the table's name.

  python tools/gpu_kpi_bench.py --table route --out profiles/kpi_bench.json
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ROWS = {"kpis": ("s", "v", "Fm", "a"), "follow": ("s", "v", "a", "xi_v", "xi_h", "xi_s", "xi_f"), "route": ("s", "v", "a")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", choices=sorted(ROWS), required=True)
    ap.add_argument("--steps", type=int, default=871)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch
    import bench
    from conftest import make_case
    from eepacc_mpc_casadi_matlab_amd._abi import OUT, OUT_N
    from eepacc_mpc_casadi_matlab_amd.engine import Engine

    n, B = a.steps, a.batch
    OPT, V, _, _ = make_case("ABO", 20)
    eng = Engine(OPT, V, device=0, max_batch=B)
    g = torch.Generator(device="cuda").manual_seed(1)
    f64 = dict(dtype=torch.float64, device="cuda")
    traj = torch.rand((n, OUT_N, B), generator=g, **f64)
    traj[:, OUT["v"]] = 25.0 * torch.rand((n, B), generator=g, **f64)
    traj[:, OUT["s"]] = torch.cumsum(0.5 * traj[:, OUT["v"]], dim=0)
    traj[:, OUT["Fm"]] = 8000.0 * torch.rand((n, B), generator=g, **f64) - 3000.0
    traj[:, OUT["a"]] = 5.0 * torch.rand((n, B), generator=g, **f64) - 3.0
    status = torch.zeros((n, B), dtype=torch.int32, device="cuda")
    s_tv = traj[:, OUT["s"]] + 40.0 * torch.rand((n, B), generator=g, **f64) + 2.0
    v_tv = 25.0 * torch.rand((n, B), generator=g, **f64)
    rows = torch.tensor([OUT[k] for k in ROWS[a.table]], device="cuda")
    dst = torch.empty((n, rows.numel(), B), **f64)
    extra = {"kpis": [status], "follow": [s_tv, v_tv], "route": []}[a.table]
    extra_dst = [torch.empty_like(x) for x in extra]
    read_bytes = dst.numel() * 8 + sum(x.numel() * x.element_size() for x in extra)

    def copy():
        torch.index_select(traj, 1, rows, out=dst)
        for x, y in zip(extra, extra_dst):
            y.copy_(x)

    kernels = {"kpis": {"kpis": lambda: eng.kpis(traj, status, float(OPT["cutOffDist"]))},
               "follow": {"follow_kpis": lambda: eng.follow_kpis(traj, status, s_tv, v_tv, weights="ab")},
               "route": {"route_kpis": lambda: eng.route_kpis(traj, status),
                         "route_kpis_with_limits": lambda: eng.route_kpis(traj, status, want_limits=True)}}[a.table]

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    spread = lambda t: (max(t) - min(t)) / statistics.median(t)
    results = {}
    for name, kernel in kernels.items():
        kernel(); copy()
        torch.cuda.synchronize()
        tk, tc = [], []
        for _ in range(a.reps):
            tk.append(timed(kernel)); tc.append(timed(copy))
        mk, mc = statistics.median(tk), statistics.median(tc)
        rec = dict(entry=name, n_steps=n, batch=B, rows_read=list(ROWS[a.table]), bytes_read=read_bytes, reps=a.reps, kernel_ms=mk,
                   copy_ms=mc, kernel_over_copy=mk / mc, kernel_read_GB_per_s=1e-6 * read_bytes / mk, copy_read_GB_per_s=1e-6 * read_bytes / mc,
                   kernel_spread=spread(tk), copy_spread=spread(tc), kernel_all_ms=tk, copy_all_ms=tc)
        print(json.dumps(rec), flush=True)
        results[name] = rec
    if a.out:
        out = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                out = json.load(f)
        out.update(source_hash=bench.source_hash(), device=torch.cuda.get_device_name(0))
        out.setdefault("result", {}).update(results)
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
