"""What eepacc_{ab,fb,bl}_build_qp costs next to writing the same bytes, in ONE process.  The kernels are writers (at N = 20
an instance is 80 KB of H and 225 KB of A for ab, 115 KB and 501 KB for fb, 12.5 KB and 82 KB for bl, against a few thousand
to a few tens of thousands of flops), so the yardstick is a plain device fill (torch.Tensor.fill_) of a buffer with the bytes
of the five output arrays.

Two sizes per family: N = 20 x batch 4096, and N = 60 x batch 1024 (ab, bl) or 512 (fb).  ABO tree, perturbed golden states;
bl on Settings_BL with the states of the saved baseline run; fb at step 0 of a fresh handle, where the model is initialised
in the kernel.  Both sides write preallocated buffers; a time is the median of --reps single launches between two events,
the sides alternating, after one untimed launch of each.  Written down: both times, the bytes and build / fill.  No
assertion.

  python tools/gpu_qp_build_bench.py --family fb --out profiles/fb_qp_bench.json
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# family: golden run of the states, batch at N = 60, arguments between inputs and outputs, arguments after the outputs
FAMILIES = {"ab": ("abo_abmpc", 1024, 0, 0), "fb": ("abo_abmpc", 512, 2, 2), "bl": ("abo_blmpc", 1024, 0, 0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--family", choices=sorted(FAMILIES), required=True)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    import bench
    from conftest import make_case, load_golden
    from eepacc_mpc_casadi_matlab_amd.engine import Engine, _check
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1
    from eepacc_mpc_casadi_matlab_amd.settings import Settings_BL

    golden, B60, n_model, n_used = FAMILIES[a.family]
    _, _, s_tv, v_tv = make_case("ABO", 20)
    G = load_golden(golden)
    f64 = dict(dtype=torch.float64, device="cuda")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    results = []
    for N, B in ((20, 4096), (60, B60)):
        OPT, V, _, _ = make_case("ABO", N)
        eng = Engine(Settings_BL(OPT) if a.family == "bl" else OPT, V, device=0, max_batch=B)
        nV, nC = getattr(eng, a.family + "_qp_size")()
        build_qp = getattr(eng.lib, "eepacc_%s_build_qp" % a.family)
        s1 = make_s1(B, G, s_tv, v_tv)
        ins = [torch.as_tensor(np.ascontiguousarray(s1[n]), **f64) for n in ("s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev")]
        sizes = (nV * nV, nV, nV * nC, nC, nC)
        outs = [torch.empty(B * n, **f64) for n in sizes]
        doubles = B * sum(sizes)
        ref = torch.empty(doubles, **f64)
        ptrs = [x.data_ptr() for x in ins] + [None] * n_model + [x.data_ptr() for x in outs] + [None] * n_used
        build = lambda: _check(build_qp(eng.h, B, *ptrs, eng._stream()))
        fill = lambda: ref.fill_(1.0)
        build(); fill()
        torch.cuda.synchronize()
        tb, tf = [], []
        for _ in range(a.reps):
            tb.append(timed(build)); tf.append(timed(fill))
        mb, mf = statistics.median(tb), statistics.median(tf)
        rec = dict(N=N, batch=B, nV=nV, nC=nC, bytes=8 * doubles, reps=a.reps, build_ms=mb, fill_ms=mf, build_over_fill=mb / mf,
                   build_GB_per_s=8e-6 * doubles / mb, fill_GB_per_s=8e-6 * doubles / mf, build_all_ms=tb, fill_all_ms=tf)
        print(json.dumps(rec), flush=True)
        results.append(rec)
        del outs, ref, eng
        torch.cuda.empty_cache()
    out = dict(source_hash=bench.source_hash(), device=torch.cuda.get_device_name(0), result=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
