"""What eepacc_classes_build_qp costs, in ONE process (the method of tools/gpu_qp_build_bench.py and
tools/gpu_classes_est_bench.py): the sides of a comparison alternate, --reps single launches each between two events, after one
untimed launch of each; the figure is the median, the spread (max - min) / median of the same side.  The kernel is a writer (at
N = 20 an instance of the ORIG tree is 80 KB of H and 290 KB of A against a few thousand flops), so the yardstick is a plain
device fill (torch.Tensor.fill_) of a buffer with the bytes of the five output arrays.  The outputs of the builder sides are
compared bit for bit before any timing.

(1) mixed:     the twelve GetUseCase scenarios of the ORIG tree at N = --horizon, --batch instances in all, as ONE
               eepacc_classes_build_qp launch on a class handle (kernel k_ab_build_cls) against the same instances as twelve
               eepacc_ab_build_qp launches on twelve ordinary handles (k_ab_build), queued back to back on one stream, and
               against the fill.
(2) one class: the ABO tree through eepacc_classes_build_qp on a handle with n_classes = 1 against eepacc_ab_build_qp on the
               ordinary handle, same states: what the class binding, the padding walk and the NULL branches cost the build when
               nothing is mixed.

No ratio is asserted; the figures are written down with their spreads.

  python tools/gpu_classes_build_bench.py --out profiles/classes_build_bench.json
"""
import argparse
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--horizon", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4096)
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
    from eepacc_mpc_casadi_matlab_amd.scenarios import make_s1, make_use_case_mix

    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    N, B = a.horizon, a.batch
    f64 = dict(dtype=torch.float64, device="cuda")
    INS = ("s", "v", "a_prev", "t0", "s_tv", "v_tv", "a_tv_prev")

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def states(tree):
        _, _, s_tv, v_tv = make_case(tree, 20)
        s1 = make_s1(B, load_golden("%s_abmpc" % tree.lower()), s_tv, v_tv)
        return [torch.as_tensor(np.ascontiguousarray(s1[n]), **f64) for n in INS]

    def outputs(n, nV, nC):
        return [torch.empty(n * k, **f64) for k in (nV * nV, nV, nV * nC, nC, nC)]

    def plain_build(eng, ins, outs):
        ptrs = [x.data_ptr() for x in ins + outs]
        n = ins[0].numel()
        return lambda: _check(eng.lib.eepacc_ab_build_qp(eng.h, n, *ptrs, eng._stream()))

    def class_build(eng, ins, outs):
        ptrs = [x.data_ptr() for x in ins] + [None] * 3 + [x.data_ptr() for x in outs]
        n = ins[0].numel()
        return lambda: _check(eng.lib.eepacc_classes_build_qp(eng.h, n, *ptrs, eng._stream()))

    def compare(name, sides, nbytes, extra):
        for fn in sides.values():
            fn()
        torch.cuda.synchronize()
        rec = dict(name=name, N=N, batch=B, bytes=nbytes, reps=a.reps, unit="ms", **extra())
        vals = {s: [] for s in sides}
        for _ in range(a.reps):
            for s, fn in sides.items():                         # alternating
                vals[s].append(timed(fn))
        for s, v in vals.items():
            med = statistics.median(v)
            rec[s] = dict(median_ms=med, spread=(max(v) - min(v)) / med, GB_per_s=1e-6 * nbytes / med, all_ms=v)
        names = list(sides)
        for s in names[1:]:
            rec[names[0] + "_over_" + s] = rec[names[0]]["median_ms"] / rec[s]["median_ms"]
        print(json.dumps(rec), flush=True)
        return rec

    results = []

    # (1) the twelve use cases in one launch against twelve launches and against the fill -----------------------------------
    rec = np.load(os.path.join(ROOT, "tests", "golden", "argonne_61505019_lead.npz"))
    mix = make_use_case_mix(list(range(1, 13)), (B + 11) // 12, "ORIG", N, argonne_lead=(rec["t"], rec["v_mph"]))
    cls = np.ascontiguousarray(mix["class_of"][:B], dtype=np.int32)                 # interleaved: 0, 1, ..., 11, 0, 1, ...
    ins = states("ORIG")
    mixed = Engine.from_classes(mix["OPT"], mix["V"], device=0, max_batch=B)
    mixed.set_classes(cls)
    nV, nC = mixed.classes_qp_size()
    outs = outputs(B, nV, nC)
    idx = [np.nonzero(cls == k)[0] for k in range(12)]
    dev_idx = [torch.as_tensor(i, device="cuda") for i in idx]
    singles = [Engine(o, v, device=0, max_batch=len(i)) for o, v, i in zip(mix["OPT"], mix["V"], idx)]
    assert all(e.ab_qp_size() == (nV, nC) for e in singles)                         # the ORIG tree: route rows in every class
    part_ins = [[x[d].contiguous() for x in ins] for d in dev_idx]
    part_outs = [outputs(len(i), nV, nC) for i in idx]
    builds = [plain_build(e, pi, po) for e, pi, po in zip(singles, part_ins, part_outs)]
    sizes = (nV * nV, nV, nV * nC, nC, nC)
    doubles = B * sum(sizes)
    ref = torch.empty(doubles, **f64)

    def twelve():
        for b in builds:                                        # twelve launches back to back on one stream
            b()

    def equal_outputs():
        same = True
        for j, k in enumerate(sizes):
            whole = outs[j].view(B, k)
            for d, po in zip(dev_idx, part_outs):
                x, y = whole[d], po[j].view(-1, k)
                same = same and bool(torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)) and torch.equal(x.isnan(), y.isnan()))
        return dict(nV=nV, nC=nC, outputs_bit_equal=same)

    results.append(compare("twelve_use_cases_build", dict(classes_one_launch=class_build(mixed, ins, outs), twelve_launches=twelve,
                                                          fill=lambda: ref.fill_(1.0)), 8 * doubles, equal_outputs))
    del mixed, singles, part_ins, part_outs, builds, outs, ref
    torch.cuda.empty_cache()

    # (2) one class through the class builder against the plain builder ------------------------------------------------------
    OPT, V, _, _ = make_case("ABO", N)
    ins = states("ABO")
    one = Engine.from_classes([OPT], [V], device=0, max_batch=B)
    one.set_classes(np.zeros(B, dtype=np.int32))
    plain = Engine(OPT, V, device=0, max_batch=B)
    nV, nC = plain.ab_qp_size()
    assert one.classes_qp_size() == (nV, nC)
    oc, op = outputs(B, nV, nC), outputs(B, nV, nC)
    doubles = B * (nV * nV + nV + nV * nC + 2 * nC)
    ref = torch.empty(doubles, **f64)
    same = lambda: dict(nV=nV, nC=nC, outputs_bit_equal=all(
        bool(torch.equal(torch.nan_to_num(x, nan=0.0), torch.nan_to_num(y, nan=0.0)) and torch.equal(x.isnan(), y.isnan())) for x, y in zip(oc, op)))
    results.append(compare("one_class_build", dict(classes_build_qp=class_build(one, ins, oc), ab_build_qp=plain_build(plain, ins, op),
                                                   fill=lambda: ref.fill_(1.0)), 8 * doubles, same))

    out = dict(source_hash=bench.source_hash(), device=torch.cuda.get_device_name(0), results=results)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
