"""First measurement of the Matern correlated field on the fused path.

Workload: CorrelatedFieldMaker with ONE add_fluctuations_matern component on
an n x n grid (default 2048), LogNormal zero mode, sigmoid, Gaussian 1e-3 on
the GeometryRemover; fp64, 4 right-hand sides, count-only controllers,
nreset 20.

1. The batched CG iteration of the sampling metric, timed as
   tools/likelihood_iter_probe.py does: the difference of two solves with N1
   and N2 iterations divided by N2 - N1, best of the repetitions, the
   problems interleaved, two runs each ("name" and "name_repeat").
     matern    the Matern field as `finalize()` gives it.  The script uses the
               public interface only, so it also runs on a tree whose
               `finalize()` builds the operator tree for a Matern component:
               where the metric does not fuse to a batched solve the k
               right-hand sides are solved one after the other by
               ConjugateGradient, and "path" says so.
     nonparam  SimpleCorrelatedField (bench.CF_ARGS) with the same likelihood:
               the two-phase amplitude kernels and the deferred iterate.
   --only matern skips the second (for the comparison run on another tree).

2. (this tree only, --kernels) nft_matern_jvp_batched / nft_matern_vjp_batched
   alone for k right-hand sides, bin-major dA, beside the non-parametric
   amplitude's native_jvp_batched / native_vjp_batched (the two-phase
   kernels: jvp 2a + 2b, vjp 2a + 2b + fin) on the same grid: HIP events
   around each call, the median.  GB/s are of the algorithmic bytes,
     Matern JVP  8 B (3 + k)      three columns in, k values per bin out
     Matern VJP  8 B (3 + k)      three columns and k cotangent rows in
     non-parametric: the same 8 B k of dA / g plus its constant vectors
     (8 B * 9 + 8 (B - 2) * 6 with flexibility and asperity); the figure
     quoted for it uses that sum.

Usage: python tools/matern_iter_probe.py [--n 2048] [--rhs 4] [--only matern]
       [--kernels 20] [--out profiles/matern_iter.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.sampling_iter_probe import gaussian, metric_of  # noqa: E402

MATERN = ((1., 0.3), (2., 0.5), (-3., 0.5))


def event_us(fn, reps, warm=3):
    """median microseconds of fn() between two HIP events"""
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return float(np.median(ts))


def solve_seconds(ift, A, bs, niter):
    """(seconds, path) of k solves of niter iterations: one batched fused
    loop where the metric allows it, else one ConjugateGradient per RHS"""
    import torch
    from nifty_amd.minimization import fused_cg
    energies = [ift.QuadraticEnergy(0 * b, A, b) for b in bs]
    spec = fused_cg.fusable_metric(A)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if spec is not None and fused_cg.batch_supported(spec[0], spec[1]):
        cg = fused_cg.FusedCGBatch(spec[0], spec[1], spec[2],
                                   [ift.GradientNormController(iteration_limit=niter) for _ in bs], 20)
        cg.run(energies)
        path = "batched " + str(cg.path)
    else:
        for e in energies:
            ift.ConjugateGradient(ift.GradientNormController(iteration_limit=niter), nreset=20)(e)
        path = "one ConjugateGradient per right-hand side"
    torch.cuda.synchronize()
    return time.perf_counter() - t0, path


def kernel_figures(ift, amps, k, reps):
    import torch
    out = {}
    dev = "cuda:0"
    for name, (cf, pos) in amps.items():
        amp = cf.amp
        B = amp.B
        lay = cf.layout
        off = dict(zip(lay.keys, lay.offsets))
        lin = amp.forward_native({kk: pos[kk].val for kk in amp.domain_dict})
        if hasattr(amp, "amp2_table"):
            amp.amp2_table(lin)
        D = torch.randn((k, lay.size), dtype=torch.float64, device=dev)
        Q = torch.zeros_like(D)
        da = torch.empty((B, k), dtype=torch.float64, device=dev)
        g = torch.randn((k, B), dtype=torch.float64, device=dev)
        if name == "matern":
            bj = bv = 8 * B * (3 + k)
        else:
            bj = bv = 8 * B * k + 8 * B * 9 + 8 * (B - 2) * 6
        us = event_us(lambda: amp.native_jvp_batched(lin, D, off, da, interleave=True), reps)
        out[f"{name}_amp_jvp_k{k}"] = {"us": round(us, 1), "GBps": round(bj / us * 1e-3, 1), "B": B,
                                       "algorithmic_bytes": bj}
        us = event_us(lambda: amp.native_vjp_batched(lin, g, Q, off, D, 1.0), reps)
        out[f"{name}_amp_vjp_k{k}"] = {"us": round(us, 1), "GBps": round(bv / us * 1e-3, 1), "B": B,
                                       "algorithmic_bytes": bv}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--only", default=None, choices=[None, "matern"])
    p.add_argument("--kernels", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    ift.config.set_device("cuda:0")
    k = args.rhs
    sp = ift.RGSpace((args.n, args.n))
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(sp, *MATERN)
    cfm.set_amplitude_total_offset(0., (1e-3, 1e-6))
    fields = {"matern": cfm.finalize(prior_info=0)}
    if args.only is None:
        fields["nonparam"] = ift.SimpleCorrelatedField(sp, **bench.CF_ARGS)
    probs, amps = {}, {}
    for name, cf in fields.items():
        with ift.random.Context(27):
            pos = 0.1 * ift.from_random(cf.domain, "normal")
        with ift.random.Context(5):
            bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
        lh = gaussian(ift, ift.GeometryRemover(sp)(ift.sigmoid(cf)), 3)
        probs[name] = (metric_of(ift, lh, pos), bs)
        amps[name] = (cf, pos)
    print("problems built:", {n: type(f).__name__ for n, f in fields.items()}, flush=True)
    res = {"workload": f"{args.n}x{args.n}, one Matern component {MATERN} with LogNormal zero mode against "
                       f"SimpleCorrelatedField (bench.CF_ARGS); sigmoid, Gaussian 1e-3 on GeometryRemover; fp64, "
                       f"{k} RHS, count-only controllers, nreset 20",
           "timing": f"solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1} for all {k} RHS, best of {args.reps}, the problems interleaved, two "
                     f"runs each; kernels: median of --kernels calls between HIP events",
           "field_class": {n: type(f).__name__ for n, f in fields.items()}}
    order = [n + s for s in ("", "_repeat") for n in fields]
    for name in order:
        A, bs = probs[name.split("_")[0]]
        res[name] = {"solve_us_per_iteration": None}
        solve_seconds(ift, A, bs, args.n1)   # warm-up
    for _ in range(args.reps):
        for name in order:
            A, bs = probs[name.split("_")[0]]
            t1, _ = solve_seconds(ift, A, bs, args.n1)
            t2, path = solve_seconds(ift, A, bs, args.n2)
            us = (t2 - t1) / (args.n2 - args.n1) * 1e6
            old = res[name]["solve_us_per_iteration"]
            res[name].update(solve_us_per_iteration=us if old is None else min(old, us), path=path)
    for name in order:
        res[name]["solve_us_per_iteration"] = round(res[name]["solve_us_per_iteration"], 1)
        print(f"{name:16s} {res[name]['solve_us_per_iteration']:10.1f} us per {k}-RHS CG iteration   "
              f"{res[name]['path']}", flush=True)
    res["matern_spread_us"] = round(abs(res["matern"]["solve_us_per_iteration"]
                                        - res["matern_repeat"]["solve_us_per_iteration"]), 1)
    if "nonparam" in fields:
        res["matern_over_nonparam"] = round(
            min(res["matern"]["solve_us_per_iteration"], res["matern_repeat"]["solve_us_per_iteration"])
            / min(res["nonparam"]["solve_us_per_iteration"], res["nonparam_repeat"]["solve_us_per_iteration"]), 4)
    if args.kernels and hasattr(fields["matern"], "amp"):
        res["kernels"] = kernel_figures(ift, amps, k, args.kernels)
        for name, v in res["kernels"].items():
            print(f"{name:26s} {v['us']:9.1f} us  {v['GBps']:8.1f} GB/s  B = {v['B']}", flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
