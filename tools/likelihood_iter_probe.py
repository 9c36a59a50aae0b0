"""First measurement of the pointwise likelihoods (BernoulliEnergy,
StudentTEnergy, InverseGammaEnergy) on the fused path.

Workload: config C3's field (2048 x 2048 SimpleCorrelatedField, sigmoid);
fp64, 4 right-hand sides, count-only controllers, nreset 20.

1. The batched CG iteration of the Bernoulli sampling metric beside the
   pointwise Gaussian one (sigmoid, GeometryRemover, Gaussian 1e-3), timed
   in one process, interleaved, two runs each.  Both middles are one grid
   tensor, so the kernels and the bytes are the same: the larger Bernoulli
   figure may exceed the larger Gaussian one by no more than the spread of
   the two Gaussian runs (`bernoulli_within_gaussian_spread`).  Figure: the
   difference of two solves with N1 and N2 iterations divided by N2 - N1
   (set-up, capture and the eager first steps cancel), best of the
   repetitions, as tools/sampling_iter_probe.py.

2. nft_lh_eval_batched (value + gradient, and the weight alone) and
   nft_lh_transform_pair for 4 and 8 rows, HIP events around REPS calls, the
   median; beside the torch restatement of the same formulas over the same
   tensors.  GB/s are of the algorithmic bytes: 8 k n in, 8 k n per output
   array, 8 n per parameter array.  There is no target for these figures.

Usage: python tools/likelihood_iter_probe.py [--n 2048] [--rhs 4]
       [--out profiles/likelihood_iter.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.sampling_iter_probe import gaussian, metric_of, solve_seconds  # noqa: E402


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


def torch_terms(kind, F, p0, p1, want):
    """the formulas of nft_lh_eval_batched as torch passes; want: 'vg' | 'w'"""
    import torch
    if kind == "bernoulli":
        if want == "w":
            return 1. / (F * (1. - F))
        return (-torch.log(F) * p0 + torch.log(1. - F) * (p0 - 1.)).sum(1), -p0 / F + (1. - p0) / (1. - F)
    if kind == "student_t":
        if want == "w":
            return ((p0 + 1.) / (p0 + 3.)).expand_as(F).contiguous()
        return ((p0 + 1.) / 2. * torch.log1p(F * F / p0)).sum(1), (p0 + 1.) * F / (p0 + F * F)
    if want == "w":
        return p0 / (F * F)
    return (p0 * torch.log(F) + p1 / F).sum(1), p0 / F - p1 / (F * F)


def kernel_figures(n, rows, reps):
    import torch
    from nifty_amd import _native
    dev = "cuda:0"
    g = torch.Generator(device=dev)
    g.manual_seed(3)
    rnd = lambda *s: torch.rand(*s, dtype=torch.float64, device=dev, generator=g)  # noqa: E731
    params = {"bernoulli": (_native.LH_BERNOULLI, (rnd(n) < 0.5).to(torch.float64), None),
              "student_t": (_native.LH_STUDENT_T, 2. + 4. * rnd(n), None),
              "invgamma": (_native.LH_INVGAMMA, 0.5 + rnd(n), 0.05 + rnd(n))}
    out = {}
    for k in rows:
        F = 0.05 + 0.9 * rnd(k, n)
        for kind, (code, p0, p1) in params.items():
            npar = 1 + (p1 is not None)
            for want, nout, kw in (("vg", 1, dict(value=True, grad=True)), ("w", 1, dict(weight=True))):
                nbytes = 8 * k * n * (1 + nout) + 8 * n * npar
                us = event_us(lambda: _native.lh_eval_batched(code, F, p0, p1, 0.0, 1.0, **kw), reps)
                ust = event_us(lambda: torch_terms(kind, F, p0, p1, want), reps)
                out[f"lh_eval_{kind}_{want}_k{k}"] = {"us": round(us, 1), "GBps": round(nbytes / us * 1e-3, 1),
                                                      "torch_us": round(ust, 1), "algorithmic_bytes": nbytes}
        Ff = F.reshape(-1)
        t, d = torch.empty_like(Ff), torch.empty_like(Ff)
        us = event_us(lambda: _native.lh_transform_pair(_native.LH_BERNOULLI, Ff, t, d), reps)
        ust = event_us(lambda: (-2. * torch.arctan(torch.sqrt((1. - Ff) / Ff)), 1. / torch.sqrt(Ff * (1. - Ff))), reps)
        nbytes = 8 * k * n * 3
        out[f"lh_transform_pair_k{k}"] = {"us": round(us, 1), "GBps": round(nbytes / us * 1e-3, 1),
                                          "torch_us": round(ust, 1), "algorithmic_bytes": nbytes}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--kreps", type=int, default=20)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    from nifty_amd.minimization.fused_cg import fusable_metric
    ift.config.set_device("cuda:0")
    k = args.rhs
    sp = ift.RGSpace((args.n, args.n))
    cf = ift.SimpleCorrelatedField(sp, **bench.CF_ARGS)
    sig = ift.sigmoid(cf)
    ift.random.push_sseq_from_seed(27)
    pos = 0.1 * ift.from_random(cf.domain, "normal")
    events = (ift.random.current_rng().random(sp.shape) < sig(pos).val.cpu().numpy()).astype(np.int64)
    ift.random.pop_sseq()
    lhs = {"gaussian": gaussian(ift, ift.GeometryRemover(sp)(sig), 3),
           "bernoulli": ift.BernoulliEnergy(ift.makeField(sp, events)) @ sig}
    print("problems built", flush=True)
    with ift.random.Context(5):
        bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
    res = {"workload": f"{args.n}x{args.n} SimpleCorrelatedField, sigmoid; Gaussian 1e-3 on GeometryRemover and "
                       f"BernoulliEnergy on the grid; fp64, {k} RHS, count-only controllers, nreset 20",
           "timing": f"solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1}, best of {args.reps}, the metrics interleaved; kernels: median of "
                     f"{args.kreps} calls between HIP events, GB/s of the algorithmic bytes"}
    order = ["gaussian", "bernoulli", "gaussian_repeat", "bernoulli_repeat"]
    specs = {}
    for name in order:
        A = metric_of(ift, lhs[name.split("_")[0]], pos)
        specs[name] = (A,) + tuple(fusable_metric(A))
        res[name] = {"solve_us_per_iteration": None}
        solve_seconds(ift, specs[name][1], specs[name][2], specs[name][3], A, bs, args.n1)   # warm-up
    for _ in range(args.reps):
        for name in order:
            A, core, W, sh = specs[name]
            t1, _ = solve_seconds(ift, core, W, sh, A, bs, args.n1)
            t2, path = solve_seconds(ift, core, W, sh, A, bs, args.n2)
            us = (t2 - t1) / (args.n2 - args.n1) * 1e6
            old = res[name]["solve_us_per_iteration"]
            res[name].update(solve_us_per_iteration=us if old is None else min(old, us), path=path)
    s = {}
    for name in order:
        s[name] = res[name]["solve_us_per_iteration"] = round(res[name]["solve_us_per_iteration"], 1)
        print(f"{name:17s} solve {s[name]:8.1f} us per {k}-RHS CG iteration   cg.path = {res[name]['path']}", flush=True)
    spread = abs(s["gaussian"] - s["gaussian_repeat"])
    res["gaussian_spread_us"] = round(spread, 1)
    res["bernoulli_over_gaussian"] = round(max(s["bernoulli"], s["bernoulli_repeat"])
                                           / max(s["gaussian"], s["gaussian_repeat"]), 4)
    res["bernoulli_within_gaussian_spread"] = bool(
        max(s["bernoulli"], s["bernoulli_repeat"]) <= max(s["gaussian"], s["gaussian_repeat"]) + spread)
    res["kernels"] = kernel_figures(args.n * args.n, (4, 8), args.kreps)
    for name, v in res["kernels"].items():
        print(f"{name:34s} {v['us']:9.1f} us  {v['GBps']:8.1f} GB/s   torch {v['torch_us']:9.1f} us", flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
