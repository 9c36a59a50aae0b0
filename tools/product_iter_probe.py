"""First measurement of the product-spectrum correlated field on the fused path.

Workload: CorrelatedFieldMaker with TWO add_fluctuations components on
RGSpace((n, n)) x RGSpace(m) (default 512 x 512 x 32: 8.4 M pixels), LogNormal
zero mode, sigmoid, Gaussian 1e-3 on the GeometryRemover; fp64, 4 right-hand
sides, count-only controllers, nreset 20.

1. The batched CG iteration of the sampling metric, timed as
   tools/matern_iter_probe.py does: the difference of two solves with N1 and N2
   iterations divided by N2 - N1, best of the repetitions, the problems
   interleaved, two runs each ("name" and "name_repeat").
     product     the field as `finalize()` gives it.  The script uses the
                 public interface only, so it also runs on a tree whose
                 `finalize()` builds the operator tree for two components:
                 where the metric does not fuse to a batched solve the k
                 right-hand sides are solved one after the other by
                 ConjugateGradient, and "path" says so (use short solves
                 there: --n1 2 --n2 6).
     nonparam3d  SimpleCorrelatedField (bench.CF_ARGS) on RGSpace((n, n, m)):
                 the same engine and grid without the table or the mix, with
                 the two-phase amplitude kernels and the deferred iterate.
   --only product skips the second (for the comparison run on another tree).

2. (this tree only, --kernels) the four new kernels alone, HIP events around
   each call, the median.  GB/s are of the algorithmic bytes,
     nft_mirror_mix        16 B N k       every element once in, once out
     nft_prod_forward      8 B (B + 2 (B1 + B2))  the table out, a_i in, a_i / z out
     nft_prod_jvp_batched  8 B (B k + (B1 + B2)(1 + k))  dA out, a_i / z and da_i in
     nft_prod_vjp_batched  8 B (B k + (B1 + B2)(1 + k))  the bin sums in, cotangents out

Usage: python tools/product_iter_probe.py [--n 512] [--m 32] [--rhs 4]
       [--only product] [--kernels 20] [--out profiles/product_iter.json]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.matern_iter_probe import event_us, solve_seconds  # noqa: E402
from tools.sampling_iter_probe import gaussian, metric_of  # noqa: E402

COMP_A = ((1., .2), (.5, .2), (.3, .1), (-3., .5))
COMP_B = ((.5, .1), (.4, .2), None, (-2., .5))


def kernel_figures(cf, pos, k, reps):
    import torch
    from nifty_amd import _native
    lib, P = _native.load(), ctypes.c_void_p
    amp, lay, dev = cf.amp, cf.layout, "cuda:0"
    B1, B2, B = amp.B1, amp.B2, amp.B
    N = int(np.prod(cf.grid))
    off = dict(zip(lay.keys, lay.offsets))
    lat = {kk: pos[kk].val for kk in amp.domain_dict}
    lin = amp.forward_native(lat)
    X = torch.randn((k, lay.size), dtype=torch.float64, device=dev)
    xo = off[cf.k_xi]
    out = {}

    def row(name, us, nbytes):
        out[name] = {"us": round(us, 1), "GBps": round(nbytes / us * 1e-3, 1), "algorithmic_bytes": nbytes}

    us = event_us(lambda: _native.mirror_mix(X[0, xo:], X[0, xo:], cf.grid, cf.split, rows=k, x_stride=lay.size,
                                             y_stride=lay.size), reps)
    row(f"mirror_mix_k{k}", us, 16 * N * k)
    a, cb, xz = lin.a, lin.cb, lat[amp.k_zm].contiguous()
    us = event_us(lambda: _native._check(lib.nft_prod_forward(
        B1, B2, P(lin.c1.a.data_ptr()), B1, P(lin.c2.a.data_ptr()), B2, P(xz.data_ptr()), 0, amp.lm_o, amp.ls_o,
        amp.s0, amp.s1, amp.s2, 1, P(a.data_ptr()), B, P(cb.data_ptr()), cb.numel(), _native.stream_ptr())), reps)
    row("prod_forward", us, 8 * (B + 2 * (B1 + B2)))
    d1, d2 = (torch.randn((k, b), dtype=torch.float64, device=dev) for b in (B1, B2))
    da = torch.empty((B, k), dtype=torch.float64, device=dev)
    nb = 8 * (B * k + (B1 + B2) * (1 + k))
    us = event_us(lambda: amp._jvp(lin, d1, d2, X[0, off[amp.k_zm]:], lay.size, da, k), reps)
    row(f"prod_jvp_k{k}", us, nb)
    g = torch.randn((k, B), dtype=torch.float64, device=dev)
    Q = torch.zeros_like(X)
    us = event_us(lambda: amp._vjp(lin, g, k, Q[0, off[amp.k_zm]:].data_ptr(), None, lay.size, 0.0), reps)
    row(f"prod_vjp_k{k}", us, nb)
    out["sizes"] = {"B1": B1, "B2": B2, "B": B, "pixels": N}
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--only", default=None, choices=[None, "product"])
    p.add_argument("--kernels", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    ift.config.set_device("cuda:0")
    k, n, m = args.rhs, args.n, args.m
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(ift.RGSpace((n, n)), *COMP_A, prefix="a")
    cfm.add_fluctuations(ift.RGSpace(m), *COMP_B, prefix="b")
    cfm.set_amplitude_total_offset(0., (1e-3, 1e-6))
    fields = {"product": cfm.finalize(prior_info=0)}
    if args.only is None:
        fields["nonparam3d"] = ift.SimpleCorrelatedField(ift.RGSpace((n, n, m)), **bench.CF_ARGS)
    probs, points = {}, {}
    for name, cf in fields.items():
        with ift.random.Context(27):
            pos = 0.1 * ift.from_random(cf.domain, "normal")
        with ift.random.Context(5):
            bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
        lh = gaussian(ift, ift.GeometryRemover(cf.target)(ift.sigmoid(cf)), 3)
        probs[name] = (metric_of(ift, lh, pos), bs)
        points[name] = pos
    print("problems built:", {nm: type(f).__name__ for nm, f in fields.items()}, flush=True)
    res = {"workload": f"RGSpace(({n}, {n})) x RGSpace({m}), two add_fluctuations components {COMP_A} / {COMP_B} "
                       f"with LogNormal zero mode against SimpleCorrelatedField (bench.CF_ARGS) on "
                       f"RGSpace(({n}, {n}, {m})); sigmoid, Gaussian 1e-3 on GeometryRemover; fp64, {k} RHS, "
                       f"count-only controllers, nreset 20",
           "timing": f"solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1} for all {k} RHS, best of {args.reps}, the problems interleaved, two "
                     f"runs each; kernels: median of --kernels calls between HIP events",
           "field_class": {nm: type(f).__name__ for nm, f in fields.items()}}
    order = [nm + s for s in ("", "_repeat") for nm in fields]
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
        print(f"{name:18s} {res[name]['solve_us_per_iteration']:10.1f} us per {k}-RHS CG iteration   "
              f"{res[name]['path']}", flush=True)
    res["product_spread_us"] = round(abs(res["product"]["solve_us_per_iteration"]
                                         - res["product_repeat"]["solve_us_per_iteration"]), 1)
    if "nonparam3d" in fields:
        res["product_over_nonparam3d"] = round(
            min(res["product"]["solve_us_per_iteration"], res["product_repeat"]["solve_us_per_iteration"])
            / min(res["nonparam3d"]["solve_us_per_iteration"], res["nonparam3d_repeat"]["solve_us_per_iteration"]), 4)
    if args.kernels and hasattr(fields["product"], "amp"):
        res["kernels"] = kernel_figures(fields["product"], points["product"], k, args.kernels)
        for name, v in res["kernels"].items():
            if "us" in v:
                print(f"{name:20s} {v['us']:9.1f} us  {v['GBps']:8.1f} GB/s", flush=True)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
