"""First measurement of the convolution on one space of a product domain
(FuncConvolutionOperator.on_space(domain, func, 0), nft_conv_space_* of
csrc/nft_conv.hip) on the fused path.

Workload: RGSpace((n, n)) x RGSpace(m) (default 512 x 512 x 32: 8.4 M pixels),
a Gaussian PSF of 1.7 pixels on space 0; fp64, k = 4 vectors / right-hand
sides.

1. One apply_rows call with column scale, row scale and the quadratic-form
   partials: the median of --calls calls between HIP events of
     native      one nft_conv_space_apply_batched call
     fallback    the two-transform path (NFT_CONV_NATIVE=0): per vector two
                 nft_hartley_fused calls over the axes of space 0, the mean,
                 one add, the scale multiply and nft_dot
   the two alternating, two runs each.  GB/s are of the algorithmic bytes
   48 k N + 16 N + 8 n^2: three passes that read and write the k vectors, the
   two scale vectors, the table.

2. The batched CG iteration of the sampling metric, timed as
   tools/product_iter_probe.py does -- (t[N2 iterations] - t[N1 iterations]) /
   (N2 - N1), best of the repetitions, the problems interleaved, two runs each
   -- on the product field of that probe (two add_fluctuations components,
   LogNormal zero mode) for
     psf         PoissonianEnergy(counts) @ Mask(Exposure(PSF(exp(cf)))), half
                 the pixels flagged, exposure in [0.5, 2]
     psf_fb      the same with NFT_CONV_NATIVE=0
     pointwise   PoissonianEnergy(counts) @ Mask(Exposure(exp(cf)))
     product     the workload of tools/product_iter_probe.py: Gaussian 1e-3 on
                 GeometryRemover(sigmoid(cf)), no response at all
   k right-hand sides, count-only controllers, nreset 20.

Usage: python tools/conv_space_iter_probe.py [--n 512] [--m 32] [--rhs 4]
       [--calls 20] [--out profiles/conv_space_iter.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tools.conv_iter_probe import SIGMA_PIX, forced_fallback  # noqa: E402
from tools.matern_iter_probe import event_us, solve_seconds  # noqa: E402
from tools.product_iter_probe import COMP_A, COMP_B  # noqa: E402
from tools.sampling_iter_probe import gaussian, metric_of  # noqa: E402


def psf(ift, dom):
    sig = SIGMA_PIX * min(dom[0].distances)
    return ift.FuncConvolutionOperator.on_space(dom, lambda r: np.exp(-0.5 * (r / sig) ** 2), space=0)


def call_figures(ift, n, m, k, calls):
    import torch
    dom = ift.DomainTuple.make((ift.RGSpace((n, n)), ift.RGSpace(m)))
    C = psf(ift, dom)
    npix = dom.size
    g = torch.Generator(device="cpu").manual_seed(1)
    X = torch.randn((k, npix), generator=g, dtype=torch.float64).to("cuda:0")
    col = (torch.rand(npix, generator=g, dtype=torch.float64) + 0.5).to("cuda:0")
    row = (torch.rand(npix, generator=g, dtype=torch.float64) + 0.5).to("cuda:0")
    Y = torch.empty_like(X)
    nbytes = 48 * k * npix + 16 * npix + 8 * n * n
    out = {}
    for name in ("native", "fallback", "native_repeat", "fallback_repeat"):
        fb = name.startswith("fallback")
        with forced_fallback(fb):
            assert C.native != fb
            q = torch.zeros((k, C.quad_blocks()), dtype=torch.float64, device="cuda:0")
            us = event_us(lambda: C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q, out=Y), calls)
        out[name] = {"us": round(us, 1), "GBps": round(nbytes / us * 1e-3, 1), "algorithmic_bytes": nbytes}
        print(f"{n}x{n}x{m} k={k} {name:16s} {us:10.1f} us  {out[name]['GBps']:8.1f} GB/s", flush=True)
    return out


def problems(ift, n, m, k):
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(ift.RGSpace((n, n)), *COMP_A, prefix="a")
    cfm.add_fluctuations(ift.RGSpace(m), *COMP_B, prefix="b")
    cfm.set_amplitude_total_offset(0., (1e-3, 1e-6))
    cf = cfm.finalize(prior_info=0)
    dom = cf.target
    rng = np.random.default_rng(27)
    M = ift.MaskOperator(ift.makeField(dom, rng.random(dom.shape) < 0.5))
    E = ift.DiagonalOperator(ift.makeField(dom, 0.5 + 1.5 * rng.random(dom.shape)))
    C = psf(ift, dom)
    with ift.random.Context(27):
        pos = 0.1 * ift.from_random(cf.domain, "normal")
    with ift.random.Context(5):
        bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
    # at 0.1 * normal this field has a standard deviation of about 50 (the
    # sigmoid of the product probe does not mind); its exponential needs a
    # point 50 times closer to zero to stay in a Poisson rate's range
    pos_exp = 0.02 * pos
    lam_psf, lam_pw = M(E(C(cf.exp()))), M(E(cf.exp()))
    counts = rng.poisson(lam_psf(pos_exp).val.cpu().numpy()).astype(np.int64)
    out = {}
    for name, lam, fb in (("psf", lam_psf, False), ("psf_fb", lam_psf, True), ("pointwise", lam_pw, False)):
        lh = ift.PoissonianEnergy(ift.makeField(M.target, counts)) @ lam
        with forced_fallback(fb):
            out[name] = (metric_of(ift, lh, pos_exp), bs, fb)
    lh = gaussian(ift, ift.GeometryRemover(dom)(ift.sigmoid(cf)), 3)
    out["product"] = (metric_of(ift, lh, pos), bs, False)
    return out


def iteration_figures(ift, n, m, k, n1, n2, reps):
    probs = problems(ift, n, m, k)
    res = {}
    order = [nm + s for s in ("", "_repeat") for nm in probs]
    for name in order:
        A, bs, fb = probs[name.replace("_repeat", "")]
        res[name] = {"solve_us_per_iteration": None}
        with forced_fallback(fb):
            solve_seconds(ift, A, bs, n1)   # warm-up
    for _ in range(reps):
        for name in order:
            A, bs, fb = probs[name.replace("_repeat", "")]
            with forced_fallback(fb):
                t1, _ = solve_seconds(ift, A, bs, n1)
                t2, path = solve_seconds(ift, A, bs, n2)
            us = (t2 - t1) / (n2 - n1) * 1e6
            old = res[name]["solve_us_per_iteration"]
            res[name].update(solve_us_per_iteration=us if old is None else min(old, us), path=path)
    for name in order:
        res[name]["solve_us_per_iteration"] = round(res[name]["solve_us_per_iteration"], 1)
        print(f"{n}x{n}x{m} {name:18s} {res[name]['solve_us_per_iteration']:10.1f} us per {k}-RHS CG iteration   "
              f"{res[name]['path']}", flush=True)
    for nm in probs:
        res[nm + "_spread_us"] = round(abs(res[nm]["solve_us_per_iteration"]
                                           - res[nm + "_repeat"]["solve_us_per_iteration"]), 1)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--m", type=int, default=32)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    ift.config.set_device("cuda:0")
    k, n, m = args.rhs, args.n, args.m
    res = {"workload": f"RGSpace(({n}, {n})) x RGSpace({m}), Gaussian PSF of {SIGMA_PIX} pixels on space 0; fp64, {k} "
                       f"vectors / right-hand sides; iterations: the product field of tools/product_iter_probe.py "
                       f"under Poisson @ Mask(Exposure(PSF(exp(cf)))), half the pixels flagged (psf, psf_fb with "
                       f"NFT_CONV_NATIVE=0), the same without the PSF (pointwise), and that probe's Gaussian "
                       f"workload (product); count-only controllers, nreset 20",
           "timing": f"calls: median of {args.calls} calls between HIP events, the variants alternating, two runs "
                     f"each; solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1} for all {k} RHS, best of {args.reps}, the problems interleaved, two runs "
                     f"each"}
    res["calls"] = call_figures(ift, n, m, k, args.calls)
    res["iteration"] = iteration_figures(ift, n, m, k, args.n1, args.n2, args.reps)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
