"""First measurement of the convolution response (FuncConvolutionOperator,
csrc/nft_conv.hip) on the fused path.

1. Per-call times on n x n grids (default 2048, then n / 2 and n / 4: 512 is
   the longest column the sandwich pass holds whole), k = 4 vectors, fp64, with
   column scale, row scale and the quadratic-form partials: the median of
   --calls calls between HIP events of
     native      one nft_conv_apply_batched call
     fallback    the two-transform path (NFT_CONV_NATIVE=0): per vector two
                 nft_hartley_fused calls, the scale multiply and nft_dot --
                 kernels the tree had before the native pipeline.
   GB/s are of the algorithmic bytes 8 * (2 k npix + 2 npix + n (n / 2 + 1)):
   the vectors in and out, the two scale vectors, the half-grid table.

2. The batched CG iteration of the sampling metric at n, n / 2 and n / 4 (at
   512 the columns fit the sandwich pass whole), timed as tools/matern_iter_probe.py
   does -- (t[N2 iterations] - t[N1 iterations]) / (N2 - N1), best of the
   repetitions, the problems interleaved, two runs each -- for
     psf         PoissonianEnergy(counts) @ Mask(Exposure(PSF(exp(cf)))), a
                 Gaussian PSF of 1.7 pixels, half the pixels flagged
     psf_fb      the same with NFT_CONV_NATIVE=0
     pointwise   PoissonianEnergy(counts) @ Mask(Exposure(exp(cf)))
   on a SimpleCorrelatedField (bench.CF_ARGS), k right-hand sides, count-only
   controllers, nreset 20.

Usage: python tools/conv_iter_probe.py [--n 2048] [--rhs 4] [--calls 20]
       [--out profiles/conv_iter.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
from tools.matern_iter_probe import event_us, solve_seconds  # noqa: E402
from tools.sampling_iter_probe import metric_of  # noqa: E402

SIGMA_PIX = 1.7


class forced_fallback:
    """NFT_CONV_NATIVE=0 inside the block (the operator reads it per call)"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        if self.on:
            os.environ["NFT_CONV_NATIVE"] = "0"

    def __exit__(self, *a):
        os.environ.pop("NFT_CONV_NATIVE", None)


def psf(ift, sp):
    sig = SIGMA_PIX * min(sp.distances)
    return ift.FuncConvolutionOperator(sp, lambda r: np.exp(-0.5 * (r / sig) ** 2))


def call_figures(ift, n, k, calls):
    import torch
    sp = ift.RGSpace((n, n))
    C = psf(ift, sp)
    npix = n * n
    g = torch.Generator(device="cpu").manual_seed(1)
    X = torch.randn((k, npix), generator=g, dtype=torch.float64).to("cuda:0")
    col = (torch.rand(npix, generator=g, dtype=torch.float64) + 0.5).to("cuda:0")
    row = (torch.rand(npix, generator=g, dtype=torch.float64) + 0.5).to("cuda:0")
    Y = torch.empty_like(X)
    nbytes = 8 * (2 * k * npix + 2 * npix + n * (n // 2 + 1))
    out = {}
    for name in ("native", "fallback", "native_repeat", "fallback_repeat"):
        fb = name.startswith("fallback")
        with forced_fallback(fb):
            assert C.native != fb
            q = torch.zeros((k, C.quad_blocks()), dtype=torch.float64, device="cuda:0")
            us = event_us(lambda: C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q, out=Y), calls)
        out[name] = {"us": round(us, 1), "GBps": round(nbytes / us * 1e-3, 1), "algorithmic_bytes": nbytes}
        print(f"{n}x{n} k={k} {name:16s} {us:10.1f} us  {out[name]['GBps']:8.1f} GB/s", flush=True)
    return out


def problems(ift, n, k):
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **bench.CF_ARGS)
    rng = np.random.default_rng(27)
    M = ift.MaskOperator(ift.makeField(sp, rng.random((n, n)) < 0.5))
    E = ift.DiagonalOperator(ift.makeField(sp, 0.5 + 1.5 * rng.random((n, n))))
    C = psf(ift, sp)
    with ift.random.Context(27):
        pos = 0.1 * ift.from_random(cf.domain, "normal")
    with ift.random.Context(5):
        bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
    out = {}
    lam_psf, lam_pw = M(E(C(cf.exp()))), M(E(cf.exp()))
    counts = rng.poisson(lam_psf(pos).val.cpu().numpy()).astype(np.int64)
    for name, lam, fb in (("psf", lam_psf, False), ("psf_fb", lam_psf, True), ("pointwise", lam_pw, False)):
        lh = ift.PoissonianEnergy(ift.makeField(M.target, counts)) @ lam
        with forced_fallback(fb):
            out[name] = (metric_of(ift, lh, pos), bs, fb)
    return out


def iteration_figures(ift, n, k, n1, n2, reps):
    probs = problems(ift, n, k)
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
        print(f"{n}x{n} {name:18s} {res[name]['solve_us_per_iteration']:10.1f} us per {k}-RHS CG iteration   "
              f"{res[name]['path']}", flush=True)
    return res


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    ift.config.set_device("cuda:0")
    k = args.rhs
    res = {"workload": f"Gaussian PSF of {SIGMA_PIX} pixels; fp64, {k} vectors / right-hand sides; iterations: "
                       f"Poisson @ Mask(Exposure(PSF(exp(SimpleCorrelatedField(bench.CF_ARGS))))), half the pixels "
                       f"flagged, count-only controllers, nreset 20",
           "timing": f"calls: median of {args.calls} calls between HIP events, the variants alternating, two "
                     f"runs each; solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1} for all {k} RHS, best of {args.reps}, the problems interleaved, two runs "
                     f"each"}
    for n in (args.n, args.n // 2, args.n // 4):
        res[f"calls_{n}"] = call_figures(ift, n, k, args.calls)
    for n in (args.n, args.n // 2, args.n // 4):
        res[f"iteration_{n}"] = iteration_figures(ift, n, k, args.n1, args.n2, args.reps)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
