"""First measurement of one block-Lanczos step at the C3 latent size.

Workload: the packed latent vector of bench.py's C3 problem (2048 x 2048
SimpleCorrelatedField, sigmoid, LOSResponse, Gaussian 1e-3), a basis of m = 64
vectors and a block of k = 8, fp64.  Timed alone, HIP events around each call,
the median of --reps (default 20) after 3 warm-up calls:

  gram_dots    nft_gram_dots  (partials + fold)    8 (m + k) n bytes
  gram_axpy    nft_gram_axpy  (beta = 1)           8 (m + 2 k) n bytes
  matvec       core.metric_flat_batch on the k rows (the fused metric; no
               algorithmic byte count of its own here: bench.py has its roofline)
  torch_matmul V @ W.T        (hipBLASLt / rocBLAS GEMM, same shape and bytes as gram_dots)
  torch_addmm  W.addmm_(T.T, V) (same shape and bytes as gram_axpy)

GB/s are of the algorithmic bytes.  The GEMMs give no fixed summation order
and no independence of the block size; they are the yardstick for the
bandwidth only.  --n overrides the grid edge (small values for a dry run).

Usage: python tools/eig_probe.py [--n 2048] [--nlos 16384] [--m 64] [--k 8]
       [--reps 20] [--out profiles/eig_probe.json]"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--nlos", type=int, default=16384)
    p.add_argument("--m", type=int, default=64)
    p.add_argument("--k", type=int, default=8)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import nifty_amd as ift
    from nifty_amd import _native
    ift.config.set_device("cuda:0")
    m, k = args.m, args.k
    cf, R, lh, pos, _ = bench.build_problem(ift, args.n, args.nlos, "C3")
    core, W, shift, X = bench.probe_setup(ift, lh, pos, k)
    n = core.layout.size
    dev = core.layout.device
    g = torch.Generator(device=dev)
    g.manual_seed(99)
    V = torch.randn((m, n), dtype=torch.float64, device=dev, generator=g)
    Wb = X[:k].double().contiguous()
    Q = torch.zeros_like(Wb)
    T = torch.randn((m, k), dtype=torch.float64, device=dev, generator=g) * 1e-3
    C = torch.empty((m, k), dtype=torch.float64, device=dev)
    Tt = T.t().contiguous()
    bytes_dots, bytes_axpy = 8 * (m + k) * n, 8 * (m + 2 * k) * n
    res = {"workload": f"C3 latent vector ({args.n}x{args.n} SimpleCorrelatedField, LOSResponse({args.nlos})): "
                       f"n = {n} doubles, basis m = {m}, block k = {k}, fp64",
           "timing": f"median of {args.reps} calls between HIP events, 3 warm-up calls; GB/s of the algorithmic bytes",
           "n": n, "m": m, "k": k, "gram_tile": int(_native.load().nft_gram_tile()),
           "gram_blocks": int(_native.load().nft_gram_blocks(n))}

    def entry(name, us, nbytes=None):
        res[name] = {"us": round(us, 1)}
        if nbytes is not None:
            res[name].update(algorithmic_bytes=nbytes, GBps=round(nbytes / us * 1e-3, 1))
        print(f"{name:14s} {us:11.1f} us" + (f"  {nbytes / us * 1e-3:8.1f} GB/s" if nbytes else ""), flush=True)

    entry("gram_dots", event_us(lambda: _native.gram_dots(V, Wb, out=C), args.reps), bytes_dots)
    entry("gram_axpy", event_us(lambda: _native.gram_axpy(V, T, Wb, 1.0), args.reps), bytes_axpy)
    entry("matvec", event_us(lambda: core.metric_flat_batch(Wb, Q, W, 0.0), args.reps))
    entry("torch_matmul", event_us(lambda: torch.matmul(V, Wb.t(), out=C), args.reps), bytes_dots)
    entry("torch_addmm", event_us(lambda: Wb.addmm_(Tt, V), args.reps), bytes_axpy)
    res["dots_over_torch"] = round(res["gram_dots"]["us"] / res["torch_matmul"]["us"], 3)
    res["axpy_over_torch"] = round(res["gram_axpy"]["us"] / res["torch_addmm"]["us"], 3)
    step = 2 * (res["gram_dots"]["us"] + res["gram_axpy"]["us"]) + res["matvec"]["us"]
    res["block_step_us"] = round(step, 1)
    res["block_step"] = "matvec + two Gram-Schmidt passes (2 x dots + 2 x axpy) at m = %d" % m
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
