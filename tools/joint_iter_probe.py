"""Wall time per batched CG iteration of a joint likelihood's sampling metric.

Workload: config C3's field and line-of-sight set (bench.build_problem: 2048 x
2048 SimpleCorrelatedField, sigmoid, LOSResponse(16384), Gaussian noise) plus
Poisson counts of exp(field) on the full grid; fp64, 4 right-hand sides,
count-only controllers -- the linear solves of one draw_samples call.

Three metrics are timed the same way, in one process:
  los      the LOS likelihood alone (the single-likelihood carried iteration)
  joint    lh_los + lh_counts through the fused joint middle
           (nft_los_adjoint_add)
  generic  the same joint metric with the branch results summed by a generic
           callable (operators/middle.SumMiddle): the fallback for
           mixes without a fused middle

Two figures per metric:
  chunk  the carried iteration as the bench line's `roofline` block times it
         (bench.kernel_probe: HIP-graph replay of a 19-iteration count-only
         chunk with the deferred iterate and its flush, per iteration; for
         `generic`, which has no carried iteration, bench.cg_iteration_wall)
  solve  whole solves by FusedCGBatch as the product runs them (nreset = 20,
         every 20th step the exact residual): the difference of two solves
         with N1 and N2 iterations divided by N2 - N1, so set-up, capture and
         the eager first steps cancel
Prints one line per metric with both and cg.path, then a JSON summary (with
the joint metric's per-kernel table).

Usage: python tools/joint_iter_probe.py [--n 2048] [--nlos 16384] [--rhs 4]
       [--out profiles/joint_iter.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def metric_of(ift, lh, pos):
    dtype, f = lh.get_transformation()
    fl = f(ift.Linearization.make_var(pos))
    return (ift.SandwichOperator.make(fl.jac, ift.ScalingOperator(f.target, 1., dtype))
            + ift.ScalingOperator(fl.domain, 1., float))


def time_solves(ift, core, W, shift, A, bs, n1, n2, reps):
    """us per iteration of the batched solve, and its path"""
    import torch
    from nifty_amd.minimization.fused_cg import FusedCGBatch

    def solve(niter):
        ctl = [ift.GradientNormController(iteration_limit=niter) for _ in bs]
        cg = FusedCGBatch(core, W, shift, ctl, 20)
        energies = [ift.QuadraticEnergy(0 * b, A, b) for b in bs]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        cg.run(energies)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, cg.path
    solve(n1)   # warm-up: plans, workspaces, caches
    best = None
    for _ in range(reps):
        t1, _ = solve(n1)
        t2, path = solve(n2)
        us = (t2 - t1) / (n2 - n1) * 1e6
        best = us if best is None else min(best, us)
    return best, path


def chunk_us(ift, cf, R, lh, pos, k, generic=False):
    """(us per iteration as bench.kernel_probe reports it, kernel table)"""
    import torch
    from nifty_amd import _native
    from nifty_amd.operators.middle import SumMiddle
    bench._CARRY_CACHE.clear()   # keyed by the core's id: the metrics share one core
    if not generic:
        kp, it = bench.kernel_probe(ift, cf, R, lh, pos, k)
        return it["us_per_iteration"], kp
    lib = _native.load()
    core, W, shift, XS = bench.probe_setup(ift, lh, pos, k)
    W = SumMiddle([W.los, W.addw])
    X, Rr, D = XS[:k].clone(), XS[k:2 * k].clone(), XS[2 * k:].clone()
    SC = torch.zeros((k, _native.CG_NSCALARS), dtype=torch.float64, device=X.device)
    SC[:, _native.CG_GAMMA] = 1.0
    SC[:, _native.CG_GPREV] = 1.0
    ws = _native.workspace(k * lib.nft_reduce_workspace(X.shape[1]), X.device, "cgb")
    return bench.cg_iteration_wall(lib, core, W, shift, (X, Rr, D, torch.zeros_like(X), SC, ws), k), None


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--nlos", type=int, default=16384)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import nifty_amd as ift
    from nifty_amd.minimization.fused_cg import fusable_metric
    from nifty_amd.operators.middle import SumMiddle
    ift.config.set_device("cuda:0")
    cf, R, lh_los, pos, _ = bench.build_problem(ift, args.n, args.nlos, "C3")
    lam = cf.exp()
    counts = np.random.default_rng(27).poisson(lam(pos).val.cpu().numpy()).astype(np.int64)
    lh_cnt = ift.PoissonianEnergy(ift.makeField(cf.target, counts)) @ lam
    with ift.random.Context(5):
        bs = [ift.from_random(cf.domain, "normal") for _ in range(args.rhs)]

    res = {"workload": f"{args.n}x{args.n} SimpleCorrelatedField, sigmoid + LOSResponse({args.nlos}) Gaussian, "
                       f"exp + Poisson on the grid; fp64, {args.rhs} RHS, count-only controllers, nreset 20",
           "timing": "us_per_iteration: bench.kernel_probe (graph replay of a 19-step count-only chunk + flush; "
                     "generic: bench.cg_iteration_wall); solve_us_per_iteration: "
                     f"(t[{args.n2} iterations] - t[{args.n1} iterations]) / {args.n2 - args.n1}, best of {args.reps}"}
    A_los = metric_of(ift, lh_los, pos)
    A_joint = metric_of(ift, lh_los + lh_cnt, pos)
    core_l, W_l, sh_l = fusable_metric(A_los)
    core_j, W_j, sh_j = fusable_metric(A_joint)
    assert callable(W_j) and hasattr(W_j, "los"), "the joint metric did not take the fused joint middle"
    W_g = SumMiddle([W_j.los, W_j.addw])
    lh_joint = lh_los + lh_cnt
    for name, (core, W, sh, A, lh) in (("los", (core_l, W_l, sh_l, A_los, lh_los)),
                                       ("joint", (core_j, W_j, sh_j, A_joint, lh_joint)),
                                       ("generic", (core_j, W_g, sh_j, A_joint, lh_joint))):
        us, path = time_solves(ift, core, W, sh, A, bs, args.n1, args.n2, args.reps)
        cu, kp = chunk_us(ift, cf, R, lh, pos, args.rhs, generic=name == "generic")
        res[name] = {"us_per_iteration": round(cu, 1), "solve_us_per_iteration": round(us, 1), "path": path}
        if name == "joint":
            res["joint_kernels"] = {k: v["avg_us"] for k, v in kp.items()}
        print(f"{name:8s} chunk {cu:8.1f} us, solve {us:8.1f} us per {args.rhs}-RHS CG iteration   "
              f"cg.path = {path}", flush=True)
    for key in ("us_per_iteration", "solve_us_per_iteration"):
        pre = "" if key == "us_per_iteration" else "solve_"
        res[pre + "joint_over_los"] = round(res["joint"][key] / res["los"][key], 4)
        res[pre + "generic_over_los"] = round(res["generic"][key] / res["los"][key], 4)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
