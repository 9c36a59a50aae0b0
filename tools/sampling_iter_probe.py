"""Wall time per batched CG iteration of sampling metrics whose response is a
MaskOperator or a LinearInterpolator, beside the pointwise and the
line-of-sight metric on the same field.

Workload: config C3's field (bench.build_problem: 2048 x 2048
SimpleCorrelatedField, sigmoid), Gaussian noise; fp64, 4 right-hand sides,
count-only controllers, nreset 20 -- the linear solves of one draw_samples
call.  Metrics, timed in one process, interleaved (every repetition runs all
of them in turn):
  pointwise   sigmoid, GeometryRemover, Gaussian (listed twice: the spread of
              the two is the yardstick for `mask`)
  mask        the same with about half the pixels flagged at random
  los         C3 itself: LOSResponse(16384)
  interp      sigmoid, LinearInterpolator at 262144 uniformly random points

Figures per metric:
  solve  whole solves by FusedCGBatch as the product runs them: the
         difference of two solves with N1 and N2 iterations divided by
         N2 - N1 (set-up, capture and the eager first steps cancel), best of
         the repetitions
  chunk  bench.kernel_probe's per-iteration figure (graph replay of a
         19-iteration count-only chunk and its flush) where it takes the
         metric
The JSON summary also holds every cg.path, the byte sizes of the LOS plan and
of the interpolation plan, the byte floors of the two sampling kernels (k grid
reads / writes plus plan bytes) and the ratios.

--kernels N: instead, N applications of the interpolator's middle alone (for a
kernel trace of the two sampling kernels in a run of its own).

Usage: python tools/sampling_iter_probe.py [--n 2048] [--nlos 16384]
       [--npoints 262144] [--rhs 4] [--out profiles/sampling_iter.json]"""
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


def solve_seconds(ift, core, W, shift, A, bs, niter):
    import torch
    from nifty_amd.minimization.fused_cg import FusedCGBatch
    ctl = [ift.GradientNormController(iteration_limit=niter) for _ in bs]
    cg = FusedCGBatch(core, W, shift, ctl, 20)
    energies = [ift.QuadraticEnergy(0 * b, A, b) for b in bs]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    cg.run(energies)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, cg.path


def gaussian(ift, op, seed):
    """GaussianEnergy(noise draw, 1e-3) @ op"""
    N = ift.ScalingOperator(op.target, 1e-3, np.float64)
    with ift.random.Context(seed):
        data = N.draw_sample()
    return ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ op


def plan_bytes(P):
    return int(sum(v.nbytes for v in P.values() if isinstance(v, np.ndarray)))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--n", type=int, default=2048)
    p.add_argument("--nlos", type=int, default=16384)
    p.add_argument("--npoints", type=int, default=262144)
    p.add_argument("--rhs", type=int, default=4)
    p.add_argument("--n1", type=int, default=40)
    p.add_argument("--n2", type=int, default=240)
    p.add_argument("--reps", type=int, default=2)
    p.add_argument("--kernels", type=int, default=0)
    p.add_argument("--out", default=None)
    args = p.parse_args()

    import torch
    import nifty_amd as ift
    from nifty_amd.minimization.fused_cg import fusable_metric
    ift.config.set_device("cuda:0")
    k = args.rhs
    rng = np.random.default_rng(27)
    pts = rng.random((2, args.npoints))

    if args.kernels:
        sp = ift.RGSpace((args.n, args.n))
        Ri = ift.LinearInterpolator(sp, pts)
        g = torch.Generator(device="cuda:0")
        g.manual_seed(1)
        dr = torch.rand(sp.shape, dtype=torch.float64, device="cuda:0", generator=g)
        S = torch.randn((k,) + sp.shape, dtype=torch.float64, device="cuda:0", generator=g)
        mid = Ri.fused_middle(dr, 1e3, 1.0)
        q = torch.empty((k, mid.quad_blocks), dtype=torch.float64, device="cuda:0")
        for _ in range(args.kernels):
            mid(S, qpart=q)
        torch.cuda.synchronize()
        print(f"{args.kernels} applications of the interpolator middle, {k} vectors", flush=True)
        return

    cf, R, lh_los, pos, _ = bench.build_problem(ift, args.n, args.nlos, "C3")
    sp = cf.target[0]
    sig = ift.sigmoid(cf)
    Ri = ift.LinearInterpolator(sp, pts)
    M = ift.MaskOperator(ift.makeField(sp, rng.random(sp.shape) < 0.5))
    lhs = {"pointwise": gaussian(ift, ift.GeometryRemover(sp)(sig), 3),
           "mask": gaussian(ift, M(sig), 4),
           "los": lh_los,
           "interp": gaussian(ift, Ri(sig), 5)}
    print("problems built", flush=True)
    with ift.random.Context(5):
        bs = [ift.from_random(cf.domain, "normal") for _ in range(k)]
    N = args.n * args.n
    npnt, nent = args.npoints, 4 * args.npoints
    res = {"workload": f"{args.n}x{args.n} SimpleCorrelatedField, sigmoid, Gaussian 1e-3; responses: GeometryRemover, "
                       f"MaskOperator ({M.target.shape[0]} of {N} pixels kept), LOSResponse({args.nlos}), "
                       f"LinearInterpolator({npnt}); fp64, {k} RHS, count-only controllers, nreset 20",
           "timing": f"solve_us_per_iteration: (t[{args.n2} iterations] - t[{args.n1} iterations]) / "
                     f"{args.n2 - args.n1}, best of {args.reps}, the metrics interleaved; us_per_iteration: "
                     "bench.kernel_probe (graph replay of a 19-step count-only chunk + flush)",
           "los_plan_bytes": plan_bytes(R._plan_np), "interp_plan_bytes": plan_bytes(Ri._plan_np),
           "mask_plan_bytes": plan_bytes(M._plan_np),
           # k grid reads (forward) / writes (adjoint), the shared pixel scale,
           # the data vectors and the plan arrays each launch touches
           "samp_fwd_floor_bytes": 8 * (k + 1) * N + 8 * k * npnt + (4 + 8) * 2 * npnt,
           "samp_adj_floor_bytes": 8 * (k + 1) * N + 4 * (N + 1) + 4 * nent + 8 * 2 * npnt + 8 * k * npnt}
    order = ["pointwise", "mask", "los", "interp", "pointwise_repeat"]
    specs = {}
    for name in order:
        lh = lhs[name.split("_")[0]]
        A = metric_of(ift, lh, pos)
        specs[name] = (lh, A) + tuple(fusable_metric(A))
        res[name] = {"solve_us_per_iteration": None}
        solve_seconds(ift, specs[name][2], specs[name][3], specs[name][4], A, bs, args.n1)   # warm-up
    for _ in range(args.reps):
        for name in order:
            lh, A, core, W, sh = specs[name]
            t1, _ = solve_seconds(ift, core, W, sh, A, bs, args.n1)
            t2, path = solve_seconds(ift, core, W, sh, A, bs, args.n2)
            us = (t2 - t1) / (args.n2 - args.n1) * 1e6
            old = res[name]["solve_us_per_iteration"]
            res[name].update(solve_us_per_iteration=us if old is None else min(old, us), path=path)
    for name in order:
        lh, A, core, W, sh = specs[name]
        bench._CARRY_CACHE.clear()   # keyed by the core's id: the metrics share one core
        try:
            kp, it = bench.kernel_probe(ift, cf, R if name == "los" else None, lh, pos, k)
            res[name]["us_per_iteration"] = it["us_per_iteration"]
            if name == "interp":
                res["interp_kernels"] = {kk: v["avg_us"] for kk, v in kp.items()}
        except Exception as e:   # the probe does not take this metric
            res[name]["us_per_iteration"] = f"not measured ({type(e).__name__}: {e})"
        res[name]["solve_us_per_iteration"] = round(res[name]["solve_us_per_iteration"], 1)
        print(f"{name:17s} solve {res[name]['solve_us_per_iteration']:8.1f} us, chunk {res[name]['us_per_iteration']} "
              f"us per {k}-RHS CG iteration   cg.path = {res[name]['path']}", flush=True)
    s = {n: res[n]["solve_us_per_iteration"] for n in order}
    pw = min(s["pointwise"], s["pointwise_repeat"])
    res["solve_pointwise_repeat_over_pointwise"] = round(s["pointwise_repeat"] / s["pointwise"], 4)
    res["solve_mask_over_pointwise"] = round(s["mask"] / s["pointwise"], 4)
    res["solve_mask_over_pointwise_repeat"] = round(s["mask"] / s["pointwise_repeat"], 4)
    res["solve_interp_over_los"] = round(s["interp"] / s["los"], 4)
    res["solve_interp_over_pointwise"] = round(s["interp"] / pw, 4)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
