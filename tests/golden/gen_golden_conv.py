"""Generate tests/golden/conv.npz: FuncConvolutionOperator evaluated by the
reference (NIFTy 8.5), alone and inside likelihoods.

Like gen_golden_sampling.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Operator cases: the grids of GRIDS ((1024, 8) is the smallest whose column
length takes the four-step passes; (16,) and (8, 6) are not served by the
native pipeline), each with two kernels -- a Gaussian of 1.7 pixels ("g") and
a broad King profile (1 + (r / r0)^2)^-2, r0 a quarter of the shortest extent
("k"), which wraps around the periodic boundary.  Stored per case: the
harmonic-space kernel and C x for x = 0.7 + default_rng(seed).standard_normal
(the seed is stored, not x).

Likelihood cases on a SimpleCorrelatedField (CF_ARGS of the sampling
fixture), 8 x 8 (the smallest grid on which the carried CG iteration runs)
and 16 x 16, PSF = the Gaussian of 1.7 pixels:
  a  GaussianEnergy(d, 1e-3) @ GeometryRemover(C(sigmoid(cf)))
  b  PoissonianEnergy(counts) @ Mask(Exposure(C(exp(cf)))), about half the
     pixels flagged, exposure in [0.5, 2]
  c  a + b as lh1 + lh2
with position, tangent, energy, transformation and metric applied to the
tangent; for b also the two samples of one MGVI draw_samples call (seed 27,
CG stopped by an iteration limit of 10).

Usage:  python tests/golden/gen_golden_conv.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402
from nifty8.minimization.kl_energies import draw_samples  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
NAMES = ("image", "counts")
GRIDS = (("g88", (8, 8), None), ("g168", (16, 8), (0.5, 0.25)), ("g832", (8, 32), None), ("g888", (8, 8, 8), None),
         ("g8168", (8, 16, 8), None), ("g10248", (1024, 8), None), ("g16", (16,), (0.5,)),
         ("g86", (8, 6), (0.5, 0.25)))
SIGMA_PIX = 1.7


def kernels(sp):
    """the two radial profiles of a position space: name -> func"""
    sig = SIGMA_PIX * min(sp.distances)
    r0 = 0.25 * min(n * d for n, d in zip(sp.shape, sp.distances))
    return (("g", lambda r: np.exp(-0.5 * (r / sig) ** 2)), ("k", lambda r: (1. + (r / r0) ** 2) ** -2))


def _pack(mf):
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def operators(d):
    for i, (tag, shape, dist) in enumerate(GRIDS):
        sp = ift.RGSpace(shape, distances=dist)
        seed = 100 + i
        x = 0.7 + np.random.default_rng(seed).standard_normal(shape)
        d[f"{tag}_shape"] = np.array(shape)
        d[f"{tag}_dist"] = np.array(sp.distances)
        d[f"{tag}_seed"] = np.array(seed)
        for kn, func in kernels(sp):
            C = ift.FuncConvolutionOperator(sp, func)
            khat = sp.get_default_codomain().get_conv_kernel_from_func(func)
            d[f"{tag}_{kn}_khat"] = khat.val
            d[f"{tag}_{kn}_Cx"] = C(ift.makeField(sp, x)).val
            # the adjoint is the same map (checked here, not stored)
            Ctx = C.adjoint_times(ift.makeField(sp, x)).val
            assert np.abs(Ctx - d[f"{tag}_{kn}_Cx"]).max() <= 1e-13 * np.abs(Ctx).max()


def problem(n, seed=27):
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    C = ift.FuncConvolutionOperator(sp, kernels(sp)[0][1])
    ift.random.push_sseq_from_seed(seed)
    rng = ift.random.current_rng()
    flags = rng.random((n, n)) < 0.5
    expo = 0.5 + 1.5 * rng.random((n, n))
    M = ift.MaskOperator(ift.makeField(sp, flags))
    E = ift.DiagonalOperator(ift.makeField(sp, expo))
    G = ift.GeometryRemover(sp)
    sr = G(C(ift.sigmoid(cf)))
    lam = M(E(C(cf.exp())))
    N = ift.ScalingOperator(G.target, 1e-3, np.float64)
    mock = ift.from_random(cf.domain, "normal")
    data = sr(mock) + N.draw_sample()
    counts = rng.poisson(lam(mock).val).astype(np.int64)
    pos = 0.1 * ift.from_random(cf.domain, "normal")
    ift.random.pop_sseq()
    lh1 = ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ sr
    lh2 = ift.PoissonianEnergy(ift.makeField(M.target, counts)) @ lam
    lh1.name, lh2.name = NAMES
    d = {"flags": flags, "expo": expo, "data": data.val, "counts": counts, "pos": _pack(pos)}
    return cf, lh1, lh2, pos, d


def tr_vec(f_lh, pos):
    r = f_lh(pos)
    return _pack(r) if isinstance(r, ift.MultiField) else np.asarray(r.val)


def case(tag, n, d):
    cf, lh1, lh2, pos, dd = problem(n)
    d.update({f"{tag}_{k}": v for k, v in dd.items()})
    with ift.random.Context(5):
        t = ift.from_random(cf.domain, "normal")
    d[f"{tag}_t"] = _pack(t)
    for c, lh in (("a", lh1), ("b", lh2), ("c", lh1 + lh2)):
        pre = f"{tag}{c}"
        d[f"{pre}_energy"] = np.array(lh(pos).val)
        dtype, f_lh = lh.get_transformation()
        d[f"{pre}_tr"] = tr_vec(f_lh, pos)
        d[f"{pre}_mt"] = _pack(lh.get_metric_at(pos)(t))
        if c != "b":
            continue
        # one MGVI draw: one mirrored pair, the CG stopped by its iteration limit
        H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-30, iteration_limit=10))
        ift.random.push_sseq_from_seed(27)
        sl = draw_samples(pos, H, None, 1, True)
        ift.random.pop_sseq()
        d[f"{pre}_mgvi_samples"] = np.stack([_pack(s) for s in sl.iterator()])


def main():
    d = {"names": np.array(NAMES), "carry_grid": np.array([8, 8]), "grids": np.array([g[0] for g in GRIDS]),
         "sigma_pix": np.array(SIGMA_PIX)}
    operators(d)
    case("s8", 8, d)
    case("s16", 16, d)
    path = os.path.join(OUT, "conv.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"conv.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
