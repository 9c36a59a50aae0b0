"""Generate tests/golden/conv_space.npz: FuncConvolutionOperator(domain, func,
space=) on ONE space of a two-space domain, evaluated by the reference
(NIFTy 8.5), alone and inside likelihoods on a product-spectrum field.

Like gen_golden_conv.py this script runs in the build container only, imports
the reference from there and writes nothing but data; the same NumPy shim
applies.

A reference quirk: FuncConvolutionOperator(product_domain, func, space=s)
raises ValueError("Mismatch...") from check_object_identity unless the
reference's DomainTuple cache already holds the harmonic product tuple built
from the kernel's own codomain object.  One seeding call makes it go through:
    khat = S.get_default_codomain().get_conv_kernel_from_func(func)
    DomainTuple.make((khat.domain[0], X))        # (X, khat.domain[0]) for space=1
`reference_operator` below seeds the cache this way.  (The project's operator
never raises for this.)

On a product domain the reference subtracts the mean over the WHOLE field and
the kernel's zero mode k0 is not 1, so with k the raw harmonic kernel of S
    C x = Re ifftn_S(k * fftn_S(x)) + (1 - k0) * mean(x)
(`formula`); every stored C x is checked against it to 1e-13 (relative
max-norm) before anything is written.

Operator cases S x X (OPERATOR_CASES; space = 0 unless the tag starts with
"e"), x = 0.7 + default_rng(seed).standard_normal (the seed is stored, not x).
Stored per case and kernel: khat, C x, and the sums of C x over S per pixel of
X.  Kernels: "g", a Gaussian of 1.7 pixels, and "k", the wrapping King profile
of gen_golden_conv.py; both for S grids under 4096 pixels, "g" alone above
(random data does not compress).

Likelihood case on a product field (the maker of gen_golden_product.py:
COMP_A, COMP_B, OFFSET, prefix "p_") over RGSpace((n, n), 0.1) x
RGSpace(8, 0.5), PSF "g" on space 0, for n = 8: the product core's
cg_blocks(1) is already positive there (nft_hartley_cg_blocks of the
(8, 8, 8) grid is 1), so 8 is also the carry grid and there is one case.
  a  GaussianEnergy(d, 1 / 1e-2) @ C(sigmoid(cf))
  b  PoissonianEnergy(counts) @ Mask(Exposure(C(exp(cf)))), about half the
     pixels flagged, exposure in [0.5, 2]
  c  a + b as lh1 + lh2
Per likelihood: position, tangent, energy, transformation, metric applied to
the tangent and CG iterates 1..5 of (metric + 1); for b the two samples of
one mirrored MGVI draw_samples call (seed 27, iteration limit 10).

Conditioning, as in gen_golden_product.py: the iterates are recomputed with
the right-hand side perturbed by 1e-15 (relative, per element); the largest
relative move is stored as <case>_cond and must stay below 1e-12, or nothing
is written (the tests ask 1e-9 of the iterates).

A MultiField is stored as one vector: its keys in sorted order, each raveled.

Usage:  python tests/golden/gen_golden_conv_space.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402
from nifty8.minimization.kl_energies import draw_samples  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

SIGMA_PIX = 1.7
NAMES = ("image", "counts")
COMP_A = ((1., .2), (.5, .2), (.3, .1), (-3., .5))
COMP_B = ((.5, .1), (.4, .2), None, (-2., .5))
OFFSET = (1., (0.3, 0.1))
COND_BOUND = 1e-12
FORMULA_BOUND = 1e-13
# tag: (shape of S, distances of S, shape of X, distances of X, space)
OPERATOR_CASES = {
    "s88e4": ((8, 8), 0.1, (4,), 0.5, 0),
    "s168e2": ((16, 8), (0.5, 0.25), (2,), None, 0),
    "s88e6": ((8, 8), None, (6,), None, 0),
    "s832e16": ((8, 32), None, (16,), None, 0),
    "s88e2x2": ((8, 8), None, (2, 2), None, 0),
    "s8512e10": ((8, 512), None, (10,), None, 0),
    "s10248e2": ((1024, 8), None, (2,), None, 0),
    "s88e5": ((8, 8), None, (5,), None, 0),
    "s86e4": ((8, 6), None, (4,), None, 0),
    "e4s88": ((8, 8), None, (4,), None, 1),
    "s16e8": ((16,), None, (8,), None, 0),
    "s888e2": ((8, 8, 8), None, (2,), None, 0),
}
BOTH_KERNELS_BELOW = 4096


def kernels(sp):
    """the two radial profiles of a position space: name -> func"""
    sig = SIGMA_PIX * min(sp.distances)
    r0 = 0.25 * min(n * d for n, d in zip(sp.shape, sp.distances))
    return (("g", lambda r: np.exp(-0.5 * (r / sig) ** 2)), ("k", lambda r: (1. + (r / r0) ** 2) ** -2))


def reference_operator(dom, func, space):
    """the reference's operator, its DomainTuple cache seeded (module docstring)"""
    khat = dom[space].get_default_codomain().get_conv_kernel_from_func(func)
    lm = list(dom)
    lm[space] = khat.domain[0]
    ift.DomainTuple.make(tuple(lm))
    return ift.FuncConvolutionOperator(dom, func, space=space), np.asarray(khat.val)


def formula(x, khat, axes):
    """Re ifftn_S(k * fftn_S(x)) + (1 - k0) * mean(x) over the axes of S"""
    k = khat.reshape([x.shape[a] if a in axes else 1 for a in range(x.ndim)])
    return np.fft.ifftn(k * np.fft.fftn(x, axes=axes), axes=axes).real + (1. - khat.reshape(-1)[0]) * x.mean()


def relmax(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def _pack(mf):
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def operators(d):
    worst = 0.
    for i, (tag, (ss, sd, xs, xd, space)) in enumerate(OPERATOR_CASES.items()):
        S, X = ift.RGSpace(ss, distances=sd), ift.RGSpace(xs, distances=xd)
        dom = ift.DomainTuple.make((S, X) if space == 0 else (X, S))
        seed = 300 + i
        x = 0.7 + np.random.default_rng(seed).standard_normal(dom.shape)
        d[f"{tag}_sshape"], d[f"{tag}_xshape"] = np.array(ss), np.array(xs)
        d[f"{tag}_sdist"], d[f"{tag}_xdist"] = np.array(S.distances), np.array(X.distances)
        d[f"{tag}_space"] = np.array(space)
        d[f"{tag}_seed"] = np.array(seed)
        axes = dom.axes[space]
        names = []
        for kn, func in kernels(S):
            if kn != "g" and S.size >= BOTH_KERNELS_BELOW:
                continue
            names.append(kn)
            C, khat = reference_operator(dom, func, space)
            f = ift.makeField(dom, x)
            Cx = np.asarray(C(f).val)
            Ctx = np.asarray(C.adjoint_times(f).val)
            assert relmax(Ctx, Cx) <= 1e-13, (tag, kn)
            err = relmax(formula(x, khat, axes), Cx)
            worst = max(worst, err)
            assert err < FORMULA_BOUND, (tag, kn, err)
            d[f"{tag}_{kn}_khat"] = khat
            d[f"{tag}_{kn}_Cx"] = Cx
            d[f"{tag}_{kn}_slicesums"] = Cx.sum(axis=axes)
        d[f"{tag}_kernels"] = np.array(names)
    print(f"operators: the formula reproduces the reference to {worst:.2e}")
    d["formula_err"] = np.array(worst)


def _iterates(A, t):
    out = []
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        e, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0. * t, A, t))
        out.append(e.position)
    return out


def tr_vec(f_lh, pos):
    r = f_lh(pos)
    return _pack(r) if isinstance(r, ift.MultiField) else np.asarray(r.val).reshape(-1)


def likelihoods(tag, n, d):
    S, X = ift.RGSpace((n, n), distances=0.1), ift.RGSpace((8,), distances=0.5)
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(S, *COMP_A, prefix="a")
    cfm.add_fluctuations(X, *COMP_B, prefix="b")
    cfm.set_amplitude_total_offset(*OFFSET)
    cf = cfm.finalize(prior_info=0)
    dom = cf.target
    C, _ = reference_operator(dom, kernels(S)[0][1], 0)
    with ift.random.Context(11):
        pos = 0.3 * ift.from_random(cf.domain, "normal")
    with ift.random.Context(5):
        t = ift.from_random(cf.domain, "normal")
    ift.random.push_sseq_from_seed(27)
    rng = ift.random.current_rng()
    flags = rng.random(dom.shape) < 0.5
    expo = 0.5 + 1.5 * rng.random(dom.shape)
    M = ift.MaskOperator(ift.makeField(dom, flags))
    E = ift.DiagonalOperator(ift.makeField(dom, expo))
    sr = C(ift.sigmoid(cf))
    lam = M(E(C(cf.exp())))
    data = sr(pos).val + 0.1 * rng.standard_normal(dom.shape)
    counts = rng.poisson(lam(pos).val).astype(np.int64)
    ift.random.pop_sseq()
    N = ift.ScalingOperator(dom, 1e-2, np.float64)
    lh1 = ift.GaussianEnergy(ift.makeField(dom, data), inverse_covariance=N.inverse) @ sr
    lh2 = ift.PoissonianEnergy(ift.makeField(M.target, counts)) @ lam
    lh1.name, lh2.name = NAMES
    d.update({f"{tag}_flags": flags, f"{tag}_expo": expo, f"{tag}_data": data, f"{tag}_counts": counts,
              f"{tag}_pos": _pack(pos), f"{tag}_t": _pack(t)})
    rng3 = np.random.default_rng(3)
    tp = ift.MultiField.from_dict({k: ift.makeField(t[k].domain,
                                                    t[k].val * (1. + 1e-15 * rng3.standard_normal(t[k].shape)))
                                   for k in t.keys()})
    for c, lh in (("a", lh1), ("b", lh2), ("c", lh1 + lh2)):
        pre = f"{tag}{c}"
        d[f"{pre}_energy"] = np.array(lh(pos).val)
        dtype, f_lh = lh.get_transformation()
        d[f"{pre}_tr"] = tr_vec(f_lh, pos)
        met = lh.get_metric_at(pos)
        d[f"{pre}_mt"] = _pack(met(t))
        A = met + ift.ScalingOperator(cf.domain, 1.)
        its = _iterates(A, t)
        for i, x in enumerate(its, 1):
            d[f"{pre}_cg{i}"] = _pack(x)
        worst = 0.
        for x, y in zip(its, _iterates(A, tp)):
            for k in x.keys():
                worst = max(worst, np.linalg.norm(y[k].val - x[k].val) / np.linalg.norm(x[k].val))
        print(f"{pre}: iterates move by {worst:.2e} under a 1e-15 perturbation of the right-hand side")
        assert worst < COND_BOUND, (pre, worst)
        d[f"{pre}_cond"] = np.array(worst)
        if c != "b":
            continue
        H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-30, iteration_limit=10))
        ift.random.push_sseq_from_seed(27)
        sl = draw_samples(pos, H, None, 1, True)
        ift.random.pop_sseq()
        d[f"{pre}_mgvi_samples"] = np.stack([_pack(s) for s in sl.iterator()])


def main():
    d = {"names": np.array(NAMES), "carry_grid": np.array(8), "cases": np.array(list(OPERATOR_CASES)),
         "sigma_pix": np.array(SIGMA_PIX)}
    operators(d)
    likelihoods("n8", 8, d)
    path = os.path.join(OUT, "conv_space.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"conv_space.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
