"""Generate tests/golden/product.npz: correlated fields with TWO
add_fluctuations components on a product domain (CorrelatedFieldMaker with a
LogNormal zero mode) evaluated by the reference (NIFTy 8.5).

Like gen_golden_matern.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

The maker: prefix "p_", component "a" on space 1 with fluctuations (1, .2),
flexibility (.5, .2), asperity (.3, .1), loglogavgslope (-3, .5), component
"b" on space 2 with (.5, .1), (.4, .2), None, (-2, .5), and
set_amplitude_total_offset(1., (0.3, 0.1)).

Cases (space 1 x space 2):
  p16x8    RGSpace(16, 0.3) x RGSpace(8, 0.5)
  p8x8x4   RGSpace((8, 8), 0.1) x RGSpace(4, 0.5)
  p4x8x8   RGSpace(4, 0.5) x RGSpace((8, 8), 0.1): group 2 two-dimensional
  p6x5     RGSpace(6, 0.3) x RGSpace(5, 0.5): not a power of two
  p64x64   RGSpace(64, 0.3) x RGSpace(64, 0.5): 4096 pixels, the smallest
           grid where the mirror fold and the pair sums engage

Per case: the latent point (0.3 * from_random, seed 11), a tangent (seed 5), a
cotangent (seed 7), the value, J t, J^T g and the two normalised amplitudes.
For p16x8, p8x8x4 and p64x64 with GaussianEnergy(data, 1 / 1e-2) @ sigmoid(cf):
get_metric_at applied to the tangent and CG iterates 1..5 of (metric + 1); for
p16x8 and p8x8x4 one mirrored geoVI draw (controllers of gen_golden_matern.py).

Conditioning: the CG iterates are recomputed with the right-hand side
perturbed by 1e-15 (relative, per element); every key of every iterate must
move by less than 1e-12 (relative 2-norm), or the 1e-9 the tests ask of the
iterates would mean nothing.  The measured maximum is stored as <case>_cond.

A MultiField is stored as one vector: its keys in sorted order, each raveled.

Usage:  python tests/golden/gen_golden_product.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

COMP_A = ((1., .2), (.5, .2), (.3, .1), (-3., .5))
COMP_B = ((.5, .1), (.4, .2), None, (-2., .5))
OFFSET = (1., (0.3, 0.1))
# per case: (shape, distances) of space 1 and of space 2
CASES = {
    "p16x8": (((16,), 0.3), ((8,), 0.5)),
    "p8x8x4": (((8, 8), 0.1), ((4,), 0.5)),
    "p4x8x8": (((4,), 0.5), ((8, 8), 0.1)),
    "p6x5": (((6,), 0.3), ((5,), 0.5)),
    "p64x64": (((64,), 0.3), ((64,), 0.5)),
}
METRIC_CASES = ("p16x8", "p8x8x4", "p64x64")
GEO_CASES = ("p16x8", "p8x8x4")
COND_BOUND = 1e-12


def _pack(mf):
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def maker(s1, s2):
    sp1, sp2 = (ift.RGSpace(sh, distances=ds) for sh, ds in (s1, s2))
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(sp1, *COMP_A, prefix="a")
    cfm.add_fluctuations(sp2, *COMP_B, prefix="b")
    cfm.set_amplitude_total_offset(*OFFSET)
    return cfm


def _iterates(A, t):
    out = []
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        e, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0. * t, A, t))
        out.append(e.position)
    return out


def case(tag, d):
    cfm = maker(*CASES[tag])
    cf = cfm.finalize(prior_info=0)
    with ift.random.Context(11):
        pos = 0.3 * ift.from_random(cf.domain, "normal")
    with ift.random.Context(5):
        t = ift.from_random(cf.domain, "normal")
    with ift.random.Context(7):
        g = ift.from_random(cf.target, "normal")
    lin = cf(ift.Linearization.make_var(pos))
    d[f"{tag}_keys"] = np.array(sorted(cf.domain.keys()))
    d[f"{tag}_pos"], d[f"{tag}_t"], d[f"{tag}_g"] = _pack(pos), _pack(t), np.asarray(g.val)
    d[f"{tag}_val"] = np.asarray(lin.val.val)
    d[f"{tag}_jt"] = np.asarray(lin.jac(t).val)
    d[f"{tag}_ja"] = _pack(lin.jac.adjoint(g))
    for i, na in enumerate(cfm.get_normalized_amplitudes()):
        d[f"{tag}_na{i}"] = np.asarray(na.force(pos).val)
    if tag not in METRIC_CASES:
        return
    p = ift.sigmoid(cf)
    ift.random.push_sseq_from_seed(27)
    data = p(pos).val + 0.1 * ift.random.current_rng().standard_normal(cf.target.shape)
    ift.random.pop_sseq()
    d[f"{tag}_data"] = data
    N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
    lh = ift.GaussianEnergy(ift.makeField(cf.target, data), inverse_covariance=N.inverse) @ p
    met = lh.get_metric_at(pos)
    d[f"{tag}_mt"] = _pack(met(t))
    A = met + ift.ScalingOperator(cf.domain, 1.)
    its = _iterates(A, t)
    for i, x in enumerate(its, 1):
        d[f"{tag}_cg{i}"] = _pack(x)
    # conditioning of the iterates under a rounding-level change of the RHS
    rng = np.random.default_rng(3)
    tp = ift.MultiField.from_dict({k: ift.makeField(t[k].domain,
                                                    t[k].val * (1. + 1e-15 * rng.standard_normal(t[k].shape)))
                                   for k in t.keys()})
    worst = 0.
    for x, y in zip(its, _iterates(A, tp)):
        for k in x.keys():
            worst = max(worst, np.linalg.norm(y[k].val - x[k].val) / np.linalg.norm(x[k].val))
    print(f"{tag}: iterates move by {worst:.2e} under a 1e-15 perturbation of the right-hand side")
    assert worst < COND_BOUND, (tag, worst)
    d[f"{tag}_cond"] = np.array(worst)
    if tag not in GEO_CASES:
        return
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    d[f"{tag}_geo_value"] = np.array(kl.value)
    d[f"{tag}_geo_samples"] = np.stack([_pack(s) for s in kl.samples.iterator()])


def main():
    d = {"cases": np.array(list(CASES)), "metric_cases": np.array(METRIC_CASES), "geo_cases": np.array(GEO_CASES)}
    for tag, (s1, s2) in CASES.items():
        d[f"{tag}_shape1"], d[f"{tag}_shape2"] = np.array(s1[0]), np.array(s2[0])
        d[f"{tag}_dist"] = np.array([s1[1], s2[1]])
        case(tag, d)
    path = os.path.join(OUT, "product.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"product.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
