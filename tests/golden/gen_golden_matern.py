"""Generate tests/golden/matern.npz: correlated fields with ONE Matern
component (CorrelatedFieldMaker.add_fluctuations_matern) evaluated by the
reference (NIFTy 8.5).

Like gen_golden_likelihoods.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Cases (Matern priors of cfm.npz's mat_ case: scale (1, 0.3), cutoff (2, 0.5),
loglogslope (-3, 0.5)):
  m8z   RGSpace((8, 8), 0.1), zero mode (1e-2, 1e-3), offset 1
  m8    the same with offset_std = None
  m16   RGSpace(16, 0.3), no zero mode, offset 1
  m3d   RGSpace((6, 8, 4)), zero mode (0.5, 0.2), offset 1

Per case: the latent point (0.3 * from_random, seed 11), a tangent (seed 5), a
cotangent (seed 7), the value, J t, J^T g and cfm.amplitude.  For m8z and m8
with GaussianEnergy(data, 1 / 1e-2) @ sigmoid(cf): get_metric_at applied to the
tangent, CG iterates 1..5 of (metric + 1) and one mirrored geoVI draw
(controllers of gen_golden_likelihoods.py).

Conditioning: the CG iterates are recomputed with the right-hand side
perturbed by 1e-15 (relative, per element); every key of every iterate must
move by less than 1e-12 (relative 2-norm), or the 1e-9 the tests ask of the
iterates would mean nothing.  The measured maximum is stored as <case>_cond.

A MultiField is stored as one vector: its keys in sorted order, each raveled.

Usage:  python tests/golden/gen_golden_matern.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

MATERN = ((1., 0.3), (2., 0.5), (-3., 0.5))
CASES = {
    "m8z": dict(shape=(8, 8), distances=0.1, offset_std=(1e-2, 1e-3)),
    "m8": dict(shape=(8, 8), distances=0.1, offset_std=None),
    "m16": dict(shape=(16,), distances=0.3, offset_std=None),
    "m3d": dict(shape=(6, 8, 4), distances=None, offset_std=(0.5, 0.2)),
}
METRIC_CASES = ("m8z", "m8")
COND_BOUND = 1e-12


def _pack(mf):
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def maker(shape, distances, offset_std):
    sp = ift.RGSpace(shape, distances=distances)
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(sp, *MATERN)
    cfm.set_amplitude_total_offset(1., offset_std)
    return sp, cfm


def _iterates(A, t):
    out = []
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        e, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0. * t, A, t))
        out.append(e.position)
    return out


def case(tag, d):
    cfg = CASES[tag]
    sp, cfm = maker(**cfg)
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
    d[f"{tag}_amp"] = np.asarray(cfm.amplitude.force(pos).val)
    if tag not in METRIC_CASES:
        return
    p = ift.sigmoid(cf)
    ift.random.push_sseq_from_seed(27)
    data = p(pos).val + 0.1 * ift.random.current_rng().standard_normal(sp.shape)
    ift.random.pop_sseq()
    d[f"{tag}_data"] = data
    N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
    lh = ift.GaussianEnergy(ift.makeField(sp, data), inverse_covariance=N.inverse) @ p
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
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    d[f"{tag}_geo_value"] = np.array(kl.value)
    d[f"{tag}_geo_samples"] = np.stack([_pack(s) for s in kl.samples.iterator()])


def main():
    d = {"cases": np.array(list(CASES)), "metric_cases": np.array(METRIC_CASES),
         "matern": np.array(MATERN)}
    for tag in CASES:
        case(tag, d)
    path = os.path.join(OUT, "matern.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"matern.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
