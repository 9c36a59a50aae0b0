"""Generate tests/golden/joint.npz: joint likelihoods (lh1 + lh2) evaluated by
the reference (NIFTy 8.5).

Like gen_golden.py this script runs in the build container only, imports the
reference from there and writes nothing but data; the same NumPy shim applies
(``np.asfarray``, removed in NumPy 2, is still called by the reference).

Cases (a correlated field seen through lines of sight with Gaussian noise,
plus Poisson counts of exp(field) on the full grid):
  j32  32 x 32, 40 lines of sight
  j8    8 x  8, 12 lines of sight -- the smallest 2-D grid on which the carried
       CG iteration runs (nft_hartley_cg_blocks > 0; recorded as carry_grid)

Usage:  python tests/golden/gen_golden_joint.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
NAMES = ("los", "counts")


def _flat(mf):
    return {k: np.asarray(mf[k].val) for k in sorted(mf.keys())}


def problem(n, nlos, seed=27):
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    ift.random.push_sseq_from_seed(seed)
    rng = ift.random.current_rng()
    starts = rng.random((nlos, 2)).T
    ends = rng.random((nlos, 2)).T
    R = ift.LOSResponse(sp, starts=list(starts), ends=list(ends))
    sr = R(ift.sigmoid(cf))
    lam = cf.exp()
    N = ift.ScalingOperator(R.target, 1e-3, np.float64)
    mock = ift.from_random(cf.domain, "normal")
    data = sr(mock) + N.draw_sample()
    counts = rng.poisson(lam(mock).val).astype(np.int64)
    pos = 0.1 * ift.from_random(cf.domain, "normal")
    ift.random.pop_sseq()
    lh1 = ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ sr
    lh2 = ift.PoissonianEnergy(ift.makeField(sp, counts)) @ lam
    lh1.name, lh2.name = NAMES
    d = {"starts": starts, "ends": ends, "data": data.val, "counts": counts}
    for k, v in _flat(pos).items():
        d["pos_" + k] = v
    return cf, lh1, lh2, pos, d


def case(tag, n, nlos, d):
    cf, lh1, lh2, pos, dd = problem(n, nlos)
    d.update({f"{tag}_{k}": v for k, v in dd.items()})
    lh = lh1 + lh2
    dtype, f_lh = lh.get_transformation()
    d[f"{tag}_trkeys"] = np.array(sorted(f_lh.target.keys()))
    d[f"{tag}_trdtypes"] = np.array([np.dtype(dtype[k]).name for k in sorted(f_lh.target.keys())])
    for k, v in _flat(f_lh(pos)).items():
        d[f"{tag}_tr_" + k] = v
    for k, v in _flat(lh.normalized_residual(pos)).items():
        d[f"{tag}_nres_" + k] = v
    d[f"{tag}_energy"] = np.array(lh(pos).val)
    with ift.random.Context(5):
        t = ift.from_random(cf.domain, "normal")
    for k, v in _flat(t).items():
        d[f"{tag}_t_" + k] = v
    for k, v in _flat(lh.get_metric_at(pos)(t)).items():
        d[f"{tag}_mt_" + k] = v
    # MGVI SampledKLEnergy as in kl32_constants: one mirrored pair, 6 CG steps
    H = ift.StandardHamiltonian(lh, ift.GradientNormController(iteration_limit=6))
    ift.random.push_sseq_from_seed(41)
    kl = ift.SampledKLEnergy(pos, H, 1, None, True)
    ift.random.pop_sseq()
    d[f"{tag}_kl_value"] = np.array(kl.value)
    for k, v in _flat(kl.gradient).items():
        d[f"{tag}_kl_grad_" + k] = v
    return lh, pos


def main():
    d = {"names": np.array(NAMES), "carry_grid": np.array([8, 8])}
    lh, pos = case("j32", 32, 40, d)
    case("j8", 8, 12, d)
    # end to end: geoVI, two mirrored pairs, controllers that stop on their
    # (tiny) iteration limits
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 2, mini, True)
    ift.random.pop_sseq()
    d["geo_value"] = np.array(kl.value)
    for i, s in enumerate(kl.samples.iterator()):
        for k, v in _flat(s).items():
            d[f"geo_s{i}_" + k] = v
    d["geo_nsamples"] = np.array(kl.samples.n_samples)
    np.savez_compressed(os.path.join(OUT, "joint.npz"), **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"joint.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw")


if __name__ == "__main__":
    main()
