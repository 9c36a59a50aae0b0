"""Generate tests/golden/likelihoods.npz: BernoulliEnergy, StudentTEnergy and
InverseGammaEnergy evaluated by the reference (NIFTy 8.5) on a
SimpleCorrelatedField.

Like gen_golden_sampling.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Grids: l8 = 8 x 8 (the smallest grid on which the carried CG iteration runs)
and l16 = 16 x 16.  Cases (CF_ARGS of the sampling fixture):
  b   BernoulliEnergy(d) @ sigmoid(cf)
  t   StudentTEnergy(sp, 3.) @ Adder(d, neg=True) @ sigmoid(cf)
  tf  the same with a Field theta (uniform in [2, 6])
  g   InverseGammaEnergy(beta, 0.7) @ exp(cf)
  j   b + GaussianEnergy(data, 1 / 1e-2) @ cf  as lh1 + lh2
  bs  b.scale(0.3)

The latent point is SCALE * from_random (seed 11; 0.5 on the 8 x 8 grid, 0.3
on the 16 x 16 one), at which sigmoid(cf) stays inside [0.05, 0.95]
(asserted).  Per case: the energy, the transformation's
value, get_metric_at applied to a fixed vector and, on the 8 x 8 grid, CG
iterates 1..5 of (metric + 1) and one mirrored geoVI draw.

Usage:  python tests/golden/gen_golden_likelihoods.py
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
NAMES = ("events", "field")
CASES = ("b", "t", "tf", "g", "j", "bs")
SCALE = {8: 0.5, 16: 0.3}    # of the latent draw: keeps sigmoid(cf) inside [0.05, 0.95]


def _pack(mf):
    """a MultiField as one vector: its keys in sorted order, each raveled"""
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def problem(n):
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    with ift.random.Context(11):
        pos = SCALE[n] * ift.from_random(cf.domain, "normal")
    p = ift.sigmoid(cf)
    pv = p(pos).val
    assert 0.05 <= pv.min() and pv.max() <= 0.95, (pv.min(), pv.max())
    ift.random.push_sseq_from_seed(27)
    rng = ift.random.current_rng()
    events = (rng.random((n, n)) < pv).astype(np.int64)
    tdata = pv + 0.1 * rng.standard_t(3., (n, n))
    theta = 2. + 4. * rng.random((n, n))
    beta = 0.5 * rng.standard_normal((n, n)) ** 2 + 0.05
    gdata = cf(pos).val + 0.1 * rng.standard_normal((n, n))
    ift.random.pop_sseq()
    d = {"pos": _pack(pos), "events": events, "tdata": tdata, "theta": theta, "beta": beta, "gdata": gdata}
    td = ift.makeField(sp, tdata)
    b = ift.BernoulliEnergy(ift.makeField(sp, events)) @ p
    t = ift.StudentTEnergy(sp, 3.) @ ift.Adder(td, neg=True) @ p
    tf = ift.StudentTEnergy(sp, ift.makeField(sp, theta)) @ ift.Adder(td, neg=True) @ p
    g = ift.InverseGammaEnergy(ift.makeField(sp, beta), 0.7) @ cf.exp()
    N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
    b2 = ift.BernoulliEnergy(ift.makeField(sp, events)) @ p
    ga = ift.GaussianEnergy(ift.makeField(sp, gdata), inverse_covariance=N.inverse) @ cf
    b2.name, ga.name = NAMES
    lhs = dict(b=b, t=t, tf=tf, g=g, j=b2 + ga, bs=b.scale(0.3))
    return cf, lhs, pos, d


def tr_vec(f_lh, pos):
    r = f_lh(pos)
    return _pack(r) if isinstance(r, ift.MultiField) else np.asarray(r.val)


def case(tag, n, d):
    cf, lhs, pos, dd = problem(n)
    d.update({f"{tag}_{k}": v for k, v in dd.items()})
    with ift.random.Context(5):
        t = ift.from_random(cf.domain, "normal")
    d[f"{tag}_t"] = _pack(t)
    for c in CASES:
        lh = lhs[c]
        pre = f"{tag}{c}"
        d[f"{pre}_energy"] = np.array(lh(pos).val)
        dtype, f_lh = lh.get_transformation()
        d[f"{pre}_tr"] = tr_vec(f_lh, pos)
        met = lh.get_metric_at(pos)
        d[f"{pre}_mt"] = _pack(met(t))
        if n != 8:
            continue
        A = met + ift.ScalingOperator(cf.domain, 1.)
        for it in range(1, 6):
            ic = ift.GradientNormController(iteration_limit=it)
            e, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0. * t, A, t))
            d[f"{pre}_cg{it}"] = _pack(e.position)
        H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
        mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
        ift.random.push_sseq_from_seed(27)
        kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
        ift.random.pop_sseq()
        d[f"{pre}_geo_value"] = np.array(kl.value)
        d[f"{pre}_geo_samples"] = np.stack([_pack(s) for s in kl.samples.iterator()])


def main():
    d = {"names": np.array(NAMES), "cases": np.array(CASES), "carry_grid": np.array([8, 8])}
    case("l8", 8, d)
    case("l16", 16, d)
    path = os.path.join(OUT, "likelihoods.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"likelihoods.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
