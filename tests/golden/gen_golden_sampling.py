"""Generate tests/golden/sampling.npz: MaskOperator and LinearInterpolator
evaluated by the reference (NIFTy 8.5), alone and inside likelihoods.

Like gen_golden_joint.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Operator cases (grids g1 = (16,) with distance 0.5, g2 = (8, 6) with
distances (0.5, 0.25), g3 = (4, 6, 8) with the default distances): 1000
points whose first 37 hold the special ones (a negative position, one beyond
the extent, points on nodes, a point in the last cell, two identical points),
followed by 300 points in one cell and random ones; the tests use the first 1,
37 and 1000.  The COO triplets are those of the 1000-point operator (the
entries of the first n points are its rows < n).  Masks: random, nothing
flagged, one pixel kept.

Likelihood cases on a SimpleCorrelatedField (CF_ARGS of the joint fixture),
8 x 8 (the smallest grid on which the carried CG iteration runs) and 16 x 16:
  a  sigmoid -> LinearInterpolator (40 points) -> Gaussian 1e-3
  b  exp -> MaskOperator -> Poisson
  c  a + b as lh1 + lh2

Usage:  python tests/golden/gen_golden_sampling.py
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
NAMES = ("points", "counts")
GRIDS = (("g1", (16,), (0.5,)), ("g2", (8, 6), (0.5, 0.25)), ("g3", (4, 6, 8), None))
NPOINTS = (1, 37, 1000)


def _pack(mf):
    """a MultiField as one vector: its keys in sorted order, each raveled
    (few arrays keep the archive small)"""
    return np.concatenate([np.asarray(mf[k].val).reshape(-1) for k in sorted(mf.keys())])


def points(shape, dist, rng):
    nd = len(shape)
    ext = np.array(shape) * np.array(dist)
    d = np.array(dist)
    p = np.empty((nd, 1000))
    p[:, 0] = -0.37 * ext                     # negative
    p[:, 1] = 1.6 * ext                       # beyond the extent
    p[:, 2] = 3 * d                           # on a node
    p[:, 3] = 0.                              # on node 0
    p[:, 4] = (np.array(shape) - 0.5) * d     # last cell: wraps to index 0
    p[:, 5] = p[:, 6] = rng.random(nd) * ext  # two identical points
    p[:, 7:37] = (rng.random((nd, 30)) * 2 - 0.5) * ext[:, None]
    p[:, 37:337] = (1 + rng.random((nd, 300))) * d[:, None]   # 300 points in cell (1, 1, 1)
    p[:, 337:] = rng.random((nd, 663)) * ext[:, None]
    return p


def operators(d):
    rng = np.random.default_rng(11)
    for tag, shape, dist in GRIDS:
        sp = ift.RGSpace(shape, distances=dist)
        pts = points(shape, sp.distances, rng)
        x = rng.standard_normal(shape)
        y = rng.standard_normal(1000)
        d[f"{tag}_shape"] = np.array(shape)
        d[f"{tag}_dist"] = np.array(sp.distances)
        d[f"{tag}_pts"], d[f"{tag}_x"], d[f"{tag}_y"] = pts, x, y
        for n in NPOINTS:
            R = ift.LinearInterpolator(sp, pts[:, :n].copy())
            if n == 1000:
                coo = R._mat.A.tocoo()
                d[f"{tag}_row"] = coo.row.astype(np.int32)
                d[f"{tag}_col"] = coo.col.astype(np.int32)
                d[f"{tag}_data"] = coo.data
                d[f"{tag}_Rx"] = R(ift.makeField(sp, x)).val
            d[f"{tag}_Rty{n}"] = R.adjoint_times(ift.makeField(R.target, y[:n].copy())).val
        npix = int(np.prod(shape))
        one = np.ones(shape, dtype=bool)
        one.reshape(-1)[npix // 3] = False
        for mtag, flags in (("rand", rng.random(shape) < 0.5), ("none", np.zeros(shape, dtype=bool)), ("one", one)):
            M = ift.MaskOperator(ift.makeField(sp, flags))
            ym = rng.standard_normal(M.target.shape)
            d[f"{tag}_m{mtag}_flags"] = flags
            d[f"{tag}_m{mtag}_y"] = ym
            d[f"{tag}_m{mtag}_Mx"] = M(ift.makeField(sp, x)).val
            d[f"{tag}_m{mtag}_Mty"] = M.adjoint_times(ift.makeField(M.target, ym)).val


def problem(n, seed=27):
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    ift.random.push_sseq_from_seed(seed)
    rng = ift.random.current_rng()
    pts = rng.random((2, 40)) * 1.4 - 0.2       # some outside [0, 1): they wrap
    flags = rng.random((n, n)) < 0.5
    R = ift.LinearInterpolator(sp, pts)
    M = ift.MaskOperator(ift.makeField(sp, flags))
    sr = R(ift.sigmoid(cf))
    lam = M(cf.exp())
    N = ift.ScalingOperator(R.target, 1e-3, np.float64)
    mock = ift.from_random(cf.domain, "normal")
    data = sr(mock) + N.draw_sample()
    counts = rng.poisson(lam(mock).val).astype(np.int64)
    pos = 0.1 * ift.from_random(cf.domain, "normal")
    ift.random.pop_sseq()
    lh1 = ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ sr
    lh2 = ift.PoissonianEnergy(ift.makeField(M.target, counts)) @ lam
    lh1.name, lh2.name = NAMES
    d = {"pts": pts, "flags": flags, "data": data.val, "counts": counts, "pos": _pack(pos)}
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
        met = lh.get_metric_at(pos)
        d[f"{pre}_mt"] = _pack(met(t))
        if n != 8:
            continue
        # CG iterates 1..5 of (sampling metric + 1) x = t from x = 0
        A = met + ift.ScalingOperator(cf.domain, 1.)
        for it in range(1, 6):
            ic = ift.GradientNormController(iteration_limit=it)
            e, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0. * t, A, t))
            d[f"{pre}_cg{it}"] = _pack(e.position)
        # one short geoVI draw: one mirrored pair, controllers that stop on
        # their (tiny) iteration limits
        H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
        mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
        ift.random.push_sseq_from_seed(27)
        kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
        ift.random.pop_sseq()
        d[f"{pre}_geo_value"] = np.array(kl.value)
        d[f"{pre}_geo_samples"] = np.stack([_pack(s) for s in kl.samples.iterator()])


def main():
    d = {"names": np.array(NAMES), "carry_grid": np.array([8, 8]), "npoints": np.array(NPOINTS)}
    operators(d)
    case("s8", 8, d)
    case("s16", 16, d)
    path = os.path.join(OUT, "sampling.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"sampling.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
