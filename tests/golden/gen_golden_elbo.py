"""Generate tests/golden/elbo.npz: estimate_evidence_lower_bound of the
reference (NIFTy 8.5, src/evidence_lower_bound.py) on four small models.

Like gen_golden_sampling.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Cases (SimpleCorrelatedField with CF_ARGS of the sampling fixture):
  a  16^2, MaskOperator leaving 24 pixels, Gaussian noise 1e-3;
     n_eigenvalues = 24 = the relevant degrees of freedom: the exact branch
  b  the model of a, n_eigenvalues = 16 in 4 batches: once with the default
     min_lh_eval ("b"), once with a min_lh_eval between the 4th and the 8th
     eigenvalue's distance from 1, so that the reference stops after the
     second batch ("b2")
  c  32^2, sigmoid, LOSResponse with 20 lines, Gaussian noise 1e-3;
     12 eigenvalues in 3 batches
  d  16^2, exp, Poisson counts on the grid; 20 eigenvalues in 2 batches

Stored per case: the latent mean (pos_<key>), the residuals (res<i>_<key>) and
their signs, the data, the parameters, the reference's _eigsh eigenvalues,
elbo_samples, the stats entries and tr_log = -0.5 sum log lambda, the dense
numpy.linalg.eigvalsh spectrum of the explicit metric (the top `ndense`), and
two discrepancies relative to lambda_max: ARPACK against dense (disc_arpack)
and LAPACK's evd against its evr driver on the explicit metric (disc_dense).
`tol` = 10 x the larger of the two is the tolerance the tests use.

The script asserts that the wanted eigenvalues of every batch are separated
from the next one by more than `tol` * lambda_max: a near-degenerate pair at
a batch boundary would let two correct solvers disagree on which copy a batch
returns.  Change SEEDS until the reference alone satisfies this.

Usage:  python tests/golden/gen_golden_elbo.py
"""
import os
import sys

import numpy as np
import scipy.linalg as slg

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402
from nifty8 import evidence_lower_bound as ref  # noqa: E402


class _Ssl:
    """scipy.sparse.linalg as the reference uses it, the LinearOperator with
    an explicit float64 dtype: this SciPy probes a dtype-less operator with an
    int8 vector, which the reference's _DomRemover rejects"""
    eigsh = staticmethod(ref.ssl.eigsh)

    @staticmethod
    def LinearOperator(shape, matvec, **kw):
        kw.setdefault("dtype", np.float64)
        return _ssl.LinearOperator(shape, matvec, **kw)


_ssl = ref.ssl
ref.ssl = _Ssl

OUT = os.path.dirname(os.path.abspath(__file__))
CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
SEEDS = {"a": 41, "c": 43, "d": 44}
NSAMP = 2          # residuals; each enters with both signs


def model(kind, seed):
    """(cf domain, likelihood, pos, data dict)"""
    n = 32 if kind == "c" else 16
    sp = ift.RGSpace((n, n))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    ift.random.push_sseq_from_seed(seed)
    rng = ift.random.current_rng()
    d = {}
    if kind == "a":
        flags = np.ones(n * n, dtype=bool)
        flags[rng.choice(n * n, 24, replace=False)] = False
        flags = flags.reshape(n, n)
        M = ift.MaskOperator(ift.makeField(sp, flags))
        sr = M(cf)
        d["flags"] = flags
    elif kind == "c":
        starts, ends = rng.random((20, 2)).T, rng.random((20, 2)).T
        R = ift.LOSResponse(sp, starts=list(starts), ends=list(ends))
        sr = R(ift.sigmoid(cf))
        d["starts"], d["ends"] = starts, ends
    else:
        sr = cf.exp()
    mock = ift.from_random(cf.domain, "normal")
    if kind == "d":
        counts = rng.poisson(sr(mock).val).astype(np.int64)
        lh = ift.PoissonianEnergy(ift.makeField(sr.target, counts)) @ sr
        d["data"] = counts
    else:
        N = ift.ScalingOperator(sr.target, 1e-3, np.float64)
        data = sr(mock) + N.draw_sample()
        lh = ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ sr
        d["data"] = data.val
    pos = 0.1 * ift.from_random(cf.domain, "normal")
    res = [0.05 * ift.from_random(cf.domain, "normal") for _ in range(NSAMP)]
    ift.random.pop_sseq()
    return cf, lh, pos, res, d


def dense_metric(H, pos):
    metric = H(ift.Linearization.make_var(pos, want_metric=True)).metric
    metric = ift.SandwichOperator.make(ref._DomRemover(metric.domain).adjoint, metric)
    size = metric.domain.size
    M = ref.ssl.LinearOperator(shape=2 * (size,), matvec=lambda x: metric(ift.makeField(metric.domain, x)).val)
    A = ref._explicify(M)
    return 0.5 * (A + A.T)


def run(tag, d, H, samples, A, n_eig, batch_number, min_lh_eval, ndofs):
    kw = {} if min_lh_eval is None else {"min_lh_eval": min_lh_eval}
    metric = H(ift.Linearization.make_var(samples._m, want_metric=True)).metric
    ev, _ = ref._eigsh(metric, n_eig, tot_dofs=ndofs, min_lh_eval=1e-3 if min_lh_eval is None else min_lh_eval,
                       batch_number=batch_number, tol=0., verbose=False)
    elbo, stats = ift.estimate_evidence_lower_bound(H, samples, n_eig, batch_number=batch_number, verbose=False, **kw)
    dense = np.linalg.eigvalsh(A)[::-1]
    lmax = dense[0]
    d[f"{tag}_n_eigenvalues"] = np.array(n_eig)
    d[f"{tag}_batch_number"] = np.array(batch_number)
    d[f"{tag}_min_lh_eval"] = np.array(1e-3 if min_lh_eval is None else min_lh_eval)
    d[f"{tag}_eigenvalues"] = ev
    d[f"{tag}_count"] = np.array(ev.size)
    d[f"{tag}_elbo_samples"] = np.array([float(s.val) for s in elbo.iterator()])
    for k, v in stats.items():
        d[f"{tag}_{k}"] = np.array(float(v.val))
    d[f"{tag}_tr_log"] = np.array(-0.5 * np.sum(np.log(ev)))
    return float(np.abs(ev - dense[:ev.size]).max() / lmax)


def separated(dense, n_eig, batch_number, tol):
    """every batch boundary of the wanted eigenvalues (and their end) is a
    gap of more than tol * lambda_max"""
    size = n_eig // batch_number
    ends = [size * (i + 1) for i in range(batch_number - 1)] + [n_eig]
    return all(dense[e - 1] - dense[e] > tol * dense[0] for e in ends if e < dense.size)


def case(kind, d):
    cf, lh, pos, res, dd = model(kind, SEEDS[kind])
    d.update({f"{kind}_{k}": v for k, v in dd.items()})
    d[f"{kind}_seed"] = np.array(SEEDS[kind])
    for k in pos.keys():
        d[f"{kind}_pos_{k}"] = pos[k].val
        for i, r in enumerate(res):
            d[f"{kind}_res{i}_{k}"] = r[k].val
    residuals = [r for r in res for _ in range(2)]
    neg = [False, True] * len(res)
    d[f"{kind}_neg"] = np.array(neg)
    samples = ift.ResidualSampleList(pos, residuals, neg)
    H = ift.StandardHamiltonian(lh)
    A = dense_metric(H, pos)
    dense = np.linalg.eigvalsh(A)[::-1]
    ndofs = min(lh.data_domain.size, H.domain.size)
    nd = min(ndofs + 4, dense.size)
    d[f"{kind}_dense"] = dense[:nd]
    d[f"{kind}_ndofs"] = np.array(ndofs)
    d[f"{kind}_metric_size"] = np.array(A.shape[0])
    evd = slg.eigh(A, eigvals_only=True, driver="evd")[::-1]
    evr = slg.eigh(A, eigvals_only=True, driver="evr")[::-1]
    disc_dense = float(np.abs(evd - evr)[:nd].max() / dense[0])
    if kind == "a":
        runs = [("a", 24, 10, None), ("b", 16, 4, None),
                ("b2", 16, 4, float(np.sqrt((dense[3] - 1.) * (dense[7] - 1.))))]
    elif kind == "c":
        runs = [("c", 12, 3, None)]
    else:
        runs = [("d", 20, 2, None)]
    disc_arpack = 0.0
    for tag, n_eig, nb, mle in runs:
        disc = run(tag, d, H, samples, A, n_eig, nb, mle, ndofs)
        if n_eig != ndofs:
            disc_arpack = max(disc_arpack, disc)
    tol = 10 * max(disc_arpack, disc_dense)
    d[f"{kind}_disc_arpack"] = np.array(disc_arpack)
    d[f"{kind}_disc_dense"] = np.array(disc_dense)
    d[f"{kind}_tol"] = np.array(tol)
    for tag, n_eig, nb, mle in runs:
        assert separated(dense, n_eig, nb, tol), (tag, "wanted eigenvalues not separated: change the seed")
    if kind == "a":
        assert d["b2_count"] == 8 and d["b_count"] in (4, 8, 12, 16), (d["b2_count"], d["b_count"])
    print(kind, "lambda_max %.4e" % dense[0], "disc_arpack %.2e disc_dense %.2e" % (disc_arpack, disc_dense),
          {t[0]: int(d[t[0] + "_count"]) for t in runs})


def main():
    d = {"nsamp": np.array(NSAMP)}
    for kind in ("a", "c", "d"):
        case(kind, d)
    path = os.path.join(OUT, "elbo.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"elbo.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
