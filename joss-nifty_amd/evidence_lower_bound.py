"""Evidence lower bound (src/evidence_lower_bound.py:107-253) from the
spectrum of the posterior metric M = 1 + J^T W J at the latent mean.

The reference asks ARPACK on the host for the largest eigenvalues, one matvec
at a time, and projects found eigenvectors out through a _Projector.  Here a
block Lanczos (minimization/block_lanczos.py) runs on the device: the matvec
is the fused metric on packed (k, n) buffers, up to 8 vectors per set of
launches, the orthogonalisation is native (csrc/nft_eig.hip), and found
eigenvectors join the locked set of that orthogonalisation.  Lanczos runs on
L = J^T W J (shift 0) and the identity's 1 is added afterwards, so the
eigenvalues near 1 -- the ones the stopping rule looks at -- keep their
relative accuracy in lambda - 1.
"""
import functools

import numpy as np
import torch

from .field import Field
from .linearization import Linearization
from .logger import logger
from .minimization.block_lanczos import NativeOps, largest_eigenpairs
from .minimization.sample_list import ResidualSampleList, SampleList
from .operators.energy_operators import StandardHamiltonian
from .operators.sampling_enabler import SamplingEnabler
from .operators.scaling_operator import ScalingOperator
from .operators.sum_operator import SumOperator
from .packing import PackedLayout
from ._native import GRAM_KMAX as MAX_BATCH    # vectors per batched matvec and per Gram call


def split_metric(metric):
    """(L, shift) with metric = L + shift * 1: a SamplingEnabler (Hamiltonian
    built with ic_samp) is unwrapped to likelihood metric + prior first."""
    if isinstance(metric, SamplingEnabler):
        metric = metric._likelihood + metric._prior
    if not isinstance(metric, SumOperator):
        return metric, 0.0
    rest, shift = [], 0.0
    for op, neg in zip(metric._ops, metric._neg):
        if isinstance(op, ScalingOperator) and complex(op._factor).imag == 0:
            shift += (-1 if neg else 1) * complex(op._factor).real
        elif neg:
            return metric, 0.0
        else:
            rest.append(op)
    if not rest:
        raise ValueError("the metric has no likelihood part")
    return functools.reduce(lambda a, b: a + b, rest), shift


class MetricMatvec:
    """Y[b] = L X[b] on packed (k, n) device rows, k <= 8.

    Fused (`fused` True): fusable_metric(L) gives (core, W, 0) and the rows go
    through core.metric_flat_batch in one set of launches; a core with a frame
    of its own (product spectra) is iterated in that frame -- its R is
    orthogonal, so the eigenvalues are those of the natural frame -- and
    `natural` maps eigenvector rows back.  Generic: any other operator is
    applied per vector on device fields."""

    def __init__(self, L, force_generic=False):
        from .minimization.fused_cg import batch_supported, fusable_metric
        self.L = L
        spec = None if force_generic else fusable_metric(L)
        self.fused = bool(spec is not None and batch_supported(spec[0], spec[1])
                          and spec[0].device.type == "cuda" and spec[0].domain == L.domain)
        if self.fused:
            self.core, self.W = spec[0], spec[1]
            self.layout = self.core.layout
        else:
            self.core = None
            self.layout = PackedLayout(L.domain)
        self.n = self.layout.size
        self.calls = 0
        mask = np.zeros(self.n)
        for o, s in zip(self.layout.offsets, self.layout.sizes):
            mask[o:o + s] = 1.0
        self.support = mask

    def __call__(self, X, Y):
        self.calls += 1
        if self.fused:
            self.core.metric_flat_batch(X, Y, self.W, 0.0)
            return
        for b in range(X.shape[0]):
            self.layout.pack(self.L(self.layout.unpack(X[b])), out=Y[b])

    def natural(self, rows):
        """eigenvector rows in the natural frame (a copy where the core has a frame)"""
        f = None if self.core is None else getattr(self.core, "from_frame", None)
        return rows if f is None else f(rows.clone())

    def explicit(self):
        """L as a host (n, n) matrix on the packed layout: identity blocks of
        8 rows through the batched matvec"""
        n, dev = self.n, self.layout.device
        out = np.empty((n, n))
        X = torch.zeros((MAX_BATCH, n), dtype=torch.float64, device=dev)
        Y = torch.zeros_like(X)
        idx = np.flatnonzero(self.support)
        out[:] = 0.0
        for a in range(0, idx.size, MAX_BATCH):
            rows = idx[a:a + MAX_BATCH]
            k = rows.size
            X.zero_()
            X[torch.arange(k, device=dev), torch.from_numpy(rows).to(dev)] = 1.0
            self(X[:k], Y[:k])
            out[rows] = Y[:k].cpu().numpy()
        return 0.5 * (out + out.T)


def batch_sizes(n_eigenvalues, batch_number):
    """the reference's batches (evidence_lower_bound.py:85-87)"""
    size = n_eigenvalues // batch_number
    return [size] * (batch_number - 1) + [n_eigenvalues - size * (batch_number - 1)]


def metric_spectrum(matvec, shift, n_eigenvalues, tot_dofs, min_lh_eval=1e-4, batch_number=10, tol=0., verbose=True,
                    solver=None):
    """The largest eigenvalues of shift + L, descending, as the reference's
    _eigsh returns them (evidence_lower_bound.py:67-104): all `tot_dofs` from
    the explicit matrix when n_eigenvalues == tot_dofs, else in batches with
    the early stop |1 - min| < min_lh_eval, found eigenvectors locked.
    matvec: a MetricMatvec (or anything with n, support, explicit()).
    solver(nev, locked) -> EigResult overrides the device solver (tests)."""
    if n_eigenvalues > tot_dofs:
        raise ValueError("Number of requested eigenvalues exceeds the number of relevant degrees of freedom!")
    if tot_dofs == n_eigenvalues:
        if verbose:
            logger.info(f"Computing all {tot_dofs} relevant metric eigenvalues.")
        ev = np.linalg.eigvalsh(matvec.explicit())
        return shift + ev[::-1][:tot_dofs]
    if solver is None:
        ops = NativeOps(matvec.layout.device)
        store = ops.zeros(n_eigenvalues, matvec.n)

        def solver(nev, nlocked):
            res = largest_eigenpairs(matvec, ops, matvec.n, nev, tol=tol, locked=store[:nlocked] if nlocked else None,
                                     support=matvec.support)
            store[nlocked:nlocked + len(res.values)] = res.vectors
            return res
    eigenvalues = np.zeros(0)
    for batch in batch_sizes(n_eigenvalues, batch_number):
        if batch < 1:
            continue
        if verbose:
            logger.info(f"\nNumber of eigenvalues being computed: {batch}")
        res = solver(batch, eigenvalues.size)
        eigenvalues = np.concatenate((eigenvalues, shift + np.asarray(res.values)))
        if abs(1.0 - np.min(eigenvalues)) < min_lh_eval:
            break
    return eigenvalues


def elbo_statistics(eigenvalues, n_relevant_dofs, metric_size):
    """(posterior contribution, lower error) of the reference
    (evidence_lower_bound.py:236-240) as floats"""
    log_eigenvalues = np.log(eigenvalues)
    tr_log_lat_cov = - 0.5 * np.sum(log_eigenvalues)
    tr_log_lat_cov_lower = 0.5 * (n_relevant_dofs - log_eigenvalues.size) * np.min(log_eigenvalues)
    return float(tr_log_lat_cov + 0.5 * metric_size), float(tr_log_lat_cov_lower)


def _sample_stat(sl):
    """mean and variance over a (possibly distributed) SampleList of scalars:
    the reference's StatCalculator on one rank, the list's all-reduce (with
    the same n - 1 normalisation) on several"""
    from .probing import StatCalculator
    n = sl.n_samples
    if n == 1:
        res = sl.average()
        return res, 0 * res
    if sl.comm is None or sl.comm.Get_size() == 1:
        sc = StatCalculator()
        for s in sl.local_iterator():
            sc.add(s)
        return sc.mean, sc.var
    mean, var = sl.sample_stat()
    return mean, var * (n / (n - 1.))


def shared_spectrum(eigenvalues, comm):
    """rank 0's eigenvalues on every rank.  Each rank solves the same
    eigenproblem, but from the start vectors of its own generator, so the
    results agree to round-off only; the posterior contribution that enters
    the all-reduced statistics must be one number."""
    if comm is None or comm.Get_size() == 1:
        return eigenvalues
    return np.asarray(comm.bcast(eigenvalues, root=0), dtype=np.float64)


def elbo_with_spectrum(hamiltonian, samples, n_eigenvalues, min_lh_eval=1e-3, batch_number=10, tol=0.,
                       verbose=True):
    """estimate_evidence_lower_bound plus what it was computed from: returns
    (elbo_samples, stats, eigenvalues, matvec)."""
    if not isinstance(samples, ResidualSampleList):
        raise TypeError("samples attribute should be of type ResidualSampleList.")
    if not isinstance(hamiltonian, StandardHamiltonian):
        raise TypeError("hamiltonian is not an instance of `ift.StandardHamiltonian`.")

    dd = hamiltonian.likelihood_energy.data_domain
    n_data_points = dd.size if dd is not None else hamiltonian.domain.size
    n_relevant_dofs = min(n_data_points, hamiltonian.domain.size)  # number of metric eigenvalues that are not one

    metric = hamiltonian(Linearization.make_var(samples._m, want_metric=True)).metric
    metric_size = metric.domain.size
    L, shift = split_metric(metric)
    matvec = MetricMatvec(L)
    eigenvalues = metric_spectrum(matvec, shift, n_eigenvalues, n_relevant_dofs, min_lh_eval=min_lh_eval,
                                  batch_number=batch_number, tol=tol, verbose=verbose)
    eigenvalues = shared_spectrum(eigenvalues, samples.comm)
    if verbose:
        logger.info(
            f"\nComputed {eigenvalues.size} largest eigenvalues (out of {n_relevant_dofs} relevant degrees of freedom)."
            f"\nThe remaining {metric_size - n_relevant_dofs} metric eigenvalues (out of {metric_size}) are equal to "
            f"1.\n\n{eigenvalues}.")

    post, lower = elbo_statistics(eigenvalues, n_relevant_dofs, metric_size)
    tr_log_lat_cov_lower = Field.scalar(lower)
    posterior_contribution = Field.scalar(post)
    elbo_samples = SampleList([posterior_contribution - hamiltonian(x) for x in samples.local_iterator()],
                              comm=samples.comm, domain=posterior_contribution.domain)

    stats = {'lower_error': tr_log_lat_cov_lower}
    elbo_mean, elbo_var = _sample_stat(elbo_samples)
    elbo_up = elbo_mean + elbo_var.sqrt()
    elbo_lw = elbo_mean - elbo_var.sqrt() - stats["lower_error"]
    stats['elbo_mean'], stats['elbo_up'], stats['elbo_lw'] = elbo_mean, elbo_up, elbo_lw
    if verbose:
        s = (f"\nELBO decomposition (in log units)"
             f"\nELBO mean : {float(elbo_mean.val):.4e} (upper: {float(elbo_up.val):.4e}, "
             f"lower: {float(elbo_lw.val):.4e})")
        logger.info(s)
    return elbo_samples, stats, eigenvalues, matvec


def estimate_evidence_lower_bound(hamiltonian, samples, n_eigenvalues, min_lh_eval=1e-3, batch_number=10, tol=0.,
                                  verbose=True):
    """Estimate of the evidence lower bound
        log p(d) >= -<H(xi, d)> + (N + Tr log Lambda) / 2
    with the reference's semantics (evidence_lower_bound.py:107-253).

    hamiltonian : StandardHamiltonian
    samples : ResidualSampleList (may be distributed: every rank solves the
        eigenproblem, rank 0's eigenvalues are used on all, the ELBO samples
        come from the rank's local samples)
    n_eigenvalues : int, at most min(data size, latent size); equal to it, all
        relevant eigenvalues come from the explicit metric
    min_lh_eval : float, the batches stop once |1 - min eigenvalue| is below it
    batch_number : int, number of batches the eigenvalues are computed in
    tol : float, eigenvalue tolerance (0: machine precision)

    Returns (elbo_samples : SampleList, stats : dict with elbo_mean, elbo_up,
    elbo_lw, lower_error)."""
    return elbo_with_spectrum(hamiltonian, samples, n_eigenvalues, min_lh_eval, batch_number, tol, verbose)[:2]
