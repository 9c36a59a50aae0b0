"""GPU: estimate_evidence_lower_bound against the reference's values
(tests/golden/elbo.npz, gen_golden_elbo.py) and against closed forms.

Tolerances
----------
Eigenvalues: relative to lambda_max, the fixture's `tol` = 10 x the larger of
its two stored discrepancies (ARPACK against dense LAPACK, LAPACK's evd
against its evr driver): both solvers are backward stable with different
constants, one decade covers that.
Hamiltonian part (elbo_samples + 0.5 sum log lambda - 0.5 n = -H(sample)):
1e-10 relative, the energy tolerance of test_likelihoods_gpu.py.
Both are checked on the one solve the public entry point made (`run`).
A problem that belongs to none of the fixtures (closed form, product spectrum)
gets the tightest of the three fixture tolerances.
Statistics: what follows from those two.  With |d lambda_i| <= tol lambda_max,
|d tr_log| <= 0.5 sum |d lambda_i| / lambda_i =: e_tr; every sample's ELBO
moves by at most e_tr + e_H, e_H = 1e-10 max |H|, and so does the mean; the
standard deviation of n samples moves by at most sqrt(n / (n - 1)) e_H <= 2 e_H
(the shift by tr_log is common to all samples); lower_error = 0.5 (ndofs -
count) log(min lambda) moves by at most e_lo = 0.5 (ndofs - count) tol
lambda_max / min lambda.  Hence elbo_mean: e_tr + e_H, elbo_up: e_tr + 3 e_H,
elbo_lw: e_tr + 3 e_H + e_lo.
"""
import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
KIND = {"a": "a", "b": "a", "b2": "a", "c": "c", "d": "d"}
_MODELS, _RUNS = {}, {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


@pytest.fixture(scope="module")
def G():
    return golden("elbo.npz")


def model(ift, G, kind):
    """(hamiltonian with ic_samp, hamiltonian without, samples) of a fixture model"""
    if kind not in _MODELS:
        n = 32 if kind == "c" else 16
        sp = ift.RGSpace((n, n))
        cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
        if kind == "a":
            sr = ift.MaskOperator(ift.makeField(sp, G["a_flags"]))(cf)
        elif kind == "c":
            R = ift.LOSResponse(sp, starts=list(G["c_starts"]), ends=list(G["c_ends"]))
            sr = R(ift.sigmoid(cf))
        else:
            sr = cf.exp()
        if kind == "d":
            lh = ift.PoissonianEnergy(ift.makeField(sr.target, G["d_data"])) @ sr
        else:
            N = ift.ScalingOperator(sr.target, 1e-3, np.float64)
            lh = ift.GaussianEnergy(ift.makeField(sr.target, G[f"{kind}_data"]), inverse_covariance=N.inverse) @ sr
        dom = cf.domain

        def mf(pre):
            return ift.MultiField.from_dict({k: ift.makeField(dom[k], G[f"{kind}_{pre}_{k}"]) for k in dom.keys()},
                                            dom)
        pos = mf("pos")
        res = [mf(f"res{i}") for i in range(int(G["nsamp"]))]
        neg = [bool(v) for v in G[f"{kind}_neg"]]
        samples = ift.ResidualSampleList(pos, [r for r in res for _ in range(2)], neg)
        H_ic = ift.StandardHamiltonian(lh, ift.GradientNormController(iteration_limit=5))
        _MODELS[kind] = (H_ic, ift.StandardHamiltonian(lh), samples)
    return _MODELS[kind]


def spectrum(ift, G, tag, force_generic=False):
    """the eigenvalues of a fixture run through metric_spectrum with a matvec
    of choice (the generic one for the fused-against-generic tests)"""
    from nifty_amd.evidence_lower_bound import MetricMatvec, metric_spectrum, split_metric
    H_ic, H, samples = model(ift, G, KIND[tag])
    # b runs on the SamplingEnabler-wrapped metric of a Hamiltonian with ic_samp
    ham = H_ic if tag == "b" else H
    metric = ham(ift.Linearization.make_var(samples.mean, want_metric=True)).metric
    if tag == "b":
        assert isinstance(metric, ift.SamplingEnabler)
    L, shift = split_metric(metric)
    assert shift == 1.0
    mv = MetricMatvec(L, force_generic=force_generic)
    ev = metric_spectrum(mv, shift, int(G[f"{tag}_n_eigenvalues"]), int(G[f"{KIND[tag]}_ndofs"]),
                         min_lh_eval=float(G[f"{tag}_min_lh_eval"]), batch_number=int(G[f"{tag}_batch_number"]),
                         verbose=False)
    return ev, mv, L


def run(ift, G, tag):
    """(eigenvalues, matvec, elbo_samples, stats) of ONE solve of a fixture
    run: the public entry point's own eigenvalues (elbo_with_spectrum is
    estimate_evidence_lower_bound plus what it was computed from)"""
    if tag not in _RUNS:
        from nifty_amd.evidence_lower_bound import elbo_with_spectrum
        H_ic, H, samples = model(ift, G, KIND[tag])
        # b runs on the SamplingEnabler-wrapped metric of a Hamiltonian with ic_samp
        ham = H_ic if tag == "b" else H
        if tag == "b":
            metric = ham(ift.Linearization.make_var(samples.mean, want_metric=True)).metric
            assert isinstance(metric, ift.SamplingEnabler)
        with ift.random.Context(17):
            elbo, stats, ev, mv = elbo_with_spectrum(
                ham, samples, int(G[f"{tag}_n_eigenvalues"]), min_lh_eval=float(G[f"{tag}_min_lh_eval"]),
                batch_number=int(G[f"{tag}_batch_number"]), verbose=False)
        _RUNS[tag] = (ev, mv, elbo, stats)
    return _RUNS[tag]


def synthetic_tol(G):
    """a problem that belongs to none of the fixtures gets the tightest of their tolerances"""
    return min(float(G[f"{k}_tol"]) for k in ("a", "c", "d"))


@pytest.mark.parametrize("tag", list(KIND))
def test_golden_eigenvalues(ift, G, tag):
    ev, mv, _, _ = run(ift, G, tag)
    want, tol = G[f"{tag}_eigenvalues"], float(G[f"{KIND[tag]}_tol"])
    assert mv.fused and mv.calls > 0
    assert ev.size == int(G[f"{tag}_count"]) == want.size
    disc = np.abs(ev - want).max() / want[0]
    dense = np.abs(ev - G[f"{KIND[tag]}_dense"][:ev.size]).max() / want[0]
    print(tag, "device solver against ARPACK", disc, "against dense", dense, "fixture tol", tol)
    assert disc <= tol


@pytest.mark.parametrize("tag", list(KIND))
def test_hamiltonian_part_and_statistics(ift, G, tag):
    from nifty_amd.evidence_lower_bound import elbo_statistics
    ev, _, elbo, stats = run(ift, G, tag)
    kind = KIND[tag]
    want_ev, tol = G[f"{tag}_eigenvalues"], float(G[f"{kind}_tol"])
    ndofs, size = int(G[f"{kind}_ndofs"]), int(G[f"{kind}_metric_size"])
    assert isinstance(elbo, ift.SampleList) and elbo.n_samples == G[f"{tag}_elbo_samples"].size
    got = np.array([float(s.val) for s in elbo.local_iterator()])
    # -H(sample): the ELBO samples less the posterior contribution each side used
    mH = got - elbo_statistics(ev, ndofs, size)[0]
    want_mH = G[f"{tag}_elbo_samples"] + 0.5 * np.log(want_ev).sum() - 0.5 * size
    print(tag, "Hamiltonian part", np.abs(mH - want_mH).max() / np.abs(want_mH).max())
    assert np.all(np.abs(mH - want_mH) <= 1e-10 * np.abs(want_mH))
    e_H = 1e-10 * np.abs(want_mH).max()
    e_tr = 0.5 * np.sum(tol * want_ev[0] / want_ev)
    e_lo = 0.5 * (ndofs - want_ev.size) * tol * want_ev[0] / want_ev.min()
    tr_log = -0.5 * np.log(ev).sum()
    assert abs(tr_log - float(G[f"{tag}_tr_log"])) <= e_tr
    assert np.all(np.abs(got - G[f"{tag}_elbo_samples"]) <= e_tr + e_H)
    bounds = dict(elbo_mean=e_tr + e_H, elbo_up=e_tr + 3 * e_H, elbo_lw=e_tr + 3 * e_H + e_lo, lower_error=e_lo)
    assert sorted(stats) == sorted(bounds)
    for key, bound in bounds.items():
        d = abs(float(stats[key].val) - float(G[f"{tag}_{key}"]))
        print(tag, key, d, "bound", bound)
        assert d <= bound, key


def test_type_and_size_errors(ift, G):
    H_ic, H, samples = model(ift, G, "a")
    with pytest.raises(TypeError, match="ResidualSampleList"):
        ift.estimate_evidence_lower_bound(H, ift.SampleList([samples.mean]), 4, verbose=False)
    with pytest.raises(TypeError, match="StandardHamiltonian"):
        ift.estimate_evidence_lower_bound(H.likelihood_energy, samples, 4, verbose=False)
    with pytest.raises(ValueError, match="exceeds the number of relevant degrees of freedom"):
        ift.estimate_evidence_lower_bound(H, samples, 25, verbose=False)


def test_closed_form_masked_gaussian_generic(ift, G):
    """GaussianEnergy(d, N^-1) @ MaskOperator directly on a plain 16^2 latent
    field: the metric is 1 + M^T N^-1 M, its eigenvalues exactly 1 + 1 /
    sigma_i^2 at the 10 observed pixels.  Three equal sigma put a degenerate
    triple across the first batch boundary (1 single + 2 copies | third copy).
    No fused core: the generic per-vector matvec runs."""
    from nifty_amd.evidence_lower_bound import MetricMatvec, metric_spectrum, split_metric
    from nifty_amd.minimization.fused_cg import fusable_metric
    sp = ift.RGSpace((16, 16))
    rng = np.random.default_rng(5)
    flags = np.ones(256, dtype=bool)
    flags[rng.choice(256, 10, replace=False)] = False
    M = ift.MaskOperator(ift.makeField(sp, flags.reshape(16, 16)))
    sig2 = np.array([0.01, 0.02, 0.02, 0.02, 0.05, 0.1, 0.3, 0.7, 1.5, 4.0])
    sig2 = sig2[rng.permutation(10)]
    Ninv = ift.DiagonalOperator(ift.makeField(M.target, 1.0 / sig2))
    lh = ift.GaussianEnergy(ift.makeField(M.target, rng.standard_normal(10)), inverse_covariance=Ninv) @ M
    H = ift.StandardHamiltonian(lh)
    pos = ift.makeField(sp, 0.1 * rng.standard_normal((16, 16)))
    want = np.sort(1.0 + 1.0 / sig2)[::-1]
    metric = H(ift.Linearization.make_var(pos, want_metric=True)).metric
    L, shift = split_metric(metric)
    assert shift == 1.0 and fusable_metric(L) is None
    mv = MetricMatvec(L)
    assert not mv.fused
    with ift.random.Context(3):
        ev = metric_spectrum(mv, shift, 6, 10, batch_number=2, verbose=False)
    tol = synthetic_tol(G)
    print("closed form", np.abs(ev - want[:6]).max() / want[0], "tol", tol)
    assert ev.size == 6 and np.abs(ev - want[:6]).max() <= tol * want[0]
    # the public entry point on the same problem: exact branch and statistics by hand
    res = [ift.makeField(sp, 0.05 * rng.standard_normal((16, 16))) for _ in range(2)]
    samples = ift.ResidualSampleList(pos, [res[0], res[0], res[1]], [False, True, False])
    elbo, stats = ift.estimate_evidence_lower_bound(H, samples, 10, verbose=False)
    e = np.array([float(s.val) for s in elbo.local_iterator()])
    hs = np.array([float(H(s).val) for s in samples.local_iterator()])
    post = -0.5 * np.log(want).sum() + 0.5 * 256
    assert np.abs(e - (post - hs)).max() <= 1e-10 * np.abs(hs).max() + 0.5 * 10 * tol * want[0]
    assert float(stats["lower_error"].val) == 0.0
    assert abs(float(stats["elbo_mean"].val) - e.mean()) <= 1e-12 * abs(e.mean())
    assert abs(float(stats["elbo_up"].val) - (e.mean() + e.std(ddof=1))) <= 1e-9 * abs(e.mean())
    assert abs(float(stats["elbo_lw"].val) - (e.mean() - e.std(ddof=1))) <= 1e-9 * abs(e.mean())


@pytest.mark.parametrize("tag", ("b", "c"))
def test_fused_against_generic(ift, G, tag):
    from nifty_amd.minimization.fused_cg import fusable_metric
    ev, mv, _, _ = run(ift, G, tag)
    with ift.random.Context(23):
        ev_g, mv_g, L = spectrum(ift, G, tag, force_generic=True)
    assert fusable_metric(L) is not None and mv.fused and not mv_g.fused and mv_g.calls > 0
    tol = float(G[f"{KIND[tag]}_tol"])
    print(tag, "fused against generic", np.abs(ev - ev_g).max() / ev[0])
    assert ev.size == ev_g.size and np.abs(ev - ev_g).max() <= tol * ev[0]


def test_fused_against_generic_product_spectrum(ift, G):
    """a product-spectrum field (the p16x8 configuration of product.npz): the
    fused matvec iterates in the core's own frame R xi, the generic one
    applies the operator in the natural frame; R is orthogonal"""
    from test_product import CASES, maker, unpack
    from nifty_amd.evidence_lower_bound import MetricMatvec, metric_spectrum
    from nifty_amd.minimization.fused_cg import fusable_metric
    P = golden("product.npz")
    tag = "p16x8"
    cf = maker(ift, *CASES[tag]).finalize(prior_info=0)
    N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
    lh = ift.GaussianEnergy(ift.makeField(cf.target, P[tag + "_data"]), inverse_covariance=N.inverse) @ ift.sigmoid(cf)
    L = lh.get_metric_at(unpack(ift, cf.domain, P[tag + "_pos"]))
    assert fusable_metric(L) is not None
    out = []
    for generic in (False, True):
        mv = MetricMatvec(L, force_generic=generic)
        assert mv.fused != generic
        if not generic:
            assert getattr(mv.core, "to_frame", None) is not None
        with ift.random.Context(29):
            out.append(metric_spectrum(mv, 1.0, 8, min(cf.target.size, cf.domain.size), batch_number=2,
                                       verbose=False))
        assert mv.calls > 0
    tol = synthetic_tol(G)
    print("product fused against generic", np.abs(out[0] - out[1]).max() / out[0][0])
    assert out[0].size == out[1].size == 8 and np.abs(out[0] - out[1]).max() <= tol * out[0][0]
