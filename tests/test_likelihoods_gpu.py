"""GPU: BernoulliEnergy, StudentTEnergy and InverseGammaEnergy through the
public interface against the reference's values (tests/golden/likelihoods.npz,
gen_golden_likelihoods.py), and the nft_lh_* kernels against fp64 numpy.

Cases on a SimpleCorrelatedField, l8 = 8 x 8 (the smallest grid on which the
carried CG iteration runs) and l16 = 16 x 16:
  b   BernoulliEnergy(d) @ sigmoid(cf)
  t   StudentTEnergy(sp, 3.) @ Adder(d, neg=True) @ sigmoid(cf)
  tf  the same with a Field theta
  g   InverseGammaEnergy(beta, 0.7) @ exp(cf)
  j   b + a Gaussian branch as lh1 + lh2
  bs  b.scale(0.3)

Tolerances are those of test_sampling_likelihood_gpu.py: metric and
transformation 1e-12 (relative max-norm), energy 1e-10, 5 carried CG steps
1e-9, short geoVI draws 1e-8; batched KL terms against the per-sample ones
1e-10.  Kernel level: fp64 1e-12, fp32 1e-4 (relative max-norm).

The fixture stores a MultiField as one vector: its keys in sorted order, each
raveled."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
SIZES = {"l8": 8, "l16": 16}
CASES = ("b", "t", "tf", "g", "j", "bs")
SINGLE = ("b", "t", "tf", "g", "bs")      # one pointwise likelihood (no sum)
_CACHE = {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def pack(mf):
    return np.concatenate([mf[k].val.cpu().numpy().reshape(-1) for k in sorted(mf.keys())])


def unpack(ift, dom, vec):
    out, o = {}, 0
    for k in sorted(dom.keys()):
        n = dom[k].size
        out[k] = ift.makeField(dom[k], vec[o:o + n].reshape(dom[k].shape).copy())
        o += n
    assert o == len(vec)
    return ift.MultiField.from_dict(out, dom)


def problem(ift, tag):
    """(cf, {case: likelihood}, pos, t, G), built once per grid"""
    if tag not in _CACHE:
        G = golden("likelihoods.npz")
        assert tuple(G["carry_grid"]) == (8, 8)
        n = SIZES[tag]
        sp = ift.RGSpace((n, n))
        cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
        p = ift.sigmoid(cf)
        ev = ift.makeField(sp, G[tag + "_events"])
        td = ift.makeField(sp, G[tag + "_tdata"])
        b = ift.BernoulliEnergy(ev) @ p
        t = ift.StudentTEnergy(sp, 3.) @ ift.Adder(td, neg=True) @ p
        tf = ift.StudentTEnergy(sp, ift.makeField(sp, G[tag + "_theta"])) @ ift.Adder(td, neg=True) @ p
        g = ift.InverseGammaEnergy(ift.makeField(sp, G[tag + "_beta"]), 0.7) @ cf.exp()
        N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
        b2 = ift.BernoulliEnergy(ev) @ p
        ga = ift.GaussianEnergy(ift.makeField(sp, G[tag + "_gdata"]), inverse_covariance=N.inverse) @ cf
        b2.name, ga.name = (str(v) for v in G["names"])
        lhs = dict(b=b, t=t, tf=tf, g=g, j=b2 + ga, bs=b.scale(0.3))
        # no golden: a scaled Gaussian reaches the batched KL terms the same way
        ga2 = ift.GaussianEnergy(ift.makeField(sp, G[tag + "_gdata"]), inverse_covariance=N.inverse) @ cf
        lhs["gs"] = ga2.scale(0.3)
        _CACHE[tag] = (cf, lhs, unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"]), G)
    return _CACHE[tag]


def geovi_sandwich(ift, lh, pos):
    dtype, f = lh.get_transformation()
    fl = f(ift.Linearization.make_var(pos))
    return ift.SandwichOperator.make(fl.jac, ift.ScalingOperator(f.target, 1., dtype))


# ------------------------------------------------------------ golden parity
@pytest.mark.parametrize("tag", list(SIZES))
@pytest.mark.parametrize("c", CASES)
def test_golden_energy_transformation_metric(ift, tag, c):
    cf, lhs, pos, t, G = problem(ift, tag)
    lh, pre = lhs[c], tag + c
    e = lh(pos).val.item()
    print(pre, "energy", abs(e - float(G[pre + "_energy"])) / abs(float(G[pre + "_energy"])))
    assert abs(e - float(G[pre + "_energy"])) <= 1e-10 * abs(float(G[pre + "_energy"]))
    dtype, f = lh.get_transformation()
    tr = f(pos)
    trv = pack(tr) if isinstance(tr, ift.MultiField) else tr.val.cpu().numpy()
    err = relmax(trv, G[pre + "_tr"])
    print(pre, "transformation", err)
    assert err < 1e-12
    met = lh.get_metric_at(pos)
    assert met.fused is not None
    sand = geovi_sandwich(ift, lh, pos)
    assert sand.fused is not None
    ref = unpack(ift, cf.domain, G[pre + "_mt"])
    for m in (met, sand):
        mt = m(t)
        for k in cf.domain.keys():
            err = relmax(mt[k].val.cpu().numpy(), ref[k].val.cpu().numpy())
            print(pre, "metric", k, err)
            assert err < 1e-12, k


def test_energy_with_metric_and_residuals(ift):
    """apply with want_metric adds the metric; normalized_residual works"""
    cf, lhs, pos, t, G = problem(ift, "l8")
    for c in SINGLE:
        lin = lhs[c](ift.Linearization.make_var(pos, want_metric=True))
        assert lin.metric is not None
        a, b = lin.metric(t), lhs[c].get_metric_at(pos)(t)
        for k in cf.domain.keys():
            assert relmax(a[k].val.cpu().numpy(), b[k].val.cpu().numpy()) < 1e-12, (c, k)
        r = lhs[c].normalized_residual(pos)
        assert r.domain is lhs[c].data_domain and bool(torch.isfinite(r.val).all())
    # Bernoulli: (f - d) / sqrt(f (1 - f))
    f = ift.sigmoid(cf)(pos).val.cpu().numpy()
    want = (f - G["l8_events"]) / np.sqrt(f * (1 - f))
    assert relmax(lhs["b"].normalized_residual(pos).val.cpu().numpy(), want) < 1e-12


# ------------------------------------------------------------------- fusion
@pytest.mark.parametrize("tag", list(SIZES))
def test_middles(ift, tag):
    """b, t, g: the middle is a contiguous fp64 tensor on the model's grid --
    the likelihood's Fisher weight times the squared derivative of the
    model's pointwise map.  Divided by that derivative it is 1 / (f (1 - f))
    for b, the constant (theta + 1) / (theta + 3) for scalar-theta t and
    alpha + 1 for g (exp model: f^2 cancels)."""
    cf, lhs, pos, t, G = problem(ift, tag)
    s = cf(pos).val
    f = 0.5 + 0.5 * torch.tanh(s)
    ds2 = (0.5 * (1 - torch.tanh(s) ** 2)) ** 2
    core = None
    for c, want in (("b", ds2 / (f * (1 - f))), ("t", ds2 * (4. / 6.)), ("g", torch.full_like(s, 1.7)),
                    ("bs", 0.3 * ds2 / (f * (1 - f)))):
        for sand in (geovi_sandwich(ift, lhs[c], pos), lhs[c].get_metric_at(pos)):
            W = sand.fused[1]
            assert torch.is_tensor(W) and W.dtype == torch.float64 and W.is_contiguous(), c
            assert W.shape == cf.target.shape, c
            core = sand.fused[0] if core is None else core
            assert sand.fused[0] is core
            assert (W > 0).all(), c
            assert relmax(W.cpu().numpy(), want.cpu().numpy()) < 1e-12, c
    Wt = geovi_sandwich(ift, lhs["t"], pos).fused[1] / ds2
    assert float((Wt.max() - Wt.min()) / Wt.max()) < 1e-12


def test_bernoulli_plus_los_takes_the_fused_los_add_middle(ift):
    """LOS data + Bernoulli events on the grid: the Bernoulli branch is a
    tensor, so the joint middle is the nft_los_adjoint_add one"""
    from nifty_amd import _native
    cf, lhs, pos, t, G = problem(ift, "l16")
    sp = cf.target[0]
    rng = np.random.default_rng(5)
    R = ift.LOSResponse(sp, starts=list(rng.random((2, 25))), ends=list(rng.random((2, 25))))
    N = ift.ScalingOperator(R.target, 1e-2, np.float64)
    lhl = ift.GaussianEnergy(ift.full(R.target, 0.4), inverse_covariance=N.inverse) @ R(ift.sigmoid(cf))
    lhl.name = "los"
    lh = lhl + lhs["b"]
    sand = geovi_sandwich(ift, lh, pos)
    assert sand.fused is not None
    W = sand.fused[1]
    lib = _native.load()
    plan = W.los.plan
    assert W.quad_blocks == lib.nft_los_quad_blocks(ctypes.byref(plan)) + lib.nft_los_add_blocks(ctypes.byref(plan))
    assert torch.is_tensor(W.addw)
    parts = lhl.get_metric_at(pos)(t) + lhs["b"].get_metric_at(pos)(t)
    joint = sand(t)
    for k in cf.domain.keys():
        assert relmax(joint[k].val.cpu().numpy(), parts[k].val.cpu().numpy()) < 1e-12, k


# -------------------------------------------------------------------- solve
@pytest.mark.parametrize("c", CASES)
def test_five_cg_steps(ift, c):
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G = problem(ift, "l8")
    A = lhs[c].get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0
    if c != "j":
        cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5))
        cg.run(ift.QuadraticEnergy(0 * t, A, t))
        assert cg.path == "carry+chunk", cg.path
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        en, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
        assert st == ic.CONVERGED
        ref = unpack(ift, cf.domain, G[f"l8{c}_cg{it}"])
        for k in cf.domain.keys():
            err = rel(en.position[k].val.cpu().numpy(), ref[k].val.cpu().numpy())
            print(c, it, "CG steps", k, err)
            assert err < 1e-9, (it, k)


# -------------------------------------------------------------------- geoVI
def _geo_draw(ift, lh, pos):
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    return kl


@pytest.mark.parametrize("c", CASES)
def test_geovi_draw_matches_reference(ift, c):
    cf, lhs, pos, t, G = problem(ift, "l8")
    kl = _geo_draw(ift, lhs[c], pos)
    ref = G[f"l8{c}_geo_samples"]
    assert kl.samples.n_samples == len(ref) == 2
    for i in range(2):
        err = rel(pack(kl.samples.local_item(i)), ref[i])
        print(c, "geoVI sample", i, err)
        assert err < 1e-8, i
    ev = abs(kl.value - float(G[f"l8{c}_geo_value"])) / abs(float(G[f"l8{c}_geo_value"]))
    print(c, "geoVI KL value", ev)
    assert ev < 1e-8


@pytest.mark.parametrize("c", SINGLE)
def test_batched_refinement_is_taken_and_matches_per_sample(ift, c):
    from nifty_amd.minimization import geovi_batch
    cf, lhs, pos, t, G = problem(ift, "l16")
    lh = lhs[c]
    dtype, f_lh = lh.get_transformation()
    mini = ift.NewtonCG(ift.GradientNormController(iteration_limit=1))
    assert geovi_batch.plan(mini, f_lh, None, pos) is not None
    bat = _geo_draw(ift, lh, pos)
    geovi_batch.ENABLED = False
    try:
        assert geovi_batch.plan(mini, f_lh, None, pos) is None
        seq = _geo_draw(ift, lh, pos)
    finally:
        geovi_batch.ENABLED = True
    for i in range(2):
        a, b = pack(bat.samples.local_item(i)), pack(seq.samples.local_item(i))
        assert np.all(np.isfinite(a))
        print(c, "batched vs per sample", i, rel(a, b))
        assert rel(a, b) < 1e-8, i
    assert abs(bat.value - seq.value) <= 1e-8 * abs(seq.value)


@pytest.mark.parametrize("c", SINGLE + ("gs",))
def test_kl_batch_and_metric_batch_match_per_sample(ift, c):
    """value, gradient and metric application of the batched KL terms against
    H(Linearization.make_var(s, want_metric=True)) per position (gs: a scaled
    Gaussian, whose nested chain the batched terms open up like bs's)"""
    from nifty_amd.minimization import geovi_batch
    cf, lhs, pos, t, G = problem(ift, "l16")
    H = ift.StandardHamiltonian(lhs[c], ift.GradientNormController(iteration_limit=5))
    with ift.random.Context(3):
        u = ift.from_random(cf.domain, "normal")
    positions = [pos, pos + 0.05 * t, pos - 0.03 * u]
    out = geovi_batch.kl_batch(H, positions)
    assert out is not None
    apply = geovi_batch.kl_metric_batch(H, positions)
    assert apply is not None
    mx = apply(t)
    for i, s in enumerate(positions):
        lin = H(ift.Linearization.make_var(s, want_metric=True))
        v = lin.val.val.item()
        print(c, i, "value", abs(out[0][i] - v) / abs(v))
        assert abs(out[0][i] - v) <= 1e-10 * abs(v), i
        g, m = lin.gradient, lin.metric(t)
        for k in cf.domain.keys():
            eg = rel(out[1][i][k].val.cpu().numpy(), g[k].val.cpu().numpy())
            em = rel(mx[i][k].val.cpu().numpy(), m[k].val.cpu().numpy())
            print(c, i, k, "gradient", eg, "metric", em)
            assert eg < 1e-10 and em < 1e-10, (i, k)


# ------------------------------------------------------------------ kernels
KINDS = ("bernoulli", "student_t", "student_t_c0", "invgamma")
NS = (1, 255, 256, 257, 4099)
KS = (1, 3, 8)
PAD = 64
TOL = {torch.float64: 1e-12, torch.float32: 1e-4}


class _Lib:
    def __init__(self, dev):
        from nifty_amd import _native
        self.nat = _native
        self.lib = _native.load()
        self.dev = dev
        self.P = _native.ptr
        self.s = _native.stream_ptr()

    def ws(self, k, n):
        return torch.empty(max(k * self.lib.nft_reduce_workspace(n), 8), dtype=torch.uint8, device=self.dev)

    def eval(self, code, F, n, p0, p1, c0, scale=1.0, value=None, grad=None, weight=None, k=None, vs=None):
        """raw nft_lh_eval_batched on the rows of the 2-D buffer F"""
        k = F.shape[0] if k is None else k
        vs = F.shape[1] if vs is None else vs
        st = self.lib.nft_lh_eval_batched(code, self.P(F), self.P(p0), self.P(p1), float(c0), n, vs, k,
                                          self.nat.dtype_code(F.dtype), float(scale), self.P(value), self.P(grad),
                                          self.P(weight), self.P(self.ws(max(k, 1), max(n, 0))), self.s)
        self.nat._check(st)


@pytest.fixture(scope="module")
def L(dev):
    return _Lib(dev)


def _params(kind, n, rng, dev):
    """(code, p0, p1, c0, host p0, host p1) of one kind"""
    from nifty_amd import _native
    up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
    if kind == "bernoulli":
        d = (rng.random(n) < 0.5).astype(np.float64)
        return _native.LH_BERNOULLI, up(d), None, 0.0, d, None
    if kind == "student_t":
        th = 2. + 4. * rng.random(n)
        return _native.LH_STUDENT_T, up(th), None, 0.0, th, None
    if kind == "student_t_c0":
        return _native.LH_STUDENT_T, None, None, 3.0, np.full(n, 3.0), None
    a, b = 0.5 + rng.random(n), 0.05 + rng.random(n)
    return _native.LH_INVGAMMA, up(a), up(b), 0.0, a, b


def _numpy_terms(kind, f, a, b):
    """fp64 (E per row, dE/df, W) of the rows of f"""
    if kind == "bernoulli":
        return ((-np.log(f) * a + np.log(1 - f) * (a - 1)).sum(1), -a / f + (1 - a) / (1 - f), 1 / (f * (1 - f)))
    if kind.startswith("student_t"):
        return (((a + 1) / 2 * np.log1p(f * f / a)).sum(1), (a + 1) * f / (a + f * f),
                np.broadcast_to((a + 1) / (a + 3), f.shape))
    return (a * np.log(f) + b / f).sum(1), a / f - b / (f * f), a / (f * f)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("dt", (torch.float64, torch.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("kind", KINDS)
def test_lh_eval_rows_strides_and_numpy(L, kind, dt, n):
    rng = np.random.default_rng(1000 + n)
    code, p0, p1, c0, a, b = _params(kind, n, rng, L.dev)
    tol = TOL[dt]
    for k in KS:
        fh = (0.05 + 0.9 * rng.random((k, n))).astype(np.float32 if dt == torch.float32 else np.float64)
        ev, eg, ew = _numpy_terms(kind, fh.astype(np.float64), a, b)
        singles = []
        for pad in (0, PAD):
            F = torch.full((k, n + pad), float("nan"), dtype=dt, device=L.dev)    # poisoned padding
            F[:, :n] = torch.from_numpy(fh).to(L.dev)
            g = torch.full((k, n + pad), 777., dtype=dt, device=L.dev)
            w = torch.full((k, n + pad), 777., dtype=dt, device=L.dev)
            v = torch.full((k,), 777., dtype=torch.float64, device=L.dev)
            L.eval(code, F, n, p0, p1, c0, value=v, grad=g, weight=w)
            assert (g[:, n:] == 777.).all() and (w[:, n:] == 777.).all(), "padding written"
            vh = v.cpu().numpy()
            print(kind, dt, n, k, pad, "value", np.abs(vh - ev).max() / np.abs(ev).max(),
                  "grad", relmax(g[:, :n].cpu().numpy(), eg), "weight", relmax(w[:, :n].cpu().numpy(), ew))
            assert np.all(np.abs(vh - ev) <= tol * np.abs(ev)), (k, pad)
            assert relmax(g[:, :n].cpu().numpy(), eg) < tol and relmax(w[:, :n].cpu().numpy(), ew) < tol, (k, pad)
            singles.append((v, g[:, :n].clone(), w[:, :n].clone()))
        # the stride does not matter, bit for bit
        for x, y in zip(*singles):
            assert torch.equal(x, y)
        # row i of the k-row call is the k = 1 call on that row (rows 1.. start
        # at other alignments than a fresh buffer)
        v, g, w = singles[0]
        for i in range(k):
            Fi = torch.from_numpy(fh[i:i + 1].copy()).to(L.dev)
            vi = torch.empty(1, dtype=torch.float64, device=L.dev)
            gi, wi = torch.empty_like(Fi), torch.empty_like(Fi)
            L.eval(code, Fi, n, p0, p1, c0, value=vi, grad=gi, weight=wi)
            assert torch.equal(vi[0], v[i]) and torch.equal(gi[0], g[i]) and torch.equal(wi[0], w[i]), (k, i)


@pytest.mark.parametrize("dt", (torch.float64, torch.float32), ids=("fp64", "fp32"))
@pytest.mark.parametrize("kind", KINDS)
def test_lh_eval_null_outputs_and_scale(L, kind, dt):
    n, k = 4099, 3
    rng = np.random.default_rng(7)
    code, p0, p1, c0, a, b = _params(kind, n, rng, L.dev)
    F = torch.from_numpy(0.05 + 0.9 * rng.random((k, n))).to(L.dev).to(dt)

    def run(scale, value=True, grad=True, weight=True):
        v = torch.full((k,), 777., dtype=torch.float64, device=L.dev) if value else None
        g = torch.full_like(F, 777.) if grad else None
        w = torch.full_like(F, 777.) if weight else None
        L.eval(code, F, n, p0, p1, c0, scale=scale, value=v, grad=g, weight=w)
        return v, g, w
    v, g, w = run(1.0)
    # NULL outputs are skipped, the others unchanged bit for bit
    for mask in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 1), (0, 1, 1)):
        out = run(1.0, *map(bool, mask))
        for want, got, m in zip((v, g, w), out, mask):
            assert (got is None) if not m else torch.equal(got, want), mask
    run(1.0, False, False, False)
    # scale multiplies all three: exactly for a power of two, and in fp64 for
    # any factor (one rounding of the product)
    for scale in (0.25,) + ((0.3,) if dt == torch.float64 else ()):
        vs, gs, ws = run(scale)
        assert torch.equal(vs, v * scale) and torch.equal(gs, g * scale) and torch.equal(ws, w * scale), scale
    # any factor in fp32 storage: the kernel rounds the fp64 product once, the
    # comparison rounds the unscaled output, the factor and their product
    vs, gs, ws = run(0.3)
    eps = 4 * (2. ** -53 if dt == torch.float64 else 2. ** -24)
    assert relmax(vs.cpu().numpy(), 0.3 * v.cpu().numpy()) < 4 * 2. ** -53
    assert relmax(gs.cpu().numpy(), 0.3 * g.cpu().numpy()) < eps
    assert relmax(ws.cpu().numpy(), 0.3 * w.cpu().numpy()) < eps


def test_lh_eval_wrapper(L):
    """_native.lh_eval_batched: the outputs asked for, one call"""
    n, k = 257, 3
    rng = np.random.default_rng(3)
    code, p0, p1, c0, a, b = _params("invgamma", n, rng, L.dev)
    fh = 0.05 + 0.9 * rng.random((k, n))
    F = torch.from_numpy(fh).to(L.dev)
    ev, eg, ew = _numpy_terms("invgamma", fh, a, b)
    v, g, w = L.nat.lh_eval_batched(code, F, p0, p1, c0, 0.5, value=True, grad=True, weight=True)
    assert relmax(v.cpu().numpy(), 0.5 * ev) < 1e-12 and relmax(g.cpu().numpy(), 0.5 * eg) < 1e-12
    assert relmax(w.cpu().numpy(), 0.5 * ew) < 1e-12
    assert L.nat.lh_eval_batched(code, F, p0, p1, c0, weight=True)[:2] == (None, None)
    with pytest.raises(L.nat.NativeError):
        L.nat.lh_eval_batched(code, F, p0[:-1], p1, c0, weight=True)
    with pytest.raises(L.nat.NativeError):
        L.nat.lh_eval_batched(code, F.cpu(), p0, p1, c0, weight=True)


@pytest.mark.parametrize("n", (0,) + NS)
@pytest.mark.parametrize("dt", (torch.float64, torch.float32), ids=("fp64", "fp32"))
def test_lh_transform_pair(L, dt, n):
    rng = np.random.default_rng(50 + n)
    fh = (0.05 + 0.9 * rng.random(n + 1)).astype(np.float32 if dt == torch.float32 else np.float64)
    buf = torch.from_numpy(fh).to(L.dev)
    f = buf[:n]
    t, d = torch.full_like(buf, 777.), torch.full_like(buf, 777.)
    L.nat.lh_transform_pair(L.nat.LH_BERNOULLI, f, t[:n], d[:n])
    assert t[n] == 777. and d[n] == 777.
    if n == 0:
        return
    x = fh[:n].astype(np.float64)
    et, ed = -2 * np.arctan(np.sqrt((1 - x) / x)), 1 / np.sqrt(x * (1 - x))
    print(dt, n, "t", relmax(t[:n].cpu().numpy(), et), "dt", relmax(d[:n].cpu().numpy(), ed))
    assert relmax(t[:n].cpu().numpy(), et) < TOL[dt] and relmax(d[:n].cpu().numpy(), ed) < TOL[dt]
    # an unaligned view gives the same bits
    f1 = buf[1:1 + n]
    t1, d1 = torch.full_like(buf, 777.), torch.full_like(buf, 777.)
    L.nat.lh_transform_pair(L.nat.LH_BERNOULLI, f1, t1[1:1 + n], d1[1:1 + n])
    assert t1[0] == 777. and d1[0] == 777.
    if n > 1:
        t2, d2 = L.nat.lh_transform_pair(L.nat.LH_BERNOULLI, f1[:n - 1].clone(), torch.empty(n - 1, dtype=dt,
                                         device=L.dev), torch.empty(n - 1, dtype=dt, device=L.dev))
        assert torch.equal(t1[1:n], t2) and torch.equal(d1[1:n], d2)


def test_bernoulli_transform_operator(ift):
    """Field -> t(f); Linearization -> DiagonalOperator(1 / sqrt(f (1 - f))) @ jac"""
    from nifty_amd.operators.energy_operators import _BernoulliTransform
    sp = ift.RGSpace((5, 7))
    rng = np.random.default_rng(2)
    x = 0.05 + 0.9 * rng.random((5, 7))
    T = _BernoulliTransform(sp)
    f = ift.makeField(sp, x)
    assert relmax(T(f).val.cpu().numpy(), -2 * np.arctan(np.sqrt((1 - x) / x))) < 1e-12
    lin = T(ift.Linearization.make_var(f))
    assert isinstance(lin.jac, ift.DiagonalOperator)
    assert torch.equal(lin.val.val, T(f).val)
    assert relmax(lin.jac.diagonal_tensor.cpu().numpy(), 1 / np.sqrt(x * (1 - x))) < 1e-12


def test_argument_errors(L):
    n, k = 16, 2
    E = L.nat.NativeError
    F = torch.full((k, n), 0.5, dtype=torch.float64, device=L.dev)
    p = torch.full((n,), 1.0, dtype=torch.float64, device=L.dev)
    g = torch.empty_like(F)
    B, T, IG = L.nat.LH_BERNOULLI, L.nat.LH_STUDENT_T, L.nat.LH_INVGAMMA
    lib, P, s = L.lib, L.P, L.s
    ws = L.ws(k, n)

    def call(kind=B, f=F, p0=p, p1=None, n_=n, vs=n, k_=k, dtype=0, grad=g):
        L.nat._check(lib.nft_lh_eval_batched(kind, P(f), P(p0), P(p1), 3.0, n_, vs, k_, dtype, 1.0, P(None),
                                             P(grad), P(None), P(ws), s))
    call()
    call(kind=T, p0=None)
    call(kind=IG, p1=p)
    for bad in (dict(kind=3), dict(kind=-1), dict(dtype=2), dict(dtype=-1), dict(n_=-1), dict(k_=0),
                dict(vs=n - 1), dict(p0=None), dict(kind=IG), dict(kind=IG, p0=None, p1=p), dict(f=None)):
        with pytest.raises(E):
            call(**bad)
    assert b"nft_lh_eval_batched" in lib.nft_last_error()
    # value without a workspace
    v = torch.empty(k, dtype=torch.float64, device=L.dev)
    with pytest.raises(E):
        L.nat._check(lib.nft_lh_eval_batched(B, P(F), P(p), P(None), 0.0, n, n, k, 0, 1.0, P(v), P(None), P(None),
                                             P(None), s))
    # n == 0: nothing is read, the energy of an empty row is 0
    L.nat._check(lib.nft_lh_eval_batched(B, P(None), P(None), P(None), 0.0, 0, 0, k, 0, 1.0, P(v), P(None), P(None),
                                         P(ws), s))
    assert (v == 0).all()
    # transform pair: as nft_sigmoid_pair
    x = F[0].contiguous()
    t, d = torch.empty_like(x), torch.empty_like(x)

    def pair(kind=B, f=x, t_=t, d_=d, n_=n, dtype=0):
        L.nat._check(lib.nft_lh_transform_pair(kind, P(f), P(t_), P(d_), n_, dtype, s))
    pair()
    pair(f=None, t_=None, d_=None, n_=0)
    for bad in (dict(kind=T), dict(kind=7), dict(dtype=2), dict(n_=-1), dict(f=None), dict(t_=None), dict(d_=None)):
        with pytest.raises(E):
            pair(**bad)
    assert b"nft_lh_transform_pair" in lib.nft_last_error()
    torch.cuda.synchronize()
