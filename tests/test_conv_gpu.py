"""GPU: FuncConvolutionOperator (csrc/nft_conv.hip) against the reference's
values (tests/golden/conv.npz, gen_golden_conv.py), alone and inside
likelihoods on a SimpleCorrelatedField:
  a  GaussianEnergy(d, 1e-3) @ GeometryRemover(C(sigmoid(cf)))
  b  PoissonianEnergy(counts) @ Mask(Exposure(C(exp(cf))))
  c  a + b as lh1 + lh2
on s8 = 8 x 8 (the smallest grid on which the carried CG iteration runs) and
s16 = 16 x 16.

Tolerances: operator against the reference 1e-12 relative max-norm (the
project's bound for a metric or transformation; the reference's own distance
to the FFT form is 4e-16); native against the two-transform path, folded
scales against torch multiplies and the zero-mode gain 1e-13; the quadratic
form 1e-12; likelihoods as test_sampling_likelihood_gpu.py (energy 1e-10,
transformation and metric 1e-12, 5 CG steps 1e-9, samples 1e-8).

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
SIGMA_PIX = 1.7
NATIVE = ("g88", "g168", "g832", "g888", "g8168", "g10248")
FALLBACK = ("g16", "g86")
KERNELS = ("g", "k")
SIZES = {"s8": 8, "s16": 16}
CASES = ("a", "b", "c")
_OPS, _CACHE = {}, {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


def kernels(sp):
    sig = SIGMA_PIX * min(sp.distances)
    r0 = 0.25 * min(n * d for n, d in zip(sp.shape, sp.distances))
    return dict(g=lambda r: np.exp(-0.5 * (r / sig) ** 2), k=lambda r: (1. + (r / r0) ** 2) ** -2)


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


def trel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def operator(ift, tag, kn):
    """(space, operator, input Field, fixture), built once per case"""
    if (tag, kn) not in _OPS:
        G = golden("conv.npz")
        shape = tuple(int(n) for n in G[tag + "_shape"])
        sp = ift.RGSpace(shape, distances=tuple(G[tag + "_dist"]))
        C = ift.FuncConvolutionOperator(sp, kernels(sp)[kn])
        x = 0.7 + np.random.default_rng(int(G[tag + "_seed"])).standard_normal(shape)
        _OPS[(tag, kn)] = (sp, C, ift.makeField(sp, x), G)
    return _OPS[(tag, kn)]


# ---------------------------------------------------------------- operator
def test_supported_grids(ift):
    from nifty_amd import _native
    G = golden("conv.npz")
    for tag in NATIVE:
        assert _native.conv_supported(tuple(int(n) for n in G[tag + "_shape"])), tag
        assert operator(ift, tag, "g")[1].native
    for tag in FALLBACK:
        assert not _native.conv_supported(tuple(int(n) for n in G[tag + "_shape"])), tag
        assert not operator(ift, tag, "g")[1].native
    assert not _native.conv_supported((8, 8), torch.float32)


@pytest.mark.parametrize("kn", KERNELS)
@pytest.mark.parametrize("tag", NATIVE + FALLBACK)
def test_times_and_adjoint_match_reference(ift, tag, kn):
    sp, C, x, G = operator(ift, tag, kn)
    ref = G[f"{tag}_{kn}_Cx"]
    for name, y in (("times", C(x)), ("adjoint", C.adjoint_times(x))):
        err = relmax(y.val.cpu().numpy(), ref)
        print(tag, kn, name, err)
        assert err < 1e-12
    # the zero-mode gain is 1: the sum is kept
    s = C(x).val.sum().item()
    s0 = x.val.sum().item()
    print(tag, kn, "sum", abs(s - s0) / abs(s0))
    assert abs(s - s0) <= 1e-13 * abs(s0)


def test_complex_field_part_by_part(ift):
    sp, C, x, G = operator(ift, "g88", "g")
    z = ift.Field(x.domain, x.val * (1 + 0j) + 1j * x.val.flip(0))
    y = C(z)
    assert trel(y.val.real, C(x).val) < 1e-14
    assert trel(y.val.imag, C(ift.Field(x.domain, x.val.flip(0).contiguous())).val) < 1e-14


@pytest.mark.parametrize("kn", KERNELS)
@pytest.mark.parametrize("tag", NATIVE)
def test_native_matches_two_transform_path(ift, tag, kn, monkeypatch):
    sp, C, x, G = operator(ift, tag, kn)
    nat = C(x).val
    monkeypatch.setenv("NFT_CONV_NATIVE", "0")
    assert not C.native
    fb = C(x).val
    monkeypatch.delenv("NFT_CONV_NATIVE")
    assert C.native
    err = trel(nat, fb)
    print(tag, kn, "native vs two transforms", err)
    assert err < 1e-13


@pytest.mark.parametrize("tag", NATIVE)
def test_batches_are_bitwise_the_single_call(ift, tag, dev):
    sp, C, x, G = operator(ift, tag, "k")
    npix = x.val.numel()
    nq = C.quad_blocks()
    assert nq >= 1
    g = torch.Generator(device="cpu").manual_seed(3)
    col = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    row = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    big = torch.randn((5, npix + 24), generator=g, dtype=torch.float64).to(dev)
    single, qsingle = [], []
    for v in range(5):
        q = torch.zeros((1, nq), dtype=torch.float64, device=dev)
        single.append(C.apply_rows(big[v:v + 1, :npix].contiguous(), colscale=col, rowscale=row, scale=0.3, qpart=q))
        qsingle.append(q)
    for k in (1, 3, 5):
        X = big[:k, :npix]                  # row stride npix + 24
        assert k == 1 or not X.is_contiguous()
        outbuf = torch.zeros((k, npix + 8), dtype=torch.float64, device=dev)
        q = torch.zeros((k, nq + 3), dtype=torch.float64, device=dev)
        Y = C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q[:, :nq], out=outbuf[:, :npix])
        assert not outbuf[:, npix:].any() and not q[:, nq:].any()
        for v in range(k):
            assert torch.equal(Y[v], single[v][0]), (k, v)
            assert torch.equal(q[v, :nq], qsingle[v][0]), (k, v)


@pytest.mark.parametrize("tag", NATIVE)
def test_folded_scales_and_quadratic_form(ift, tag, dev):
    sp, C, x, G = operator(ift, tag, "g")
    npix = x.val.numel()
    g = torch.Generator(device="cpu").manual_seed(4)
    col = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) - 0.3
    row = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) - 0.3
    X = x.val.reshape(1, -1)
    t = C.apply_rows(X * col)
    want = 0.3 * row * t
    q = torch.zeros((1, C.quad_blocks()), dtype=torch.float64, device=dev)
    got = C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q)
    err = trel(got, want)
    print(tag, "folded scales", err)
    assert err < 1e-13
    dot = torch.dot(t[0], want[0]).item()
    qs = q.sum().item()
    print(tag, "quadratic form", abs(qs - dot) / abs(dot))
    assert abs(qs - dot) <= 1e-12 * abs(dot)
    # one scale at a time
    assert trel(C.apply_rows(X, colscale=col), t) < 1e-13
    assert trel(C.apply_rows(X, rowscale=row), row * C.apply_rows(X)) < 1e-13


def test_bad_plan_is_an_argument_error(ift, dev):
    from nifty_amd import _native
    lib = _native.load()
    x = torch.ones((1, 64), dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    table = torch.full((8, 5), 1. / 64, dtype=torch.float64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)

    def call(plan):
        return lib.nft_conv_apply_batched(ctypes.byref(plan), _native.ptr(x), 64, None, _native.ptr(y), 64, None, 1.0,
                                          1, 0, None, 0, _native.ptr(ws), ctypes.c_size_t(ws.numel()),
                                          _native.stream_ptr())
    good = _native.conv_plan((8, 8), table)
    assert call(good) == 0
    torch.cuda.synchronize()
    assert trel(y, x) < 1e-14       # all gains 1: the identity
    for ndim in (0, 4):
        p = _native.conv_plan((8, 8), table)
        p.ndim = ndim
        assert call(p) == -1        # NFT_ERR_ARG
    p = _native.conv_plan((8, 8), table)
    p.table = None
    assert call(p) == -1
    assert lib.nft_conv_workspace(ctypes.byref(p), 1) == 0 and lib.nft_conv_quad_blocks(ctypes.byref(p)) == 0


# -------------------------------------------------------------- likelihoods
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
    """(cf, {a, b, c: likelihood}, pos, t, G, response of b), built once per grid"""
    if tag not in _CACHE:
        G = golden("conv.npz")
        assert tuple(G["carry_grid"]) == (8, 8)
        n = SIZES[tag]
        sp = ift.RGSpace((n, n))
        cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
        C = ift.FuncConvolutionOperator(sp, kernels(sp)["g"])
        M = ift.MaskOperator(ift.makeField(sp, G[tag + "_flags"]))
        E = ift.DiagonalOperator(ift.makeField(sp, G[tag + "_expo"]))
        R = ift.GeometryRemover(sp)
        N = ift.ScalingOperator(R.target, 1e-3, np.float64)
        lh1 = ift.GaussianEnergy(ift.makeField(R.target, G[tag + "_data"]),
                                 inverse_covariance=N.inverse) @ R(C(ift.sigmoid(cf)))
        lh2 = ift.PoissonianEnergy(ift.makeField(M.target, G[tag + "_counts"])) @ M(E(C(cf.exp())))
        lh1.name, lh2.name = (str(v) for v in G["names"])
        lhs = dict(a=lh1, b=lh2, c=lh1 + lh2)
        _CACHE[tag] = (cf, lhs, unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"]), G,
                       M @ E @ C)
    return _CACHE[tag]


def geovi_sandwich(ift, lh, pos):
    dtype, f = lh.get_transformation()
    fl = f(ift.Linearization.make_var(pos))
    return ift.SandwichOperator.make(fl.jac, ift.ScalingOperator(f.target, 1., dtype))


@pytest.mark.parametrize("tag", list(SIZES))
@pytest.mark.parametrize("c", CASES)
def test_golden_energy_transformation_metric(ift, tag, c):
    cf, lhs, pos, t, G, resp = problem(ift, tag)
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


@pytest.mark.parametrize("tag", list(SIZES))
def test_middles(ift, tag):
    from nifty_amd import _native
    cf, lhs, pos, t, G, resp = problem(ift, tag)
    sa, sb, sc = (geovi_sandwich(ift, lhs[c], pos) for c in CASES)
    for W in (sa.fused[1], sb.fused[1]):
        assert callable(W) and W.supports_batch and not W.supports_fp32 and not W.supports_fold
        assert W.quad_blocks == _native.conv_quad_blocks(W.conv_plan) > 0
        assert not hasattr(W, "plan") and not hasattr(W, "scales")
        with pytest.raises(NotImplementedError):
            W(torch.zeros(cf.target.shape, dtype=torch.float64, device=pos["xi"].val.device), fold=object())
    # a: a scalar data weight; b: mask x exposure^2 as the grid weight, zero
    # exactly at the flagged pixels
    assert sa.fused[1].conv_scales(torch.float64)[1] is None
    dr, cv = sb.fused[1].conv_scales(torch.float64)
    flags = torch.from_numpy(G[tag + "_flags"]).to(cv.device).reshape(-1)
    assert dr is not None and cv.dtype == torch.float64
    assert not cv[flags].any() and (cv[~flags] > 0).all()
    # c: the generic sum of both
    Wc = sc.fused[1]
    assert callable(Wc) and Wc.quad_blocks == 0 and len(Wc.parts) == 2 and Wc.supports_batch


def _rhs(ift, cf, n):
    out = []
    for i in range(n):
        with ift.random.Context(40 + i):
            out.append(ift.from_random(cf.domain, "normal"))
    return out


def test_batched_solve_is_carried_bitwise_single_and_matches_unfused(ift):
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G, resp = problem(ift, "s8")
    met = lhs["b"].get_metric_at(pos)
    one = ift.ScalingOperator(cf.domain, 1., float)
    A = met + one
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0
    bs = _rhs(ift, cf, 4)
    es = [ift.QuadraticEnergy(0 * b, A, b) for b in bs]
    single = [fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5)).run(e) for e in es]
    cg = fused_cg.FusedCGBatch(core, W, shift, [ift.GradientNormController(iteration_limit=5) for _ in es])
    bat = cg.run(es)
    assert cg.path == "carry+chunk", cg.path
    for (e1, s1), (e2, s2) in zip(single, bat):
        assert s1 == s2
        for k in cf.domain.keys():
            assert torch.equal(e1.position[k].val, e2.position[k].val), k
    # the same solve on the operator-by-operator metric
    plain = met._op + one
    assert getattr(plain, "fused", None) is None
    for b, (eb, sb) in zip(bs, bat):
        ic = ift.GradientNormController(iteration_limit=5)
        ep, sp_ = ift.ConjugateGradient(ic, allow_fused=False)(ift.QuadraticEnergy(0 * b, plain, b))
        assert sp_ == sb
        for k in cf.domain.keys():
            err = rel(eb.position[k].val.cpu().numpy(), ep.position[k].val.cpu().numpy())
            print("5 CG steps, fused vs operator by operator", k, err)
            assert err < 1e-9, k


def test_fp32_request_leaves_the_solve_in_fp64(ift):
    from nifty_amd import config
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G, resp = problem(ift, "s8")
    A = lhs["b"].get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    ic = ift.GradientNormController(iteration_limit=5)
    e64, _ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
    config.set_cg_precision("fp32")
    try:
        assert not fused_cg.mixed_precision(core, W)
        ic = ift.GradientNormController(iteration_limit=5)
        e32, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
    finally:
        config.set_cg_precision("fp64")
    assert st == ic.CONVERGED
    for k in cf.domain.keys():
        assert e32.position[k].val.dtype == torch.float64
        assert torch.equal(e32.position[k].val, e64.position[k].val), k


def test_mgvi_samples_match_reference(ift):
    cf, lhs, pos, t, G, resp = problem(ift, "s8")
    H = ift.StandardHamiltonian(lhs["b"], ift.AbsDeltaEnergyController(deltaE=1e-30, iteration_limit=10))
    ift.random.push_sseq_from_seed(27)
    sl = ift.draw_samples(pos, H, None, 1, True)
    ift.random.pop_sseq()
    ref = G["s8b_mgvi_samples"]
    assert sl.n_samples == len(ref) == 2
    for i in range(2):
        err = rel(pack(sl.local_item(i)), ref[i])
        print("MGVI sample", i, err)
        assert err < 1e-8, i


@pytest.mark.parametrize("tag", list(SIZES))
def test_lowered_response_matches_operators(ift, tag):
    from nifty_amd.lowering import lower
    cf, lhs, pos, t, G, resp = problem(ift, tag)
    fwd, adj = lower(resp), lower(resp, adjoint=True)
    assert fwd is not None and adj is not None
    with ift.random.Context(9):
        x = ift.from_random(resp.domain, "normal")
        y = ift.from_random(resp.target, "normal")
    err = trel(fwd(x.val).reshape(-1), resp(x).val.reshape(-1))
    print(tag, "lowered response", err)
    assert err < 1e-13
    err = trel(adj(y.val).reshape(-1), resp.adjoint_times(y).val.reshape(-1))
    print(tag, "lowered adjoint", err)
    assert err < 1e-13
