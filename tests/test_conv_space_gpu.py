"""GPU: FuncConvolutionOperator on one space of a two-space domain
(nft_conv_space_*, csrc/nft_conv.hip) against the reference's values
(tests/golden/conv_space.npz, gen_golden_conv_space.py), alone and inside
likelihoods on a product-spectrum field over RGSpace((8, 8), 0.1) x
RGSpace(8, 0.5) (the carry grid: the product core's cg_blocks(1) > 0 there):
  a  GaussianEnergy(d, 1 / 1e-2) @ C(sigmoid(cf))
  b  PoissonianEnergy(counts) @ Mask(Exposure(C(exp(cf))))
  c  a + b as lh1 + lh2

Case by case the tests of test_conv_gpu.py.  s8512e10: the 512-point axis-1
pass has the fewest lines per tile, L = 256 * 8 / 512 = 4; inner = 5 exceeds
it and is no multiple of it, so a tile spans two pixels of S and the last
tile of a vector is partial.

Tolerances: operator against the reference 1e-12 relative max-norm, the total
sum kept to 1e-13, the per-slice sums against the stored ones 1e-12 (a
per-slice "zero-mode gain 1" implementation misses these by (1 - k0) times a
slice mean); native against the two-transform path and folded scales against
torch multiplies 1e-13; the quadratic form 1e-12; batches bitwise;
likelihoods: energy, transformation and metric 1e-12, 5 CG steps 1e-9, samples
1e-8.

The fixture stores a MultiField as one vector: its keys in sorted order, each
raveled."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from test_conv_space import FALLBACK, NATIVE, case_kernels, domain, kernels
from test_product import maker, unpack

pytestmark = pytest.mark.gpu

CASES = ("a", "b", "c")
TAG_KERNELS = [(t, k) for t in NATIVE + FALLBACK for k in (("g", "k") if t not in ("s8512e10", "s10248e2") else ("g",))]
_OPS, _CACHE = {}, {}


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


def trel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


def operator(ift, tag, kn):
    """(domain, operator, input Field, fixture, axes of S), built once per case"""
    if (tag, kn) not in _OPS:
        G = golden("conv_space.npz")
        assert kn in case_kernels(G, tag)
        dom, S, space = domain(ift, G, tag)
        C = ift.FuncConvolutionOperator.on_space(dom, kernels(S)[kn], space=space)
        x = 0.7 + np.random.default_rng(int(G[tag + "_seed"])).standard_normal(dom.shape)
        _OPS[(tag, kn)] = (dom, C, ift.makeField(dom, x), G, dom.axes[space])
    return _OPS[(tag, kn)]


# ---------------------------------------------------------------- operator
def test_native_and_fallback_tags(ift):
    from nifty_amd import _native
    for tag in NATIVE:
        C = operator(ift, tag, "g")[1]
        assert C.native and C.conv_plan() is not None
        assert C.quad_blocks() == _native.conv_space_quad_blocks(C.conv_plan()) >= 1
    for tag in FALLBACK:
        C = operator(ift, tag, "g")[1]
        assert not C.native and C.quad_blocks() == 1
    # the smallest-L case: 4 lines per tile, 8 * 5 lines per vector
    assert operator(ift, "s8512e10", "g")[1].quad_blocks() == 10


@pytest.mark.parametrize("tag,kn", TAG_KERNELS)
def test_times_and_adjoint_match_reference(ift, tag, kn):
    dom, C, x, G, axes = operator(ift, tag, kn)
    ref = G[f"{tag}_{kn}_Cx"]
    for name, y in (("times", C(x)), ("adjoint", C.adjoint_times(x))):
        err = relmax(y.val.cpu().numpy(), ref)
        print(tag, kn, name, err)
        assert err < 1e-12
    y = C(x).val
    # the total sum is kept
    s, s0 = y.sum().item(), x.val.sum().item()
    print(tag, kn, "sum", abs(s - s0) / abs(s0))
    assert abs(s - s0) <= 1e-13 * abs(s0)
    # the per-slice sums are the reference's (not those of x: k0 != 1)
    err = relmax(y.sum(dim=axes).cpu().numpy(), G[f"{tag}_{kn}_slicesums"])
    print(tag, kn, "slice sums", err)
    assert err < 1e-12


def test_complex_field_part_by_part(ift):
    dom, C, x, G, axes = operator(ift, "s88e4", "g")
    z = ift.Field(x.domain, x.val * (1 + 0j) + 1j * x.val.flip(0))
    y = C(z)
    assert trel(y.val.real, C(x).val) < 1e-14
    assert trel(y.val.imag, C(ift.Field(x.domain, x.val.flip(0).contiguous())).val) < 1e-14


@pytest.mark.parametrize("tag,kn", [tk for tk in TAG_KERNELS if tk[0] in NATIVE])
def test_native_matches_two_transform_path(ift, tag, kn, monkeypatch):
    dom, C, x, G, axes = operator(ift, tag, kn)
    nat = C(x).val
    monkeypatch.setenv("NFT_CONV_NATIVE", "0")
    assert not C.native
    fb = C(x).val
    monkeypatch.delenv("NFT_CONV_NATIVE")
    assert C.native
    err = trel(nat, fb)
    print(tag, kn, "native vs two transforms", err)
    assert err < 1e-13


def _batch_kernel(tag):
    return "k" if tag not in ("s8512e10", "s10248e2") else "g"


@pytest.mark.parametrize("tag", NATIVE)
def test_batches_are_bitwise_the_single_call(ift, tag, dev):
    """1, 3, 5 and 9 vectors (9 crosses the CONV_KMAX chunk) with padded row
    strides: bitwise the single calls, the mean term and the qpart rows
    included; the padding of out and qpart untouched"""
    from nifty_amd import _native
    dom, C, x, G, axes = operator(ift, tag, _batch_kernel(tag))
    assert _native.CONV_KMAX == 8
    npix = x.val.numel()
    nq = C.quad_blocks()
    assert nq >= 1
    g = torch.Generator(device="cpu").manual_seed(3)
    col = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    row = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    big = torch.randn((9, npix + 24), generator=g, dtype=torch.float64).to(dev)
    single, qsingle = [], []
    for v in range(9):
        q = torch.zeros((1, nq), dtype=torch.float64, device=dev)
        single.append(C.apply_rows(big[v:v + 1, :npix].contiguous(), colscale=col, rowscale=row, scale=0.3, qpart=q))
        qsingle.append(q)
    for k in (1, 3, 5, 9):
        X = big[:k, :npix]                  # row stride npix + 24
        assert k == 1 or not X.is_contiguous()
        outbuf = torch.zeros((k, npix + 8), dtype=torch.float64, device=dev)
        q = torch.zeros((k, nq + 3), dtype=torch.float64, device=dev)
        Y = C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q[:, :nq], out=outbuf[:, :npix])
        assert not outbuf[:, npix:].any() and not q[:, nq:].any()
        for v in range(k):
            assert torch.equal(Y[v], single[v][0]), (k, v)
            assert torch.equal(q[v, :nq], qsingle[v][0]), (k, v)


def test_odd_row_strides_are_bitwise_too(ift, dev):
    """an odd row stride puts every second vector off the 16-byte grid: the
    8-byte accesses give the same bits"""
    dom, C, x, G, axes = operator(ift, "s88e6", "k")
    npix = x.val.numel()
    nq = C.quad_blocks()
    g = torch.Generator(device="cpu").manual_seed(5)
    col = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    big = torch.randn((3, npix + 25), generator=g, dtype=torch.float64).to(dev)
    outbuf = torch.zeros((3, npix + 7), dtype=torch.float64, device=dev)
    q = torch.zeros((3, nq), dtype=torch.float64, device=dev)
    Y = C.apply_rows(big[:, :npix], colscale=col, scale=0.3, qpart=q, out=outbuf[:, :npix])
    assert not outbuf[:, npix:].any()
    for v in range(3):
        q1 = torch.zeros((1, nq), dtype=torch.float64, device=dev)
        y1 = C.apply_rows(big[v:v + 1, :npix].contiguous(), colscale=col, scale=0.3, qpart=q1)
        assert torch.equal(Y[v], y1[0]) and torch.equal(q[v], q1[0]), v


@pytest.mark.parametrize("tag", NATIVE)
def test_folded_scales_and_quadratic_form(ift, tag, dev):
    """signed scales; the mean in C is that of colscale * x"""
    dom, C, x, G, axes = operator(ift, tag, "g")
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


def test_argument_errors(ift, dev):
    from nifty_amd import _native
    lib = _native.load()
    n0, n1, ne = 8, 8, 4
    npix = n0 * n1 * ne
    x = torch.ones((1, npix), dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    table = torch.full((n0, n1), 1. / (n0 * n1), dtype=torch.float64, device=dev)
    ws = torch.zeros(1 << 16, dtype=torch.uint8, device=dev)
    q = torch.zeros((1, 8), dtype=torch.float64, device=dev)

    def call(plan, xp=x, xs=npix, yp=y, ys=npix, nvec=1, dtype=0, qp=None, qs=0, wsp=ws, wsb=None):
        return lib.nft_conv_space_apply_batched(ctypes.byref(plan), _native.ptr(xp), xs, None, _native.ptr(yp), ys,
                                                None, 1.0, nvec, dtype, _native.ptr(qp), qs, _native.ptr(wsp),
                                                ctypes.c_size_t(ws.numel() if wsb is None else wsb),
                                                _native.stream_ptr())
    good = _native.conv_space_plan(n0, n1, ne, table, 1.0)
    need = lib.nft_conv_space_workspace(ctypes.byref(good), 1)
    nq = lib.nft_conv_space_quad_blocks(ctypes.byref(good))
    assert 0 < need <= ws.numel() and nq == 1
    assert call(good, qp=q, qs=nq) == 0
    torch.cuda.synchronize()
    assert trel(y, x) < 1e-14       # all gains 1, k0 = 1: the identity
    assert abs(q[0, 0].item() - npix) < 1e-12 * npix and not q[0, 1:].any()
    ARG, UNSUPPORTED = -1, -2               # NFT_ERR_ARG, NFT_ERR_UNSUPPORTED
    assert call(_native.conv_space_plan(n0, 6, ne, table[:, :6].contiguous(), 1.0)) == UNSUPPORTED
    for field in ("n0", "n1", "inner"):
        p = _native.conv_space_plan(n0, n1, ne, table, 1.0)
        setattr(p, field, 0)
        assert call(p) == ARG, field
    p = _native.conv_space_plan(n0, n1, ne, table, 1.0)
    p.table = None
    assert call(p) == ARG
    assert lib.nft_conv_space_workspace(ctypes.byref(p), 1) == 0
    assert lib.nft_conv_space_quad_blocks(ctypes.byref(p)) == 0
    assert call(good, xp=None) == ARG and call(good, yp=None) == ARG and call(good, nvec=0) == ARG
    assert call(good, xs=npix - 1) == ARG and call(good, ys=npix - 1) == ARG
    assert call(good, wsp=None) == ARG and call(good, wsb=need - 1) == ARG
    assert call(good, qp=q, qs=nq - 1) == ARG
    assert call(good, dtype=1) == UNSUPPORTED
    torch.cuda.synchronize()


def test_captured_batch_replays_bitwise(ift, dev):
    dom, C, x, G, axes = operator(ift, "s88e6", "k")
    npix = x.val.numel()
    nq = C.quad_blocks()
    g = torch.Generator(device="cpu").manual_seed(6)
    col = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    row = torch.rand(npix, generator=g, dtype=torch.float64).to(dev) + 0.5
    X = torch.randn((3, npix), generator=g, dtype=torch.float64).to(dev)
    q0 = torch.zeros((3, nq), dtype=torch.float64, device=dev)
    eager = C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q0)    # also warms the workspace
    out = torch.zeros_like(eager)
    q = torch.zeros_like(q0)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        C.apply_rows(X, colscale=col, rowscale=row, scale=0.3, qpart=q, out=out)
    for _ in range(2):
        out.zero_()
        q.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, eager) and torch.equal(q, q0)


# -------------------------------------------------------------- likelihoods
def pack(mf):
    return np.concatenate([mf[k].val.cpu().numpy().reshape(-1) for k in sorted(mf.keys())])


def build(ift, G, fused=True):
    """(cf, {a, b, c: likelihood}, response of b) on the fused field or on the
    operator tree of the same maker"""
    tag = "n8"
    n = int(G["carry_grid"])
    cfm = maker(ift, ((n, n), 0.1), ((8,), 0.5))
    if not fused:
        cfm._fusable = lambda: False
    cf = cfm.finalize(prior_info=0)
    dom = cf.target
    C = ift.FuncConvolutionOperator.on_space(dom, kernels(dom[0])["g"], space=0)
    M = ift.MaskOperator(ift.makeField(dom, G[tag + "_flags"]))
    E = ift.DiagonalOperator(ift.makeField(dom, G[tag + "_expo"]))
    N = ift.ScalingOperator(dom, 1e-2, np.float64)
    lh1 = ift.GaussianEnergy(ift.makeField(dom, G[tag + "_data"]), inverse_covariance=N.inverse) @ C(ift.sigmoid(cf))
    lh2 = ift.PoissonianEnergy(ift.makeField(M.target, G[tag + "_counts"])) @ M(E(C(cf.exp())))
    lh1.name, lh2.name = (str(v) for v in G["names"])
    return cf, dict(a=lh1, b=lh2, c=lh1 + lh2), M @ E @ C


def problem(ift):
    """(cf, likelihoods, pos, t, G, response of b), built once"""
    if "p" not in _CACHE:
        G = golden("conv_space.npz")
        assert int(G["carry_grid"]) == 8
        for c in CASES:
            assert float(G[f"n8{c}_cond"]) < 1e-12
        cf, lhs, resp = build(ift, G)
        _CACHE["p"] = (cf, lhs, unpack(ift, cf.domain, G["n8_pos"]), unpack(ift, cf.domain, G["n8_t"]), G, resp)
    return _CACHE["p"]


@pytest.mark.parametrize("c", CASES)
def test_golden_energy_transformation_metric(ift, c):
    cf, lhs, pos, t, G, resp = problem(ift)
    lh, pre = lhs[c], "n8" + c
    e = lh(pos).val.item()
    print(pre, "energy", abs(e - float(G[pre + "_energy"])) / abs(float(G[pre + "_energy"])))
    assert abs(e - float(G[pre + "_energy"])) < 1e-12 * abs(float(G[pre + "_energy"]))
    dtype, f = lh.get_transformation()
    tr = f(pos)
    trv = pack(tr) if isinstance(tr, ift.MultiField) else tr.val.cpu().numpy().reshape(-1)
    err = relmax(trv, G[pre + "_tr"])
    print(pre, "transformation", err)
    assert err < 1e-12
    met = lh.get_metric_at(pos)
    assert met.fused is not None
    ref = unpack(ift, cf.domain, G[pre + "_mt"])
    mt = met(t)
    for k in cf.domain.keys():
        err = relmax(mt[k].val.cpu().numpy(), ref[k].val.cpu().numpy())
        print(pre, "metric", k, err)
        assert err < 1e-12, k


@pytest.mark.parametrize("c", CASES)
def test_five_cg_steps(ift, c):
    cf, lhs, pos, t, G, resp = problem(ift)
    A = lhs[c].get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        en, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
        assert st == ic.CONVERGED
        ref = unpack(ift, cf.domain, G[f"n8{c}_cg{it}"])
        for k in cf.domain.keys():
            err = rel(en.position[k].val.cpu().numpy(), ref[k].val.cpu().numpy())
            print(c, it, "CG steps", k, err)
            assert err < 1e-9, (it, k)


def test_middle_of_b(ift, dev):
    from nifty_amd import _native
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G, resp = problem(ift)
    A = lhs["b"].get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0 and core.cg_blocks(1) > 0
    assert callable(W) and W.supports_batch and not W.supports_fp32 and not W.supports_fold
    assert W.response.native
    assert W.quad_blocks == _native.conv_space_quad_blocks(W.conv_plan) > 0
    assert not hasattr(W, "plan") and not hasattr(W, "scales")
    with pytest.raises(NotImplementedError):
        W(torch.zeros(cf.target.shape, dtype=torch.float64, device=dev), fold=object())
    dr, cv = W.conv_scales(torch.float64)
    flags = torch.from_numpy(G["n8_flags"]).to(cv.device).reshape(-1)
    assert dr is not None and cv.dtype == torch.float64
    assert not cv[flags].any() and (cv[~flags] > 0).all()


def _rhs(ift, cf, n):
    out = []
    for i in range(n):
        with ift.random.Context(40 + i):
            out.append(ift.from_random(cf.domain, "normal"))
    return out


def test_batched_solve_is_carried_bitwise_single_and_matches_the_operator_tree(ift):
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G, resp = problem(ift)
    one = ift.ScalingOperator(cf.domain, 1., float)
    A = lhs["b"].get_metric_at(pos) + one
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0 and W.quad_blocks > 0
    bs = _rhs(ift, cf, 4)
    es = [ift.QuadraticEnergy(0 * b, A, b) for b in bs]
    single = [fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5)).run(e) for e in es]
    cg = fused_cg.FusedCGBatch(core, W, shift, [ift.GradientNormController(iteration_limit=5) for _ in es])
    bat = cg.run(es)
    assert cg.path == "carry+chunk", cg.path
    assert fused_cg._carry_flavour(core, 1) == "seg"
    for (e1, s1), (e2, s2) in zip(single, bat):
        assert s1 == s2
        for k in cf.domain.keys():
            assert torch.equal(e1.position[k].val, e2.position[k].val), k
    # the same model built on the operator tree
    tree, tlhs, _ = build(ift, G, fused=False)
    assert isinstance(cf, _FusedFieldBase) and not isinstance(tree, _FusedFieldBase)
    assert tree.domain is cf.domain
    At = tlhs["b"].get_metric_at(pos) + one
    for b, (eb, sb) in zip(bs, bat):
        ic = ift.GradientNormController(iteration_limit=5)
        ep, sp_ = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * b, At, b))
        assert sp_ == sb
        for k in cf.domain.keys():
            err = rel(eb.position[k].val.cpu().numpy(), ep.position[k].val.cpu().numpy())
            print("5 CG steps, fused vs operator tree", k, err)
            assert err < 1e-9, k


def test_fp32_request_leaves_the_solve_in_fp64(ift):
    from nifty_amd import config
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G, resp = problem(ift)
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
    cf, lhs, pos, t, G, resp = problem(ift)
    H = ift.StandardHamiltonian(lhs["b"], ift.AbsDeltaEnergyController(deltaE=1e-30, iteration_limit=10))
    ift.random.push_sseq_from_seed(27)
    sl = ift.draw_samples(pos, H, None, 1, True)
    ift.random.pop_sseq()
    ref = G["n8b_mgvi_samples"]
    assert sl.n_samples == len(ref) == 2
    for i in range(2):
        err = rel(pack(sl.local_item(i)), ref[i])
        print("MGVI sample", i, err)
        assert err < 1e-8, i


def test_lowered_response_matches_operators(ift):
    from nifty_amd.lowering import lower
    cf, lhs, pos, t, G, resp = problem(ift)
    fwd, adj = lower(resp), lower(resp, adjoint=True)
    assert fwd is not None and adj is not None
    with ift.random.Context(9):
        x = ift.from_random(resp.domain, "normal")
        y = ift.from_random(resp.target, "normal")
    err = trel(fwd(x.val).reshape(-1), resp(x).val.reshape(-1))
    print("lowered response", err)
    assert err < 1e-13
    err = trel(adj(y.val).reshape(-1), resp.adjoint_times(y).val.reshape(-1))
    print("lowered adjoint", err)
    assert err < 1e-13
