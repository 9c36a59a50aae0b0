"""GPU: the product-spectrum kernels (csrc/nft_prod.hip) against torch
restatements, and the fused product field (library/product.py) through the
public interface against the reference (tests/golden/product.npz,
gen_golden_product.py) and against the operator tree of the same maker.

Tolerances (fp64):
  nft_mirror_mix against the same-order torch restatement   bitwise
  R R x against x                                            rel 1e-14
  table kernels against torch                               rel 1e-13 (a handful of
      products per entry; the sums of the VJP against their own condition:
      1e-13 of sum |terms|)
  batched against single                                    bitwise
  value, J t, J^T g, amplitudes vs fixture                  1e-10  (test_matern_gpu.py)
  fused field against the operator tree                     1e-11
  metric application vs fixture                             1e-12
  5 CG steps vs fixture / vs the tree, per key              1e-9
  geoVI draw vs fixture                                     1e-8
The fixture's conditioning bound (<case>_cond < 1e-12) is checked here too.

Table sizes: the (B1, B2) of the golden cases, (65, 33) of RGSpace(128) x
RGSpace(64) (5 row tiles of 16, no multiple of the 16 x 256 tile) and (3, 513)
of RGSpace(4) x RGSpace(1024) (3 column tiles)."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from test_product import CASES, COMP_A, COMP_B, maker, unpack

pytestmark = pytest.mark.gpu

P = ctypes.c_void_p


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


def rel(a, b):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    nb = np.linalg.norm(b)
    return np.linalg.norm(a - b) / (nb if nb > 0 else 1.)


def pack(mf):
    return np.concatenate([mf[k].val.cpu().numpy().reshape(-1) for k in sorted(mf.keys())])


def randn(shape, seed, dev, dtype=torch.float64):
    return torch.randn(shape, dtype=torch.float64, generator=torch.Generator().manual_seed(seed)).to(dtype).to(dev)


# --------------------------------------------------------------- mirror mix
def t_mirror(x, axes):
    for a in axes:
        x = torch.roll(torch.flip(x, (a,)), 1, a)
    return x


def t_mix(x, split):
    """R on the trailing grid axes of x (leading axis: rows), the kernel's order"""
    nd = x.ndim - 1
    g1, g2 = tuple(range(1, 1 + split)), tuple(range(1 + split, 1 + nd))
    return ((x + t_mirror(x, g1)) + t_mirror(x, g2) - t_mirror(x, g1 + g2)) * 0.5


MIX_SHAPES = [((16, 8), 1), ((8, 8, 4), 2), ((4, 8, 8), 1), ((6, 5), 1), ((2, 2), 1), ((1, 8), 1), ((64, 64), 1)]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("shape,split", MIX_SHAPES)
def test_mirror_mix_bitwise(dev, shape, split, k, dtype):
    from nifty_amd import _native
    N = int(np.prod(shape))
    stride = N + 5                                   # rows wider than the grid
    buf = randn((k, stride), 1, dev, dtype)
    x = buf[:, :N].reshape((k,) + shape)
    want = t_mix(x, split)
    out = torch.full((k, stride), 7.0, dtype=dtype, device=dev)
    _native.mirror_mix(buf, out, shape, split, rows=k, x_stride=stride, y_stride=stride)
    assert torch.equal(out[:, :N].reshape(want.shape), want)
    assert bool((out[:, N:] == 7.0).all())
    # in place, and once more: R is an involution
    inp = buf.clone()
    _native.mirror_mix(inp, inp, shape, split, rows=k, x_stride=stride, y_stride=stride)
    assert torch.equal(inp[:, :N].reshape(want.shape), want)
    assert torch.equal(inp[:, N:], buf[:, N:])
    _native.mirror_mix(inp, inp, shape, split, rows=k, x_stride=stride, y_stride=stride)
    eps = 1e-14 if dtype == torch.float64 else 1e-6
    assert rel(inp[:, :N], buf[:, :N]) < eps


def test_mirror_mix_argument_checks(dev):
    from nifty_amd import _native
    lib = _native.load()
    x = torch.zeros((2, 32), dtype=torch.float64, device=dev)
    y = torch.zeros_like(x)
    s = _native.stream_ptr()

    def mm(xp=x, yp=y, xs=32, ys=32, rows=2, shape=(4, 8), split=1, dt=0):
        sh = (ctypes.c_int64 * len(shape))(*shape)
        return lib.nft_mirror_mix(P(xp.data_ptr()) if xp is not None else None, xs,
                                  P(yp.data_ptr()) if yp is not None else None, ys, rows, len(shape), sh, split, dt, s)
    assert mm() == 0
    assert mm(xp=None) == -1 and mm(yp=None) == -1 and mm(rows=0) == -1 and mm(dt=2) == -1
    assert mm(split=0) == -1 and mm(split=2) == -1 and mm(shape=(32,)) == -1 and mm(shape=(2, 2, 2, 4), split=2) == -1
    assert mm(shape=(4, 0)) == -1
    assert mm(ys=31) == -1 and mm(xs=31) == -1           # rows overlap
    assert mm(yp=x, ys=32, xs=32) == 0 and mm(yp=x, ys=40, xs=32, rows=1) == -1
    assert b"nft_mirror_mix" in lib.nft_last_error()
    torch.cuda.synchronize()


# ------------------------------------------------------------ table kernels
TABLES = {"p16x8": (9, 5), "p8x8x4": (15, 3), "p4x8x8": (3, 15), "p6x5": (4, 3), "p64x64": (33, 33),
          "x128x64": (65, 33), "x4x1024": (3, 513)}
SC = (6.0, 1.5, 4.0)        # s0, s1, s2
ZM = (-1.2, 0.3)            # lm_o, ls_o


def table_inputs(tag, dev, nitem=3):
    B1, B2 = TABLES[tag]
    m1 = torch.exp(0.5 * randn((nitem, B1 + 3), 11, dev))      # rows wider than B_i
    m2 = torch.exp(0.5 * randn((nitem, B2 + 1), 12, dev))
    xz = randn((nitem, 7), 13, dev)                             # the zero-mode key of packed rows
    return B1, B2, m1, m2, xz


def forward(dev, B1, B2, m1, m2, xz, nitem):
    from nifty_amd import _native
    lib = _native.load()
    nc = int(lib.nft_prod_const_size(B1, B2))
    assert nc == 2 + (B1 + 1) // 2 * 2 + (B2 + 1) // 2 * 2
    A = torch.full((nitem, B1 * B2 + 2), 7.0, dtype=torch.float64, device=dev)
    cb = torch.zeros((nitem, nc), dtype=torch.float64, device=dev)
    _native._check(lib.nft_prod_forward(B1, B2, P(m1.data_ptr()), m1.stride(0), P(m2.data_ptr()), m2.stride(0),
                                        P(xz[:, 2:].data_ptr()), xz.stride(0), ZM[0], ZM[1], *SC, nitem,
                                        P(A.data_ptr()), A.stride(0), P(cb.data_ptr()), nc, _native.stream_ptr()))
    return A, cb


def t_forward(B1, B2, m1, m2, xz, r):
    """(table, z, p1, p2) of item r in torch"""
    z = SC[0] * torch.exp(ZM[0] + ZM[1] * xz[r, 2])
    a1, a2 = SC[1] * m1[r, :B1], SC[2] * m2[r, :B2]
    A = torch.outer(a1, a2) / z
    A[:, 0], A[0, :] = a1, a2
    A[0, 0] = z
    p1, p2 = a1 / z, a2 / z
    p1[0] = p2[0] = 0.
    return A.reshape(-1), z, p1, p2


@pytest.mark.parametrize("tag", list(TABLES))
def test_prod_forward_against_torch(dev, tag):
    B1, B2, m1, m2, xz = table_inputs(tag, dev)
    A, cb = forward(dev, B1, B2, m1, m2, xz, 3)
    o2 = 2 + (B1 + 1) // 2 * 2
    for r in range(3):
        want, z, p1, p2 = t_forward(B1, B2, m1, m2, xz, r)
        assert rel(A[r, :B1 * B2], want) < 1e-13
        assert float((A[r, :B1 * B2] / want - 1).abs().max()) < 1e-13
        assert bool((A[r, B1 * B2:] == 7.0).all())
        assert rel(cb[r, :2], torch.stack([z, z * ZM[1]])) < 1e-13
        assert rel(cb[r, 2:2 + B1], p1) < 1e-13 and rel(cb[r, o2:o2 + B2], p2) < 1e-13
        # batched is bitwise the single call
        A1, cb1 = forward(dev, B1, B2, m1[r:r + 1], m2[r:r + 1], xz[r:r + 1], 1)
        assert torch.equal(A1[0], A[r]) and torch.equal(cb1[0, :2 + B1], cb[r, :2 + B1])
        assert torch.equal(cb1[0, o2:o2 + B2], cb[r, o2:o2 + B2])


def _jvp(dev, B1, B2, cb, d1, d2, T, k):
    from nifty_amd import _native
    lib = _native.load()
    da = torch.full((B1 * B2 * k + 1,), 7.0, dtype=torch.float64, device=dev)
    _native._check(lib.nft_prod_jvp_batched(B1, B2, P(cb.data_ptr()), SC[1], SC[2], P(d1.data_ptr()), d1.stride(0),
                                            P(d2.data_ptr()), d2.stride(0), P(T[:, 2:].data_ptr()), T.stride(0),
                                            P(da.data_ptr()), k, _native.stream_ptr()))
    assert float(da[-1]) == 7.0
    return da[:-1].reshape(B1 * B2, k)


def _vjp(dev, B1, B2, cb, g, k, D=None, shift=0.0):
    from nifty_amd import _native
    lib = _native.load()
    g1 = torch.full((k, B1 + 2), 7.0, dtype=torch.float64, device=dev)
    g2 = torch.full((k, B2 + 2), 7.0, dtype=torch.float64, device=dev)
    Q = torch.full((k, 7), 7.0, dtype=torch.float64, device=dev)
    ws = torch.empty(k * int(lib.nft_prod_workspace(B1, B2)), dtype=torch.uint8, device=dev)
    _native._check(lib.nft_prod_vjp_batched(B1, B2, P(cb.data_ptr()), SC[1], SC[2], P(g.data_ptr()), g.stride(0),
                                            P(g1.data_ptr()), g1.stride(0), P(g2.data_ptr()), g2.stride(0),
                                            P(Q[:, 2:].data_ptr()), P(D[:, 2:].data_ptr()) if D is not None else None,
                                            7, shift, P(ws.data_ptr()), k, _native.stream_ptr()))
    assert bool((g1[:, B1:] == 7.0).all()) and bool((g2[:, B2:] == 7.0).all())
    assert bool((Q[:, :2] == 7.0).all()) and bool((Q[:, 3:] == 7.0).all())
    return g1[:, :B1], g2[:, :B2], Q[:, 2]


@pytest.mark.parametrize("k", [1, 4])
@pytest.mark.parametrize("tag", list(TABLES))
def test_prod_jvp_vjp_against_torch(dev, tag, k):
    B1, B2, m1, m2, xz = table_inputs(tag, dev, 1)
    _, cb = forward(dev, B1, B2, m1, m2, xz, 1)
    _, z, p1, p2 = t_forward(B1, B2, m1, m2, xz, 0)
    gz = z * ZM[1]
    d1, d2, T = randn((k, B1 + 1), 21, dev), randn((k, B2), 22, dev), randn((k, 7), 23, dev)
    da = _jvp(dev, B1, B2, cb[0], d1, d2, T, k)
    want = []
    for r in range(k):
        e1, e2, dz = SC[1] * d1[r, :B1], SC[2] * d2[r], gz * T[r, 2]
        w = torch.outer(e1, p2) + torch.outer(p1, e2) - torch.outer(p1, p2) * dz
        w[:, 0], w[0, :] = e1, e2
        w[0, 0] = dz
        want.append(w.reshape(-1))
        assert rel(da[:, r], want[r]) < 1e-13, r
        one = _jvp(dev, B1, B2, cb[0], d1[r:r + 1], d2[r:r + 1], T[r:r + 1], 1)
        assert torch.equal(one[:, 0], da[:, r]), r
    # the transpose
    g, D = randn((k, B1 * B2 + 3), 24, dev), randn((k, 7), 25, dev)
    w1, w2 = p1.clone(), p2.clone()
    w1[0] = w2[0] = 1.
    for shift in (0.0, 0.7):
        g1, g2, gq = _vjp(dev, B1, B2, cb[0], g, k, D, shift)
        for r in range(k):
            G = g[r, :B1 * B2].reshape(B1, B2)
            r1, r2 = SC[1] * (G @ w2), SC[2] * (w1 @ G)
            r1[0] = r2[0] = 0.
            assert rel(g1[r], r1) < 1e-13 and rel(g2[r], r2) < 1e-13, (r, shift)
            full = p1[1:] @ G[1:, 1:] @ p2[1:]
            wz = gz * (G[0, 0] - full) + shift * D[r, 2]
            cond = gz * (G[0, 0].abs() + p1[1:] @ G[1:, 1:].abs() @ p2[1:]) + abs(shift * D[r, 2])
            assert abs(float(gq[r] - wz)) <= 1e-13 * float(cond), (r, shift)
            # adjointness against the JVP of the same constants
            lhs = float(torch.dot(da[:, r], g[r, :B1 * B2]))
            rhs = float(torch.dot(d1[r, :B1], g1[r]) + torch.dot(d2[r], g2[r])) + float(T[r, 2] * (gq[r] - shift * D[r, 2]))
            scale = float(da[:, r].norm() * g[r, :B1 * B2].norm())
            assert abs(lhs - rhs) <= 1e-13 * scale, (r, shift)
            o1, o2, oq = _vjp(dev, B1, B2, cb[0], g[r:r + 1], 1, D[r:r + 1], shift)
            assert torch.equal(o1[0], g1[r]) and torch.equal(o2[0], g2[r]) and torch.equal(oq[0], gq[r]), (r, shift)


def test_prod_argument_checks(dev):
    from nifty_amd import _native
    lib = _native.load()
    B1, B2, m1, m2, xz = table_inputs("p16x8", dev, 2)
    A, cb = forward(dev, B1, B2, m1, m2, xz, 2)
    s = _native.stream_ptr()
    nc = cb.shape[1]

    def fwd(b1=B1, m=m1, n=2, As=A.stride(0), cs=nc, s0=SC[0], out=A):
        return lib.nft_prod_forward(b1, B2, P(m.data_ptr()) if m is not None else None, m1.stride(0),
                                    P(m2.data_ptr()), m2.stride(0), P(xz.data_ptr()), 7, ZM[0], ZM[1], s0, SC[1], SC[2],
                                    n, P(out.data_ptr()) if out is not None else None, As, P(cb.data_ptr()), cs, s)
    assert fwd() == 0
    assert fwd(b1=1) == -1 and fwd(m=None) == -1 and fwd(n=0) == -1 and fwd(out=None) == -1 and fwd(s0=0.0) == -1
    assert fwd(As=B1 * B2 - 1) == -1 and fwd(cs=nc - 1) == -1
    assert b"nft_prod_forward" in lib.nft_last_error()
    d1, d2, T = randn((2, B1), 1, dev), randn((2, B2), 2, dev), randn((2, 7), 3, dev)
    da = torch.zeros(B1 * B2 * 2, dtype=torch.float64, device=dev)

    def jvp(b2=B2, c=cb, d=d1, ds=B1, n=2, o=da):
        return lib.nft_prod_jvp_batched(B1, b2, P(c.data_ptr()) if c is not None else None, SC[1], SC[2],
                                        P(d.data_ptr()) if d is not None else None, ds, P(d2.data_ptr()), B2,
                                        P(T.data_ptr()), 7, P(o.data_ptr()) if o is not None else None, n, s)
    assert jvp() == 0
    assert jvp(b2=1) == -1 and jvp(c=None) == -1 and jvp(d=None) == -1 and jvp(o=None) == -1 and jvp(n=0) == -1
    assert jvp(ds=B1 - 1) == -1
    assert b"nft_prod_jvp_batched" in lib.nft_last_error()
    g = torch.zeros((2, B1 * B2), dtype=torch.float64, device=dev)
    g1, g2 = torch.zeros((2, B1), dtype=torch.float64, device=dev), torch.zeros((2, B2), dtype=torch.float64, device=dev)
    Q = torch.zeros((2, 7), dtype=torch.float64, device=dev)
    ws = torch.empty(2 * int(lib.nft_prod_workspace(B1, B2)), dtype=torch.uint8, device=dev)

    def vjp(gs=B1 * B2, g1s=B1, ls=7, n=2, w=ws, gg=g, oz=Q):
        return lib.nft_prod_vjp_batched(B1, B2, P(cb.data_ptr()), SC[1], SC[2], P(gg.data_ptr()) if gg is not None else
                                        None, gs, P(g1.data_ptr()), g1s, P(g2.data_ptr()), B2,
                                        P(oz.data_ptr()) if oz is not None else None, None, ls, 0.0,
                                        P(w.data_ptr()) if w is not None else None, n, s)
    assert vjp() == 0
    assert vjp(gs=B1 * B2 - 1) == -1 and vjp(g1s=B1 - 1) == -1 and vjp(ls=0) == -1 and vjp(n=0) == -1
    assert vjp(w=None) == -1 and vjp(gg=None) == -1 and vjp(oz=None) == -1
    assert b"nft_prod_vjp_batched" in lib.nft_last_error()
    assert lib.nft_prod_workspace(1, 5) == 0 and lib.nft_prod_const_size(5, 1) == 0
    torch.cuda.synchronize()


@pytest.mark.parametrize("tag", ["p16x8", "p4x8x8", "p64x64"])
def test_amplitude_model_native_against_torch(ift, dev, tag):
    """_ProductAmplitudeModel's native passes (the components' nft_amp kernels
    composed with the table's) against its torch restatement; 1e-12 as the
    component kernels' own tests (test_amp2_gpu.py)"""
    op = maker(ift, *CASES[tag]).finalize(prior_info=0)
    amp, G = op.amp, golden("product.npz")
    pos = unpack(ift, op.domain, G[tag + "_pos"])
    lat = {k: pos[k].val for k in op.domain.keys()}
    a, c = amp.forward(lat)
    lin = amp.forward_native(lat)
    assert rel(lin.a[0], a) < 1e-12
    lay = op.layout
    off = dict(zip(lay.keys, lay.offsets))
    k = 4
    D = randn((k, lay.size), 31, dev)
    da = torch.empty((amp.B, k), dtype=torch.float64, device=dev)
    amp.native_jvp_batched(lin, D, off, da, interleave=True)
    g = randn((k, amp.B), 32, dev)
    Q = torch.zeros((k, lay.size), dtype=torch.float64, device=dev)
    amp.native_vjp_batched(lin, g, Q, off, D=D, shift=0.5)
    for r in range(k):
        t = lay.views(D[r])
        assert rel(da[:, r], amp.jvp(c, {kk: t[kk] for kk in amp.domain_dict})) < 1e-12
        ref = amp.vjp(c, g[r])
        got, q = lay.views(Q[r]), lay.views(D[r])
        want = np.concatenate([(ref[kk].reshape(-1) + 0.5 * q[kk].reshape(-1)).cpu().numpy() for kk in amp.domain_dict])
        have = np.concatenate([got[kk].reshape(-1).cpu().numpy() for kk in amp.domain_dict])
        assert rel(have, want) < 1e-12, r
        assert not got[op.k_xi].any()


# -------------------------------------------------------------------- field
def _lin(ift, op, x):
    return op(ift.Linearization.make_var(x))


@pytest.mark.parametrize("tag", list(CASES))
def test_field_against_reference_and_operator_tree(ift, tag):
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase
    from nifty_amd.library.product import _ProductFieldModel
    G = golden("product.npz")
    cfm = maker(ift, *CASES[tag])
    op = cfm.finalize(prior_info=0)
    assert isinstance(op, _ProductFieldModel)
    x, t = unpack(ift, op.domain, G[tag + "_pos"]), unpack(ift, op.domain, G[tag + "_t"])
    g = ift.makeField(op.target, G[tag + "_g"])
    lin = _lin(ift, op, x)
    assert rel(lin.val.val, G[tag + "_val"]) < 1e-10
    assert rel(op(x).val, G[tag + "_val"]) < 1e-10
    assert rel(lin.jac(t).val, G[tag + "_jt"]) < 1e-10
    ja = lin.jac.adjoint(g)
    ref = unpack(ift, op.domain, G[tag + "_ja"])
    for k in op.domain.keys():
        assert rel(ja[k].val, ref[k].val) < 1e-10, k
    for i, na in enumerate(cfm.get_normalized_amplitudes()):
        assert rel(na.force(x).val, G[f"{tag}_na{i}"]) < 1e-10
    # the reference's operator tree from the same maker
    cfm._fusable = lambda: False
    tree = cfm.finalize(prior_info=0)
    assert not isinstance(tree, _FusedFieldBase)
    assert tree.domain is op.domain
    lt = _lin(ift, tree, x)
    assert rel(lin.val.val, lt.val.val) < 1e-11
    assert rel(lin.jac(t).val, lt.jac(t).val) < 1e-11
    jt = lt.jac.adjoint(g)
    for k in op.domain.keys():
        assert rel(ja[k].val, jt[k].val) < 1e-11, k


# ------------------------------------------------------------ metric and CG
METRIC = ["p16x8", "p8x8x4", "p64x64"]
_PROBLEMS = {}


def problem(ift, tag):
    """(cf, likelihood, pos, t, G) of a metric case, built once"""
    if tag not in _PROBLEMS:
        G = golden("product.npz")
        assert tag in [str(c) for c in G["metric_cases"]]
        assert float(G[tag + "_cond"]) < 1e-12
        cf = maker(ift, *CASES[tag]).finalize(prior_info=0)
        N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
        lh = ift.GaussianEnergy(ift.makeField(cf.target, G[tag + "_data"]), inverse_covariance=N.inverse) @ ift.sigmoid(cf)
        _PROBLEMS[tag] = (cf, lh, unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"]), G)
    return _PROBLEMS[tag]


def _metric(ift, tag):
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    return (A,) + fused_cg.fusable_metric(A)


@pytest.mark.parametrize("tag", METRIC)
def test_metric_against_reference(ift, tag):
    cf, lh, pos, t, G = problem(ift, tag)
    met = lh.get_metric_at(pos)
    assert met.fused is not None
    got, ref = met(t), unpack(ift, cf.domain, G[tag + "_mt"])
    for k in cf.domain.keys():
        assert rel(got[k].val, ref[k].val) < 1e-12, k


def _matern_path(ift, tag, G):
    """cg.path of a one-space Matern field on an RGSpace of the joint grid
    shape under the same likelihood and controller"""
    from nifty_amd.minimization import fused_cg
    sp = ift.RGSpace(G[tag + "_val"].shape, distances=0.3)
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(sp, (1., 0.3), (2., 0.5), (-3., 0.5))
    cfm.set_amplitude_total_offset(1., (0.3, 0.1))
    cf = cfm.finalize(prior_info=0)
    N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
    lh = ift.GaussianEnergy(ift.makeField(sp, G[tag + "_data"]), inverse_covariance=N.inverse) @ ift.sigmoid(cf)
    with ift.random.Context(3):
        pos = 0.3 * ift.from_random(cf.domain, "normal")
        t = ift.from_random(cf.domain, "normal")
    A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5))
    cg.run(ift.QuadraticEnergy(0 * t, A, t))
    return cg.path, core.cg_blocks(1)


@pytest.mark.parametrize("tag", METRIC)
def test_five_cg_steps(ift, tag):
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A, core, W, shift = _metric(ift, tag)
    assert shift == 1.0
    cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5))
    cg.run(ift.QuadraticEnergy(0 * t, A, t))
    mpath, mblocks = _matern_path(ift, tag, G)
    assert cg.path == mpath, (cg.path, mpath)
    assert core.cg_blocks(1) == mblocks
    if tag in ("p16x8", "p64x64"):
        assert core.cg_blocks(1) > 0
    if core.cg_blocks(1) > 0:
        assert fused_cg._carry_flavour(core, 1) == "seg" and cg.path == "carry+chunk", cg.path
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        en, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
        assert st == ic.CONVERGED
        ref = unpack(ift, cf.domain, G[f"{tag}_cg{it}"])
        for k in cf.domain.keys():
            err = rel(en.position[k].val, ref[k].val)
            print(tag, it, "CG steps", k, err)
            assert err < 1e-9, (it, k)


def _rhs(ift, cf, n):
    out = []
    for i in range(n):
        with ift.random.Context(40 + i):
            out.append(ift.from_random(cf.domain, "normal"))
    return out


@pytest.mark.parametrize("tag", METRIC)
def test_batched_solve_is_bitwise_single(ift, tag):
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A, core, W, shift = _metric(ift, tag)
    es = [ift.QuadraticEnergy(0 * b, A, b) for b in _rhs(ift, cf, 4)]
    single = [fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=6)).run(e) for e in es]
    cg = fused_cg.FusedCGBatch(core, W, shift, [ift.GradientNormController(iteration_limit=6) for _ in es])
    bat = cg.run(es)
    for (e1, s1), (e2, s2) in zip(single, bat):
        assert s1 == s2
        for k in cf.domain.keys():
            assert torch.equal(e1.position[k].val, e2.position[k].val), k


@pytest.mark.parametrize("tag", METRIC)
def test_fp32_request_leaves_the_solve_in_fp64(ift, tag):
    from nifty_amd import config
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A, core, W, shift = _metric(ift, tag)
    assert core.supports_fp32 is False
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


@pytest.mark.parametrize("tag", METRIC)
def test_mix_launches_do_not_grow_with_the_iteration_count(ift, tag):
    """b, x0 and the start residual rotated in, x and the residual rotated
    out: 5 launches per solve, whatever its length"""
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A, core, W, shift = _metric(ift, tag)
    counts = []
    for n in (3, 12):
        before = fused_cg.STATS["frame_launches"]
        cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=n))
        cg.run(ift.QuadraticEnergy(0 * t, A, t))
        assert cg.niter == n
        counts.append(fused_cg.STATS["frame_launches"] - before)
    assert counts[0] == counts[1] == 5, counts


# -------------------------------------------------------------------- geoVI
def _geo_draw(ift, lh, pos):
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    return kl


@pytest.mark.parametrize("tag", ["p16x8", "p8x8x4"])
def test_geovi_draw_matches_reference(ift, tag):
    from nifty_amd.minimization import geovi_batch
    cf, lh, pos, t, G = problem(ift, tag)
    assert tag in [str(c) for c in G["geo_cases"]]
    dtype, f_lh = lh.get_transformation()
    mini = ift.NewtonCG(ift.GradientNormController(iteration_limit=1))
    assert geovi_batch.ENABLED and geovi_batch.plan(mini, f_lh, None, pos) is None
    kl = _geo_draw(ift, lh, pos)
    ref = G[tag + "_geo_samples"]
    assert kl.samples.n_samples == len(ref) == 2
    for i in range(2):
        err = rel(pack(kl.samples.local_item(i)), ref[i])
        print(tag, "geoVI sample", i, err)
        assert err < 1e-8, i
    ev = abs(kl.value - float(G[tag + "_geo_value"])) / abs(float(G[tag + "_geo_value"]))
    print(tag, "geoVI KL value", ev)
    assert ev < 1e-8


# ---------------------------------------------------------- callable middle
def test_masked_solve_against_the_operator_tree(ift):
    """a MaskOperator between the field and the data: the frame change
    touches the latent side only"""
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase
    from nifty_amd.minimization import fused_cg
    tag = "p16x8"
    G = golden("product.npz")
    cfm = maker(ift, *CASES[tag])
    cf = cfm.finalize(prior_info=0)
    cfm._fusable = lambda: False
    tree = cfm.finalize(prior_info=0)
    assert isinstance(cf, _FusedFieldBase) and not isinstance(tree, _FusedFieldBase)
    flags = np.random.default_rng(9).random(cf.target.shape) < 0.3
    M = ift.MaskOperator(ift.makeField(cf.target, flags))
    data = ift.makeField(M.target, G[tag + "_data"][~flags])
    N = ift.ScalingOperator(M.target, 1e-2, np.float64)
    pos, t = unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"])
    sol = []
    for op in (cf, tree):
        lh = ift.GaussianEnergy(data, inverse_covariance=N.inverse) @ (M @ ift.sigmoid(op))
        A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
        if op is cf:
            core, W, shift = fused_cg.fusable_metric(A)
            assert hasattr(core, "to_frame")
        ic = ift.GradientNormController(iteration_limit=5)
        en, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
        assert st == ic.CONVERGED
        sol.append(en.position)
    for k in cf.domain.keys():
        assert rel(sol[0][k].val, sol[1][k].val) < 1e-9, k
