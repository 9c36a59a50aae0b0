"""GPU: the sampling kernels (csrc/nft_samp.hip) behind MaskOperator and
LinearInterpolator against the reference's values (tests/golden/sampling.npz,
gen_golden_sampling.py).

Cases as test_sampling_plan.py: grids g1 = (16,), g2 = (8, 6), g3 = (4, 6, 8),
the first 1 / 37 / 1000 points (1000 points = 4 blocks of the forward and
hundreds of entries on single pixels; 1 and 37 leave pixels untouched), 1 / 3
/ 8 vectors per launch (the 1, 4-masked and 8 instances), fp64 and fp32.

Tolerances: fp64 1e-13 relative max-norm (that of dispatch.npz; the sums hold
at most ~600 products of the same sign pattern as the reference's).  fp32
storage: inputs cast to fp32 on the host, the expectation computed in fp64
from the cast inputs, agreement to 2^-23 max|expected| (the accumulation is
fp64, so the stored value is one rounding of the exact one)."""
import ctypes

import numpy as np
import pytest
import scipy.sparse
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

GRIDS = ("g1", "g2", "g3")
NPOINTS = (1, 37, 1000)
KS = (1, 3, 8)
MASKS = ("rand", "none", "one")
_CACHE = {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


@pytest.fixture(scope="module")
def G():
    return golden("sampling.npz")


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def space(ift, G, tag):
    return ift.RGSpace(tuple(int(v) for v in G[tag + "_shape"]), distances=tuple(G[tag + "_dist"]))


def case(ift, G, tag, n):
    """(R, dense reference matrix of the first n points, X (8, npix), Y (8, n)):
    vector 0 of X / Y is the fixture's, the others are drawn once"""
    if (tag, n) not in _CACHE:
        sp = space(ift, G, tag)
        R = ift.LinearInterpolator(sp, np.ascontiguousarray(G[tag + "_pts"][:, :n]))
        keep = G[tag + "_row"] < n
        A = scipy.sparse.coo_matrix((G[tag + "_data"][keep], (G[tag + "_row"][keep], G[tag + "_col"][keep])),
                                    shape=(n, sp.size)).toarray()
        rng = np.random.default_rng(3)
        X = rng.standard_normal((8, sp.size))
        Y = rng.standard_normal((8, n))
        X[0] = G[tag + "_x"].ravel()
        Y[0] = G[tag + "_y"][:n]
        _CACHE[(tag, n)] = (R, A, X, Y)
    return _CACHE[(tag, n)]


def dev_t(a, dtype=torch.float64):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0").to(dtype)


# ------------------------------------------------------------------ parity
@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("n", NPOINTS)
def test_interpolator_fp64(ift, G, tag, n):
    R, A, X, Y = case(ift, G, tag, n)
    fx = R(ift.makeField(R.domain, G[tag + "_x"])).val.cpu().numpy()
    assert relmax(fx, G[tag + "_Rx"][:n]) < 1e-13
    fy = R.adjoint_times(ift.makeField(R.target, G[tag + "_y"][:n].copy())).val.cpu().numpy()
    assert fy.shape == tuple(G[tag + "_shape"]) and relmax(fy, G[f"{tag}_Rty{n}"]) < 1e-13
    assert np.all(fy[G[f"{tag}_Rty{n}"] == 0] == 0)            # untouched pixels are written as 0
    for k in KS:
        got = R._fwd(dev_t(X[:k])).cpu().numpy()
        err = relmax(got, X[:k] @ A.T)
        print(tag, n, k, "forward", err)
        assert err < 1e-13
        got = R._adj(dev_t(Y[:k])).cpu().numpy()
        err = relmax(got, Y[:k] @ A)
        print(tag, n, k, "adjoint", err)
        assert err < 1e-13
    # <R x, y> = <x, R^T y>
    Rx = R._fwd(dev_t(X[:1])).cpu().numpy()[0]
    Rty = R._adj(dev_t(Y[:1])).cpu().numpy()[0]
    lhs, rhs = float(Rx @ Y[0]), float(X[0] @ Rty)
    assert abs(lhs - rhs) <= 1e-13 * max(abs(lhs), abs(rhs), np.abs(Rx).max() * np.abs(Y[0]).max())


@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("n", NPOINTS)
def test_interpolator_fp32_storage(ift, G, tag, n):
    R, A, X, Y = case(ift, G, tag, n)
    X32, Y32 = X.astype(np.float32), Y.astype(np.float32)
    for k in KS:
        got = R._fwd(dev_t(X32[:k], torch.float32))
        assert got.dtype == torch.float32
        exp = X32[:k].astype(np.float64) @ A.T
        assert np.abs(got.cpu().numpy().astype(np.float64) - exp).max() <= 2.0 ** -23 * np.abs(exp).max()
        got = R._adj(dev_t(Y32[:k], torch.float32))
        assert got.dtype == torch.float32
        exp = Y32[:k].astype(np.float64) @ A
        assert np.abs(got.cpu().numpy().astype(np.float64) - exp).max() <= 2.0 ** -23 * np.abs(exp).max()


@pytest.mark.parametrize("tag", GRIDS)
def test_scales_and_strides(ift, G, tag):
    """colscale (shared and per vector), rowscale, scalar: the formulas of
    nifty_amd.h, at 1e-13"""
    R, A, X, Y = case(ift, G, tag, 37)
    rng = np.random.default_rng(8)
    k = 3
    cs1, csk = rng.standard_normal(X.shape[1]), rng.standard_normal((k, X.shape[1]))
    rs = rng.standard_normal(37)
    got = R._fwd(dev_t(X[:k]), colscale=dev_t(cs1), rowscale=dev_t(rs), scale=0.7).cpu().numpy()
    assert relmax(got, 0.7 * rs * ((X[:k] * cs1) @ A.T)) < 1e-13
    got = R._fwd(dev_t(X[:k]), colscale=dev_t(csk), scale=-2.).cpu().numpy()
    assert relmax(got, -2. * ((X[:k] * csk) @ A.T)) < 1e-13
    got = R._adj(dev_t(Y[:k]), colscale=dev_t(rs), rowscale=dev_t(cs1), scale=0.7).cpu().numpy()
    assert relmax(got, 0.7 * cs1 * ((Y[:k] * rs) @ A)) < 1e-13
    got = R._adj(dev_t(Y[:k]), rowscale=dev_t(csk)).cpu().numpy()
    assert relmax(got, csk * (Y[:k] @ A)) < 1e-13


# ----------------------------------------------------------- reproducibility
@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("dtype", (torch.float64, torch.float32))
def test_bitwise_batch_and_repeat(ift, G, tag, dtype):
    """per vector the result does not depend on the number of vectors of the
    launch; a second identical call gives the same bits; every output
    element is written (outputs pre-filled with NaN)"""
    from nifty_amd import _native
    for n in NPOINTS:
        R, A, X, Y = case(ift, G, tag, n)
        plan = R._samp_plan()
        Xd, Yd = dev_t(X, dtype), dev_t(Y, dtype)
        nq = _native.samp_quad_blocks(plan)
        assert nq == -(-n // 256)
        single_f, single_a, single_q = [], [], []
        for v in range(8):
            y = torch.full((1, n), float("nan"), dtype=dtype, device="cuda:0")
            q = torch.full((1, nq), float("nan"), dtype=torch.float64, device="cuda:0")
            _native.samp_forward(plan, Xd[v:v + 1], y, qpart=q)
            o = torch.full((1, X.shape[1]), float("nan"), dtype=dtype, device="cuda:0")
            _native.samp_adjoint(plan, Yd[v:v + 1], o)
            assert not torch.isnan(y).any() and not torch.isnan(o).any() and not torch.isnan(q).any()
            single_f.append(y[0]), single_a.append(o[0]), single_q.append(q[0])
        for k in (3, 8):
            for rep in range(2):
                y = torch.full((k, n), float("nan"), dtype=dtype, device="cuda:0")
                q = torch.full((k, nq), float("nan"), dtype=torch.float64, device="cuda:0")
                _native.samp_forward(plan, Xd[:k], y, qpart=q)
                o = torch.full((k, X.shape[1]), float("nan"), dtype=dtype, device="cuda:0")
                _native.samp_adjoint(plan, Yd[:k], o)
                for v in range(k):
                    assert torch.equal(y[v], single_f[v]), (n, k, v)
                    assert torch.equal(o[v], single_a[v]), (n, k, v)
                    assert torch.equal(q[v], single_q[v]), (n, k, v)
            # the partials do not change the forward's output
            y2 = torch.full((k, n), float("nan"), dtype=dtype, device="cuda:0")
            _native.samp_forward(plan, Xd[:k], y2)
            assert torch.equal(y2, y)


# ------------------------------------------------------------------- middle
@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("n", (37, 1000))
def test_fused_middle(ift, G, tag, n):
    """fct * dr * R^T (c * R (dr * s)) against operator-by-operator
    application (1e-13); the curvature partials summed against s . middle(s)
    (1e-12); nine vectors take the 8 + 1 chunks"""
    from nifty_amd import _native
    R, A, X, Y = case(ift, G, tag, n)
    shape = R.domain.shape
    rng = np.random.default_rng(12)
    dr = dev_t(rng.standard_normal(shape))
    c = dev_t(rng.random(n) + 0.5)
    S = dev_t(rng.standard_normal((9,) + shape))
    for drv, cv, fct in ((dr, c, 0.3), (None, 2.5, 1.0), (dr, 4.0, 2.0)):
        mid = R.fused_middle(drv, cv, fct)
        assert callable(mid) and mid.supports_batch and mid.supports_fp32 and not mid.supports_fold
        assert mid.quad_blocks == _native.samp_quad_blocks(R._samp_plan()) > 0
        assert not (hasattr(mid, "plan") or hasattr(mid, "scales"))       # not an LOS middle
        ref = []
        for v in range(9):
            f = ift.makeField(R.domain, S[v] if drv is None else S[v] * drv)
            g = R(f).val * cv
            h = R.adjoint_times(ift.makeField(R.target, g)).val
            ref.append((h if drv is None else h * drv) * fct)
        ref = torch.stack(ref).cpu().numpy()
        got = mid(S)
        assert got.shape == S.shape
        assert relmax(got.cpu().numpy(), ref) < 1e-13
        one = mid(S[4])
        assert one.shape == shape and torch.equal(one, got[4])
        q = torch.full((9, mid.quad_blocks + 3), float("nan"), dtype=torch.float64, device="cuda:0")
        got_q = mid(S, qpart=q)
        assert torch.equal(got_q, got)
        quad = q[:, :mid.quad_blocks].sum(1).cpu().numpy()
        exp = (S * got).reshape(9, -1).sum(1).cpu().numpy()
        assert np.abs(quad - exp).max() <= 1e-12 * np.abs(exp).max()
        assert torch.isnan(q[:, mid.quad_blocks:]).all()
        # fp32 storage: the scales follow the input's dtype.  Expectation in
        # fp64 from the cast operands; y and out are each stored with one
        # rounding (2^-24 relative), so per element
        # |error| <= 2^-24 (|dr| |R|^T |y| + |out|) (+ 0.1 % for second order
        # terms and the fp64 sums)
        got32 = mid(S.float())
        assert got32.dtype == torch.float32
        s32 = S.float().double().cpu().numpy().reshape(9, -1)
        d32 = np.ones(s32.shape[1]) if drv is None else drv.float().double().cpu().numpy().ravel()
        c32 = cv.float().double().cpu().numpy() if torch.is_tensor(cv) else float(cv)
        yex = fct * c32 * ((s32 * d32) @ A.T)
        exp = d32 * (yex @ A)
        bound = 2.0 ** -24 * 1.001 * (np.abs(d32) * (np.abs(yex) @ np.abs(A)) + np.abs(exp))
        assert np.all(np.abs(got32.double().cpu().numpy().reshape(9, -1) - exp) <= bound)


# --------------------------------------------------------------------- mask
@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("mtag", MASKS)
def test_mask(ift, G, tag, mtag):
    flags = G[f"{tag}_m{mtag}_flags"]
    sp = space(ift, G, tag)
    M = ift.MaskOperator(ift.makeField(sp, flags))
    got = M(ift.makeField(sp, G[tag + "_x"])).val
    assert np.array_equal(got.cpu().numpy(), G[f"{tag}_m{mtag}_Mx"])
    y = G[f"{tag}_m{mtag}_y"]
    back = M.adjoint_times(ift.makeField(M.target, y)).val
    assert back.shape == sp.shape and np.array_equal(back.cpu().numpy(), G[f"{tag}_m{mtag}_Mty"])
    # batched, fp32 storage, bitwise repeatable, every pixel written
    n = M.target.shape[0]
    rng = np.random.default_rng(4)
    X = dev_t(rng.standard_normal((8, sp.size)), torch.float32)
    Y = dev_t(rng.standard_normal((8, n)), torch.float32)
    keep = np.flatnonzero(~flags.ravel())
    for k in KS:
        f = M._fwd(X[:k])
        assert torch.equal(f, X[:k][:, torch.from_numpy(keep).to(X.device)])
        a = M._adj(Y[:k])
        exp = np.zeros((k, sp.size), dtype=np.float32)
        exp[:, keep] = Y[:k].cpu().numpy()
        assert np.array_equal(a.cpu().numpy(), exp)
    # the sandwich is diagonal: fused_middle is the grid tensor fct * dr^2 * R^T c
    dr = dev_t(rng.standard_normal(sp.shape))
    c = dev_t(rng.random(n) + 0.5)
    for cv in (c, 3.0):
        w = M.fused_middle(dr, cv, 0.25)
        assert torch.is_tensor(w) and w.dtype == torch.float64 and w.shape == sp.shape and w.is_contiguous()
        exp = np.zeros(sp.size)
        exp[keep] = c.cpu().numpy() if torch.is_tensor(cv) else cv
        exp = 0.25 * dr.cpu().numpy().ravel() ** 2 * exp
        assert relmax(w.cpu().numpy().ravel(), exp) < 1e-14
    w = M.fused_middle(None, 2.0, 1.0)
    assert np.array_equal(w.cpu().numpy().ravel(), np.where(flags.ravel(), 0., 2.))


def test_empty_responses_are_handled_on_the_host(ift, G):
    sp = space(ift, G, "g2")
    M = ift.MaskOperator(ift.makeField(sp, np.ones(sp.shape, dtype=bool)))
    R = ift.LinearInterpolator(sp, np.zeros((2, 0)))
    for op in (M, R):
        assert op.target.shape == (0,)
        assert op(ift.makeField(sp, G["g2_x"])).val.shape == (0,)
        back = op.adjoint_times(ift.makeField(op.target, np.zeros(0))).val
        assert back.shape == sp.shape and back.is_cuda and not back.any()
    w = R.fused_middle(None, 1.0, 1.0)
    assert torch.is_tensor(w) and not w.any()


# ---------------------------------------------------------------- arguments
def test_bad_arguments_return_err_arg(ift, G):
    """NFT_ERR_ARG before any launch: the outputs stay untouched"""
    from nifty_amd import _native
    lib = _native.load()
    R, A, X, Y = case(ift, G, "g2", 37)
    good = R._samp_plan()
    x = dev_t(X[:2])
    y = torch.full((2, 37), float("nan"), dtype=torch.float64, device="cuda:0")
    out = torch.full((2, X.shape[1]), float("nan"), dtype=torch.float64, device="cuda:0")
    yin = dev_t(Y[:2])
    npix = X.shape[1]
    p, s = _native.ptr, _native.stream_ptr()
    ERR = -1

    def fwd(plan=good, nvec=2, xs=npix, ys=37, css=0, dtype=0, cs=None, qpart=None, qs=0):
        return lib.nft_samp_forward_batched(ctypes.byref(plan) if plan is not None else None, p(x), p(cs), css,
                                            p(None), p(y), dtype, 1.0, nvec, xs, ys, p(qpart), qs, s)

    def adj(plan=good, nvec=2, ys=37, os_=npix, rss=0, dtype=0, rs=None):
        return lib.nft_samp_adjoint_batched(ctypes.byref(plan) if plan is not None else None, p(yin), p(None),
                                            p(rs), rss, p(out), dtype, 1.0, nvec, ys, os_, s)

    def broken(**kw):
        q = _native.SampPlan()
        ctypes.memmove(ctypes.byref(q), ctypes.byref(good), ctypes.sizeof(q))
        for k, v in kw.items():
            setattr(q, k, v)
        return q
    bad_plans = [None, broken(idx=None), broken(frac=None), broken(pix_ptr=None), broken(ent=None),
                 broken(ndim=0), broken(ndim=4), broken(ncorner=3), broken(npix=npix + 1), broken(npoints=-1)]
    for bp in bad_plans:
        assert fwd(plan=bp) == ERR
        assert adj(plan=bp) == ERR
    q = torch.zeros((2, 1), dtype=torch.float64, device="cuda:0")
    for kw in (dict(nvec=0), dict(nvec=9), dict(xs=0), dict(ys=0), dict(cs=x, css=-1), dict(dtype=2),
               dict(qpart=q, qs=0)):
        assert fwd(**kw) == ERR, kw
    for kw in (dict(nvec=0), dict(nvec=9), dict(ys=0), dict(os_=0), dict(rs=out, rss=-1), dict(dtype=7)):
        assert adj(**kw) == ERR, kw
    assert b"nft_samp" in lib.nft_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(y).all() and torch.isnan(out).all()
    # the same calls with good arguments succeed
    assert fwd() == 0 and adj() == 0
    torch.cuda.synchronize()
    assert not torch.isnan(y).any() and not torch.isnan(out).any()
    # the Python wrappers refuse host tensors: no CPU fallback
    with pytest.raises(_native.NativeError):
        R._fwd(torch.zeros((1, npix), dtype=torch.float64))
