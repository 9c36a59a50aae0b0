"""Host side of FuncConvolutionOperator on one space of a two-space domain
(FuncConvolutionOperator.on_space) against the reference's values
(tests/golden/conv_space.npz, gen_golden_conv_space.py): on_space's argument
checks, the table the kernels use, the
numpy restatement of the operator

    C x = Re ifftn_S(k * fftn_S(x)) + (1 - k0) * mean(x)

(raw k, the mean over ALL pixels), the complex-pair identity the native
kernels rest on, nft_conv_space_supported and the header.  No GPU."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

SIGMA_PIX = 1.7
NATIVE = ("s88e4", "s168e2", "s88e6", "s832e16", "s88e2x2", "s8512e10", "s10248e2")
FALLBACK = ("s88e5", "s86e4", "e4s88", "s16e8", "s888e2")


def kernels(sp):
    sig = SIGMA_PIX * min(sp.distances)
    r0 = 0.25 * min(n * d for n, d in zip(sp.shape, sp.distances))
    return dict(g=lambda r: np.exp(-0.5 * (r / sig) ** 2), k=lambda r: (1. + (r / r0) ** 2) ** -2)


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def domain(ift, G, tag):
    """(domain, S, space) of a fixture case"""
    S = ift.RGSpace(tuple(int(n) for n in G[tag + "_sshape"]), distances=tuple(G[tag + "_sdist"]))
    X = ift.RGSpace(tuple(int(n) for n in G[tag + "_xshape"]), distances=tuple(G[tag + "_xdist"]))
    space = int(G[tag + "_space"])
    return ift.DomainTuple.make((S, X) if space == 0 else (X, S)), S, space


def case_kernels(G, tag):
    return [str(k) for k in G[tag + "_kernels"]]


def test_fixture_lists_the_cases():
    G = golden("conv_space.npz")
    assert sorted(str(t) for t in G["cases"]) == sorted(NATIVE + FALLBACK)
    assert float(G["formula_err"]) < 1e-13
    for tag in NATIVE + FALLBACK:
        npix_s = int(np.prod(G[tag + "_sshape"]))
        assert case_kernels(G, tag) == (["g", "k"] if npix_s < 4096 else ["g"]), tag


def test_on_space_accepts_a_product_domain():
    """fails on the parent commit, which has no on_space and whose
    constructor raises NotImplementedError for two spaces -- as the plain
    constructor here still does (tests/test_conv.py pins that)"""
    import nifty_amd as ift
    S, X = ift.RGSpace((8, 8), 0.1), ift.RGSpace(4, 0.5)
    func = kernels(S)["g"]
    for dom, space in (((S, X), 0), ((X, S), 1)):
        with pytest.raises(NotImplementedError):
            ift.FuncConvolutionOperator(dom, func, space=space)
        op = ift.FuncConvolutionOperator.on_space(dom, func, space=space)
        assert isinstance(op, ift.FuncConvolutionOperator)
        assert op.domain == op.target == ift.DomainTuple.make(dom)
        assert op.capability == op.TIMES | op.ADJOINT_TIMES
        assert op.gain.shape == S.shape
    # a DomainTuple works as well as a tuple of spaces
    ift.FuncConvolutionOperator.on_space(ift.DomainTuple.make((S, X)), func, space=0)
    # 1-D and 3-D sub-spaces, a second space of any kind
    ift.FuncConvolutionOperator.on_space((ift.RGSpace(16), X), func, space=0)
    ift.FuncConvolutionOperator.on_space((ift.RGSpace((8, 8, 8)), ift.UnstructuredDomain(3)), func, space=0)


def test_constructor_errors():
    import nifty_amd as ift
    S, X = ift.RGSpace((8, 8), 0.1), ift.RGSpace(4, 0.5)
    func = kernels(S)["g"]
    with pytest.raises(ValueError):     # infer_space: two spaces need `space`
        ift.FuncConvolutionOperator.on_space((S, X), func)
    with pytest.raises(ValueError):     # infer_space: out of range
        ift.FuncConvolutionOperator.on_space((S, X), func, space=2)
    with pytest.raises(TypeError, match="unsupported domain"):
        ift.FuncConvolutionOperator.on_space((S, ift.UnstructuredDomain(4)), func, space=1)
    with pytest.raises(TypeError):      # a harmonic space
        ift.FuncConvolutionOperator.on_space((S.get_default_codomain(), X), func, space=0)
    with pytest.raises(NotImplementedError):
        ift.FuncConvolutionOperator.on_space((S, X, ift.RGSpace(2)), func, space=0)
    with pytest.raises(NotImplementedError):
        ift.FuncConvolutionOperator.on_space((ift.RGSpace((4, 4, 4, 4)), X), func, space=0)


def test_one_space_operator_keeps_its_table():
    """one space: kt with zero mode 1, as before; gain0 is the raw zero mode"""
    import nifty_amd as ift
    from nifty_amd.operators.convolution_operators import conv_gain, conv_kernel
    S = ift.RGSpace((8, 8), 0.1)
    func = kernels(S)["g"]
    op = ift.FuncConvolutionOperator(S, func)
    assert np.array_equal(op.gain, ift.FuncConvolutionOperator.on_space(S, func).gain)
    assert np.array_equal(op.gain, conv_gain(S, func)) and op.gain.reshape(-1)[0] == 1.
    k = conv_kernel(S, func)
    assert op.gain0 == k.reshape(-1)[0]
    assert abs(op.gain0 - 1.5625) < 1e-12       # not 1: the issue's example
    assert np.array_equal(op.gain.reshape(-1)[1:], k.reshape(-1)[1:])


@pytest.mark.parametrize("tag", NATIVE + FALLBACK)
def test_gain_matches_reference(tag):
    import nifty_amd as ift
    G = golden("conv_space.npz")
    dom, S, space = domain(ift, G, tag)
    for kn in case_kernels(G, tag):
        op = ift.FuncConvolutionOperator.on_space(dom, kernels(S)[kn], space=space)
        khat = G[f"{tag}_{kn}_khat"]
        err = relmax(op.gain, khat)
        print(tag, kn, "gain", err)
        assert err < 1e-14
        # the raw table: the zero mode is k0, not 1
        assert op.gain.reshape(-1)[0] == op.gain0
        assert abs(op.gain0 - khat.reshape(-1)[0]) <= 1e-14 * abs(khat.reshape(-1)[0])


@pytest.mark.parametrize("tag", NATIVE + FALLBACK)
def test_formula_matches_reference(tag):
    """C x = Re ifftn_S(k * fftn_S(x)) + (1 - k0) * mean(x), and its sums"""
    import nifty_amd as ift
    G = golden("conv_space.npz")
    dom, S, space = domain(ift, G, tag)
    axes = dom.axes[space]
    x = 0.7 + np.random.default_rng(int(G[tag + "_seed"])).standard_normal(dom.shape)
    for kn in case_kernels(G, tag):
        k = ift.FuncConvolutionOperator.on_space(dom, kernels(S)[kn], space=space).gain
        kb = k.reshape([dom.shape[a] if a in axes else 1 for a in range(len(dom.shape))])
        cx = np.fft.ifftn(kb * np.fft.fftn(x, axes=axes), axes=axes).real + (1. - k.reshape(-1)[0]) * x.mean()
        ref = G[f"{tag}_{kn}_Cx"]
        err = relmax(cx, ref)
        print(tag, kn, "C x", err)
        assert err < 1e-13
        assert relmax(ref.sum(axis=axes), G[f"{tag}_{kn}_slicesums"]) < 1e-14
        # the total sum is kept, the per-slice sums are not (k0 != 1)
        assert abs(ref.sum() - x.sum()) <= 1e-13 * abs(x.sum())


@pytest.mark.parametrize("tag", NATIVE)
def test_complex_pair_identity(tag):
    """the real (n0, n1, ne) array read as complex (n0, n1, ne / 2): a full
    complex transform over axes 0 and 1 times the real table convolves slice
    2j in the real part and slice 2j + 1 in the imaginary part"""
    import nifty_amd as ift
    G = golden("conv_space.npz")
    dom, S, space = domain(ift, G, tag)
    assert space == 0
    n0, n1 = S.shape
    ne = dom.size // S.size
    assert ne % 2 == 0
    x = 0.7 + np.random.default_rng(int(G[tag + "_seed"])).standard_normal(dom.shape)
    z = np.ascontiguousarray(x.reshape(n0, n1, ne)).view(np.complex128)
    assert z.shape == (n0, n1, ne // 2)
    for kn in case_kernels(G, tag):
        k = ift.FuncConvolutionOperator.on_space(dom, kernels(S)[kn], space=0).gain
        w = np.fft.ifftn(k[..., None] * np.fft.fftn(z, axes=(0, 1)), axes=(0, 1))
        cx = np.ascontiguousarray(w).view(np.float64).reshape(dom.shape) + (1. - k[0, 0]) * x.mean()
        err = relmax(cx, G[f"{tag}_{kn}_Cx"])
        print(tag, kn, "complex pairs", err)
        assert err < 1e-13


def test_supported_truth_table():
    import torch
    from nifty_amd import _native
    G = golden("conv_space.npz")
    for tag in NATIVE + FALLBACK:
        ss = tuple(int(n) for n in G[tag + "_sshape"])
        ne = int(np.prod(G[tag + "_xshape"]))
        want = tag in NATIVE
        if len(ss) == 2:
            assert _native.conv_space_supported(ss[0], ss[1], ne) == (want or tag == "e4s88"), tag
        else:
            assert not want
    # e4s88: the shape would be served, space = 1 is what keeps it off the native path
    assert not _native.conv_space_supported(8, 8, 4, torch.float32)
    assert not _native.conv_space_supported(8, 8, 0) and not _native.conv_space_supported(8, 8, 3)
    assert not _native.conv_space_supported(4, 8, 2) and not _native.conv_space_supported(8, 1024, 2)
    assert _native.conv_space_supported(512, 512, 32) and _native.conv_space_supported(16384, 8, 2)
    assert not _native.conv_space_supported(768, 8, 2) and not _native.conv_space_supported(32768, 8, 2)
    assert not _native.conv_space_supported(16384, 512, 256)    # 2^31 pixels


def test_header_and_binding_agree_on_the_new_entries():
    """as test_host.py for the whole header: the four nft_conv_space_* entry
    points are declared, exported and bound, with the argument counts of the
    declarations"""
    import ctypes
    from nifty_amd import _native
    txt = open(os.path.join(ROOT, "include", "nifty_amd.h")).read()
    new = ("nft_conv_space_supported", "nft_conv_space_workspace", "nft_conv_space_quad_blocks",
           "nft_conv_space_apply_batched")
    lib = ctypes.CDLL(_native.LIB_PATH)
    for name in new:
        m = re.search(r"^\s*(int|size_t)\s+" + name + r"\s*\(([^;]*)\);", txt, re.M)
        assert m, name
        assert hasattr(lib, name), name
        res, args = _native.SIGNATURES[name]
        assert len(args) == len(m.group(2).split(",")), name
        assert res is (ctypes.c_size_t if m.group(1) == "size_t" else ctypes.c_int), name
    # the old entry takes the same argument list as the new one
    assert _native.SIGNATURES["nft_conv_space_apply_batched"] == _native.SIGNATURES["nft_conv_apply_batched"]
    assert re.search(r"typedef struct nft_conv_space_plan \{[^}]*int64_t n0, n1, inner;[^}]*const double\* table;"
                     r"[^}]*double gain0;[^}]*\} nft_conv_space_plan;", txt)
    assert [f[0] for f in _native.ConvSpacePlan._fields_] == ["n0", "n1", "inner", "table", "gain0"]


def test_host_argument_checks_without_a_device():
    """workspace and block counts are host arithmetic: bad plans give 0"""
    import ctypes
    from nifty_amd import _native
    lib = _native.load()
    p = _native.ConvSpacePlan()
    p.n0, p.n1, p.inner, p.table, p.gain0 = 8, 512, 5, 256, 1.0      # table: any non-NULL address, never read
    assert lib.nft_conv_space_quad_blocks(ctypes.byref(p)) == (8 * 5 + 3) // 4      # 4 lines per 512-point tile
    grid = 8 * 512 * 5 * 16
    assert lib.nft_conv_space_workspace(ctypes.byref(p), 1) == grid + 256 + 256
    assert lib.nft_conv_space_workspace(ctypes.byref(p), 0) == 0
    p.table = None
    assert lib.nft_conv_space_workspace(ctypes.byref(p), 1) == 0
    assert lib.nft_conv_space_quad_blocks(ctypes.byref(p)) == 0
    p.table, p.n1 = 256, 6
    assert lib.nft_conv_space_quad_blocks(ctypes.byref(p)) == 0
