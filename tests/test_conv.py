"""Host side of FuncConvolutionOperator against the reference's values
(tests/golden/conv.npz, gen_golden_conv.py): the harmonic-space kernel of
RGSpace.get_conv_kernel_from_func, the FFT restatement of the operator, and
the constructor's argument checks.  No GPU."""
import numpy as np
import pytest

from conftest import golden

SIGMA_PIX = 1.7


def kernels(sp):
    sig = SIGMA_PIX * min(sp.distances)
    r0 = 0.25 * min(n * d for n, d in zip(sp.shape, sp.distances))
    return (("g", lambda r: np.exp(-0.5 * (r / sig) ** 2)), ("k", lambda r: (1. + (r / r0) ** 2) ** -2))


def relmax(a, b):
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


def cases():
    G = golden("conv.npz")
    return G, [str(t) for t in G["grids"]]


@pytest.mark.parametrize("tag", cases()[1])
def test_kernel_table_matches_reference(tag):
    import nifty_amd as ift
    G = cases()[0]
    sp = ift.RGSpace(tuple(G[tag + "_shape"]), distances=tuple(G[tag + "_dist"]))
    for kn, func in kernels(sp):
        k = sp.get_default_codomain().get_conv_kernel_from_func(func)
        assert k.domain[0] == sp.get_default_codomain()
        err = relmax(k.val_np(), G[f"{tag}_{kn}_khat"])
        print(tag, kn, "kernel", err)
        assert err < 1e-14


@pytest.mark.parametrize("tag", cases()[1])
def test_fft_restatement_matches_reference(tag):
    """C x = Re ifftn(kt * fftn(x)) with kt the kernel and kt[0] = 1"""
    from nifty_amd.operators.convolution_operators import conv_gain
    import nifty_amd as ift
    G = cases()[0]
    shape = tuple(G[tag + "_shape"])
    sp = ift.RGSpace(shape, distances=tuple(G[tag + "_dist"]))
    x = 0.7 + np.random.default_rng(int(G[tag + "_seed"])).standard_normal(shape)
    for kn, func in kernels(sp):
        kt = conv_gain(sp, func)
        assert kt.reshape(-1)[0] == 1.
        cx = np.fft.ifftn(kt * np.fft.fftn(x)).real
        err = relmax(cx, G[f"{tag}_{kn}_Cx"])
        print(tag, kn, "C x", err)
        assert err < 1e-13


def test_wrapped_kernel_is_not_positive():
    """nothing may assume kt > 0: the periodic wrap-around makes it negative"""
    import nifty_amd as ift
    from nifty_amd.operators.convolution_operators import conv_gain
    sp = ift.RGSpace((8, 8))
    assert conv_gain(sp, kernels(sp)[0][1]).min() < 0


def test_constructor_errors():
    import nifty_amd as ift
    sp = ift.RGSpace((8, 8))
    func = kernels(sp)[0][1]
    with pytest.raises(TypeError):
        ift.FuncConvolutionOperator(ift.UnstructuredDomain(8), func)
    with pytest.raises(NotImplementedError):
        ift.FuncConvolutionOperator((sp, ift.RGSpace(4)), func, space=0)
    with pytest.raises(NotImplementedError):
        ift.FuncConvolutionOperator(ift.RGSpace((4, 4, 4, 4)), func)
    with pytest.raises(NotImplementedError):
        sp.get_conv_kernel_from_func(func)
    op = ift.FuncConvolutionOperator(sp, func)
    assert op.domain == op.target == ift.DomainTuple.make(sp)
    assert op.capability == op.TIMES | op.ADJOINT_TIMES
