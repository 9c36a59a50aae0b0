"""CPU: the two identities behind the fused product-spectrum field
(library/product.py) restated in numpy, which CorrelatedFieldMaker
configurations with two components lower to it and which keep the operator
tree, and its latent keys, target shapes and torch restatement against the
reference's (tests/golden/product.npz, gen_golden_product.py).  No native
kernel runs here."""
import numpy as np
import pytest

from conftest import golden

COMP_A = ((1., .2), (.5, .2), (.3, .1), (-3., .5))
COMP_B = ((.5, .1), (.4, .2), None, (-2., .5))
CASES = {
    "p16x8": (((16,), 0.3), ((8,), 0.5)),
    "p8x8x4": (((8, 8), 0.1), ((4,), 0.5)),
    "p4x8x8": (((4,), 0.5), ((8, 8), 0.1)),
    "p6x5": (((6,), 0.3), ((5,), 0.5)),
    "p64x64": (((64,), 0.3), ((64,), 0.5)),
}


def maker(ift, s1, s2, offset_mean=1., offset_std=(0.3, 0.1)):
    """the makers of gen_golden_product.py"""
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(ift.RGSpace(s1[0], distances=s1[1]), *COMP_A, prefix="a")
    cfm.add_fluctuations(ift.RGSpace(s2[0], distances=s2[1]), *COMP_B, prefix="b")
    cfm.set_amplitude_total_offset(offset_mean, offset_std)
    return cfm


def unpack(ift, dom, vec):
    out, o = {}, 0
    for k in sorted(dom.keys()):
        n = dom[k].size
        out[k] = ift.makeField(dom[k], vec[o:o + n].reshape(dom[k].shape).copy())
        o += n
    assert o == len(vec)
    return ift.MultiField.from_dict(out, dom)


# ------------------------------------------------------ numpy restatements
def mirror(x, axes):
    """the point mirror k -> -k on `axes`"""
    for a in axes:
        x = np.roll(np.flip(x, a), 1, a)
    return x


def mix(x, split):
    """R x = ((x + P1 x) + P2 x - P1 P2 x) / 2 in the kernel's order"""
    g1, g2 = tuple(range(split)), tuple(range(split, x.ndim))
    return ((x + mirror(x, g1)) + mirror(x, g2) - mirror(x, g1 + g2)) * 0.5


def hartley(x, axes, sign=1.):
    """genuine Hartley transform over `axes`: Re F + sign * Im F"""
    f = np.fft.fftn(x, axes=axes)
    return f.real + sign * f.imag


SHAPES = [((8, 6), 1), ((6, 8, 4), 2), ((5, 7), 1), ((4, 6, 8), 1), ((2, 2), 1), ((1, 8), 1), ((16, 8), 1)]


@pytest.mark.parametrize("shape,split", SHAPES)
def test_mirror_mix_is_a_symmetric_involution(shape, split):
    rng = np.random.default_rng(1)
    x, y = rng.standard_normal(shape), rng.standard_normal(shape)
    assert np.max(np.abs(mix(mix(x, split), split) - x)) <= 4e-16 * np.max(np.abs(x))
    a, b = np.vdot(y, mix(x, split)), np.vdot(mix(y, split), x)
    assert abs(a - b) <= 1e-14 * np.linalg.norm(x) * np.linalg.norm(y)
    # orthogonal
    assert abs(np.linalg.norm(mix(x, split)) - np.linalg.norm(x)) <= 1e-14 * np.linalg.norm(x)


@pytest.mark.parametrize("sign", [1., -1.])
@pytest.mark.parametrize("shape,split", SHAPES)
def test_separable_hartley_is_the_mixed_joint_one(shape, split, sign):
    """H_1 (x) H_2 = R H_joint = H_joint R for both Hartley conventions"""
    x = np.random.default_rng(2).standard_normal(shape)
    g1, g2 = tuple(range(split)), tuple(range(split, len(shape)))
    sep = hartley(hartley(x, g1, sign), g2, sign)
    joint = hartley(x, g1 + g2, sign)
    scale = np.max(np.abs(sep))
    assert np.max(np.abs(sep - mix(joint, split))) <= 1e-14 * scale
    assert np.max(np.abs(sep - hartley(mix(x, split), g1 + g2, sign))) <= 1e-14 * scale


# ------------------------------------------------------------------ maker
@pytest.mark.parametrize("tag", list(CASES))
def test_fusable_product_makers_give_the_fused_field(tag):
    import nifty_amd as ift
    from nifty_amd.library.correlated_fields_simple import _CorrelatedFieldModel, _FusedFieldBase
    from nifty_amd.library.product import _ProductFieldModel
    G = golden("product.npz")
    assert [str(c) for c in G["cases"]] == list(CASES)
    cfm = maker(ift, *CASES[tag])
    op = cfm.finalize(prior_info=0)
    assert isinstance(op, _ProductFieldModel) and isinstance(op, _FusedFieldBase)
    assert not isinstance(op, _CorrelatedFieldModel)
    assert not issubclass(_ProductFieldModel, _CorrelatedFieldModel)
    assert sorted(op.domain.keys()) == [str(k) for k in G[tag + "_keys"]]
    assert {"p_xi", "p_zeromode", "p_aasperity", "p_aspectrum", "p_bflexibility"} <= set(op.domain.keys())
    assert op.target.shape == G[tag + "_val"].shape
    assert len(op.target) == 2 and op.domain["p_xi"].shape == op.target.shape
    B1, B2 = (G[f"{tag}_na{i}"].shape[0] for i in range(2))
    assert (op.amp.B1, op.amp.B2, op.amp.B) == (B1, B2, B1 * B2)
    # the combined bin index is mirror symmetric on every axis
    p = op.amp.pspace.pindex
    assert p.shape == op.target.shape and p.max() == B1 * B2 - 1
    for ax in range(p.ndim):
        assert np.array_equal(p, mirror(p, (ax,)))
    assert (op.jbins.fold is not None) == (tag == "p64x64")
    assert op.amp.amp2_tiles(None, 4) == 0 and op.amp.supports_fp32 is False
    with pytest.raises(NotImplementedError):
        cfm.amplitude
    # the switch the other tests use still gives the operator tree
    cfm._fusable = lambda: False
    tree = cfm.finalize(prior_info=0)
    assert not isinstance(tree, _FusedFieldBase)
    assert tree.domain is op.domain and tree.target == op.target


def test_other_makers_keep_the_operator_tree():
    import nifty_amd as ift
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase
    s1, s2 = CASES["p16x8"]
    sp1 = ift.RGSpace(*s1)
    # unit, disabled-in-name-only and operator-valued zero modes
    assert not isinstance(maker(ift, s1, s2, offset_std=1.).finalize(prior_info=0), _FusedFieldBase)
    zm = ift.LognormalTransform(0.3, 0.1, "zz", 0)
    assert not isinstance(maker(ift, s1, s2, offset_std=zm).finalize(prior_info=0), _FusedFieldBase)
    # a Field offset
    dom = ift.makeDomain((sp1, ift.RGSpace(*s2)))
    op = maker(ift, s1, s2, offset_mean=ift.full(dom, 0.5)).finalize(prior_info=0)
    assert not isinstance(op, _FusedFieldBase)
    # three components
    cfm = maker(ift, s1, s2)
    cfm.add_fluctuations(ift.RGSpace(4), *COMP_B, prefix="c")
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # a Matern component in a product
    cfm = ift.CorrelatedFieldMaker("p_")
    cfm.add_fluctuations(sp1, *COMP_A, prefix="a")
    cfm.add_fluctuations_matern(ift.RGSpace(8), (1., 0.3), (2., 0.5), (-3., 0.5), prefix="b")
    cfm.set_amplitude_total_offset(1., (0.3, 0.1))
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # more than three grid axes in total
    cfm = maker(ift, ((4, 4), 0.1), ((4, 4), 0.2))
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # stacked fields stay out of scope
    with pytest.raises(NotImplementedError):
        ift.CorrelatedFieldMaker("p_", total_N=2)


@pytest.mark.parametrize("tag", list(CASES))
def test_torch_restatement_against_the_reference(tag):
    """s = offset + c_h H_joint[A[pindex] (R xi)] with the table of
    _ProductAmplitudeModel.forward (plain torch) and numpy's FFT against the
    reference's value, and the table's jvp / vjp against each other; fp64,
    different transforms and summation orders: 1e-12"""
    import torch
    import nifty_amd as ift
    G = golden("product.npz")
    op = maker(ift, *CASES[tag]).finalize(prior_info=0)
    pos = unpack(ift, op.domain, G[tag + "_pos"])
    lat = {k: pos[k].val for k in op.domain.keys()}
    A, c = op.amp.forward(lat)
    afull = A.cpu().numpy()[op.amp.pspace.pindex]
    xi = lat["p_xi"].cpu().numpy()
    sign = 1. if ift.config.hartley_convention_code() == 0 else -1.
    s = 1. + op.c_h * hartley(afull * mix(xi, op.split), tuple(range(xi.ndim)), sign)
    ref = G[tag + "_val"]
    assert np.linalg.norm(s - ref) <= 1e-12 * np.linalg.norm(ref)
    # the table's rows and columns are the normalised amplitudes times z
    z = float(c["z"])
    T = A.cpu().numpy().reshape(op.amp.B1, op.amp.B2)
    V1, V2 = (a.total_vol for a in op.amp.parts)
    n0, n1 = G[tag + "_na0"], G[tag + "_na1"]
    assert np.allclose(T[1:, 0] / z, n0[1:] / V1, rtol=1e-12) and np.allclose(T[0, 1:] / z, n1[1:] / V2, rtol=1e-12)
    assert np.allclose(T[1:, 1:], np.outer(n0[1:], n1[1:]) * z / (V1 * V2), rtol=1e-12)
    # adjointness of the torch jvp / vjp
    rng = np.random.default_rng(4)
    t = {k: torch.as_tensor(rng.standard_normal(op.domain[k].shape)).to(A.device) for k in op.amp.domain_dict}
    g = torch.as_tensor(rng.standard_normal(op.amp.B)).to(A.device)
    lhs = float(torch.dot(op.amp.jvp(c, t), g))
    out = op.amp.vjp(c, g)
    rhs = sum(float(torch.sum(out[k].reshape(t[k].shape) * t[k])) for k in t)
    assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.)
