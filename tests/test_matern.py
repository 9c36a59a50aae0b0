"""CPU: which CorrelatedFieldMaker configurations with a Matern component
(add_fluctuations_matern, src/library/correlated_fields.py:597-690) lower to
the fused field, their latent keys and target shapes against the reference's
(tests/golden/matern.npz, gen_golden_matern.py), and the torch restatement of
the closed-form amplitude against the reference's `cfm.amplitude`.  No native
code runs here."""
import numpy as np
import pytest

from conftest import golden

MATERN = ((1., 0.3), (2., 0.5), (-3., 0.5))
CASES = {
    "m8z": dict(shape=(8, 8), distances=0.1, offset_std=(1e-2, 1e-3)),
    "m8": dict(shape=(8, 8), distances=0.1, offset_std=None),
    "m16": dict(shape=(16,), distances=0.3, offset_std=None),
    "m3d": dict(shape=(6, 8, 4), distances=None, offset_std=(0.5, 0.2)),
}


def maker(ift, shape, distances, offset_std, offset_mean=1.):
    """the makers of gen_golden_matern.py"""
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(ift.RGSpace(shape, distances=distances), *MATERN)
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


@pytest.mark.parametrize("tag", list(CASES))
def test_fusable_matern_makers_give_the_fused_field(tag):
    import nifty_amd as ift
    from nifty_amd.library.correlated_fields_simple import (_CorrelatedFieldModel, _FusedFieldBase,
                                                            _MaternFieldModel)
    G = golden("matern.npz")
    assert [str(c) for c in G["cases"]] == list(CASES)
    assert np.array_equal(G["matern"], np.array(MATERN))
    cfm = maker(ift, **CASES[tag])
    op = cfm.finalize(prior_info=0)
    assert isinstance(op, _MaternFieldModel) and isinstance(op, _FusedFieldBase)
    assert not isinstance(op, _CorrelatedFieldModel)
    assert not issubclass(_MaternFieldModel, _CorrelatedFieldModel)
    assert sorted(op.domain.keys()) == [str(k) for k in G[tag + "_keys"]]
    assert op.target.shape == G[tag + "_val"].shape
    has_zm = CASES[tag]["offset_std"] is not None
    assert ("m_zeromode" in op.domain.keys()) == has_zm
    assert op.amp.amp2_tiles(None, 4) == 0 and op.amp.amp2_table(None) is None
    assert op.amp.supports_fp32 is False


def test_other_matern_makers_keep_the_operator_tree():
    import nifty_amd as ift
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase
    sp = ift.RGSpace((8, 8), distances=0.1)
    # unit zero mode
    cfm = maker(ift, (8, 8), 0.1, 1.)
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # an operator-valued zero mode
    cfm = maker(ift, (8, 8), 0.1, ift.LognormalTransform(1e-2, 1e-3, "zz", 0))
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # Matern beside a second component (either kind)
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(sp, *MATERN)
    cfm.add_fluctuations(ift.RGSpace(6), (1., 0.5), None, None, (-3., 1.), prefix="b")
    cfm.set_amplitude_total_offset(1., (1e-2, 1e-3))
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    cfm = ift.CorrelatedFieldMaker("m_")
    cfm.add_fluctuations_matern(sp, *MATERN, prefix="a")
    cfm.add_fluctuations_matern(ift.RGSpace(6), *MATERN, prefix="b")
    cfm.set_amplitude_total_offset(1., (1e-2, 1e-3))
    assert not isinstance(cfm.finalize(prior_info=0), _FusedFieldBase)
    # a Field offset
    cfm = maker(ift, (8, 8), 0.1, (1e-2, 1e-3), offset_mean=ift.full(sp, 0.5))
    op = cfm.finalize(prior_info=0)
    assert not isinstance(op, _FusedFieldBase)
    assert sorted(op.domain.keys()) == ["m_cutoff", "m_loglogslope", "m_scale", "m_xi", "m_zeromode"]


@pytest.mark.parametrize("tag", list(CASES))
def test_amplitude_of_the_fusable_maker(tag):
    """`amplitude` has the fused model's amplitude domain, and the closed
    form (matern._MaternAmplitudeModel.forward, plain torch) is the
    reference's cfm.amplitude; fp64, two evaluation orders apart: 1e-13"""
    import nifty_amd as ift
    G = golden("matern.npz")
    cfm = maker(ift, **CASES[tag])
    op = cfm.finalize(prior_info=0)
    a = cfm.amplitude
    assert a.domain is op.amplitude.domain
    assert sorted(a.domain.keys()) == sorted(k for k in op.domain.keys() if k != "m_xi")
    assert a.target.shape == G[tag + "_amp"].shape
    pos = unpack(ift, op.domain, G[tag + "_pos"])
    got = a.force(pos).val.cpu().numpy()
    ref = G[tag + "_amp"]
    assert np.linalg.norm(got - ref) <= 1e-13 * np.linalg.norm(ref)
    # adjust_for_volume=False: V = 1
    cfm1 = ift.CorrelatedFieldMaker("m_")
    cfm1.add_fluctuations_matern(ift.RGSpace(CASES[tag]["shape"], distances=CASES[tag]["distances"]), *MATERN,
                                 adjust_for_volume=False)
    cfm1.set_amplitude_total_offset(1., CASES[tag]["offset_std"])
    assert cfm1.finalize(prior_info=0).amp.total_vol == 1.0
    # the statistics still come from the operator amplitudes
    assert cfm.total_fluctuation is cfm._a[0].fluctuation_amplitude
    assert len(cfm.get_normalized_amplitudes()) == 1
