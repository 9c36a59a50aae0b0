"""CPU: construction of joint likelihoods (lh1 + lh2 -> _LikelihoodSum,
src/operators/energy_operators.py:137-141, 208-301), PrependKey, and the C
declarations of the LOS adjoint with a pointwise branch.  No kernel runs."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

import nifty_amd as ift
from nifty_amd import _native
from nifty_amd.operators.energy_operators import _LikelihoodSum

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))


@pytest.fixture(scope="module")
def lhs():
    """three likelihoods on one 8 x 8 correlated field (j8 of joint.npz)"""
    G = golden("joint.npz")
    sp = ift.RGSpace((8, 8))
    cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
    R = ift.LOSResponse(sp, starts=list(G["j8_starts"]), ends=list(G["j8_ends"]))
    N = ift.ScalingOperator(R.target, 1e-3, np.float64)
    lh1 = ift.GaussianEnergy(ift.makeField(R.target, G["j8_data"]), inverse_covariance=N.inverse) @ R(ift.sigmoid(cf))
    lh2 = ift.PoissonianEnergy(ift.makeField(sp, G["j8_counts"])) @ cf.exp()
    Rg = ift.GeometryRemover(sp)
    lh3 = ift.GaussianEnergy(ift.full(Rg.target, 0.), inverse_covariance=ift.ScalingOperator(
        Rg.target, 4., np.float64)) @ (Rg @ cf)
    return cf, lh1, lh2, lh3, G


def test_sum_is_likelihood_sum_and_flattens(lhs):
    cf, lh1, lh2, lh3, _ = lhs
    s = lh1 + lh2
    assert isinstance(s, _LikelihoodSum) and isinstance(s, ift.LikelihoodEnergyOperator)
    assert s._ops == (lh1, lh2)
    assert s.domain is cf.domain and s.target is ift.DomainTuple.scalar_domain()
    t = s + lh3
    assert isinstance(t, _LikelihoodSum) and t._ops == (lh1, lh2, lh3)
    assert (lh1 + (lh2 + lh3))._ops == (lh1, lh2, lh3)
    assert _LikelihoodSum.make([lh1]) is lh1
    assert "_LikelihoodSum" in repr(t) and "*Likelihood 2*" in repr(t)


def test_other_operand_pairs_keep_operator_add(lhs):
    cf, lh1, _, _, _ = lhs
    from nifty_amd.operators.operator import _OpSum
    other = ift.Squared2NormOperator(cf.domain)
    assert type(lh1 + other) is _OpSum and type(other + lh1) is _OpSum
    assert type(cf + cf) is _OpSum


def test_names_and_errors(lhs):
    cf, lh1, lh2, lh3, _ = lhs
    assert (lh1 + lh2 + lh3)._all_names() == ["Likelihood 0", "Likelihood 1", "Likelihood 2"]
    lh1.name, lh2.name = "los", "counts"
    try:
        s = lh1 + lh2
        assert s._all_names() == ["los", "counts"]
        assert s.name is None
        with pytest.raises(RuntimeError):
            s.name = "joint"
        lh2.name = "los"
        with pytest.raises(ValueError):
            lh1 + lh2
    finally:
        lh1.name = lh2.name = None
    with pytest.raises(NotImplementedError):
        _LikelihoodSum([lh1, lh2])
    # DomainTuple and MultiDomain domains do not mix
    sp = ift.RGSpace((8, 8))
    plain = ift.GaussianEnergy(domain=sp, sampling_dtype=np.float64)
    with pytest.raises(RuntimeError):
        lh1 + plain


def test_transformation_keys_and_dtypes_match_reference(lhs):
    cf, lh1, lh2, _, G = lhs
    lh1.name, lh2.name = (str(n) for n in G["names"])
    try:
        dtype, tr = (lh1 + lh2).get_transformation()
    finally:
        lh1.name = lh2.name = None
    assert tr.domain is cf.domain
    assert sorted(tr.target.keys()) == [str(k) for k in G["j8_trkeys"]]
    assert [np.dtype(dtype[k]).name for k in sorted(dtype)] == [str(v) for v in G["j8_trdtypes"]]
    assert tr.target["los"].shape == (G["j8_starts"].shape[1],) and tr.target["counts"].shape == (8, 8)
    # a component without a transformation leaves the sum without one

    class NoTrafo(ift.LikelihoodEnergyOperator):
        def __init__(self, dom):
            super().__init__(None, None)
            self._domain = dom

        def get_transformation(self):
            return None
    assert (lh1 + NoTrafo(cf.domain)).get_transformation() is None


def test_multidomain_components_get_prefixed_keys():
    sp = ift.RGSpace((4,))
    dom = ift.MultiDomain.make({"a": sp, "b": sp})
    lh1 = ift.GaussianEnergy(domain=dom, sampling_dtype=np.float64)
    lh2 = ift.GaussianEnergy(domain=dom, sampling_dtype=np.float64)
    lh2.name = "second"
    dtype, tr = (lh1 + lh2).get_transformation()
    want = ["Likelihood 0: a", "Likelihood 0: b", "second: a", "second: b"]
    assert sorted(tr.target.keys()) == want and sorted(dtype) == want
    assert sorted((lh1 + lh2).data_domain.keys()) == want


def test_prepend_key():
    sp, un = ift.RGSpace((4,)), ift.UnstructuredDomain(3)
    dom = ift.MultiDomain.make({"a": sp, "b": un})
    op = ift.PrependKey(dom, "x: ")
    assert op.domain is dom
    assert op.target is ift.MultiDomain.make({"x: a": sp, "x: b": un})
    assert op.capability == op.TIMES | op.ADJOINT_TIMES
    with pytest.raises(ValueError):
        ift.PrependKey(ift.DomainTuple.make(sp), "x")


def test_header_and_signatures_agree_for_new_entries():
    txt = open(os.path.join(ROOT, "include", "nifty_amd.h")).read()
    import ctypes
    code = {"int": ctypes.c_int, "double": ctypes.c_double, "int64_t": ctypes.c_int64}
    for name in ("nft_los_add_blocks", "nft_los_adjoint_add"):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", txt, re.S)
        assert m, name
        args = []
        for a in m.group(1).split(","):
            a = " ".join(a.split())
            if "*" in a or a.startswith("hipStream_t"):
                args.append(ctypes.c_void_p)
            else:
                args.append(code[a.rsplit(" ", 1)[0]])
        res, sig = _native.SIGNATURES[name]
        assert res is ctypes.c_int and list(sig) == args, name
    assert callable(_native.los_adjoint_add)
