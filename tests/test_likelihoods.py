"""CPU: BernoulliEnergy, StudentTEnergy and InverseGammaEnergy
(src/operators/energy_operators.py:628-761): exports, constructor checks,
operator algebra, the C declarations of the nft_lh_* entry points and the
keys of tests/golden/likelihoods.npz.  No kernel runs."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

import nifty_amd as ift
from nifty_amd import _native
from nifty_amd.operators.energy_operators import _BernoulliTransform, _LikelihoodChain, _LikelihoodSum

CASES = ("b", "t", "tf", "g", "j", "bs")


def test_names_are_exported():
    for name in ("BernoulliEnergy", "StudentTEnergy", "InverseGammaEnergy", "ConstantOperator"):
        assert hasattr(ift, name), name
    for cls in (ift.BernoulliEnergy, ift.StudentTEnergy, ift.InverseGammaEnergy):
        assert issubclass(cls, ift.LikelihoodEnergyOperator)


def test_bernoulli_constructor_errors():
    sp = ift.RGSpace((4,))
    with pytest.raises(TypeError):
        ift.BernoulliEnergy(ift.makeField(sp, np.array([0., 1., 1., 0.])))
    with pytest.raises(TypeError):
        ift.BernoulliEnergy(np.array([0, 1, 1, 0]))
    with pytest.raises(ValueError):
        ift.BernoulliEnergy(ift.makeField(sp, np.array([0, 1, 2, 0])))
    with pytest.raises(ValueError):
        ift.BernoulliEnergy(ift.makeField(sp, np.array([0, -1, 1, 0])))
    lh = ift.BernoulliEnergy(ift.makeField(sp, np.array([0, 1, 1, 0])))
    assert lh.domain is ift.DomainTuple.make(sp) and lh.target is ift.DomainTuple.scalar_domain()
    assert lh.data_domain is lh.domain
    dtype, tr = lh.get_transformation()
    assert dtype is np.float64 and isinstance(tr, _BernoulliTransform)
    assert tr.domain is lh.domain and tr.target is lh.domain


def test_inverse_gamma_constructor_errors():
    sp = ift.RGSpace((4,))
    beta = ift.makeField(sp, np.array([0.5, 1., 2., 0.1]))
    with pytest.raises(TypeError):
        ift.InverseGammaEnergy(np.array([0.5, 1., 2., 0.1]))
    with pytest.raises(TypeError):
        ift.InverseGammaEnergy(ift.makeField(sp, np.array([0.5, 1., 2., 0.1], dtype=np.float32)))
    with pytest.raises(TypeError):
        ift.InverseGammaEnergy(ift.makeField(sp, np.array([1, 1, 2, 1])))
    with pytest.raises(TypeError):
        ift.InverseGammaEnergy(beta, alpha=np.array([1., 1., 1., 1.]))
    with pytest.raises(TypeError):
        ift.InverseGammaEnergy(beta, alpha="0.5")
    for alpha in (-0.5, 0.7, ift.makeField(sp, np.array([0.1, 0.2, 0.3, 0.4]))):
        lh = ift.InverseGammaEnergy(beta, alpha)
        assert lh.domain is ift.DomainTuple.make(sp)
        dtype, tr = lh.get_transformation()
        assert np.dtype(dtype) == np.float64 and tr.domain is lh.domain
    assert ift.InverseGammaEnergy(beta)._alphap1.val.tolist() == [0.5] * 4


def test_student_t_theta_scalar_or_field():
    sp = ift.RGSpace((4,))
    for theta in (3., ift.makeField(sp, np.array([2., 3., 4., 5.]))):
        lh = ift.StudentTEnergy(sp, theta)
        assert lh.domain is ift.DomainTuple.make(sp)
        dtype, tr = lh.get_transformation()
        assert dtype is np.float64 and isinstance(tr, ift.DiagonalOperator)
    w = ift.StudentTEnergy(sp, 3.).get_transformation()[1].diagonal_tensor.cpu().numpy()
    np.testing.assert_allclose(w, np.sqrt(4. / 6.), rtol=1e-15)


def test_constant_operator():
    sp = ift.RGSpace((4,))
    f = ift.makeField(sp, np.arange(4.))
    op = ift.ConstantOperator(f, domain=sp)
    assert op.domain is ift.DomainTuple.make(sp) and op.target is f.domain
    x = ift.full(sp, 7.)
    assert op(x) is f
    lin = op(ift.Linearization.make_var(x))
    assert lin.val is f and isinstance(lin.jac, ift.NullOperator)
    assert ift.ConstantOperator(f).domain is ift.MultiDomain.make({})


def test_they_are_ordinary_likelihoods():
    """@, .scale, name and lh1 + lh2 as for GaussianEnergy / PoissonianEnergy"""
    sp = ift.RGSpace((4,))
    model = ift.ScalingOperator(ift.DomainTuple.make(sp), 1.).sigmoid()
    b = ift.BernoulliEnergy(ift.makeField(sp, np.array([0, 1, 1, 0]))) @ model
    t = ift.StudentTEnergy(sp, 3.) @ ift.Adder(ift.full(sp, 0.3), neg=True) @ model
    g = ift.InverseGammaEnergy(ift.full(sp, 0.5), 0.7) @ model
    for lh in (b, t, g):
        assert isinstance(lh, _LikelihoodChain) and lh.name is None
        assert lh.get_transformation()[1].domain is model.domain
        s = lh.scale(0.3)
        assert isinstance(s, _LikelihoodChain) and isinstance(s._op._ops[0], ift.ScalingOperator)
        assert isinstance(s.get_transformation()[1]._ops[0], ift.ScalingOperator)
    b.name, t.name = "events", "robust"
    j = b + t + g
    assert isinstance(j, _LikelihoodSum) and j._all_names() == ["events", "robust", "Likelihood 2"]
    dtype, tr = j.get_transformation()
    assert sorted(tr.target.keys()) == ["Likelihood 2", "events", "robust"]
    assert all(np.dtype(v) == np.float64 for v in dtype.values())
    # the Bernoulli transformation stays one chain link of the scaled likelihood
    ops = b.scale(0.3).get_transformation()[1]._ops
    assert sum(isinstance(o, _BernoulliTransform) for o in ops) == 1


def test_pipeline_parses_the_new_chain_links():
    """geovi_batch.Pipeline.parse: a stage for Bernoulli's transformation and
    one for Adder; chains that parsed before keep their stages"""
    from nifty_amd.minimization import geovi_batch as gb
    G = golden("likelihoods.npz")
    sp = ift.RGSpace((8, 8))
    cf = ift.SimpleCorrelatedField(sp, offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
                                   loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
    p = ift.sigmoid(cf)
    b = ift.BernoulliEnergy(ift.makeField(sp, G["l8_events"])) @ p
    t = ift.StudentTEnergy(sp, 3.) @ ift.Adder(ift.makeField(sp, G["l8_tdata"]), neg=True) @ p
    g = ift.InverseGammaEnergy(ift.makeField(sp, G["l8_beta"]), 0.7) @ cf.exp()
    kinds = lambda lh: [type(s).__name__ + (":" + s.kind if isinstance(s, gb._LinStage) else "")  # noqa: E731
                        for s in gb.Pipeline.parse(lh.get_transformation()[1]).stages]
    assert kinds(b) == ["_CFStage", "_PtwStage", "_BernoulliStage"]
    assert kinds(b.scale(0.3)) == ["_CFStage", "_PtwStage", "_BernoulliStage", "_LinStage:scale"]
    assert kinds(t) == ["_CFStage", "_PtwStage", "_AddStage", "_LinStage:diag"]
    assert kinds(g) == ["_CFStage", "_PtwStage", "_LinStage:scale", "_PtwStage", "_LinStage:diag"]
    po = ift.PoissonianEnergy(ift.makeField(sp, G["l8_events"])) @ cf.exp()
    assert kinds(po) == ["_CFStage", "_PtwStage", "_LinStage:scale", "_PtwStage", "_LinStage:scale"]
    # an Adder of a MultiField is no stage
    assert gb.Pipeline.parse([ift.Adder(ift.full(cf.domain, 1.)), cf]) is None


def test_header_and_signatures_agree_for_new_entries():
    txt = open(os.path.join(ROOT, "include", "nifty_amd.h")).read()
    code = {"int": ctypes.c_int, "double": ctypes.c_double, "int64_t": ctypes.c_int64}
    for name in ("nft_lh_transform_pair", "nft_lh_eval_batched"):
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
    assert callable(_native.lh_transform_pair) and callable(_native.lh_eval_batched)
    for kind, macro in ((_native.LH_BERNOULLI, "NFT_LH_BERNOULLI"), (_native.LH_STUDENT_T, "NFT_LH_STUDENT_T"),
                        (_native.LH_INVGAMMA, "NFT_LH_INVGAMMA")):
        assert re.search(r"#define\s+" + macro + r"\s+" + str(kind) + r"\b", txt), macro
    mk = open(os.path.join(ROOT, "joss-nifty_amd", "csrc", "Makefile")).read()
    assert "nft_lh.hip" in mk


def test_fixture_holds_every_key_the_gpu_tests_read():
    G = golden("likelihoods.npz")
    assert tuple(str(c) for c in G["cases"]) == CASES and tuple(G["carry_grid"]) == (8, 8)
    assert len(G["names"]) == 2
    for tag, n in (("l8", 8), ("l16", 16)):
        for k in ("pos", "t", "events", "tdata", "theta", "beta", "gdata"):
            assert f"{tag}_{k}" in G.files, (tag, k)
        assert G[tag + "_events"].shape == (n, n) and set(np.unique(G[tag + "_events"])) <= {0, 1}
        assert G[tag + "_events"].dtype == np.int64
        assert (G[tag + "_beta"] > 0).all() and (G[tag + "_theta"] >= 2).all()
        for c in CASES:
            keys = ["energy", "tr", "mt"]
            if n == 8:
                keys += [f"cg{it}" for it in range(1, 6)] + ["geo_value", "geo_samples"]
            for k in keys:
                assert f"{tag}{c}_{k}" in G.files, (tag, c, k)
            assert G[f"{tag}{c}_mt"].shape == G[tag + "_pos"].shape
        assert G[f"{tag}b_tr"].shape == (n, n)
    assert G["l8b_geo_samples"].shape == (2, G["l8_pos"].size)
