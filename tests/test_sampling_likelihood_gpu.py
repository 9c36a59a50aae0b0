"""GPU: likelihoods on MaskOperator / LinearInterpolator responses through the
public interface, against the reference's values (tests/golden/sampling.npz,
gen_golden_sampling.py).

Cases on a SimpleCorrelatedField, s8 = 8 x 8 (the smallest 2-D grid on which
the carried CG iteration runs) and s16 = 16 x 16:
  a  sigmoid -> LinearInterpolator (40 points) -> Gaussian 1e-3
  b  exp -> MaskOperator (about half the pixels flagged) -> Poisson
  c  a + b as lh1 + lh2

Tolerances are those of test_joint_likelihood_gpu.py: metric / transformation
1e-12 (relative max-norm), energy 1e-10, 5 carried CG steps 1e-9, short geoVI
draws 1e-8; batched against per-sample refinement as test_geovi_batch_gpu.py
(10x the per-sample path's own sensitivity, floor 1e-8, where the decision
traces are stable).

The fixture stores a MultiField as one vector: its keys in sorted order, each
raveled."""
import numpy as np
import pytest
import torch

from conftest import golden

pytestmark = pytest.mark.gpu

CF_ARGS = dict(offset_mean=0, offset_std=(1e-3, 1e-6), fluctuations=(1., 0.8),
               loglogavgslope=(-3., 1), flexibility=(2, 1.), asperity=(0.5, 0.4))
SIZES = {"s8": 8, "s16": 16}
CASES = ("a", "b", "c")
_CACHE = {}


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
    """(cf, {a, b, c: likelihood}, pos, t, G), built once per grid"""
    if tag not in _CACHE:
        G = golden("sampling.npz")
        assert tuple(G["carry_grid"]) == (8, 8)
        n = SIZES[tag]
        sp = ift.RGSpace((n, n))
        cf = ift.SimpleCorrelatedField(sp, **CF_ARGS)
        R = ift.LinearInterpolator(sp, G[tag + "_pts"])
        M = ift.MaskOperator(ift.makeField(sp, G[tag + "_flags"]))
        N = ift.ScalingOperator(R.target, 1e-3, np.float64)
        lh1 = ift.GaussianEnergy(ift.makeField(R.target, G[tag + "_data"]),
                                 inverse_covariance=N.inverse) @ R(ift.sigmoid(cf))
        lh2 = ift.PoissonianEnergy(ift.makeField(M.target, G[tag + "_counts"])) @ M(cf.exp())
        lh1.name, lh2.name = (str(v) for v in G["names"])
        lhs = dict(a=lh1, b=lh2, c=lh1 + lh2)
        _CACHE[tag] = (cf, lhs, unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"]), G)
    return _CACHE[tag]


def geovi_sandwich(ift, lh, pos):
    dtype, f = lh.get_transformation()
    fl = f(ift.Linearization.make_var(pos))
    return ift.SandwichOperator.make(fl.jac, ift.ScalingOperator(f.target, 1., dtype))


# ------------------------------------------------------------ golden parity
@pytest.mark.parametrize("tag", list(SIZES))
@pytest.mark.parametrize("c", CASES)
def test_golden_energy_transformation_metric(ift, tag, c):
    cf, lhs, pos, t, G = problem(ift, tag)
    lh, pre = lhs[c], tag + c
    e = lh(pos).val.item()
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


# ------------------------------------------------------------------- fusion
@pytest.mark.parametrize("tag", list(SIZES))
def test_middles(ift, tag):
    from nifty_amd import _native
    cf, lhs, pos, t, G = problem(ift, tag)
    sa, sb, sc = (geovi_sandwich(ift, lhs[c], pos) for c in CASES)
    # a: the interpolator's two launches with the curvature partials
    W = sa.fused[1]
    assert callable(W) and W.supports_batch and W.supports_fp32 and not W.supports_fold
    assert W.quad_blocks == _native.samp_quad_blocks(W.samp_plan) == 1
    # b: a mask's sandwich is diagonal -- the pointwise path, a grid tensor
    Wb = sb.fused[1]
    assert torch.is_tensor(Wb) and Wb.dtype == torch.float64 and Wb.is_contiguous()
    assert Wb.shape == cf.target.shape and sb.fused[0] is sa.fused[0]
    flags = torch.from_numpy(G[tag + "_flags"]).to(Wb.device)
    assert not Wb[flags].any() and (Wb[~flags] > 0).all()
    # c: the generic sum of both (no fused interpolator + tensor middle)
    Wc = sc.fused[1]
    assert callable(Wc) and Wc.quad_blocks == 0 and len(Wc.parts) == 2 and Wc.supports_batch


def test_mask_plus_los_takes_the_fused_los_add_middle(ift):
    """LOS data + masked counts: the mask branch is a tensor, so the joint
    middle is the nft_los_adjoint_add one"""
    import ctypes
    from nifty_amd import _native
    cf, lhs, pos, t, G = problem(ift, "s16")
    sp = cf.target[0]
    rng = np.random.default_rng(5)
    R = ift.LOSResponse(sp, starts=list(rng.random((2, 25))), ends=list(rng.random((2, 25))))
    N = ift.ScalingOperator(R.target, 1e-2, np.float64)
    lhl = ift.GaussianEnergy(ift.full(R.target, 0.4), inverse_covariance=N.inverse) @ R(ift.sigmoid(cf))
    lhl.name = "los"
    lh = lhl + lhs["b"]
    sand = geovi_sandwich(ift, lh, pos)
    assert sand.fused is not None
    W = sand.fused[1]
    lib = _native.load()
    plan = W.los.plan
    assert W.quad_blocks == lib.nft_los_quad_blocks(ctypes.byref(plan)) + lib.nft_los_add_blocks(ctypes.byref(plan))
    assert torch.is_tensor(W.addw)
    parts = lhl.get_metric_at(pos)(t) + lhs["b"].get_metric_at(pos)(t)
    joint = sand(t)
    for k in cf.domain.keys():
        assert relmax(joint[k].val.cpu().numpy(), parts[k].val.cpu().numpy()) < 1e-12, k


# -------------------------------------------------------------------- solve
@pytest.mark.parametrize("c", CASES)
def test_five_cg_steps(ift, c):
    from nifty_amd.minimization import fused_cg
    cf, lhs, pos, t, G = problem(ift, "s8")
    A = lhs[c].get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0
    if c != "c":
        cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5))
        cg.run(ift.QuadraticEnergy(0 * t, A, t))
        assert cg.path == "carry+chunk", cg.path
    for it in range(1, 6):
        ic = ift.GradientNormController(iteration_limit=it)
        en, st = ift.ConjugateGradient(ic)(ift.QuadraticEnergy(0 * t, A, t))
        assert st == ic.CONVERGED
        ref = unpack(ift, cf.domain, G[f"s8{c}_cg{it}"])
        for k in cf.domain.keys():
            err = rel(en.position[k].val.cpu().numpy(), ref[k].val.cpu().numpy())
            print(c, it, "CG steps", k, err)
            assert err < 1e-9, (it, k)


# -------------------------------------------------------------------- geoVI
@pytest.mark.parametrize("c", CASES)
def test_geovi_draw_matches_reference(ift, c):
    cf, lhs, pos, t, G = problem(ift, "s8")
    H = ift.StandardHamiltonian(lhs[c], ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    ref = G[f"s8{c}_geo_samples"]
    assert kl.samples.n_samples == len(ref) == 2
    for i in range(2):
        err = rel(pack(kl.samples.local_item(i)), ref[i])
        print(c, "geoVI sample", i, err)
        assert err < 1e-8, i
    ev = abs(kl.value - float(G[f"s8{c}_geo_value"])) / abs(float(G[f"s8{c}_geo_value"]))
    print(c, "geoVI KL value", ev)
    assert ev < 1e-8


@pytest.mark.parametrize("c", ("a", "b"))
def test_batched_refinement_is_taken_and_lowers(ift, c):
    from nifty_amd.lowering import lowered_metric
    from nifty_amd.minimization import geovi_batch
    cf, lhs, pos, t, G = problem(ift, "s16")
    lh = lhs[c]
    dtype, f_lh = lh.get_transformation()
    mini = ift.NewtonCG(ift.GradientNormController(iteration_limit=1))
    assert geovi_batch.plan(mini, f_lh, None, pos) is not None
    # the geoVI Newton metric (1 + A^T B)^T (1 + A^T B) lowers to native calls
    fl = f_lh(ift.Linearization.make_var(pos))
    transformation = ift.ScalingOperator(f_lh.domain, 1.) + fl.jac.adjoint @ f_lh
    x = pos + 0.05 * t
    en = ift.EnergyAdapter(x, ift.GaussianEnergy(transformation(pos)) @ transformation, want_metric=True)
    M = en.metric
    lm = lowered_metric(M)
    assert lm is not None
    ref = M(t)
    lay = lm.layout
    q = lay.empty()
    lm.metric_flat(lay.pack(t), q, None, 0.5)
    out = lay.unpack(q)
    for k in cf.domain.keys():
        assert rel(out[k].val.cpu().numpy(), (ref[k] + 0.5 * t[k]).val.cpu().numpy()) < 1e-12, k


def _draw(ift, cf, H, pos, batched):
    """one geoVI draw (2 mirrored pairs, 2 Newton steps of 5 CG iterations)
    with the decision trace on: (flat residual samples, trace events)"""
    from nifty_amd.minimization import geovi_batch, trace
    geovi_batch.ENABLED = batched
    trace.TRACE = []
    try:
        mini = ift.NewtonCG(ift.GradientNormController(iteration_limit=2), max_cg_iterations=5)
        ift.random.push_sseq_from_seed(5)
        sl = ift.draw_samples(pos, H, mini, 2, True)
        ift.random.pop_sseq()
        ev = trace.TRACE
    finally:
        trace.TRACE = None
        geovi_batch.ENABLED = True
    res = [np.concatenate([np.ravel(r[k].val.cpu().numpy()) for k in cf.domain.keys()]) for r in sl._r]
    return res, ev


@pytest.mark.parametrize("c", ("a", "b"))
def test_batched_refinement_matches_per_sample(ift, c):
    """as tests/test_geovi_batch_gpu.py: the same decisions per sample, the
    samples within 10x the per-sample path's own sensitivity (floor 1e-8)
    where the decision traces are stable"""
    from trace_compare import compare, our_events
    cf, lhs, pos, t, G = problem(ift, "s16")
    H = ift.StandardHamiltonian(lhs[c], ift.GradientNormController(iteration_limit=100))
    bat, ebat = _draw(ift, cf, H, pos, True)
    seq, eseq = _draw(ift, cf, H, pos, False)
    sens, epert = 0.0, []
    for f in (1 + 1e-15, 1 - 1e-15):
        pp = ift.MultiField.from_dict({k: (v * f if k == "xi" else v) for k, v in pos.items()})
        per, ep = _draw(ift, cf, H, pp, False)
        epert.append(ep)
        sens = max([sens] + [np.linalg.norm(a - b) / np.linalg.norm(b) for a, b in zip(per, seq)])
    all_stable = True
    for s in range(4):
        n, stable, worst, log = compare(our_events(ebat, s), our_events(eseq, s),
                                        [our_events(e, s) for e in epert])
        print(f"{c} sample {s}: {n} events, stable={stable}, worst {worst:.3g}", *log)
        all_stable &= stable
    tol = max(1e-8, 10 * sens)
    for a, b in zip(bat, seq):
        assert np.all(np.isfinite(a))
        err = np.linalg.norm(a - b) / np.linalg.norm(b)
        print(c, "batched vs per sample", err, "tol", tol, "stable", all_stable)
        if all_stable:
            assert err <= tol, (c, err, sens)
