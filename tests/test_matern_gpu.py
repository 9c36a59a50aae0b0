"""GPU: the Matern amplitude kernels (csrc/nft_matern.hip) against the torch
restatement of library/matern.py, and the fused Matern field through the
public interface against the reference (tests/golden/matern.npz,
gen_golden_matern.py).

Tolerances are the project's own for the same kind of comparison (fp64):
  kernels against torch                     rel 1e-12   (test_amp2_gpu.py:97)
  batched against single                    bitwise     (test_amp2_gpu.py:107-110)
  value, J t, J^T g, amplitude vs fixture   1e-10       (test_maker_gpu.py:157-161)
  fused field against the operator tree     1e-11       (test_maker_gpu.py:107-113)
  metric application vs fixture             1e-12       (test_likelihoods_gpu.py)
  5 carried CG steps vs fixture, per key    1e-9        (test_likelihoods_gpu.py:210-219)
  geoVI draw vs fixture, lock-step vs
  per-sample refinement                     1e-8        (test_likelihoods_gpu.py:241,
                                                         test_geovi_batch_gpu.py)
The fixture's own conditioning bound (<case>_cond < 1e-12: how far the
reference's iterates move under a 1e-15 change of the right-hand side) is
checked here too, so the 1e-9 means something.

Kernel grids: B of (8, 8), (16,) and (6, 8, 4) (a few bins: one workgroup,
odd and even B) and of (128, 128), whose B spans more than two reduction
tiles of 512 bins and is no multiple of the tile."""
import numpy as np
import pytest
import torch

from conftest import golden
from test_matern import CASES, MATERN, maker, unpack

pytestmark = pytest.mark.gpu

TILE = 512      # bins per reduction workgroup (MTILE of nft_matern.hip)
GRIDS = {"g8": ((8, 8), 0.1), "g16": ((16,), 0.3), "g3d": ((6, 8, 4), None), "g128": ((128, 128), 0.1)}
_AMPS = {}


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


# ------------------------------------------------------------------ kernels
SIZE = 6                                     # packed row: 4 keys and 2 unused slots


def amp_model(ift, grid, zm):
    """(amplitude model, key offsets in a packed row), built once per case"""
    from nifty_amd.library.matern import _MaternAmplitudeModel
    if (grid, zm) not in _AMPS:
        shape, dist = GRIDS[grid]
        sp = ift.RGSpace(shape, distances=dist)
        amp = _MaternAmplitudeModel(sp.get_default_codomain(), (0.5, 0.2) if zm else None, *MATERN,
                                    sp.total_volume, "p_")
        off = {amp.k_slope: 0, amp.k_zm: 1, amp.k_cutoff: 3, amp.k_scale: 4}
        if not zm:
            del off[amp.k_zm]
        _AMPS[(grid, zm)] = amp, off
    return _AMPS[(grid, zm)]


def rows(k, seed, dev, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (scale * torch.randn((k, SIZE), dtype=torch.float64, generator=g)).to(dev)


def lat_of(amp, off, X, r):
    return {key: X[r, o].clone() for key, o in off.items()}


@pytest.mark.parametrize("zm", [True, False])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_forward_against_torch(ift, dev, grid, zm):
    amp, off = amp_model(ift, grid, zm)
    if grid == "g128":
        assert amp.B > 2 * TILE and amp.B % TILE != 0
    X = rows(3, 1, dev, 0.5)
    lin = amp.forward_rows(amp._ptrs(X, off), 3, SIZE, dev)
    Bp = (amp.B + 1) // 2 * 2
    assert lin.buf.shape == (3, 3 * Bp)
    for r in range(3):
        a, c = amp.forward(lat_of(amp, off, X, r))
        assert rel(lin.a[r], a) < 1e-12
        for j, n in enumerate(("gs", "gc", "gl")):
            assert rel(lin.buf[r, j * Bp:j * Bp + amp.B], c[n]) < 1e-12, n
        if not zm:
            assert float(lin.a[r, 0]) == 0.0
    one = amp.forward_native(lat_of(amp, off, X, 1))
    assert torch.equal(one.a[0], lin.a[1])
    for j in range(3):      # the pad slot of an odd B is never written or read
        assert torch.equal(one.buf[0, j * Bp:j * Bp + amp.B], lin.buf[1, j * Bp:j * Bp + amp.B])


def _consts(amp, off, X, mode, k):
    """(const, item_consts, per-row torch caches) for item_mode 0 / 1 / 2"""
    dev = X.device
    if mode == 1:
        lin = amp.forward_rows(amp._ptrs(X, off), k, SIZE, dev)
        return lin, lin.dconst.data_ptr(), [amp.forward(lat_of(amp, off, X, r))[1] for r in range(k)], lin
    c = amp.forward(lat_of(amp, off, X, 0))[1]
    if mode == 0:
        const, keep = amp.native_const(c)
        return const, None, [c] * k, keep
    lin = amp.forward_native(lat_of(amp, off, X, 0))
    return lin, None, [c] * k, lin


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("k", [1, 3, 4, 8])
@pytest.mark.parametrize("zm", [True, False])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_jvp_vjp_against_torch(ift, dev, grid, zm, k, mode):
    amp, off = amp_model(ift, grid, zm)
    X = rows(k, 2, dev, 0.5)
    const, items, caches, keep = _consts(amp, off, X, mode, k)
    T = rows(k, 3, dev)
    want = torch.stack([amp.jvp(caches[r], lat_of(amp, off, T, r)) for r in range(k)])
    planar = torch.full((k, amp.B), float("nan"), dtype=torch.float64, device=dev)
    amp.native_jvp_batched(const, T, off, planar, item_consts=items)
    assert rel(planar, want) < 1e-12
    il = torch.full((amp.B, k), float("nan"), dtype=torch.float64, device=dev)
    amp.native_jvp_batched(const, T, off, il, interleave=True, item_consts=items)
    assert torch.equal(il.t().contiguous(), planar)
    # VJP with and without the shift * d term; the slots of no key stay untouched
    g = torch.randn((k, amp.B), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(dev)
    D = rows(k, 5, dev)
    for shift in (0.0, 0.7):
        Q = torch.full((k, SIZE), 7.0, dtype=torch.float64, device=dev)
        amp.native_vjp_batched(const, g, Q, off, D=D, shift=shift, item_consts=items)
        for r in range(k):
            ref = amp.vjp(caches[r], g[r])
            # the whole cotangent to rel 1e-12, each key within 1e-12 of its
            # norm (a key is a sum with cancellation: _close_keys of
            # test_amp2_gpu.py)
            want = np.array([float(ref[key]) + shift * float(D[r, o]) for key, o in off.items()])
            got = np.array([float(Q[r, o]) for o in off.values()])
            assert rel(got, want) < 1e-12, (r, shift)
            assert np.abs(got - want).max() <= 1e-12 * np.linalg.norm(want), (r, shift)
        untouched = [o for o in range(SIZE) if o not in off.values()]
        assert bool((Q[:, untouched] == 7.0).all())


@pytest.mark.parametrize("k", [4, 8])
@pytest.mark.parametrize("zm", [True, False])
@pytest.mark.parametrize("grid", ["g8", "g16", "g128"])
def test_batched_is_bitwise_single(ift, dev, grid, zm, k):
    amp, off = amp_model(ift, grid, zm)
    X = rows(1, 2, dev, 0.5)
    lin = amp.forward_native(lat_of(amp, off, X, 0))
    T = rows(k, 3, dev)
    g = torch.randn((k, amp.B), dtype=torch.float64, generator=torch.Generator().manual_seed(4)).to(dev)
    D = rows(k, 5, dev)
    da = torch.empty((k, amp.B), dtype=torch.float64, device=dev)
    il = torch.empty((amp.B, k), dtype=torch.float64, device=dev)
    Q = torch.zeros((k, SIZE), dtype=torch.float64, device=dev)
    amp.native_jvp_batched(lin, T, off, da)
    amp.native_jvp_batched(lin, T, off, il, interleave=True)
    amp.native_vjp_batched(lin, g, Q, off, D=D, shift=0.3)
    for r in range(k):
        da1 = torch.empty((1, amp.B), dtype=torch.float64, device=dev)
        Q1 = torch.zeros((1, SIZE), dtype=torch.float64, device=dev)
        amp.native_jvp_batched(lin, T[r:r + 1].contiguous(), off, da1)
        amp.native_vjp_batched(lin, g[r:r + 1].contiguous(), Q1, off, D=D[r:r + 1].contiguous(), shift=0.3)
        assert torch.equal(da1[0], da[r]) and torch.equal(da1[0], il[:, r]), r
        assert torch.equal(Q1[0], Q[r]), r


def test_argument_checks(ift, dev):
    """NFT_ERR_ARG instead of a launch: B < 2, nrhs < 1, a NULL required
    pointer, rows that overlap"""
    import ctypes
    from nifty_amd import _native
    lib = _native.load()
    amp, off = amp_model(ift, "g8", True)
    lin = amp.forward_native(lat_of(amp, off, rows(1, 2, dev, 0.5), 0))
    T = rows(4, 3, dev)
    t4 = amp._key_ptrs(T, off)
    da = torch.zeros((4, amp.B), dtype=torch.float64, device=dev)
    P, s = ctypes.c_void_p, _native.stream_ptr()
    host, ic = lin.host, P(lin.items(1))

    def jvp(h=host, t=t4, d=da, ds=amp.B, es=1, n=4, mode=2, items=ic):
        return lib.nft_matern_jvp_batched(ctypes.byref(h), items, mode, t, SIZE, P(d.data_ptr()) if d is not None
                                          else None, ds, es, n, 0, s)
    assert jvp() == 0
    small = _native.MaternConst()
    small.B, small.has_zm = 1, 1
    assert jvp(h=small) == -1
    assert jvp(n=0) == -1 and jvp(d=None) == -1 and jvp(t=None) == -1 and jvp(items=None) == -1
    assert jvp(ds=amp.B - 1) == -1            # planar rows overlap
    assert jvp(ds=1, es=3) == -1              # bin-major runs shorter than nrhs
    assert b"nft_matern_jvp_batched" in lib.nft_last_error()
    assert jvp(ds=1, es=4) == 0
    g = torch.zeros((4, amp.B), dtype=torch.float64, device=dev)
    Q = torch.zeros((4, SIZE), dtype=torch.float64, device=dev)
    q4 = amp._key_ptrs(Q, off)
    ws = _native.workspace(4 * lib.nft_matern_workspace(amp.B), dev, "matern")

    def vjp(gs=amp.B, out=q4, ls=SIZE, n=4, w=ws, gg=g):
        return lib.nft_matern_vjp_batched(ctypes.byref(host), ic, 2, P(gg.data_ptr()) if gg is not None else None,
                                          gs, out, None, ls, 0.0, P(w.data_ptr()) if w is not None else None, n, s)
    assert vjp() == 0
    assert vjp(gs=amp.B - 1) == -1 and vjp(ls=0) == -1 and vjp(n=0) == -1
    assert vjp(out=None) == -1 and vjp(w=None) == -1 and vjp(gg=None) == -1
    assert lib.nft_matern_workspace(1) == 0 and lib.nft_matern_forward_buf(1) == 0
    torch.cuda.synchronize()


# -------------------------------------------------------------------- field
def _lin(ift, op, x):
    return op(ift.Linearization.make_var(x))


@pytest.mark.parametrize("tag", list(CASES))
def test_field_against_reference_and_operator_tree(ift, tag):
    from nifty_amd.library.correlated_fields_simple import _FusedFieldBase, _MaternFieldModel
    G = golden("matern.npz")
    cfm = maker(ift, **CASES[tag])
    op = cfm.finalize(prior_info=0)
    assert isinstance(op, _MaternFieldModel)
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
    assert rel(cfm.amplitude.force(x).val, G[tag + "_amp"]) < 1e-10
    # the reference's operator tree from the same maker
    cfm._fusable = lambda: False
    tree = cfm.finalize(prior_info=0)
    assert not isinstance(tree, _FusedFieldBase)
    assert sorted(tree.domain.keys()) == sorted(op.domain.keys())
    lt = _lin(ift, tree, x)
    assert rel(lin.val.val, lt.val.val) < 1e-11
    assert rel(lin.jac(t).val, lt.jac(t).val) < 1e-11
    jt = lt.jac.adjoint(g)
    for k in op.domain.keys():
        assert rel(ja[k].val, jt[k].val) < 1e-11, k


# ------------------------------------------------------------ metric and CG
_PROBLEMS = {}


def problem(ift, tag):
    """(cf, likelihood, pos, t, G) of a metric case, built once"""
    if tag not in _PROBLEMS:
        G = golden("matern.npz")
        assert tag in [str(c) for c in G["metric_cases"]]
        assert float(G[tag + "_cond"]) < 1e-12
        cf = maker(ift, **CASES[tag]).finalize(prior_info=0)
        sp = cf.target[0]
        N = ift.ScalingOperator(cf.target, 1e-2, np.float64)
        lh = ift.GaussianEnergy(ift.makeField(sp, G[tag + "_data"]), inverse_covariance=N.inverse) @ ift.sigmoid(cf)
        _PROBLEMS[tag] = (cf, lh, unpack(ift, cf.domain, G[tag + "_pos"]), unpack(ift, cf.domain, G[tag + "_t"]), G)
    return _PROBLEMS[tag]


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_metric_against_reference(ift, tag):
    cf, lh, pos, t, G = problem(ift, tag)
    met = lh.get_metric_at(pos)
    assert met.fused is not None
    got, ref = met(t), unpack(ift, cf.domain, G[tag + "_mt"])
    for k in cf.domain.keys():
        assert rel(got[k].val, ref[k].val) < 1e-12, k


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_five_carried_cg_steps(ift, tag):
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    assert shift == 1.0 and core.cg_blocks(1) > 0
    assert fused_cg._carry_flavour(core, 1) == "seg"
    cg = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=5))
    cg.run(ift.QuadraticEnergy(0 * t, A, t))
    assert cg.path == "carry+chunk", cg.path
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


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_batched_solve_is_bitwise_single(ift, tag):
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
    es = [ift.QuadraticEnergy(0 * b, A, b) for b in _rhs(ift, cf, 4)]
    single = [fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=6)).run(e) for e in es]
    cg = fused_cg.FusedCGBatch(core, W, shift, [ift.GradientNormController(iteration_limit=6) for _ in es])
    bat = cg.run(es)
    assert cg.path == "carry+chunk", cg.path
    for (e1, s1), (e2, s2) in zip(single, bat):
        assert s1 == s2
        for k in cf.domain.keys():
            assert torch.equal(e1.position[k].val, e2.position[k].val), k


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_fp32_request_leaves_the_solve_in_fp64(ift, tag):
    from nifty_amd import config
    from nifty_amd.minimization import fused_cg
    cf, lh, pos, t, G = problem(ift, tag)
    A = lh.get_metric_at(pos) + ift.ScalingOperator(cf.domain, 1., float)
    core, W, shift = fused_cg.fusable_metric(A)
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


# -------------------------------------------------------------------- geoVI
def _geo_draw(ift, lh, pos):
    H = ift.StandardHamiltonian(lh, ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=4))
    mini = ift.NewtonCG(ift.AbsDeltaEnergyController(deltaE=1e-10, iteration_limit=1))
    ift.random.push_sseq_from_seed(27)
    kl = ift.SampledKLEnergy(pos, H, 1, mini, True)
    ift.random.pop_sseq()
    return kl


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_geovi_draw_matches_reference(ift, tag):
    cf, lh, pos, t, G = problem(ift, tag)
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


@pytest.mark.parametrize("tag", ["m8z", "m8"])
def test_lockstep_refinement_is_taken_and_matches_per_sample(ift, tag):
    from nifty_amd.minimization import geovi_batch
    cf, lh, pos, t, G = problem(ift, tag)
    dtype, f_lh = lh.get_transformation()
    mini = ift.NewtonCG(ift.GradientNormController(iteration_limit=1))
    assert geovi_batch.plan(mini, f_lh, None, pos) is not None
    bat = _geo_draw(ift, lh, pos)
    geovi_batch.ENABLED = False
    try:
        assert geovi_batch.plan(mini, f_lh, None, pos) is None
        seq = _geo_draw(ift, lh, pos)
    finally:
        geovi_batch.ENABLED = True
    for i in range(2):
        a, b = pack(bat.samples.local_item(i)), pack(seq.samples.local_item(i))
        assert np.all(np.isfinite(a))
        assert rel(a, b) < 1e-8, i
    assert abs(bat.value - seq.value) <= 1e-8 * abs(seq.value)
