"""GPU: the nft_los kernels on box plans outside the ordinary regime, against
the float64 CSR product of the same triplets (R.coo, fp32 weights upcast
exactly).

Plans (tests/los_cases.py, each asserting its regime):
  dense16   (16, 16), 301 lines, one box: 16-bit line indices, tab == false
            (line values from global memory), two adjoint chunks, forward box
            split by segment count; nlos % 4 != 0.
  dense32   (32, 32), 600 lines, four such boxes.
  mixed     (32, 48): one wide box, boxes of 1..256 lines (tab == true in the
            uint16 instantiation) and an empty box in one plan.
  dense1d   (300,): 1 x 256 boxes, a ragged second one, 14 forward items and
            13 adjoint chunks in a box.
  dense3d   (2, 16, 16): two layers, empty rows.
  short16   (16, 16), 302 short lines: more than 256 segments but fewer than
            LOS_CAP_F entries in the box, so the forward split is by segment
            count alone and the adjoint stages a single chunk with tab == false.
  degen, sig  narrow controls (8-bit plans) from los_edge.npz.
  empty     every line beside the grid: no entries at all.

Which instantiation runs: batches of k = 1, 2, 3|4, 5|8 vectors take
los_adj_boxes<T, IDX, K> with K = 1, 2, 4, 8 (k = 3 and 5 masked), IDX =
unsigned short on the plans with lidx8 == 0; `fold=` adds the carried fold,
los_adjoint_add (k = 1, 2, 3, 8) the ADD variant; both dtypes throughout.

Tolerances are derived (los_cases.bound64 / bound32), per element:
|got - ref| <= 2 (n_i + 4) 2^-53 (|A| |v|)_i with the scales inside |v| and
the magnitude, plus 2^-24 |ref| for fp32 storage; exactly 0 where n_i = 0.
Two-stage fused_middle: the same formula with n_i replaced by the largest
column count plus the largest row count (the forward rounds n_l + 3 times, the
adjoint with unit scale n_i + 1 times), the magnitude carried through both
stages, fct |dr| |A^T| (|c| (|A| (|dr| |s|))); with fp32 storage the
intermediate data vector is rounded too, 2^-24 of that magnitude, propagated
through |A^T|.  Quadratic forms sum_l t_l y_l: each t_l within its forward
bound e_l, so 2 e_l |rs_l| T_l per line (T = |A| |v|), plus the sum's own
2 (nlos + 4) 2^-53 sum |rs_l| T_l^2, plus 2^-24 of that sum when y is stored
in fp32.  Every test prints its largest error as a fraction of the bound."""
import ctypes

import numpy as np
import pytest
import torch

import los_cases as lc
from test_los_add_gpu import _inputs, _run

pytestmark = pytest.mark.gpu

PLANS = lc.WIDE + ("degen", "sig", "empty")
KS = (2, 3, 4, 5, 8)
DT = {"f64": torch.float64, "f32": torch.float32}
_CACHE = {}
_WORST = {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


class Case:
    """one plan: the response, its device plan, the float64 reference
    matrices and one set of inputs (8 vectors each side, scales)"""

    def __init__(self, ift, name, dev):
        shape, dist, starts, ends, sigmas, trunc = lc.case(name)
        self.name, self.shape, self.dev = name, shape, dev
        self.R = ift.LOSResponse(ift.RGSpace(shape, distances=dist), starts=list(starts), ends=list(ends),
                                 sigmas=sigmas, truncation=trunc)
        lc.assert_regime(name, self.R._plan_np)
        print(lc.describe(name, self.R._plan_np))
        self.plan = self.R._box_plan()
        self.npix, self.nlos = int(np.prod(shape)), self.R.target.size
        rows, cols, w = self.R.coo
        assert w.dtype == np.float32
        self.A, self.Aabs, self.nrow, self.ncol = lc.csr(rows, cols, w, self.nlos, self.npix)
        rng = np.random.default_rng(17)
        sign = lambda n: np.where(rng.random(n) < 0.5, -1., 1.)  # noqa: E731
        self.X = rng.standard_normal((8, self.npix))
        self.Y = rng.standard_normal((8, self.nlos))
        self.cs = (rng.random(self.npix) + 0.5) * sign(self.npix)       # pixel side
        self.rs = (rng.random(self.nlos) + 0.5) * sign(self.nlos)       # data side
        self.D = (rng.random((8, self.npix)) + 0.5) * sign((8, self.npix))   # per-vector pixel side
        self.nq = (self.nlos + 3) // 4

    def up(self, a, dt):
        """device tensor in dt and the float64 numpy values it holds"""
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(self.dev)
        return t, t.double().cpu().numpy()

    def nan(self, shape, dt):
        return torch.full(shape, float("nan"), dtype=dt, device=self.dev)

    def items_plan(self):
        p = type(self.plan).from_buffer_copy(self.plan)
        p.box_item = None
        return p


def _case(ift, name, dev):
    if name not in _CACHE:
        _CACHE[name] = Case(ift, name, dev)
    return _CACHE[name]


def _close(got, ref, n, mag, dt, what):
    """element-wise |got - ref| <= bound; prints the worst fraction of it"""
    g = got.double().cpu().numpy()
    assert g.shape == ref.shape and not np.isnan(g).any(), f"{what}: unwritten output"
    bnd = lc.bound64(n, mag) if dt == torch.float64 else lc.bound32(n, mag, ref)
    _within(np.abs(g - ref), bnd, dt, what)


def _within(err, bnd, dt, what):
    err, bnd = np.broadcast_arrays(np.asarray(err, dtype=np.float64), np.asarray(bnd, dtype=np.float64))
    pos = bnd > 0
    frac = float((err[pos] / bnd[pos]).max()) if pos.any() else 0.
    key = "f64" if dt == torch.float64 else "f32"
    _WORST[key] = max(_WORST.get(key, 0.), frac)
    print(f"{what} {key}: max err / bound {frac:.3e} (worst so far {_WORST[key]:.3e})")
    assert np.all(err[~pos] == 0.), f"{what}: nonzero where the bound is exactly 0"
    assert np.all(err <= bnd), f"{what}: {frac:.3e} of the bound"


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_forward(ift, dev, name, dtn):
    """los_forward (colscale, rowscale, scale), los_forward_batched and
    los_forward_ex (per-vector colscale) for k = 2, 3, 4, 5, 8; a batch is
    bitwise its single calls; the per-item kernel is bitwise the per-box one"""
    from nifty_amd import _native
    c, dt = _case(ift, name, dev), DT[dtn]
    X, Xn = c.up(c.X, dt)
    cs, csn = c.up(c.cs, dt)
    rs, rsn = c.up(c.rs, dt)
    D, Dn = c.up(c.D, dt)
    scale = 0.5

    def ref(xn, coln):
        v = coln * xn
        return scale * rsn * (c.A @ v.T).T, abs(scale) * np.abs(rsn) * (c.Aabs @ np.abs(v).T).T

    single, single_d = [], []
    for j in range(8):
        y = c.nan((c.nlos,), dt)
        _native.los_forward(c.plan, X[j].contiguous(), y, colscale=cs, rowscale=rs, scale=scale)
        single.append(y)
        y = c.nan((c.nlos,), dt)
        _native.los_forward(c.plan, X[j].contiguous(), y, colscale=D[j].contiguous(), rowscale=rs, scale=scale)
        single_d.append(y)
    r, m = ref(Xn, csn)
    _close(torch.stack(single), r, c.nrow, m, dt, f"{name} forward k=1")
    rd, md = ref(Xn, Dn)
    _close(torch.stack(single_d), rd, c.nrow, md, dt, f"{name} forward k=1 per-vector scale")
    items = c.items_plan()
    for k in KS:
        y = c.nan((k, c.nlos), dt)
        _native.los_forward_batched(c.plan, X[:k].contiguous(), y, colscale=cs, rowscale=rs, scale=scale)
        _close(y, r[:k], c.nrow, m[:k], dt, f"{name} forward_batched k={k}")
        assert torch.equal(y, torch.stack(single[:k])), k
        yi = c.nan((k, c.nlos), dt)
        _native.los_forward_batched(items, X[:k].contiguous(), yi, colscale=cs, rowscale=rs, scale=scale)
        assert torch.equal(yi, y), k
        y = c.nan((k, c.nlos), dt)
        _native.los_forward_ex(c.plan, X[:k].contiguous(), y, colscale=D[:k].contiguous(), rowscale=rs, scale=scale)
        _close(y, rd[:k], c.nrow, md[:k], dt, f"{name} forward_ex k={k}")
        assert torch.equal(y, torch.stack(single_d[:k])), k
        yi = c.nan((k, c.nlos), dt)
        _native.los_forward_ex(items, X[:k].contiguous(), yi, colscale=D[:k].contiguous(), rowscale=rs, scale=scale)
        assert torch.equal(yi, y), k


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_adjoint(ift, dev, name, dtn):
    """los_adjoint (colscale, rowscale, scale), los_adjoint_batched and
    los_adjoint_ex (per-vector rowscale) for k = 2, 3, 4, 5, 8; a batch is
    bitwise its single calls"""
    from nifty_amd import _native
    c, dt = _case(ift, name, dev), DT[dtn]
    Y, Yn = c.up(c.Y, dt)
    cs, csn = c.up(c.rs, dt)      # data side, on the way in
    rs, rsn = c.up(c.cs, dt)      # pixel side, on the way out
    D, Dn = c.up(c.D, dt)
    scale = 2.0

    def ref(rown):
        v = csn * Yn
        return scale * rown * (c.A.T @ v.T).T, abs(scale) * np.abs(rown) * (c.Aabs.T @ np.abs(v).T).T

    single, single_d = [], []
    for j in range(8):
        o = c.nan((c.npix,), dt)
        _native.los_adjoint(c.plan, Y[j].contiguous(), o, colscale=cs, rowscale=rs, scale=scale)
        single.append(o)
        o = c.nan((c.npix,), dt)
        _native.los_adjoint(c.plan, Y[j].contiguous(), o, colscale=cs, rowscale=D[j].contiguous(), scale=scale)
        single_d.append(o)
    r, m = ref(rsn)
    _close(torch.stack(single), r, c.ncol, m, dt, f"{name} adjoint k=1")
    rd, md = ref(Dn)
    _close(torch.stack(single_d), rd, c.ncol, md, dt, f"{name} adjoint k=1 per-vector scale")
    for k in KS:
        o = c.nan((k, c.npix), dt)
        _native.los_adjoint_batched(c.plan, Y[:k].contiguous(), o, colscale=cs, rowscale=rs, scale=scale)
        _close(o, r[:k], c.ncol, m[:k], dt, f"{name} adjoint_batched k={k}")
        assert torch.equal(o, torch.stack(single[:k])), k
        o = c.nan((k, c.npix), dt)
        _native.los_adjoint_ex(c.plan, Y[:k].contiguous(), o, colscale=cs, rowscale=D[:k].contiguous(), scale=scale)
        _close(o, rd[:k], c.ncol, md[:k], dt, f"{name} adjoint_ex k={k}")
        assert torch.equal(o, torch.stack(single_d[:k])), k


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_adjoint_fold_bitwise(ift, dev, name, dtn):
    """los_adjoint_batched(..., fold=...) is the plain call plus a separate
    nft_fold_partials, bitwise in `out` and in the folded scalars (the set-up
    of test_cg_carried_kernels_gpu.py: 3 rows of 40 partials, output stride 2)"""
    from nifty_amd import _native
    c, dt = _case(ift, name, dev), DT[dtn]
    Y, _ = c.up(c.Y, dt)
    rs, _ = c.up(c.cs, dt)
    part, _ = c.up(np.random.default_rng(5).standard_normal((3, 40)), torch.float64)
    ref = c.nan((3, 2), torch.float64)
    _native._check(_native.load().nft_fold_partials(_native.ptr(part), 40, 3, _native.ptr(ref), 2,
                                                    _native.stream_ptr()))
    assert not torch.isnan(ref[:, 0]).any() and torch.isnan(ref[:, 1]).all()
    for k in (1,) + KS:
        plain = c.nan((k, c.npix), dt)
        _native.los_adjoint_batched(c.plan, Y[:k].contiguous(), plain, rowscale=rs)
        got = c.nan((3, 2), torch.float64)
        out = c.nan((k, c.npix), dt)
        _native.los_adjoint_batched(c.plan, Y[:k].contiguous(), out, rowscale=rs,
                                    fold=(part, 40, 3, got.data_ptr(), 2))
        assert not torch.isnan(out).any()
        assert torch.equal(out, plain), k
        assert torch.equal(got[:, 0], ref[:, 0]) and torch.isnan(got[:, 1]).all(), k


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_forward_quad(ift, dev, name, dtn):
    """los_forward_quad_batched: the blocks' partials of every vector summed
    against t . (scale rs t), t = A (cs x); a batch is bitwise its single
    calls, and nothing is written past nft_los_quad_blocks"""
    from nifty_amd import _native
    c, dt = _case(ift, name, dev), DT[dtn]
    assert _native.load().nft_los_quad_blocks(ctypes.byref(c.plan)) == c.nq
    X, Xn = c.up(c.X, dt)
    cs, csn = c.up(c.cs, dt)
    rs, rsn = c.up(c.rs, dt)
    scale = 0.5
    t = (c.A @ (csn * Xn).T).T
    T = (c.Aabs @ np.abs(csn * Xn).T).T
    rsa = np.abs(scale * rsn)
    ref = (t * (scale * rsn * t)).sum(axis=1)
    e = lc.bound64(c.nrow, T)
    bnd = (2. * e * rsa * T).sum(axis=1) + 2. * (c.nlos + 4) * lc.U * (rsa * T * T).sum(axis=1)
    if dt == torch.float32:
        bnd = bnd + lc.U32 * (rsa * T * T).sum(axis=1)
    yref = scale * rsn * t
    ymag = abs(scale) * np.abs(rsn) * T
    singles = []
    for k in (1, 1, 1) + KS:
        j0 = len(singles) if k == 1 else 0
        y = c.nan((k, c.nlos), dt)
        q = c.nan((k, c.nq + 2), torch.float64)
        _native.los_forward_quad_batched(c.plan, X[j0:j0 + k].contiguous(), y, q, colscale=cs, rowscale=rs, scale=scale)
        assert torch.isnan(q[:, c.nq:]).all() and not torch.isnan(q[:, :c.nq]).any()
        _close(y, yref[j0:j0 + k], c.nrow, ymag[j0:j0 + k], dt, f"{name} forward_quad y k={k}")
        got = q[:, :c.nq].sum(dim=1).cpu().numpy()
        _within(np.abs(got - ref[j0:j0 + k]), bnd[j0:j0 + k], dt, f"{name} forward_quad q k={k}")
        if k == 1:
            singles.append((y[0], q[0, :c.nq]))
        else:
            for j in range(min(k, len(singles))):
                assert torch.equal(y[j], singles[j][0]) and torch.equal(q[j, :c.nq], singles[j][1]), (k, j)


@pytest.mark.parametrize("shared", [True, False], ids=["sharedw", "perw"])
@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_adjoint_add(ift, dev, name, dtn, shared):
    """los_adjoint_add for k = 1, 2, 3, 8 (K = 1, 2, 4 masked, 8; the harness of
    test_los_add_gpu.py):
    out against A^T y + w x -- two more roundings, inside the n_i + 4, on the
    magnitude |A^T| |y| + |w x| --, the boxes' partials summed against
    sum w x^2 (bound of an npix-term sum), a batch bitwise its single calls"""
    from nifty_amd import _native
    c, dt = _case(ift, name, dev), DT[dtn]
    nb = _native.load().nft_los_add_blocks(ctypes.byref(c.plan))
    assert nb == c.plan.nbox > 0
    for k in (1, 2, 3, 8):
        y, x, w = _inputs(c.R, k, dt, shared, dev)
        out, q = _run(c.plan, y, w, x, nb)
        assert torch.isnan(q[:, nb:]).all() and not torch.isnan(q[:, :nb]).any()
        yn, xn, wn = (v.double().cpu().numpy() for v in (y, x, w))
        wx = wn * xn
        ref = (c.A.T @ yn.T).T + wx
        mag = (c.Aabs.T @ np.abs(yn).T).T + np.abs(wx)
        _close(out, ref, c.ncol, mag, dt, f"{name} adjoint_add k={k}")
        terms = wx * xn
        got = q[:, :nb].sum(dim=1).cpu().numpy()
        _within(np.abs(got - terms.sum(axis=1)), lc.bound64(c.npix, np.abs(terms).sum(axis=1)), torch.float64,
                f"{name} adjoint_add partials k={k} ({dtn} storage)")
        if name == "empty":
            assert torch.equal(out, (w.double() * x.double()).to(dt))
        for j in range(k):
            wj = w if shared else w[j:j + 1].contiguous()
            oj, qj = _run(c.plan, y[j:j + 1].contiguous(), wj, x[j:j + 1].contiguous(), nb)
            assert torch.equal(oj[0], out[j]) and torch.equal(qj[0, :nb], q[j, :nb]), (k, j)


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", PLANS)
def test_fused_middle(ift, dev, name, dtn):
    """fused_middle(dr, c, fct) on 11 vectors (one launch of 8, then a masked
    4), with and without qpart, against fct dr A^T (c (A (dr s))) in float64"""
    c, dt = _case(ift, name, dev), DT[dtn]
    rng = np.random.default_rng(23)
    k, fct = 11, 0.7
    S, Sn = c.up(rng.standard_normal((k,) + c.shape), dt)
    Sn = Sn.reshape(k, c.npix)
    # the middle keeps its scales in float64 and casts them to the vectors' dtype
    dr64, _ = c.up(c.cs.reshape(c.shape), torch.float64)
    cw64, _ = c.up(c.rs, torch.float64)
    drn, cwn = dr64.to(dt).double().cpu().numpy().ravel(), cw64.to(dt).double().cpu().numpy()
    middle = c.R.fused_middle(dr64, cw64, fct)
    assert middle.quad_blocks == c.nq
    t = (c.A @ (drn * Sn).T).T
    T = (c.Aabs @ np.abs(drn * Sn).T).T
    ref = fct * drn * (c.A.T @ (cwn * t).T).T
    mag = abs(fct) * np.abs(drn) * (c.Aabs.T @ (np.abs(cwn) * T).T).T
    n2 = int(c.nrow.max(initial=0)) + int(c.ncol.max(initial=0))
    bnd = lc.bound64(n2, mag)
    if dt == torch.float32:
        bnd = np.where(mag == 0., 0., np.maximum(bnd + lc.U32 * mag + lc.U32 * np.abs(ref), lc.TINY32))
    out = middle(S)
    assert out.shape == S.shape and out.dtype == dt
    _within(np.abs(out.double().cpu().numpy().reshape(k, c.npix) - ref), bnd, dt, f"{name} fused_middle")
    q = c.nan((k, c.nq + 1), torch.float64)
    out_q = middle(S, qpart=q)
    assert torch.equal(out_q, out)
    assert torch.isnan(q[:, c.nq:]).all() and not torch.isnan(q[:, :c.nq]).any()
    rsa = np.abs(fct * cwn)
    qref = (t * (fct * cwn * t)).sum(axis=1)
    qb = (2. * lc.bound64(c.nrow, T) * rsa * T).sum(axis=1) + 2. * (c.nlos + 4) * lc.U * (rsa * T * T).sum(axis=1)
    if dt == torch.float32:
        qb = qb + lc.U32 * (rsa * T * T).sum(axis=1)
    _within(np.abs(q[:, :c.nq].sum(dim=1).cpu().numpy() - qref), qb, dt, f"{name} fused_middle q")
    # one vector without a batch axis: the K = 1 kernels, bitwise the batch's row
    assert torch.equal(middle(S[0].contiguous()), out[0])


@pytest.mark.parametrize("dtn", list(DT))
def test_empty_plan_writes_exact_zeros(ift, dev, dtn):
    """no entries at all: the forward writes 0 to all nlos outputs, the
    adjoint 0 to every pixel (scales or not, every batch size)"""
    from nifty_amd import _native
    c, dt = _case(ift, "empty", dev), DT[dtn]
    X, _ = c.up(c.X, dt)
    Y, _ = c.up(c.Y, dt)
    cs, _ = c.up(c.cs, dt)
    rs, _ = c.up(c.rs, dt)
    y = c.nan((c.nlos,), dt)
    _native.los_forward(c.plan, X[0].contiguous(), y, colscale=cs, rowscale=rs, scale=0.5)
    assert torch.equal(y, torch.zeros_like(y))
    o = c.nan((c.npix,), dt)
    _native.los_adjoint(c.plan, Y[0].contiguous(), o, colscale=rs, rowscale=cs, scale=2.0)
    assert torch.equal(o, torch.zeros_like(o))
    for k in KS:
        y = c.nan((k, c.nlos), dt)
        _native.los_forward_batched(c.plan, X[:k].contiguous(), y)
        assert torch.equal(y, torch.zeros_like(y)), k
        o = c.nan((k, c.npix), dt)
        _native.los_adjoint_batched(c.plan, Y[:k].contiguous(), o)
        assert torch.equal(o, torch.zeros_like(o)), k
