"""GPU: the row interface shared by the responses that can stand in the middle
of a fused sampling metric (operators/middle.py)

    R._fwd(V, colscale=None, rowscale=None, scale=1.0, qpart=None) -> (k, ndata)
    R._adj(Y, colscale=None, rowscale=None, scale=1.0, ...)        -> (k, npix)

on LOSResponse, LinearInterpolator, MaskOperator and FuncConvolutionOperator
(one space and on one space of a product domain), and ResponseMiddle, which is
written against it.

Families (the smallest shapes on which the kernels still take every path the
interface chooses between):
  los2d   32 x 32 grid, 40 random lines: four 16 x 16 boxes, quad_blocks 10
  los1d   512 pixels: two 256-pixel boxes
  interp  16 x 16 grid, 50 points
  mask    16 x 16 grid, a third flagged
  psf     8 x 8, the smallest native grid of test_conv_gpu.py
  psfsp   (8, 8) x 4, the smallest native product domain of
          test_conv_space_gpu.py
k = 1, 3 (a 4-vector group with 3 live vectors) and 9 (crosses the 8-vector
chunk); fp64 everywhere, fp32 for LOS and sampling.

Everything here is bitwise: a batch is the same kernels on the same operands
as its single-vector calls through the _native wrappers, and the middle is the
composition of the two row calls.  The bounds against the float64 oracles are
in test_los_regimes_gpu.py, test_sampling_gpu.py and test_conv*_gpu.py."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

KS = (1, 3, 9)
FAMILIES = ("los2d", "los1d", "interp", "mask", "psf", "psfsp")
DT = {"f64": torch.float64, "f32": torch.float32}
CASES = [(f, d) for f in FAMILIES for d in DT if d == "f64" or not f.startswith("psf")]
_CACHE = {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


def _gauss(sp):
    sig = 1.7 * min(sp.distances)
    return lambda r: np.exp(-0.5 * (r / sig) ** 2)


class Family:
    """one response, how a single vector goes through today's _native
    wrappers, and one set of float64 inputs (9 vectors each side, scales)"""

    def __init__(self, ift, name, dev):
        from nifty_amd import _native
        self.name, self.dev, self.nat = name, dev, _native
        rng = np.random.default_rng(31)
        self.per = not name.startswith("psf")      # per-vector pixel scales: where the kernels take them
        self.fold = name.startswith("los")
        if name == "los2d":
            sp = ift.RGSpace((32, 32), distances=1. / 32)
            self.R = ift.LOSResponse(sp, starts=list(rng.random((2, 40))), ends=list(rng.random((2, 40))))
        elif name == "los1d":
            sp = ift.RGSpace((512,), distances=1. / 512)
            self.R = ift.LOSResponse(sp, starts=list(rng.random((1, 40))), ends=list(rng.random((1, 40))))
        elif name == "interp":
            sp = ift.RGSpace((16, 16), distances=0.25)
            self.R = ift.LinearInterpolator(sp, 4. * rng.random((2, 50)))
        elif name == "mask":
            sp = ift.RGSpace((16, 16))
            self.R = ift.MaskOperator(ift.makeField(sp, (np.arange(256) % 3 == 0).reshape(16, 16)))
        elif name == "psf":
            sp = ift.RGSpace((8, 8), distances=0.1)
            self.R = ift.FuncConvolutionOperator(sp, _gauss(sp))
            assert self.R.native
        else:
            sp = ift.RGSpace((8, 8), distances=0.1)
            dom = ift.DomainTuple.make((sp, ift.RGSpace(4, distances=0.5)))
            self.R = ift.FuncConvolutionOperator.on_space(dom, _gauss(sp), space=0)
            assert self.R.native
        self.shape = tuple(self.R.domain.shape)
        self.npix, self.ndata = self.R.domain.size, self.R.target.size
        self.nq = self.R.quad_blocks()
        assert self.nq > 0
        if name == "los2d":
            assert self.R._plan_np["nbox"] == 4 and self.nq == 10
        if name == "los1d":
            assert self.R._plan_np["nbox"] == 2
        if name == "mask":
            assert self.ndata == 256 - 86
        sign = lambda n: np.where(rng.random(n) < 0.5, -1., 1.)  # noqa: E731
        self.V = rng.standard_normal((9, self.npix))
        self.Y = rng.standard_normal((9, self.ndata))
        self.cs = (rng.random(self.npix) + 0.5) * sign(self.npix)                # pixel side, shared
        self.D = (rng.random((9, self.npix)) + 0.5) * sign((9, self.npix))       # pixel side, per vector
        self.rs = (rng.random(self.ndata) + 0.5) * sign(self.ndata)              # data side

    def up(self, a, dt):
        return torch.from_numpy(np.ascontiguousarray(a)).to(dt).to(self.dev)

    def nan(self, shape, dt):
        return torch.full(shape, float("nan"), dtype=dt, device=self.dev)

    def single_fwd(self, x, colscale, rowscale, scale):
        """(y, q[:nq]) of one vector x (npix,): the value from the family's
        single-vector call, the partials from its one-row call with qpart"""
        n = self.nat
        y = self.nan((1, self.ndata), x.dtype)
        q = self.nan((1, self.nq), torch.float64)
        if self.fold:
            plan = self.R._box_plan()
            n.los_forward(plan, x, y[0], colscale=colscale, rowscale=rowscale, scale=scale)
            yq = self.nan((1, self.ndata), x.dtype)
            n.los_forward_quad_batched(plan, x.reshape(1, -1), yq, q, colscale=colscale, rowscale=rowscale,
                                       scale=scale)
            assert torch.equal(yq, y)
        elif self.per:
            n.samp_forward(self.R._samp_plan(), x.reshape(1, -1), y, colscale=colscale, rowscale=rowscale,
                           scale=scale, qpart=q)
        else:
            self.R.apply_rows(x.reshape(1, -1), colscale=colscale, rowscale=rowscale, scale=scale, qpart=q, out=y)
        assert not torch.isnan(y).any() and not torch.isnan(q).any()
        return y[0], q[0]

    def single_adj(self, y, colscale, rowscale, scale):
        n = self.nat
        o = self.nan((1, self.npix), y.dtype)
        if self.fold:
            n.los_adjoint(self.R._box_plan(), y, o[0], colscale=colscale, rowscale=rowscale, scale=scale)
        elif self.per:
            n.samp_adjoint(self.R._samp_plan(), y.reshape(1, -1), o, colscale=colscale, rowscale=rowscale,
                           scale=scale)
        else:
            self.R.apply_rows(y.reshape(1, -1), colscale=colscale, rowscale=rowscale, scale=scale, out=o)
        assert not torch.isnan(o).any()
        return o[0]

    def middle(self, dr, c, fct):
        from nifty_amd.operators.middle import ResponseMiddle
        if self.name == "mask":
            # MaskOperator.fused_middle is a grid tensor (R^T C R is diagonal);
            # the class serves the mask all the same
            return ResponseMiddle(self.R, dr, c, fct)
        m = self.R.fused_middle(dr, c, fct)
        assert type(m) is ResponseMiddle
        return m


def family(ift, name, dev):
    if name not in _CACHE:
        _CACHE[name] = Family(ift, name, dev)
    return _CACHE[name]


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,dtn", CASES)
def test_forward_rows_are_the_single_calls(ift, dev, name, dtn, k):
    """_fwd with a shared and with per-vector colscale, a data-side rowscale,
    a scalar and qpart: outputs and partial rows bitwise the k single calls;
    qpart columns beyond quad_blocks keep their NaN; qpart does not change
    the output"""
    f, dt = family(ift, name, dev), DT[dtn]
    V, cs, D, rs = f.up(f.V[:k], dt), f.up(f.cs, dt), f.up(f.D[:k], dt), f.up(f.rs, dt)
    scale = 0.5
    for what, col in (("shared", cs), ("per-vector", D)):
        if what == "per-vector" and not f.per:
            continue
        q = f.nan((k, f.nq + 2), torch.float64)
        got = f.R._fwd(V, colscale=col, rowscale=rs, scale=scale, qpart=q)
        assert got.shape == (k, f.ndata) and got.dtype == dt
        assert torch.isnan(q[:, f.nq:]).all() and not torch.isnan(q[:, :f.nq]).any(), what
        for j in range(k):
            yj, qj = f.single_fwd(V[j].contiguous(), col if col.dim() == 1 else col[j].contiguous(), rs, scale)
            assert torch.equal(got[j], yj), (what, j)
            assert torch.equal(q[j, :f.nq], qj), (what, j)
        assert torch.equal(f.R._fwd(V, colscale=col, rowscale=rs, scale=scale), got), what
    # no scales at all
    plain = f.R._fwd(V)
    for j in range(k):
        assert torch.equal(plain[j], f.single_fwd(V[j].contiguous(), None, None, 1.0)[0]), j


@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("name,dtn", CASES)
def test_adjoint_rows_are_the_single_calls(ift, dev, name, dtn, k):
    """_adj with a data-side colscale, a shared and a per-vector rowscale and
    a scalar: bitwise the k single calls"""
    f, dt = family(ift, name, dev), DT[dtn]
    Y, cs, D, rs = f.up(f.Y[:k], dt), f.up(f.cs, dt), f.up(f.D[:k], dt), f.up(f.rs, dt)
    scale = 2.0
    for what, row in (("shared", cs), ("per-vector", D)):
        if what == "per-vector" and not f.per:
            continue
        got = f.R._adj(Y, colscale=rs, rowscale=row, scale=scale)
        assert got.shape == (k, f.npix) and got.dtype == dt
        for j in range(k):
            oj = f.single_adj(Y[j].contiguous(), rs, row if row.dim() == 1 else row[j].contiguous(), scale)
            assert torch.equal(got[j], oj), (what, j)
    plain = f.R._adj(Y)
    for j in range(k):
        assert torch.equal(plain[j], f.single_adj(Y[j].contiguous(), None, None, 1.0)), j


@pytest.mark.parametrize("name,dtn", CASES)
def test_middle_is_the_composed_row_calls(ift, dev, name, dtn):
    """ResponseMiddle(R, dr, c, fct)(S) = R._adj(R._fwd(S, dr, c, fct), dr)
    composed by hand, bitwise, for a batch of 9 and for one grid without a
    batch axis, with and without qpart; the capabilities are the family's"""
    f, dt = family(ift, name, dev), DT[dtn]
    k, fct = 9, 0.7
    dr64, c64 = f.up(f.cs.reshape(f.shape), torch.float64), f.up(f.rs, torch.float64)
    m = f.middle(dr64, c64, fct)
    assert m.response is f.R and m.factor == fct and m.quad_blocks == f.nq
    assert m.supports_batch and m.supports_fold == f.fold and m.supports_fp32 == (not name.startswith("psf"))
    # the scales are kept in float64 and cast to the vectors' dtype
    d, w = m.scales_as(dt)
    assert torch.equal(d, dr64.reshape(-1).to(dt)) and torch.equal(w, c64.to(dt))
    S = f.up(np.random.default_rng(37).standard_normal((k,) + f.shape), dt)
    q1 = f.nan((k, f.nq + 1), torch.float64)
    hand = f.R._adj(f.R._fwd(S.reshape(k, f.npix), colscale=d, rowscale=w, scale=fct, qpart=q1), rowscale=d)
    hand = hand.reshape(S.shape)
    q2 = f.nan((k, f.nq + 1), torch.float64)
    got = m(S, qpart=q2)
    assert got.shape == S.shape and got.dtype == dt
    assert torch.equal(got, hand)
    assert torch.equal(q2[:, :f.nq], q1[:, :f.nq]) and torch.isnan(q2[:, f.nq:]).all()
    assert torch.equal(m(S), hand)
    one = m(S[4].contiguous())
    assert one.shape == f.shape and torch.equal(one, hand[4])
    qo = f.nan((1, f.nq), torch.float64)
    assert torch.equal(m(S[4].contiguous(), qpart=qo), hand[4]) and torch.equal(qo[0], q1[4, :f.nq])
    # a float weight goes into the factor, no pixel diagonal: no scales
    m2 = f.middle(None, 2.5, fct)
    assert m2.factor == fct * 2.5 and m2.scales_as(dt) == (None, None)
    assert torch.equal(m2(S), f.R._adj(f.R._fwd(S.reshape(k, f.npix), scale=fct * 2.5)).reshape(S.shape))
    if not f.fold:
        with pytest.raises(NotImplementedError):
            m(S, qpart=q2, fold=(q2, f.nq, k, q2.data_ptr(), 1))


@pytest.mark.parametrize("dtn", list(DT))
@pytest.mark.parametrize("name", ("los2d", "los1d"))
def test_los_fold_rides_the_last_chunk(ift, dev, name, dtn, monkeypatch):
    """the LOS middle's fold= form at k = 9 (chunks of 8 and 1): bitwise the
    middle without it plus a separate nft_fold_partials (3 rows of 40
    partials, output stride 2, as test_los_regimes_gpu.py), and only the
    adjoint launch that ends at k carries it"""
    from nifty_amd import _native
    f, dt = family(ift, name, dev), DT[dtn]
    k = 9
    m = f.middle(f.up(f.cs.reshape(f.shape), torch.float64), f.up(f.rs, torch.float64), 0.7)
    S = f.up(np.random.default_rng(41).standard_normal((k,) + f.shape), dt)
    part = f.up(np.random.default_rng(5).standard_normal((3, 40)), torch.float64)
    ref = f.nan((3, 2), torch.float64)
    _native._check(_native.load().nft_fold_partials(_native.ptr(part), 40, 3, _native.ptr(ref), 2,
                                                    _native.stream_ptr()))
    assert not torch.isnan(ref[:, 0]).any() and torch.isnan(ref[:, 1]).all()
    q1 = f.nan((k, f.nq), torch.float64)
    plain = m(S, qpart=q1)
    calls = []
    orig = _native.los_adjoint_batched

    def spy(*a, **kw):
        calls.append(kw.get("fold") is not None)
        return orig(*a, **kw)
    monkeypatch.setattr(_native, "los_adjoint_batched", spy)
    got = f.nan((3, 2), torch.float64)
    q2 = f.nan((k, f.nq), torch.float64)
    out = m(S, qpart=q2, fold=(part, 40, 3, got.data_ptr(), 2))
    assert calls == [False, True]
    assert torch.equal(out, plain) and torch.equal(q2, q1)
    assert torch.equal(got[:, 0], ref[:, 0]) and torch.isnan(got[:, 1]).all()
