"""GPU: nft_los_adjoint_add -- the LOS adjoint with a pointwise branch,
out = R^T y + addw * addx, and the per-box partials of sum addw * addx^2.

Grids: one box row/column multiples (32 x 32), ragged edge boxes (40 x 24),
boxes without entries (64 x 64, all lines in one quadrant), 1-D (1 x 256
boxes, 512) and 3-D layers (4 x 32 x 32).  nvec 1, 3, 8 take the single, the
masked 4-vector and the 8-vector instance."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GRIDS = {"32x32": ((32, 32), 60, 1.0), "40x24": ((40, 24), 60, 1.0), "64x64q": ((64, 64), 60, 0.5),
         "512": ((512,), 20, 1.0), "4x32x32": ((4, 32, 32), 80, 1.0)}
_CACHE = {}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


def _response(ift, name):
    """(LOSResponse, plan) per grid, built once"""
    if name not in _CACHE:
        shape, nlos, extent = GRIDS[name]
        rng = np.random.default_rng(11)
        starts = extent * rng.random((len(shape), nlos))
        ends = extent * rng.random((len(shape), nlos))
        R = ift.LOSResponse(ift.RGSpace(shape), starts=list(starts), ends=list(ends))
        _CACHE[name] = (R, R._box_plan())
    return _CACHE[name]


def _inputs(R, k, dt, shared, dev, seed=3):
    g = torch.Generator(device="cpu").manual_seed(seed)
    npix, nlos = R.domain.size, R.target.size
    y = torch.randn((k, nlos), generator=g, dtype=torch.float64).to(dt).to(dev)
    x = torch.randn((k, npix), generator=g, dtype=torch.float64).to(dt).to(dev)
    w = (torch.rand((1 if shared else k, npix), generator=g, dtype=torch.float64) + 0.25).to(dt).to(dev)
    return y, x, (w[0].contiguous() if shared else w)


def _run(plan, y, w, x, nb, pad=2):
    from nifty_amd import _native
    out = torch.full_like(x, float("nan"))
    q = torch.full((y.shape[0], nb + pad), float("nan"), dtype=torch.float64, device=y.device)
    _native.los_adjoint_add(plan, y, out, w, x, qpart=q)
    return out, q


@pytest.mark.parametrize("shared", [True, False], ids=["sharedw", "perw"])
@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_los_adjoint_add(ift, dev, grid, k, dt, shared):
    from nifty_amd import _native
    R, plan = _response(ift, grid)
    npix = R.domain.size
    nb = _native.load().nft_los_add_blocks(ctypes.byref(plan))
    assert nb == plan.nbox > 0
    if grid == "64x64q":
        # boxes no line crosses are part of the case
        assert (np.diff(R._plan_np["box_ent"]) == 0).sum() >= 8
    y, x, w = _inputs(R, k, dt, shared, dev)
    out, q = _run(plan, y, w, x, nb)
    assert torch.isnan(q[:, nb:]).all() and not torch.isnan(q[:, :nb]).any() and not torch.isnan(out).any()

    # composition: the plain adjoint's output plus a separate multiply and add
    y64, x64, w64 = y.double(), x.double(), w.double()
    L = torch.empty((k, npix), dtype=torch.float64, device=dev)
    _native.los_adjoint_ex(plan, y64.contiguous(), L)
    want = L + w64 * x64
    if dt == torch.float64:
        assert torch.equal(out, want)
    else:
        w32 = want.float()
        ulp = torch.maximum(torch.nextafter(w32.abs(), torch.full_like(w32, float("inf"))) - w32.abs(),
                            torch.full_like(w32, 2.0 ** -149))
        assert ((out.double() - w32.double()).abs() <= ulp.double()).all()

    # partials: sum over the blocks against the fp64 sum of the same terms
    terms = (w64 * x64) * x64
    got, ref, mag = q[:, :nb].sum(1), terms.sum(1), terms.abs().sum(1)
    print(f"{grid} k={k} partial sums: max rel err {float(((got - ref).abs() / mag).max()):.3e}")
    assert ((got - ref).abs() <= npix * np.finfo(np.float64).eps * mag).all()

    # a batch of k equals k single calls, bitwise
    for j in range(k):
        wj = w if shared else w[j:j + 1].contiguous()
        oj, qj = _run(plan, y[j:j + 1].contiguous(), wj, x[j:j + 1].contiguous(), nb)
        assert torch.equal(oj[0], out[j]) and torch.equal(qj[0, :nb], q[j, :nb]), j

    # a second call reproduces the first, bitwise
    out2, q2 = _run(plan, y, w, x, nb)
    assert torch.equal(out2, out) and torch.equal(q2[:, :nb], q[:, :nb])


@pytest.mark.parametrize("dt", [torch.float64, torch.float32], ids=["f64", "f32"])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_partials_of_ones_count_every_pixel_once(ift, dev, grid, dt):
    """addw = addx = 1: the partials sum to exactly npix, so every pixel of
    the grid lies in exactly one block (empty and ragged boxes included)"""
    from nifty_amd import _native
    R, plan = _response(ift, grid)
    npix, nlos = R.domain.size, R.target.size
    nb = _native.load().nft_los_add_blocks(ctypes.byref(plan))
    for k in (1, 3, 8):
        y = torch.zeros((k, nlos), dtype=dt, device=dev)
        one = torch.ones((k, npix), dtype=dt, device=dev)
        out, q = _run(plan, y, one[0].contiguous(), one, nb)
        assert torch.equal(out, one)
        assert (q[:, :nb].sum(1) == float(npix)).all()
        assert (q[:, :nb] == q[:, :nb].round()).all() and (q[:, :nb] >= 0).all() and (q[:, :nb] <= 256).all()


def test_without_partials_and_bad_arguments(ift, dev):
    from nifty_amd import _native
    R, plan = _response(ift, "40x24")
    y, x, w = _inputs(R, 3, torch.float64, True, dev)
    nb = _native.load().nft_los_add_blocks(ctypes.byref(plan))
    ref, _ = _run(plan, y, w, x, nb)
    out = torch.empty_like(x)
    _native.los_adjoint_add(plan, y, out, w, x)
    assert torch.equal(out, ref)
    with pytest.raises(_native.NativeError):
        _native.los_adjoint_add(plan, y, out, w, x, qpart=torch.zeros((3, nb - 1), dtype=torch.float64, device=dev))
    with pytest.raises(_native.NativeError):
        _native.los_adjoint_add(plan, y, out, w[:-1].contiguous(), x)
    with pytest.raises(_native.NativeError):
        _native.los_adjoint_add(plan, y, out, w.float(), x)
