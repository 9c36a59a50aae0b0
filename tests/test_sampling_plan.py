"""CPU: MaskOperator / LinearInterpolator construction and the host sampling
plan (operators/sampling_plan.py) against the reference's values
(tests/golden/sampling.npz, gen_golden_sampling.py).  No GPU compute here.

Cases: grids g1 = (16,) with distance 0.5, g2 = (8, 6) with distances (0.5,
0.25), g3 = (4, 6, 8); the first 1, 37 and 1000 of 1000 points that hold a
negative position, one beyond the extent, points on nodes, one in the last
cell (wraps to index 0), two identical points and 300 points in one cell;
with 1 and 37 points most pixels are touched by no point.  Masks: random,
nothing flagged, one pixel kept.

Tolerance of samp_plan_apply: 1e-14 relative max-norm (the same products in
the same order as the reference's COO matvec; indices exact, weights
bitwise)."""
import numpy as np
import pytest

from conftest import golden

GRIDS = ("g1", "g2", "g3")
MASKS = ("rand", "none", "one")


def relmax(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)


@pytest.fixture(scope="module")
def G():
    return golden("sampling.npz")


def space(ift, G, tag):
    return ift.RGSpace(tuple(int(v) for v in G[tag + "_shape"]), distances=tuple(G[tag + "_dist"]))


def coo(G, tag, n):
    """COO (row, col, data) of the first n points, in the reference's order"""
    keep = G[tag + "_row"] < n
    return G[tag + "_row"][keep], G[tag + "_col"][keep], G[tag + "_data"][keep]


def test_constructor_errors_and_targets(G):
    import nifty_amd as ift
    sp = space(ift, G, "g2")
    pts = np.ascontiguousarray(G["g2_pts"][:, :37])
    R = ift.LinearInterpolator(sp, pts)
    assert isinstance(R, ift.LinearOperator)
    assert R.domain == ift.DomainTuple.make(sp)
    assert R.target == ift.DomainTuple.make(ift.UnstructuredDomain(37))
    assert R.capability == R.TIMES | R.ADJOINT_TIMES
    with pytest.raises(TypeError):
        ift.LinearInterpolator(ift.UnstructuredDomain(8), pts)
    with pytest.raises(NotImplementedError):
        ift.LinearInterpolator((ift.RGSpace(4), ift.RGSpace(4)), pts)
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, pts.tolist())
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, pts[0])
    with pytest.raises(TypeError):
        ift.LinearInterpolator(sp, np.zeros((3, 5)))
    # more than 2^31 - 1 entries (a zero-stride view: nothing is allocated)
    with pytest.raises(ValueError):
        ift.LinearInterpolator(ift.RGSpace((4, 4, 4)), np.broadcast_to(np.zeros((3, 1)), (3, 2 ** 28)))
    assert ift.LinearInterpolator(sp, np.zeros((2, 0))).target.shape == (0,)
    flags = G["g2_mrand_flags"]
    M = ift.MaskOperator(ift.makeField(sp, flags))
    assert isinstance(M, ift.LinearOperator)
    assert M.domain == ift.DomainTuple.make(sp)
    assert M.target == ift.DomainTuple.make(ift.UnstructuredDomain(int((~flags).sum())))
    assert M.capability == M.TIMES | M.ADJOINT_TIMES
    with pytest.raises(TypeError):
        ift.MaskOperator(flags)
    # any DomainTuple of the flags; non-boolean flags are converted
    dom = ift.DomainTuple.make((ift.RGSpace(3), ift.UnstructuredDomain(4)))
    M2 = ift.MaskOperator(ift.makeField(dom, np.arange(12.).reshape(3, 4) % 3))
    assert M2.domain == dom and M2.target.shape == (4,)
    assert ift.MaskOperator(ift.makeField(sp, np.ones(sp.shape, dtype=bool))).target.shape == (0,)


@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("n", (1, 37, 1000))
def test_interpolator_plan_matches_reference_coo(G, tag, n):
    import nifty_amd as ift
    from nifty_amd.operators import sampling_plan as sp_
    R = ift.LinearInterpolator(space(ift, G, tag), np.ascontiguousarray(G[tag + "_pts"][:, :n]))
    P = R._plan_np
    row, col, data = coo(G, tag, n)
    nc = P["ncorner"]
    assert nc == 2 ** len(P["shape"]) and len(row) == nc * n
    # forward side: (corner, point)-major, the reference's storage order
    np.testing.assert_array_equal(np.tile(np.arange(n), nc), row)
    np.testing.assert_array_equal(sp_.samp_cols(P).reshape(-1), col)
    w = sp_.samp_weights(P)
    assert w.dtype == np.float64
    np.testing.assert_array_equal(w.reshape(-1).view(np.uint64), data.view(np.uint64))   # bitwise
    # adjoint side: per pixel the entries in ascending (corner, point) order
    ptr, ent = P["pix_ptr"], P["ent"]
    assert ptr[0] == 0 and ptr[-1] == nc * n and len(ptr) == P["npix"] + 1 and np.all(np.diff(ptr) >= 0)
    s, c = np.divmod(ent.astype(np.int64), nc)        # position in the plan's order, corner
    assert sorted(P["point"].tolist()) == list(range(n))
    p = P["point"][s].astype(np.int64)                # its datum
    pix = np.repeat(np.arange(P["npix"]), np.diff(ptr))
    np.testing.assert_array_equal(sp_.samp_cols(P)[c, p], pix)
    key = (pix * nc + c) * n + p
    assert np.all(np.diff(key) > 0)
    assert sorted(ent.tolist()) == list(range(nc * n))
    if n == 1000:
        assert np.diff(ptr).max() >= 300          # 300 points in one cell: no cap
    elif n == 1 or tag != "g1":                   # (37 points reach all 16 pixels of g1)
        assert np.any(np.diff(ptr) == 0)          # pixels no point touches
    assert P["frac"].dtype == np.float64 and P["idx"].dtype == np.int32


@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("n", (1, 37, 1000))
def test_interpolator_plan_apply(G, tag, n):
    import nifty_amd as ift
    from nifty_amd.operators.sampling_plan import samp_plan_apply
    R = ift.LinearInterpolator(space(ift, G, tag), np.ascontiguousarray(G[tag + "_pts"][:, :n]))
    got = samp_plan_apply(R._plan_np, G[tag + "_x"], "times")
    assert relmax(got, G[tag + "_Rx"][:n]) <= 1e-14
    got = samp_plan_apply(R._plan_np, G[tag + "_y"][:n], "adjoint")
    ref = G[f"{tag}_Rty{n}"]
    assert relmax(got, ref.ravel()) <= 1e-14
    assert np.all(got[ref.ravel() == 0] == 0)


@pytest.mark.parametrize("tag", GRIDS)
@pytest.mark.parametrize("mtag", MASKS)
def test_mask_plan(G, tag, mtag):
    import nifty_amd as ift
    from nifty_amd.operators.sampling_plan import samp_plan_apply
    flags = G[f"{tag}_m{mtag}_flags"]
    M = ift.MaskOperator(ift.makeField(space(ift, G, tag), flags))
    P = M._plan_np
    assert P["ncorner"] == 1 and P["frac"] is None and P["npix"] == flags.size
    np.testing.assert_array_equal(P["idx"][0], np.flatnonzero(~flags.ravel()))   # C order of the grid
    np.testing.assert_array_equal(samp_plan_apply(P, G[tag + "_x"], "times"), G[f"{tag}_m{mtag}_Mx"])
    got = samp_plan_apply(P, G[f"{tag}_m{mtag}_y"], "adjoint")
    np.testing.assert_array_equal(got, G[f"{tag}_m{mtag}_Mty"].ravel())
    assert np.all(got[flags.ravel()] == 0)


def test_tile_order():
    """the order in which a plan lists its points: a permutation, stable
    within a pixel, ascending pixels in 1-D, tile by tile in 2-D / 3-D"""
    from nifty_amd.operators.sampling_plan import tile_order
    rng = np.random.default_rng(6)
    idx = rng.integers(0, 50, (1, 400))
    o = tile_order((50,), idx)
    assert sorted(o.tolist()) == list(range(400))
    key = idx[0][o] * 400 + o
    assert np.all(np.diff(key) > 0)                       # ascending pixel, data order within one
    for shape in ((64, 96), (3, 64, 96)):
        idx = np.stack([rng.integers(0, s, 5000) for s in shape])
        o = tile_order(shape, idx, tile=(16, 32))
        assert sorted(o.tolist()) == list(range(5000))
        lead = idx[0][o] if len(shape) == 3 else np.zeros(5000, dtype=np.int64)
        y, x = idx[-2][o], idx[-1][o]
        tile = (lead * 4 + y // 16) * 3 + x // 32
        assert np.all(np.diff(tile) >= 0)                 # one tile after the other
        inner = ((tile * 16 + y % 16) * 96 + x) * 5000 + o
        assert np.all(np.diff(inner) > 0)                 # rows within a tile, stable within a pixel
        assert sorted(tile_order(shape, idx).tolist()) == list(range(5000))   # the default tile side


def test_plan_rejects_oversized_grids():
    from nifty_amd.operators import sampling_plan as sp_
    with pytest.raises(ValueError):
        sp_.samp_plan((2 ** 31,), np.zeros((1, 0), dtype=np.int32))
    with pytest.raises(ValueError):
        sp_.samp_plan((4, 4, 4, 4), np.zeros((4, 1), dtype=np.int32), np.zeros((4, 1)))
