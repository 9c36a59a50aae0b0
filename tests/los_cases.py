"""Shared by test_los_regimes.py (host) and test_los_regimes_gpu.py (device):
line sets whose box plans take the wide-index (uint16 line index, no
box_ent_adj), multi-chunk and multi-item paths of csrc/nft_los.hip, the regime
each one has to be in, and the element-wise error bound of a fixed-order
float64 sparse product.  Not a test module."""
import numpy as np

from conftest import golden

LOS_CH_A = 2048      # adjoint entries per LDS chunk (csrc/nft_los.hip)
U = 2.0 ** -53       # unit roundoff, float64
U32 = 2.0 ** -24     # unit roundoff, float32
TINY32 = 2.0 ** -149  # smallest float32 subnormal


def _unit(shape, nlos, seed):
    rng = np.random.default_rng(seed)
    nd = len(shape)
    return rng.random((nd, nlos)), rng.random((nd, nlos))


def _mixed():
    """(32, 48), 2 x 3 boxes: 300 lines with both ends inside the first box
    (wide there), 40 lines over the grid's lower-left triangle p0 / 32 +
    p1 / 48 <= 1 (convex, so no line reaches the far corner box, which stays
    empty; the boxes between get a few lines each)"""
    shape = (32, 48)
    rng = np.random.default_rng(43)
    d = 1. / np.array(shape).reshape(-1, 1)
    a = (0.2 + 15.6 * rng.random((2, 300)) - 0.5) * d
    b = (0.2 + 15.6 * rng.random((2, 300)) - 0.5) * d
    t = rng.random((2, 2, 40))
    t = np.where(t.sum(axis=1, keepdims=True) > 1., 1. - t, t)
    return shape, np.concatenate([a, t[0]], axis=1), np.concatenate([b, t[1]], axis=1)


def dense_case(name):
    """name -> (shape, distances or None, starts, ends, sigmas or None, truncation)"""
    if name == "dense16":
        return ((16, 16), None) + _unit((16, 16), 301, 41) + (None, 3.)   # 301 % 4 != 0 (4 lines per reduce block)
    if name == "dense32":
        return ((32, 32), None) + _unit((32, 32), 600, 42) + (None, 3.)
    if name == "mixed":
        shape, s, e = _mixed()
        return shape, None, s, e, None, 3.
    if name == "dense1d":
        return ((300,), None) + _unit((300,), 300, 44) + (None, 3.)
    if name == "dense3d":
        return ((2, 16, 16), None) + _unit((2, 16, 16), 400, 45) + (None, 3.)
    if name == "short16":
        # 302 lines of at most 2.4 pixels per axis inside one box: more than 256 segments but fewer than
        # LOS_CAP_F entries -- the forward box is split by its segment count alone, the adjoint stages one chunk
        rng = np.random.default_rng(47)
        s = rng.random((2, 302))
        return (16, 16), None, s, s + 0.3 * (rng.random((2, 302)) - 0.5), None, 3.
    if name == "empty":
        # every line beside the grid (which ends at 1 - 1 / 40): no entries at all
        rng = np.random.default_rng(46)
        return (20, 20), None, 1.5 + rng.random((2, 7)), 1.5 + rng.random((2, 7)), None, 3.
    raise KeyError(name)


DENSE = ("dense16", "dense32", "mixed", "dense1d", "dense3d")
WIDE = DENSE + ("short16",)     # every plan with 16-bit line indices
FIXTURES = ("sig", "aniso", "degen", "tiny")


def fixture_case(tag):
    G = golden("los_edge.npz")
    return (tuple(int(s) for s in G[f"{tag}_shape"]), tuple(float(v) for v in G[f"{tag}_dist"]), G[f"{tag}_starts"],
            G[f"{tag}_ends"], G[f"{tag}_sigmas"], float(G[f"{tag}_trunc"]))


def case(name):
    return fixture_case(name) if name in FIXTURES else dense_case(name)


def regime(P):
    """lines, entries and forward work items per box (arrays over the boxes)"""
    return dict(lines=np.diff(P["box_lptr"]), entries=np.diff(P["box_ent"]), items=np.diff(P["box_item"]))


def assert_regime(name, P):
    """the paths of nft_los.hip a case is there for; a change of the inputs
    that turns it back into an ordinary plan fails here"""
    r = regime(P)
    if name in DENSE:
        assert P["lidx8"] == 0 and "box_ent_adj" not in P and P["ent_lidx"].dtype == np.uint16
        assert r["lines"].max() > 256            # tab == false for that box, forward split by segment count
        assert r["entries"].max() > LOS_CH_A     # several adjoint chunks
        assert r["items"].max() > 1              # several forward work items
    if name == "short16":
        assert P["lidx8"] == 0 and "box_ent_adj" not in P and r["lines"].max() > 256
        assert r["entries"].max() <= LOS_CH_A and r["items"].max() > 1   # split by segment count alone
    if name == "dense16":
        assert P["nlos"] % 4 != 0 and P["nbox"] == 1
    if name == "mixed":
        assert ((r["lines"] >= 1) & (r["lines"] <= 256)).any()   # tab == true inside a wide plan
        assert (r["entries"] == 0).any()
    if name == "dense1d":
        assert P["bh"] == 1 and P["W"] % 256 != 0 and r["items"].max() > 8
    if name == "dense3d":
        assert P["L"] == 2 and (np.diff(P["los_ptr"]) == 0).any()   # empty rows
    if name in ("sig", "degen"):
        assert P["lidx8"] == 1 and "box_ent_adj" in P and r["lines"].max() <= 256
    if name == "degen":
        assert (np.diff(P["los_ptr"]) == 0).sum() >= 5
    if name == "empty":
        assert P["nitems"] == 0 and P["nseg"] == 0 and P["nbox"] > 0 and r["entries"].max() == 0
        assert P["nlos"] % 4 != 0


def describe(name, P):
    r = regime(P)
    return (f"{name}: lidx8={P['lidx8']} nlos={P['nlos']} nbox={P['nbox']} lines/box max {int(r['lines'].max())} "
            f"entries/box max {int(r['entries'].max())} items/box max {int(r['items'].max())} "
            f"empty rows {int((np.diff(P['los_ptr']) == 0).sum())}")


def csr(rows, cols, w, nlos, npix):
    """float64 CSR of the triplets (fp32 weights upcast exactly), |A| and the
    nonzeros per row and per column"""
    import scipy.sparse
    A = scipy.sparse.coo_matrix((np.asarray(w, dtype=np.float64), (rows, cols)), shape=(nlos, npix)).tocsr()
    Aabs = abs(A)
    return A, Aabs, np.bincount(rows, minlength=nlos), np.bincount(cols, minlength=npix)


def bound64(n, mag):
    """|got - ref| <= 2 (n_i + 4) 2^-53 (|A| |v|)_i: a float64 sum of n_i
    products in any fixed order, with up to two scale factors on the way in and
    two on the way out, is within (n_i + 4) u of the exact value relative to
    the sum of magnitudes (to first order; (n_i + 3) roundings, the rest
    absorbs the second-order terms); kernel and reference each stay within
    that, hence the factor 2.  n_i = 0 gives mag = 0: exact."""
    return 2. * (np.asarray(n) + 4.) * U * mag


def bound32(n, mag, ref):
    """fp32 storage (inputs cast first, reference in float64 from the casts):
    the float64 bound plus the final rounding 2^-24 |ref|, at least one
    subnormal step -- and exactly 0 where the row or column is empty"""
    b = np.maximum(bound64(n, mag) + U32 * np.abs(ref), TINY32)
    return np.where(mag == 0., 0., b)
