"""CPU: LOS construction inputs and box-plan regimes that the uniformly random
lines of los.npz never reach.

Fixture cases (tests/golden/los_edge.npz, written by gen_golden_los_edge.py
from the reference): parallax errors with a truncation (`_apply_erf`),
anisotropic distances, axis-parallel / on-edge / outside lines, a grid smaller
than one box.  los_coo is held bit-exact against the reference's COO matrix,
and the box plan of the triplets, applied by box_plan_apply (the numpy
restatement of the kernels' arithmetic), against the reference's R x and
R^T y at rtol 1e-13.

Dense cases (tests/los_cases.py; no fixture, the reference is the float64 CSR
product of the same triplets): plans with more than 256 lines in a box (16-bit
line indices, no box_ent_adj), more than LOS_CH_A entries in a box and boxes
of several forward work items; short16 has more than 256 lines but fewer than
LOS_CAP_F entries in its box (split by segment count alone).  Every case
asserts the regime it is there for.
"""
import numpy as np
import pytest

import los_cases as lc
from conftest import golden


def _coo(name):
    from nifty_amd.library.los_response import los_coo
    shape, dist, starts, ends, sigmas, trunc = lc.case(name)
    if dist is None:
        dist = tuple(1. / np.array(shape))
    return shape, los_coo(shape, dist, starts, ends, sigmas, trunc)


@pytest.mark.parametrize("tag", lc.FIXTURES)
def test_los_edge_construction_bit_exact(tag):
    G = golden("los_edge.npz")
    _, (rows, cols, w, nlos) = _coo(tag)
    assert w.dtype == np.float32 and nlos == len(G[f"{tag}_y"])
    np.testing.assert_array_equal(rows, G[f"{tag}_row"])
    np.testing.assert_array_equal(cols, G[f"{tag}_col"])
    np.testing.assert_array_equal(w, G[f"{tag}_wgt"])


def test_los_edge_fixture_holds_its_cases():
    """what the generator asserted, from the data: tapered weights, lines
    parallel to either axis, empty rows"""
    G = golden("los_edge.npz")
    assert int(G["sig_ntapered"]) > 0 and (G["sig_sigmas"] > 0).any() and (G["sig_sigmas"] == 0).any()
    assert float(G["sig_trunc"]) == 2.
    assert tuple(G["aniso_dist"]) == (0.1, 0.01)
    d = (G["degen_ends"] - G["degen_starts"]) / G["degen_dist"].reshape(-1, 1)
    assert (d[0] == 0).sum() >= 3 and (d[1] == 0).sum() >= 3
    per_line = np.bincount(G["degen_row"], minlength=d.shape[1])
    assert (per_line == 0).sum() == 5 and (per_line[(d == 0).any(axis=0)] > 0).sum() >= 6
    assert np.prod(G["tiny_shape"]) < 256


@pytest.mark.parametrize("tag", lc.FIXTURES)
def test_los_edge_box_plan_layout(tag):
    from nifty_amd.library import los_response as lr
    G = golden("los_edge.npz")
    shape = tuple(int(s) for s in G[f"{tag}_shape"])
    rows, cols, w = G[f"{tag}_row"], G[f"{tag}_col"], G[f"{tag}_wgt"]
    P = lr.box_plan(rows, cols, w, shape, len(G[f"{tag}_y"]))
    lc.assert_regime(tag, P)
    print(lc.describe(tag, P))
    assert np.allclose(lr.box_plan_apply(P, G[f"{tag}_x"], "times"), G[f"{tag}_Rx"], rtol=1e-13, atol=0)
    assert np.allclose(lr.box_plan_apply(P, G[f"{tag}_y"], "adjoint"), G[f"{tag}_Rty"].ravel(), rtol=1e-13, atol=0)


@pytest.mark.parametrize("name", lc.WIDE)
def test_dense_box_plan_layout(name):
    from nifty_amd.library import los_response as lr
    shape, (rows, cols, w, nlos) = _coo(name)
    npix = int(np.prod(shape))
    P = lr.box_plan(rows, cols, w, shape, nlos)
    lc.assert_regime(name, P)
    print(lc.describe(name, P))
    assert lr.LOS_CAP_F == 2048 and P["item_seg"][-1] == P["nseg"] and P["box_ent"][-1] == len(rows)
    assert np.all(np.diff(P["item_seg"]) <= lr.BOX)
    assert np.all(np.diff(P["item_ent"]) <= lr.LOS_CAP_F)
    assert int(P["ent_lidx"].max()) >= 256      # an index that needs the second byte
    A, Aabs, nrow, ncol = lc.csr(rows, cols, w, nlos, npix)
    rng = np.random.default_rng(9)
    # positive vectors: the weights are >= 0, nothing cancels, and rtol 1e-13
    # per element means what it says (a line of the 1-D case sums ~100 signed
    # terms to 2e-4 of their magnitude; no relative bound holds there)
    x, y = rng.random(npix) + 0.5, rng.random(nlos) + 0.5
    assert np.allclose(lr.box_plan_apply(P, x, "times"), A @ x, rtol=1e-13, atol=0)
    assert np.allclose(lr.box_plan_apply(P, y, "adjoint"), A.T @ y, rtol=1e-13, atol=0)
    # signed vectors: the element-wise bound of a fixed-order float64 sum
    x, y = rng.standard_normal(npix), rng.standard_normal(nlos)
    assert np.all(np.abs(lr.box_plan_apply(P, x, "times") - A @ x) <= lc.bound64(nrow, Aabs @ np.abs(x)))
    assert np.all(np.abs(lr.box_plan_apply(P, y, "adjoint") - A.T @ y) <= lc.bound64(ncol, Aabs.T @ np.abs(y)))


def test_all_lines_outside_plan():
    from nifty_amd.library import los_response as lr
    shape, (rows, cols, w, nlos) = _coo("empty")
    assert len(rows) == 0 and nlos == 7
    P = lr.box_plan(rows, cols, w, shape, nlos)
    lc.assert_regime("empty", P)
    rng = np.random.default_rng(9)
    got = lr.box_plan_apply(P, rng.standard_normal(shape), "times")
    assert got.shape == (nlos,) and np.all(got == 0.)
    got = lr.box_plan_apply(P, rng.standard_normal(nlos), "adjoint")
    assert got.shape == (int(np.prod(shape)),) and np.all(got == 0.)
