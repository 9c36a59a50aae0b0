"""Generate tests/golden/distributor.npz: PowerDistributor on ONE space of a
product domain, evaluated by the reference (NIFTy 8.5).

Like the other generators this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

The harmonic grid h is the default codomain of RGSpace((6, 5), (0.3, 0.7));
A = UnstructuredDomain(3), B = UnstructuredDomain(4).
  mid    (A, h, B), space=1: pre = 3, post = 4
  first  (h, B),    space=0: post = 4 alone
  last   (A, h),    space=1: pre = 3 alone
Per case: x on the operator's domain, y on its target (standard normal, seeds
below), times(x) and adjoint_times(y).  The reference's adjoint is
special_add_at (utilities.py:223-242): np.bincount over the raveled grid per
(pre, post) item, i.e. each bin summed in ascending pixel order -- the order
the tests hold the native scatter to, bit for bit.  The script asserts that
restatement before it writes anything.

Usage:  python tests/golden/gen_golden_distributor.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))
SHAPE, POS_DIST, NA, NB = (6, 5), (0.3, 0.7), 3, 4


def main():
    h = ift.RGSpace(SHAPE, distances=POS_DIST).get_default_codomain()
    ps = ift.PowerSpace(h)
    a, b = ift.UnstructuredDomain(NA), ift.UnstructuredDomain(NB)
    pindex = np.asarray(ps.pindex)
    nbin = int(pindex.max()) + 1
    d = {"shape": np.array(SHAPE), "pos_dist": np.array(POS_DIST), "na": np.array(NA), "nb": np.array(NB),
         "pindex": pindex}
    for i, (tag, dom, space) in enumerate((("mid", (a, h, b), 1), ("first", (h, b), 0), ("last", (a, h), 1))):
        pd = ift.PowerDistributor(ift.DomainTuple.make(dom), ps, space=space)
        rng = np.random.default_rng(500 + i)
        x = rng.standard_normal(pd.domain.shape)
        y = rng.standard_normal(pd.target.shape)
        t = np.asarray(pd(ift.makeField(pd.domain, x)).val)
        at = np.asarray(pd.adjoint_times(ift.makeField(pd.target, y)).val)
        # the restatement the tests rely on
        pre = NA if tag != "first" else 1
        post = NB if tag != "last" else 1
        y3, at3 = y.reshape(pre, -1, post), at.reshape(pre, nbin, post)
        for p in range(pre):
            for q in range(post):
                assert np.array_equal(at3[p, :, q], np.bincount(pindex.ravel(), weights=y3[p, :, q], minlength=nbin))
        assert np.array_equal(t.reshape(pre, -1, post), x.reshape(pre, nbin, post)[:, pindex.ravel(), :])
        d.update({f"{tag}_x": x, f"{tag}_y": y, f"{tag}_times": t, f"{tag}_adjoint_times": at})
    path = os.path.join(OUT, "distributor.npz")
    np.savez_compressed(path, **d)
    print(f"distributor.npz: {len(d)} arrays, {nbin} bins, {os.path.getsize(path) / 1e3:.1f} kB on disk")


if __name__ == "__main__":
    main()
