"""Generate tests/golden/los_edge.npz: LOSResponse construction inputs that
gen_golden.py's gen_los (both ends uniform in the unit box) never draws,
evaluated by the reference (NIFTy 8.5).

Like gen_golden_sampling.py this script runs in the build container only,
imports the reference from there and writes nothing but data; the same NumPy
shim applies.

Cases (per case: shape, dist, starts, ends, sigmas, trunc, the COO triplets
row / col / wgt in the reference's storage order, one x, one y, Rx, Rty):
  sig     (48, 40), 60 lines from near the origin to 0.3 .. 0.7 with parallax
          errors sigma in [0, 0.25) (a few exactly 0) and truncation 2: the
          lines are prolonged to 1 / (1 / length - 2 sigma) and their far part
          tapered by the Gaussian survival function (apply_erf).
  aniso   (30, 50) with distances (0.1, 0.01), 60 lines over the 3 x 0.5 extent.
  degen   (40, 24): lines parallel to axis 0 and to axis 1 (direction == 0 in
          one component, both senses, one longer than the grid), one lying
          exactly on the edge between two pixel rows, lines that start and end
          outside and pass through, lines wholly outside (empty rows: diagonal,
          beyond the far side, axis-parallel beside the grid), and 16 ordinary
          lines.
  tiny    (5, 7): a grid smaller than one 16 x 16 box, ends drawn from
          [-0.2, 1.2), so some lie outside.

apply_erf is wrapped to count which of its two masks are hit.  The taper mask
(lo < dist <= hi) must be hit, and entries below lo must stay untouched.  The
zeroing mask (dist > hi) is counted and stored as sig_nzeroed: the reference
cuts every line at hi (real_ends) and stops 1e-7 of the line short of it, so
no midpoint distance exceeds hi and the count is 0 by construction; the case
still runs the statement.

Usage:  python tests/golden/gen_golden_los_edge.py
"""
import os
import sys

import numpy as np

np.asfarray = lambda a, dtype=np.float64: np.asarray(a, dtype=dtype)  # noqa: E731
sys.path.insert(0, "/root/reference")
import nifty8 as ift  # noqa: E402
from nifty8.library import los_response as ref_los  # noqa: E402

OUT = os.path.dirname(os.path.abspath(__file__))

COUNT = {"zeroed": 0, "tapered": 0, "plain": 0}
_apply_erf = ref_los.apply_erf


def _counting_apply_erf(wgt, dist, lo, mid, hi, sig, erf):
    COUNT["zeroed"] += int(np.sum(dist > hi))
    COUNT["tapered"] += int(np.sum((dist > lo) & (dist <= hi)))
    COUNT["plain"] += int(np.sum(dist <= lo))
    return _apply_erf(wgt, dist, lo, mid, hi, sig, erf)


ref_los.apply_erf = _counting_apply_erf


def phys(p, dist):
    """pixel coordinates (grid = [0, n] per axis) -> positions, (ndim, nlos)"""
    return (np.asarray(p, dtype=np.float64).T - 0.5) * np.asarray(dist).reshape(-1, 1)


def case_sig(rng):
    n = 60
    starts = 0.04 * rng.random((2, n))
    ends = 0.3 + 0.4 * rng.random((2, n))
    sigmas = 0.25 * rng.random(n)
    sigmas[::7] = 0.
    return (48, 40), None, starts, ends, sigmas, 2.


def case_aniso(rng):
    n = 60
    ext = np.array([[3.0], [0.5]])
    return (30, 50), (0.1, 0.01), ext * rng.random((2, n)), ext * rng.random((2, n)), None, 3.


def case_degen(rng):
    shape = (40, 24)
    dist = tuple(1. / np.array(shape))
    # an edge between two pixel rows that survives positions -> pixel coordinates exactly
    edge = next(k for k in range(8, 32) if ((k - 0.5) * dist[0]) / dist[0] + 0.5 == float(k))
    s = [(3.3, 7.4), (35.2, 7.4), (-5., 10.5),            # parallel to axis 0
         (12.6, 2.2), (12.6, 20.9), (30.1, -4.),          # parallel to axis 1
         (float(edge), 1.5),                              # on a pixel edge
         (-3.2, -2.1), (-4., 12.3), (20.4, -6.), (44., 30.),   # through, both ends outside
         (-5., -5.), (45., 3.), (-2.5, 3.), (-3., 2.), (10., 26.5)]   # wholly outside
    e = [(35.2, 7.4), (3.3, 7.4), (50., 10.5),
         (12.6, 20.9), (12.6, 2.2), (30.1, 29.),
         (float(edge), 22.5),
         (44.7, 27.3), (45., 9.1), (18.2, 30.), (-2., -3.),
         (-1., -2.), (50., 20.), (-2.5, 20.), (2., -3.), (30., 26.5)]
    starts = np.concatenate([phys(s, dist), rng.random((2, 16))], axis=1)
    ends = np.concatenate([phys(e, dist), rng.random((2, 16))], axis=1)
    ps, pe = starts / np.reshape(dist, (-1, 1)) + 0.5, ends / np.reshape(dist, (-1, 1)) + 0.5
    d = pe - ps
    assert np.all(d[1, :3] == 0.) and np.all(d[0, 3:7] == 0.) and ps[0, 6] == float(edge)
    return shape, None, starts, ends, None, 3.


def case_tiny(rng):
    n = 12
    return (5, 7), None, rng.random((2, n)), 1.4 * rng.random((2, n)) - 0.2, None, 3.


def main():
    d = {}
    for i, (tag, make) in enumerate((("sig", case_sig), ("aniso", case_aniso), ("degen", case_degen),
                                     ("tiny", case_tiny))):
        rng = np.random.default_rng(200 + i)
        shape, dist, starts, ends, sigmas, trunc = make(rng)
        sp = ift.RGSpace(shape, distances=dist)
        nlos = starts.shape[1]
        for k in COUNT:
            COUNT[k] = 0
        R = ift.LOSResponse(sp, starts=list(starts), ends=list(ends), sigmas=sigmas, truncation=trunc)
        coo = R._smat.A
        x = rng.standard_normal(shape)
        y = rng.standard_normal(nlos)
        per_line = np.bincount(coo.row, minlength=nlos)
        d[f"{tag}_shape"] = np.array(shape)
        d[f"{tag}_dist"] = np.array(sp.distances)
        d[f"{tag}_starts"] = starts
        d[f"{tag}_ends"] = ends
        d[f"{tag}_sigmas"] = np.zeros(nlos) if sigmas is None else sigmas
        d[f"{tag}_trunc"] = np.array(trunc)
        d[f"{tag}_row"] = coo.row.astype(np.int32)
        d[f"{tag}_col"] = coo.col.astype(np.int32)
        d[f"{tag}_wgt"] = coo.data
        d[f"{tag}_x"] = x
        d[f"{tag}_y"] = y
        d[f"{tag}_Rx"] = R(ift.makeField(sp, x)).val
        d[f"{tag}_Rty"] = R.adjoint(ift.makeField(R.target, y)).val
        assert coo.data.dtype == np.float32
        if tag == "sig":
            assert COUNT["tapered"] > 0 and COUNT["plain"] > 0, COUNT
            d["sig_nzeroed"] = np.array(COUNT["zeroed"])
            d["sig_ntapered"] = np.array(COUNT["tapered"])
        if tag == "degen":
            assert np.all(per_line[:11] > 0) and np.all(per_line[11:16] == 0), per_line
        print(f"{tag}: {shape}, {nlos} lines, {coo.nnz} nonzeros, {int((per_line == 0).sum())} empty rows, "
              f"apply_erf masks {dict(COUNT)}")
    path = os.path.join(OUT, "los_edge.npz")
    np.savez_compressed(path, **d)
    tot = sum(v.nbytes for v in d.values())
    print(f"los_edge.npz: {len(d)} arrays, {tot / 1e6:.2f} MB raw, {os.path.getsize(path) / 1e3:.0f} kB on disk")


if __name__ == "__main__":
    main()
