"""Sampling responses: the plan shared by MaskOperator and LinearInterpolator
(csrc/nft_samp.hip, nft_samp_plan in include/nifty_amd.h).

Every data point reads ncorner = 1 (mask) or 2^ndim (multilinear
interpolation) grid values.  The plan (host, numpy) holds per point its cell
index per axis and, for the interpolation, its ndim fp64 fractions; for the
adjoint the entries regrouped by destination pixel (a CSR over all grid
pixels, the entries of a pixel in ascending (corner, datum) order -- the
reference's COO order).  The points are listed in tile order (tile_order;
`point` maps a position of the plan to its datum), so that the lanes of a
wave gather from neighbouring grid lines.  No weights are stored: the kernels recompute them
from the fractions in fp64, bitwise the reference's
(src/operators/linear_interpolation.py:_build_mat).

`samp_plan_apply` restates the kernels' arithmetic in numpy (host-side check
of the layout; tests only)."""
import numpy as np
import torch

from .. import _native, config
from ..field import Field
from .linear_operator import LinearOperator

MAX_ENTRIES = 2 ** 31 - 1


def interp_points(shape, distances, sampling_points):
    """(idx [ndim, n] int32 in [0, shape), frac [ndim, n] fp64) of the
    positions: pos = points / distances, frac = pos - floor(pos),
    idx = floor(pos) mod shape (periodic), as _build_mat."""
    dist = np.array(list(distances), dtype=np.float64).reshape(-1, 1)
    pos = sampling_points / dist
    fl = np.floor(pos)
    frac = pos - fl
    idx = fl.astype(np.int64) % np.array(shape, dtype=np.int64).reshape(-1, 1)
    return idx.astype(np.int32), np.ascontiguousarray(frac, dtype=np.float64)


def _bits(ndim, c):
    """the corner's offset per axis: np.mgrid ravel order, first axis slowest"""
    return [(c >> (ndim - 1 - d)) & 1 for d in range(ndim)]


def _by_datum(P, a):
    """columns of `a` from plan positions to data order"""
    if P["point"] is None:
        return a
    out = np.empty_like(a)
    out[:, P["point"]] = a
    return out


def _cols(shape, idx, ncorner):
    """[ncorner, n] int64 flat pixel of every corner of the cells idx"""
    idx = idx.astype(np.int64)
    ndim = len(shape)
    if ncorner == 1:
        return idx.reshape(1, -1)
    cols = np.empty((ncorner, idx.shape[1]), dtype=np.int64)
    for c in range(ncorner):
        j = np.zeros(idx.shape[1], dtype=np.int64)
        for d, bit in enumerate(_bits(ndim, c)):
            i = idx[d] + bit
            j = j * shape[d] + np.where(i >= shape[d], 0, i)
        cols[c] = j
    return cols


def samp_cols(P):
    """[ncorner, npoints] int64 flat pixel of every (corner, datum)"""
    return _by_datum(P, _cols(P["shape"], P["idx"], P["ncorner"]))


def samp_weights(P):
    """[ncorner, npoints] fp64 weights of every (corner, datum) as the kernels
    recompute them: per axis the factor (bit ? e : 1 - e), multiplied in axis
    order."""
    if P["ncorner"] == 1:
        return np.ones((1, P["npoints"]))
    e = P["frac"]
    ndim = len(P["shape"])
    w = np.empty((P["ncorner"], P["npoints"]))
    for c in range(P["ncorner"]):
        bits = _bits(ndim, c)
        acc = e[0] if bits[0] else 1.0 - e[0]
        for d in range(1, ndim):
            acc = acc * (e[d] if bits[d] else 1.0 - e[d])
        w[c] = acc
    return _by_datum(P, w)


def tile_order(shape, idx, tile=None):
    """The order in which the plan lists the points: by tile of the last two
    grid axes (leading axis outermost), rows within a tile, so that the
    points of a 256-thread block fall into one roughly square patch of
    pixels and neighbouring lanes gather from the same few grid lines.  The
    tile side (a power of two, 8 to 256) is chosen for about 256 points per
    tile.  Stable: points of one pixel keep their data order.  1-D grids:
    ascending pixel."""
    n = idx.shape[1]
    idx = idx.astype(np.int64)
    if len(shape) == 1:
        return np.argsort(idx[0], kind="stable")
    y, x = idx[-2], idx[-1]
    if tile is None:
        per_pixel = max(n, 1) / float(np.prod(shape))
        side = int(2 ** np.clip(np.round(0.5 * np.log2(256. / per_pixel)), 3, 8))
        tile = (side, side)
    ty, tx = tile
    lead = idx[0] if len(shape) == 3 else np.zeros(n, dtype=np.int64)
    nty, ntx = -(-shape[-2] // ty), -(-shape[-1] // tx)
    t = (lead * nty + y // ty) * ntx + x // tx
    return np.argsort((t * ty + y % ty) * shape[-1] + x, kind="stable")


def samp_plan(shape, idx, frac=None):
    """The layout of nft_samp_plan as a dict of numpy arrays and ints.
    idx: [ndim, npoints] cell indices; frac: [ndim, npoints] fractions
    (interpolation) or None (mask: one corner of weight 1)."""
    shape = tuple(int(v) for v in shape)
    ndim = len(shape)
    if not 1 <= ndim <= 3:
        raise ValueError("sampling plan: 1 to 3 grid axes")
    idx = np.ascontiguousarray(idx, dtype=np.int32).reshape(ndim, -1)
    npoints = idx.shape[1]
    ncorner = 1 if frac is None else 2 ** ndim
    if frac is None and ndim != 1:
        raise ValueError("sampling plan: a mask takes the grid flat")
    npix = int(np.prod(shape))
    if npoints * ncorner > MAX_ENTRIES or npix > MAX_ENTRIES:
        raise ValueError("sampling response too large for int32 entry offsets")
    point = pos = None
    if frac is not None:
        # the points in tile order (a mask's kept pixels already ascend)
        frac = np.asarray(frac, dtype=np.float64).reshape(ndim, -1)
        point = tile_order(shape, idx)
        pos = np.empty(npoints, dtype=np.int64)
        pos[point] = np.arange(npoints)
        idx, frac = np.ascontiguousarray(idx[:, point]), np.ascontiguousarray(frac[:, point])
        point = point.astype(np.int32)
    P = dict(shape=shape, ndim=ndim, npoints=npoints, npix=npix, ncorner=ncorner, point=point, idx=idx, frac=frac)
    # adjoint: the entries, (corner, datum)-major, stably sorted by pixel
    flat = samp_cols(P).reshape(-1)
    order = np.argsort(flat, kind="stable")
    c, p = np.divmod(order, max(npoints, 1))
    if pos is not None:
        p = pos[p]
    P["ent"] = (p * ncorner + c).astype(np.int32)
    P["pix_ptr"] = np.r_[0, np.cumsum(np.bincount(flat, minlength=npix))].astype(np.int32)
    return P


def samp_plan_bytes(P):
    return int(sum(v.nbytes for v in P.values() if isinstance(v, np.ndarray)))


def samp_plan_apply(P, x, mode):
    """numpy restatement of the nft_samp kernels' arithmetic on a plan
    (host-side check of the layout; tests only)."""
    w = samp_weights(P)
    nc, npnt = P["ncorner"], P["npoints"]
    point = np.arange(npnt) if P["point"] is None else P["point"]
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    if mode == "times":
        cols = samp_cols(P)
        if nc == 1:
            return x[cols[0]].copy()
        acc = np.zeros(npnt)
        for c in range(nc):
            acc = acc + w[c] * x[cols[c]]
        return acc
    out = np.zeros(P["npix"])
    ptr, ent = P["pix_ptr"], P["ent"]
    for j in np.flatnonzero(np.diff(ptr)):
        acc = 0.
        for k in range(ptr[j], ptr[j + 1]):
            s, c = divmod(int(ent[k]), nc)
            p = point[s]
            acc = x[p] if nc == 1 else acc + w[c, p] * x[p]
        out[j] = acc
    return out


class SamplingResponse(LinearOperator):
    """Base of the responses on a sampling plan: subclasses set _domain,
    _target and _plan_np (samp_plan)."""

    def _init_plan(self, P):
        self._capability = self.TIMES | self.ADJOINT_TIMES
        self._plan_np = P
        self._plan = None

    @property
    def npoints(self):
        return self._plan_np["npoints"]

    def _samp_plan(self):
        """Device copy of the plan + its ctypes descriptor."""
        if self._plan is None:
            P = self._plan_np
            dev = config.device()
            keep = {k: torch.from_numpy(v).to(dev) for k, v in P.items() if isinstance(v, np.ndarray)}
            d = _native.SampPlan()
            d.npoints, d.npix, d.ndim, d.ncorner = P["npoints"], P["npix"], P["ndim"], P["ncorner"]
            for i, n in enumerate(P["shape"]):
                d.shape[i] = n
            for k, v in keep.items():
                setattr(d, k, v.data_ptr() if v.numel() else None)
            self._plan = (d, keep)
        return self._plan[0]

    def quad_blocks(self):
        """qpart columns of `_fwd` (nft_samp_quad_blocks)"""
        return _native.samp_quad_blocks(self._samp_plan())

    def _fwd(self, V, colscale=None, rowscale=None, scale=1.0, qpart=None):
        """rows of V (k, npix) -> (k, npoints), 8 vectors per launch; colscale
        one pixel vector or (k, npix) rows"""
        k = V.shape[0]
        V = V.contiguous()
        y = torch.empty((k, self.npoints), dtype=V.dtype, device=V.device)
        if self.npoints == 0:
            _native.require_device(V)
            return y
        plan = self._samp_plan()
        per = colscale is not None and colscale.numel() != V[0].numel()
        for a in range(0, k, _native.SAMP_KMAX):
            b = min(k, a + _native.SAMP_KMAX)
            _native.samp_forward(plan, V[a:b], y[a:b], colscale=colscale.reshape(k, -1)[a:b] if per else colscale,
                                 rowscale=rowscale, scale=scale, qpart=None if qpart is None else qpart[a:b])
        return y

    def _adj(self, Y, colscale=None, rowscale=None, scale=1.0):
        """rows of Y (k, npoints) -> (k, npix), every pixel written; rowscale
        one pixel vector or (k, npix) rows"""
        k = Y.shape[0]
        Y = Y.contiguous()
        npix = self._plan_np["npix"]
        if self.npoints == 0:
            _native.require_device(Y)
            return torch.zeros((k, npix), dtype=Y.dtype, device=Y.device)
        out = torch.empty((k, npix), dtype=Y.dtype, device=Y.device)
        plan = self._samp_plan()
        per = rowscale is not None and rowscale.numel() != npix
        for a in range(0, k, _native.SAMP_KMAX):
            b = min(k, a + _native.SAMP_KMAX)
            _native.samp_adjoint(plan, Y[a:b], out[a:b], colscale=colscale,
                                 rowscale=rowscale.reshape(k, -1)[a:b] if per else rowscale, scale=scale)
        return out

    def apply(self, x, mode):
        self._check_input(x, mode)
        v = x.val.reshape(1, -1)
        if mode == self.TIMES:
            return Field(self._target, self._fwd(v).reshape(self._target.shape))
        return Field(self._domain, self._adj(v).reshape(self._domain.shape))
