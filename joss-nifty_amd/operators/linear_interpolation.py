"""LinearInterpolator (src/operators/linear_interpolation.py:32-103):
multilinear interpolation of an RGSpace field at arbitrary positions.

The reference builds a scipy COO matrix with 2^ndim entries per point.  Here
the plan keeps the cell indices and the fp64 fractions of every point and the
kernels (csrc/nft_samp.hip) recompute the weights, bitwise the reference's;
the adjoint sums per grid pixel in the COO order.  Positions wrap
periodically."""
import numpy as np
import torch

from .. import _native
from ..domain_tuple import DomainTuple
from ..domains import RGSpace, UnstructuredDomain
from .sampling_plan import MAX_ENTRIES, SamplingResponse, interp_points, samp_plan


class LinearInterpolator(SamplingResponse):
    """Parameters: domain (one RGSpace of 1 to 3 dimensions), sampling_points
    (numpy.ndarray of shape (ndim, npoints))."""

    def __init__(self, domain, sampling_points):
        self._domain = DomainTuple.make(domain)
        for i in range(len(self._domain)):
            if not isinstance(self._domain[i], RGSpace):
                raise TypeError("The domain must consist of RGSpaces.")
        if len(self._domain) != 1:
            raise NotImplementedError("LinearInterpolator: exactly one RGSpace (the fused model has one space)")
        sp = self._domain[0]
        ndim = len(sp.shape)
        if not 1 <= ndim <= 3:
            raise NotImplementedError("LinearInterpolator: RGSpaces of 1 to 3 dimensions")
        if not (isinstance(sampling_points, np.ndarray) and sampling_points.ndim == 2):
            raise TypeError("sampling_points must be a numpy array of shape (ndim, npoints)")
        if sampling_points.shape[0] != ndim:
            raise TypeError("sampling_points must be a numpy array of shape (ndim, npoints)")
        npoints = sampling_points.shape[1]
        if npoints * 2 ** ndim > MAX_ENTRIES:
            raise ValueError("LinearInterpolator: more than 2^31 - 1 matrix entries")
        self._target = DomainTuple.make(UnstructuredDomain(npoints))
        idx, frac = interp_points(sp.shape, sp.distances, sampling_points)
        self._init_plan(samp_plan(sp.shape, idx, frac))

    def fused_middle(self, dr, c, fct=1.0):
        """Callable s -> fct * dr * R^T (c * R (dr * s)) on grid tensors: the
        middle of a sampling metric J^T D R^T C R D J with pixel-space diagonal
        dr (tensor or None) and data-space weight c (tensor or float) folded
        into the two sampling launches (column / row scales)."""
        npnt = self.npoints
        shape = self._domain.shape
        npix = int(np.prod(shape))
        if npnt == 0:
            # no data: the zero map, as a pointwise weight
            from .. import config
            return torch.zeros(shape, dtype=torch.float64, device=config.device())
        drf = None if dr is None else dr.reshape(-1).contiguous()
        scale = float(fct)
        cv = None
        if torch.is_tensor(c):
            cv = c.reshape(-1).expand(npnt).contiguous()
        else:
            scale *= float(c)
        cast = {}

        def scales(dt):
            # fp32 CG storage (config.set_cg_precision): scales in the input's dtype
            if dt == torch.float64:
                return drf, cv
            if dt not in cast:
                cast[dt] = (None if drf is None else drf.to(dt), None if cv is None else cv.to(dt))
            return cast[dt]

        def middle(s, qpart=None, fold=None):
            """qpart (optional, (k, >= quad_blocks) fp64): per-block partials
            of the quadratic form s . middle(s), from the data space"""
            if fold is not None:
                raise NotImplementedError("sampling middle: the curvature fold runs as its own launch")
            d, w = scales(s.dtype)
            batched = s.dim() > len(shape)
            k = s.shape[0] if batched else 1
            y = self._fwd(s.reshape(k, npix), colscale=d, rowscale=w, scale=scale, qpart=qpart)
            out = self._adj(y, rowscale=d).reshape((k,) + tuple(shape))
            return out if batched else out[0]
        middle.supports_batch = True
        middle.supports_fp32 = True
        middle.supports_fold = False
        middle.quad_blocks = _native.samp_quad_blocks(self._samp_plan())
        # what the middle is made of (read-only); named apart from the LOS
        # middle's `plan` / `scales` (operators/joint_middle.py tells by them)
        middle.response = self
        middle.samp_plan = self._samp_plan()
        middle.samp_scales = scales
        middle.factor = scale
        return middle
