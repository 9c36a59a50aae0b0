"""LinearInterpolator (src/operators/linear_interpolation.py:32-103):
multilinear interpolation of an RGSpace field at arbitrary positions.

The reference builds a scipy COO matrix with 2^ndim entries per point.  Here
the plan keeps the cell indices and the fp64 fractions of every point and the
kernels (csrc/nft_samp.hip) recompute the weights, bitwise the reference's;
the adjoint sums per grid pixel in the COO order.  Positions wrap
periodically."""
import numpy as np
import torch

from ..domain_tuple import DomainTuple
from ..domains import RGSpace, UnstructuredDomain
from .middle import ResponseMiddle
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
        if self.npoints == 0:
            # no data: the zero map, as a pointwise weight
            from .. import config
            return torch.zeros(self._domain.shape, dtype=torch.float64, device=config.device())
        m = ResponseMiddle(self, dr, c, fct)
        m.samp_plan, m.samp_scales = self._samp_plan(), m.scales_as
        return m
