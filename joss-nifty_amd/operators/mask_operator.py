"""MaskOperator (src/operators/mask_operator.py:26-59): the values of a field
on the pixels that are not flagged, in an UnstructuredDomain.

A sampling response with one corner of weight 1 per data point
(operators/sampling_plan.py, csrc/nft_samp.hip): the forward gathers the kept
pixels in C order of the grid, the adjoint writes every pixel, zeros at the
flagged ones.  Its sandwich R^T C R is diagonal, so inside a sampling metric
it is a pointwise weight (fused_middle returns a tensor)."""
import numpy as np
import torch

from .. import config
from ..domain_tuple import DomainTuple
from ..domains import UnstructuredDomain
from ..field import Field
from .sampling_plan import SamplingResponse, samp_plan


class MaskOperator(SamplingResponse):
    """flags: Field, converted to boolean; where True the input is flagged
    (dropped)."""

    def __init__(self, flags):
        if not isinstance(flags, Field):
            raise TypeError("flags must be a Field")
        self._domain = DomainTuple.make(flags.domain)
        keep = np.logical_not(flags.val_np().astype(bool))
        kept = np.flatnonzero(keep.reshape(-1))
        self._target = DomainTuple.make(UnstructuredDomain(int(kept.size)))
        self._init_plan(samp_plan((int(keep.size),), kept.reshape(1, -1)))

    def fused_middle(self, dr, c, fct=1.0):
        """The grid tensor fct * dr^2 * R^T c (c a scalar or a per-datum
        weight): R^T C R is diagonal, so the sampling metric keeps its
        pointwise path."""
        shape = self._domain.shape
        dev = config.device()
        if torch.is_tensor(c):
            cv = c.reshape(-1).expand(self.npoints).to(torch.float64)
        else:
            cv = torch.full((self.npoints,), float(c), dtype=torch.float64, device=dev)
        w = self._adj(cv.reshape(1, -1), scale=float(fct)).reshape(shape)
        if dr is not None:
            d = dr.reshape(shape).to(torch.float64)
            w = w * d * d
        return w.contiguous()
