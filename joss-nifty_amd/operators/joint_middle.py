"""The middle of a joint likelihood's sampling metric.

For lh1 + lh2 + ... on one model with Jacobian J the transformation's branches
write to distinct keys, so the metric is  J^T (sum_i M_i^T C_i M_i) J: one
pair of model transforms around a SUM of branch middles.  `joint_middle` forms
that sum from the branches' own middles (the second element of
SandwichOperator.fused):

  all grid tensors            -> their sum, a tensor: the pointwise paths run
                                 as for a single likelihood
  one LOS middle + tensors    -> LosAddMiddle: the LOS forward followed by
                                 the LOS adjoint that adds  sum(W) * s  while
                                 it stores its tile (nft_los_adjoint_add),
                                 with the curvature partials of both branches
  anything else               -> SumMiddle: the branches' results summed
                                 (correct, one extra pass per branch; no
                                 data-space curvature)

The classes are in operators/middle.py.
"""
import torch

from .middle import LosAddMiddle, ResponseMiddle, SumMiddle


def joint_middle(core, parts):
    """Sum of the branch middles `parts` (grid tensors or callables on grid
    tensors) of sandwiches sharing the fused Jacobian `core`."""
    from ..library.los_response import LOSResponse
    parts = list(parts)
    if not parts:
        raise ValueError("joint_middle: no branches")
    if len(parts) == 1:
        return parts[0]
    shape = tuple(core.target.shape)
    tensors = [p for p in parts if torch.is_tensor(p)]
    los = [p for p in parts if isinstance(p, ResponseMiddle) and isinstance(p.response, LOSResponse)]
    addw = None
    if tensors:
        addw = tensors[0].expand(shape)
        for t in tensors[1:]:
            addw = addw + t.expand(shape)
        addw = addw.contiguous()
    if len(tensors) == len(parts):
        return addw
    if len(los) == 1 and len(tensors) == len(parts) - 1:
        return LosAddMiddle(los[0], addw)
    return SumMiddle(parts)
