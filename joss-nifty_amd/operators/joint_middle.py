"""The middle of a joint likelihood's sampling metric.

For lh1 + lh2 + ... on one model with Jacobian J the transformation's branches
write to distinct keys, so the metric is  J^T (sum_i M_i^T C_i M_i) J: one
pair of model transforms around a SUM of branch middles.  `joint_middle` forms
that sum from the branches' own middles (the second element of
SandwichOperator.fused):

  all grid tensors            -> their sum, a tensor: the pointwise paths run
                                 as for a single likelihood
  one LOS middle + tensors    -> the LOS forward followed by the LOS adjoint
                                 that adds  sum(W) * s  while it stores its
                                 tile (nft_los_adjoint_add), with the
                                 curvature partials of both branches
  anything else               -> a callable summing the branches' results
                                 (correct, one extra pass per branch; no
                                 data-space curvature)
"""
import ctypes

import numpy as np
import torch

from .. import _native


def _is_los(p):
    return callable(p) and hasattr(p, "plan") and hasattr(p, "scales")


def joint_middle(core, parts):
    """Sum of the branch middles `parts` (grid tensors or callables on grid
    tensors) of sandwiches sharing the fused Jacobian `core`."""
    parts = list(parts)
    if not parts:
        raise ValueError("joint_middle: no branches")
    if len(parts) == 1:
        return parts[0]
    shape = tuple(core.target.shape)
    tensors = [p for p in parts if torch.is_tensor(p)]
    los = [p for p in parts if _is_los(p)]
    addw = None
    if tensors:
        addw = tensors[0].expand(shape)
        for t in tensors[1:]:
            addw = addw + t.expand(shape)
        addw = addw.contiguous()
    if len(tensors) == len(parts):
        return addw
    if len(los) == 1 and len(tensors) == len(parts) - 1:
        return _los_add_middle(los[0], addw, shape)
    return _sum_middle(parts)


def _los_add_middle(lm, addw, shape):
    from ..library.los_response import LOS_KMAX
    plan = lm.plan
    lib = _native.load()
    nql = int(lib.nft_los_quad_blocks(ctypes.byref(plan)))
    nqa = int(lib.nft_los_add_blocks(ctypes.byref(plan)))
    npix = int(np.prod(shape))
    nlos = int(plan.nlos)
    scale = float(lm.factor)
    aw = {addw.dtype: addw.reshape(-1)}

    def middle(s, qpart=None, fold=None):
        """s -> LOS middle(s) + addw * s.  qpart ((k, >= quad_blocks) fp64):
        the partials of s . middle(s) -- the LOS forward's in the first
        nft_los_quad_blocks columns, the pointwise branch's in the following
        nft_los_add_blocks."""
        if fold is not None:
            raise NotImplementedError("joint middle: the curvature fold runs as its own launch")
        drf, cv = lm.scales(s.dtype)
        if s.dtype not in aw:
            aw[s.dtype] = aw[addw.dtype].to(s.dtype)
        w = aw[s.dtype]
        batched = s.dim() > len(shape)
        k = s.shape[0] if batched else 1
        v = s.reshape(k, npix).contiguous()
        y = torch.empty((k, nlos), dtype=v.dtype, device=v.device)
        out = torch.empty((k,) + shape, dtype=v.dtype, device=v.device)
        for a in range(0, k, LOS_KMAX):
            b = min(k, a + LOS_KMAX)
            if qpart is not None:
                _native.los_forward_quad_batched(plan, v[a:b], y[a:b], qpart[a:b], colscale=drf, rowscale=cv,
                                                 scale=scale)
                _native.los_adjoint_add(plan, y[a:b], out[a:b].view(b - a, npix), w, v[a:b], rowscale=drf,
                                        qpart=qpart[a:b, nql:])
            else:
                _native.los_forward_batched(plan, v[a:b], y[a:b], colscale=drf, rowscale=cv, scale=scale)
                _native.los_adjoint_add(plan, y[a:b], out[a:b].view(b - a, npix), w, v[a:b], rowscale=drf)
        return out if batched else out[0]
    middle.supports_batch = True
    middle.supports_fp32 = True
    middle.supports_fold = False
    middle.quad_blocks = nql + nqa
    middle.los = lm
    middle.addw = addw
    return middle


def _sum_middle(parts):
    cast = {}

    def weight(i, dt):
        p = parts[i]
        if p.dtype == dt:
            return p
        if (i, dt) not in cast:
            cast[(i, dt)] = p.to(dt)
        return cast[(i, dt)]

    def middle(s):
        res = None
        for i, p in enumerate(parts):
            g = s * weight(i, s.dtype) if torch.is_tensor(p) else p(s)
            res = g if res is None else res + g
        return res
    middle.supports_batch = all(torch.is_tensor(p) or getattr(p, "supports_batch", False) for p in parts)
    middle.supports_fp32 = all(torch.is_tensor(p) or getattr(p, "supports_fp32", False) for p in parts)
    middle.supports_fold = False
    middle.quad_blocks = 0
    middle.parts = tuple(parts)
    return middle
