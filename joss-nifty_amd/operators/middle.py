"""The middle of a fused sampling metric  J^T M J  (SandwichOperator.fused[1]).

A middle is a grid tensor (a pointwise weight), None, or a callable on grid
tensors.  `Middle` is the callable's protocol as a type: what the CG drivers
(minimization/fused_cg.py) and the model Jacobian's mv_grid read from it.  The
drivers read the attributes and do not test for the class, so any callable
serves; one without the attributes has none of the capabilities.

Every response that can stand in a middle has one row interface

    R._fwd(V, colscale=None, rowscale=None, scale=1.0, qpart=None) -> (k, ndata)
    R._adj(Y, colscale=None, rowscale=None, scale=1.0, ...)        -> (k, npix)
    R.quad_blocks()                                   qpart columns of _fwd

on (k, n) rows with any k >= 1: the method chunks into launches of at most its
family's KMAX vectors and allocates the output; the pixel-side scale
(colscale of _fwd, rowscale of _adj) is one shared vector or (k, npix) rows
where the kernels take it.  LOSResponse (library/los_response.py),
SamplingResponse (MaskOperator, LinearInterpolator) and
FuncConvolutionOperator provide it; `ResponseMiddle` is written against it
alone."""
import ctypes

import numpy as np
import torch

from .. import _native


class Middle:
    """s -> M s on grid tensors, s one grid or, with supports_batch, a batch
    along a leading axis.  The capabilities are plain attributes (an instance
    may set its own):

    supports_batch  a leading batch axis is accepted
    supports_fp32   fp32 vectors are accepted (config.set_cg_precision)
    supports_fold   `fold`, an nft_fold_partials call (part, nb, nrhs, out
                    address, out stride) that needs the partials in qpart, is
                    carried by the middle's last launch
    quad_blocks     columns of `qpart`, (k, >= quad_blocks) fp64 rows that
                    receive the per-block partials of the quadratic form
                    s . M s from the data space; 0: no such partials"""
    supports_batch = False
    supports_fp32 = False
    supports_fold = False
    quad_blocks = 0

    def __call__(self, s, qpart=None, fold=None):
        raise NotImplementedError

    def _no_fold(self, fold):
        if fold is not None and not self.supports_fold:
            raise NotImplementedError(f"{type(self).__name__}: the curvature fold runs as its own launch")


class ResponseMiddle(Middle):
    """s -> fct * dr * R^T (c * R (dr * s)): the middle of a sampling metric
    J^T D R^T C R D J with the pixel-space diagonal dr (tensor or None) and
    the data-space weight c (tensor or float) folded into the response's two
    calls (column / row scales).  The families differ in data alone: the
    response's quad_blocks(), fold (LOS: the fold rides in the adjoint) and
    fp32 (False: an fp64-only response, its scales cast to fp64 once, here).

    Read-only for callers: response, factor, quad_blocks, scales_as.  The
    family's fused_middle adds its plan and scales_as under the names its
    readers know: plan / scales (LOS), samp_plan / samp_scales
    (interpolator), conv_plan / conv_scales (PSF).  Nothing here or in the
    drivers looks at those names."""
    supports_batch = True

    def __init__(self, response, dr, c, fct=1.0, fp32=True, fold=False):
        self.response = response
        self.shape = tuple(response.domain.shape)
        self.npix = int(np.prod(self.shape))
        self.quad_blocks = int(response.quad_blocks())
        self.supports_fp32 = fp32
        self.supports_fold = fold
        drf = None if dr is None else dr.reshape(-1)
        self.factor = float(fct)
        cv = None
        if torch.is_tensor(c):
            cv = c.reshape(-1).expand(response.target.size)
        else:
            self.factor *= float(c)
        if not fp32:
            drf, cv = (None if t is None else t.to(torch.float64) for t in (drf, cv))
        self._scales = {torch.float64: tuple(None if t is None else t.contiguous() for t in (drf, cv))}

    def scales_as(self, dt):
        """(pixel-side diagonal, data-side weight), None each where there is
        none, in the vectors' dtype (fp32 CG storage: cast once per dtype; an
        fp64-only response takes no other vectors and keeps fp64)"""
        if not self.supports_fp32:
            dt = torch.float64
        if dt not in self._scales:
            self._scales[dt] = tuple(None if t is None else t.to(dt) for t in self._scales[torch.float64])
        return self._scales[dt]

    def rows(self, s):
        """(s as (k, npix) rows, whether s came with a batch axis)"""
        batched = s.dim() > len(self.shape)
        return s.reshape(s.shape[0] if batched else 1, self.npix), batched

    def grids(self, out, batched):
        """rows back on the grid, in the form `rows` found"""
        out = out.reshape((out.shape[0],) + self.shape)
        return out if batched else out[0]

    def __call__(self, s, qpart=None, fold=None):
        self._no_fold(fold)
        d, w = self.scales_as(s.dtype)
        v, batched = self.rows(s)
        R = self.response
        y = R._fwd(v, colscale=d, rowscale=w, scale=self.factor, qpart=qpart)
        out = R._adj(y, rowscale=d) if fold is None else R._adj(y, rowscale=d, fold=fold)
        return self.grids(out, batched)


class LosAddMiddle(Middle):
    """s -> LOS middle(s) + addw * s: one LOS branch `los` (a ResponseMiddle
    over an LOSResponse) and the summed pointwise branches `addw`, which the
    LOS adjoint adds while it stores its tile (nft_los_adjoint_add).  qpart:
    the LOS forward's partials in the first nft_los_quad_blocks columns, the
    pointwise branches' in the following nft_los_add_blocks."""
    supports_batch = True
    supports_fp32 = True

    def __init__(self, los, addw):
        self.los, self.addw = los, addw
        plan = los.response._box_plan()
        self.quad_blocks = los.quad_blocks + int(_native.load().nft_los_add_blocks(ctypes.byref(plan)))
        self._aw = {addw.dtype: addw.reshape(-1)}

    def __call__(self, s, qpart=None, fold=None):
        self._no_fold(fold)
        lm = self.los
        d, w = lm.scales_as(s.dtype)
        if s.dtype not in self._aw:
            self._aw[s.dtype] = self._aw[self.addw.dtype].to(s.dtype)
        v, batched = lm.rows(s)
        v = v.contiguous()
        R = lm.response
        y = R._fwd(v, colscale=d, rowscale=w, scale=lm.factor, qpart=qpart)
        out = R._adj(y, rowscale=d, addw=self._aw[s.dtype], addx=v,
                     qpart=None if qpart is None else qpart[:, lm.quad_blocks:])
        return lm.grids(out, batched)


class SumMiddle(Middle):
    """s -> sum of the branches' results, `parts` grid tensors or callables:
    correct for any mix, one extra pass per branch, no data-space curvature"""

    def __init__(self, parts):
        self.parts = tuple(parts)
        self.supports_batch = all(torch.is_tensor(p) or getattr(p, "supports_batch", False) for p in parts)
        self.supports_fp32 = all(torch.is_tensor(p) or getattr(p, "supports_fp32", False) for p in parts)
        self._cast = {}

    def _weight(self, i, dt):
        p = self.parts[i]
        if p.dtype == dt:
            return p
        if (i, dt) not in self._cast:
            self._cast[(i, dt)] = p.to(dt)
        return self._cast[(i, dt)]

    def __call__(self, s, qpart=None, fold=None):
        self._no_fold(fold)
        if qpart is not None:
            raise NotImplementedError("SumMiddle: no data-space curvature (quad_blocks is 0)")
        res = None
        for i, p in enumerate(self.parts):
            g = s * self._weight(i, s.dtype) if torch.is_tensor(p) else p(s)
            res = g if res is None else res + g
        return res


class OperatorMiddle(Middle):
    """s -> fct * mid^T cheese mid s through the generic operator tree on
    Fields of `target` (mid None: the cheese alone): a middle no response
    fuses.  One grid at a time, fp64."""

    def __init__(self, mid, cheese, target, fct):
        self.mid, self.cheese, self.target, self.factor = mid, cheese, target, fct

    def __call__(self, s, qpart=None, fold=None):
        from ..field import Field
        self._no_fold(fold)
        if qpart is not None:
            raise NotImplementedError("OperatorMiddle: no data-space curvature (quad_blocks is 0)")
        f = Field(self.target, s)
        if self.mid is None:
            r = self.cheese(f)
        else:
            r = self.mid.adjoint_times(self.cheese(self.mid(f)))
        return r.val * self.factor if self.factor != 1. else r.val
