"""FuncConvolutionOperator (src/operators/convolution_operators.py:30-97):
periodic convolution of an RGSpace field with a radially symmetric kernel.

The reference applies  mean(x) + HT diag(k V) HT^T wgt (x - mean(x))  with
k = codomain.get_conv_kernel_from_func(func).  All volume factors cancel and
k is real and even, so this is  C x = Re ifftn(kt * fftn(x))  with kt = k and
kt[0] = 1 (the mean subtraction is exactly "zero-mode gain 1").  C is
symmetric: adjoint_times is times.

Native grids (nft_conv_supported: 2-D / 3-D powers of two) run one
nft_conv_apply_batched call per application (csrc/nft_conv.hip).  Every other
grid the FFT engine transforms takes two nft_hartley_fused calls with the
Hartley-layout table in the first one's epilogue, and a separate
nft_dot_batched for the quadratic form; NFT_CONV_NATIVE=0 forces that path
(the device-side cross-check of the native one).  fp64 only."""
import os

import numpy as np
import torch

from .. import _native, config, utilities
from ..domain_tuple import DomainTuple
from ..domains import RGSpace
from ..field import Field
from .endomorphic_operator import EndomorphicOperator


def conv_gain(space, func):
    """kt on the full harmonic grid of the position RGSpace `space` (numpy):
    the values of get_conv_kernel_from_func with the zero mode set to 1."""
    kt = space.get_default_codomain().get_conv_kernel_from_func(func).val_np().astype(np.float64).copy()
    kt.reshape(-1)[0] = 1.
    return kt


def _native_wanted():
    """NFT_CONV_NATIVE=0: every grid takes the two-transform path.  Read at
    every call (a graph keeps the choice made at its capture)."""
    return os.environ.get("NFT_CONV_NATIVE", "1") != "0"


class FuncConvolutionOperator(EndomorphicOperator):
    """Parameters: domain (one RGSpace of 1 to 3 dimensions), func (takes the
    distance from the centre, in the units of the RGSpace distances, returns
    the kernel amplitude), space (None or 0)."""

    def __init__(self, domain, func, space=None):
        self._domain = DomainTuple.make(domain)
        space = utilities.infer_space(self._domain, space)
        if not isinstance(self._domain[space], RGSpace):
            raise TypeError("unsupported domain")
        if len(self._domain) != 1:
            raise NotImplementedError("FuncConvolutionOperator: exactly one RGSpace (the fused model has one space)")
        sp = self._domain[0]
        if sp.harmonic:
            raise TypeError("FuncConvolutionOperator: the domain must be a position space")
        if not 1 <= len(sp.shape) <= 3:
            raise NotImplementedError("FuncConvolutionOperator: RGSpaces of 1 to 3 dimensions")
        self._capability = self.TIMES | self.ADJOINT_TIMES
        self._shape = tuple(sp.shape)
        self._npix = int(np.prod(self._shape))
        self._gain = conv_gain(sp, func)
        self._dev = None

    @property
    def gain(self):
        """kt (numpy, full grid, zero mode 1)."""
        return self._gain

    # ---------------------------------------------------------------- device
    def _device(self):
        if self._dev is None:
            dev = config.device()
            full = torch.from_numpy(self._gain / self._npix).to(dev).contiguous()
            nh = self._shape[-1] // 2 + 1
            half = full[..., :nh].contiguous()
            self._dev = dict(full=full, half=half, plan=_native.conv_plan(self._shape, half),
                             native=_native.conv_supported(self._shape))
        return self._dev

    @property
    def native(self):
        """True where applications run nft_conv_apply_batched."""
        return self._device()["native"] and _native_wanted()

    def conv_plan(self):
        return self._device()["plan"]

    def quad_blocks(self):
        """qpart columns of `apply_rows` (the two-transform path sums one)."""
        return _native.conv_quad_blocks(self.conv_plan()) if self.native else 1

    def apply_rows(self, X, colscale=None, rowscale=None, scale=1.0, qpart=None, out=None):
        """rows of X (k, npix) -> scale * rowscale * C (colscale * row), at
        most 8 vectors per call; qpart (k, >= quad_blocks) fp64 rows: the
        partials of t . y (t the convolution before scale * rowscale)."""
        if X.dtype != torch.float64:
            raise TypeError("FuncConvolutionOperator: fp64 fields only")
        k = X.shape[0]
        if out is None:
            out = torch.empty((k, self._npix), dtype=X.dtype, device=X.device)
        d = self._device()
        cs = None if colscale is None else colscale.reshape(-1).contiguous()
        rs = None if rowscale is None else rowscale.reshape(-1).contiguous()
        if self.native:
            for a in range(0, k, _native.CONV_KMAX):
                b = min(k, a + _native.CONV_KMAX)
                _native.conv_apply(d["plan"], X[a:b], out[a:b], colscale=cs, rowscale=rs, scale=scale,
                                   qpart=None if qpart is None else qpart[a:b])
            return out
        axes = tuple(range(len(self._shape)))
        table = d["full"]
        for v in range(k):
            x = X[v].contiguous().reshape(self._shape)
            h = torch.empty_like(x)
            if cs is None:
                _native.hartley_fused(h, axes, x=x, epi=dict(a=table))
            else:
                _native.hartley_fused(h, axes, pro=dict(a=cs.reshape(self._shape), x=x), epi=dict(a=table))
            t = torch.empty_like(x)
            _native.hartley_fused(t, axes, x=h)
            y = t * scale if rs is None else t * rs.reshape(self._shape) * scale
            out[v].copy_(y.reshape(-1))
            if qpart is not None:
                _native.dot(t.reshape(-1), y.reshape(-1).contiguous(), out=qpart[v, :1])
        return out

    def apply(self, x, mode):
        self._check_input(x, mode)
        if x.val.is_complex():
            return self._apply_real(x.real) + self._apply_real(x.imag) * 1j
        return self._apply_real(x)

    def _apply_real(self, x):
        v = x.val.reshape(1, -1)
        return Field(self._domain, self.apply_rows(v).reshape(self._shape))

    # ---------------------------------------------------------------- metric
    def fused_middle(self, dr, c, fct=1.0):
        """Callable s -> dr * C (fct * c * C (dr * s)) on grid tensors: the
        middle of a sampling metric J^T D C^T W C D J with the pixel-space
        diagonal dr (tensor or None) in the first call's column scale and the
        second call's row scale, and the grid weight c (tensor or float) in
        the first call's row scale."""
        shape = self._shape
        npix = self._npix
        drf = None if dr is None else dr.reshape(-1).to(torch.float64).contiguous()
        scale = float(fct)
        cv = None
        if torch.is_tensor(c):
            cv = c.reshape(-1).expand(npix).to(torch.float64).contiguous()
        else:
            scale *= float(c)

        def scales(dt):
            return drf, cv

        def middle(s, qpart=None, fold=None):
            """qpart (optional, (k, >= quad_blocks) fp64): per-block partials
            of the quadratic form s . middle(s), from the data space"""
            if fold is not None:
                raise NotImplementedError("convolution middle: the curvature fold runs as its own launch")
            batched = s.dim() > len(shape)
            k = s.shape[0] if batched else 1
            y = self.apply_rows(s.reshape(k, npix), colscale=drf, rowscale=cv, scale=scale, qpart=qpart)
            out = self.apply_rows(y, rowscale=drf).reshape((k,) + shape)
            return out if batched else out[0]
        middle.supports_batch = True
        middle.supports_fp32 = False
        middle.supports_fold = False
        middle.quad_blocks = self.quad_blocks()
        # what the middle is made of (read-only); named apart from the LOS
        # middle's `plan` / `scales` (operators/joint_middle.py tells by them)
        middle.response = self
        middle.conv_plan = self.conv_plan()
        middle.conv_scales = scales
        middle.factor = scale
        return middle
