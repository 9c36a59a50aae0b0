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
(the device-side cross-check of the native one).  fp64 only.

On a domain of two spaces (S, X) with `space` naming the position RGSpace S
(FuncConvolutionOperator.on_space; the plain constructor takes one space, as
it always did) the reference subtracts the mean over the WHOLE field, not the mean of each
slice, and the kernel's zero mode k0 is not 1 in general, so with m(x) the
mean over all pixels of both spaces

    C x = Re ifftn_S(k * fftn_S(x)) + (1 - k0) * m(x)

with the RAW k (zero mode k0, not 1) broadcast over X.  The second term is
(1 - k0) / N * 1 1^T: C stays symmetric and keeps the total sum, but not the
sums of the slices.  With one space this is the kt[0] = 1 form above, which
keeps its own code path.  space = 0, a 2-D power-of-two S and an even number
of pixels in X run one nft_conv_space_apply_batched call: the real array
(n0, n1, ne) read as complex (n0, n1, ne / 2) carries two slices of X through
full-length complex transforms over the axes of S and the real table
(csrc/nft_conv.hip).  Every other accepted product domain takes two
nft_hartley_fused calls over the axes of S with the table broadcast over X in
the first one's epilogue, then the mean term as one add."""
import os

import numpy as np
import torch

from .. import _native, config, utilities
from ..domain_tuple import DomainTuple
from ..domains import RGSpace
from ..field import Field
from .endomorphic_operator import EndomorphicOperator
from .middle import ResponseMiddle


def conv_gain(space, func):
    """kt on the full harmonic grid of the position RGSpace `space` (numpy):
    the values of get_conv_kernel_from_func with the zero mode set to 1."""
    kt = space.get_default_codomain().get_conv_kernel_from_func(func).val_np().astype(np.float64).copy()
    kt.reshape(-1)[0] = 1.
    return kt


def conv_kernel(space, func):
    """k on the full harmonic grid of the position RGSpace `space` (numpy):
    the raw values of get_conv_kernel_from_func."""
    return space.get_default_codomain().get_conv_kernel_from_func(func).val_np().astype(np.float64).copy()


def _native_wanted():
    """NFT_CONV_NATIVE=0: every grid takes the two-transform path.  Read at
    every call (a graph keeps the choice made at its capture)."""
    return os.environ.get("NFT_CONV_NATIVE", "1") != "0"


class FuncConvolutionOperator(EndomorphicOperator):
    """Parameters: domain (one RGSpace of 1 to 3 dimensions), func (takes the
    distance from the centre, in the units of the RGSpace distances, returns
    the kernel amplitude), space (None or 0).

    The constructor keeps what it always did: a domain of more than one space
    is a NotImplementedError.  `FuncConvolutionOperator.on_space(domain, func,
    space)` builds the operator on one space of a two-space domain (the
    module docstring has its formula: the mean term is that of the WHOLE
    field, which a caller should have asked for by name).  Unlike the
    reference, which on a product domain raises ValueError("Mismatch...")
    unless its DomainTuple cache already holds the harmonic product tuple,
    on_space never raises for that."""

    def __init__(self, domain, func, space=None):
        self._setup(domain, func, space, 1)

    @classmethod
    def on_space(cls, domain, func, space=None):
        """The operator on `domain[space]` of a DomainTuple of one or two
        spaces: the reference's FuncConvolutionOperator(domain, func, space)."""
        op = cls.__new__(cls)
        op._setup(domain, func, space, 2)
        return op

    def _setup(self, domain, func, space, max_spaces):
        self._domain = DomainTuple.make(domain)
        space = utilities.infer_space(self._domain, space)
        if not isinstance(self._domain[space], RGSpace):
            raise TypeError("unsupported domain")
        if len(self._domain) > max_spaces:
            if max_spaces == 1:
                raise NotImplementedError("FuncConvolutionOperator: exactly one RGSpace (on_space takes a domain "
                                          "of two spaces)")
            raise NotImplementedError("FuncConvolutionOperator.on_space: domains of one or two spaces")
        sp = self._domain[space]
        if sp.harmonic:
            raise TypeError("FuncConvolutionOperator: the domain must be a position space")
        if not 1 <= len(sp.shape) <= 3:
            raise NotImplementedError("FuncConvolutionOperator: RGSpaces of 1 to 3 dimensions")
        self._capability = self.TIMES | self.ADJOINT_TIMES
        self._space = space
        self._product = len(self._domain) == 2
        self._shape = tuple(self._domain.shape)
        self._npix = int(np.prod(self._shape))
        k = conv_kernel(sp, func)
        self._gain0 = float(k.reshape(-1)[0])
        if self._product:
            # the raw table: the zero mode's share of the global mean is the
            # (1 - k0) * m(x) term
            self._gain = k
            self._sub_shape = tuple(sp.shape)
            self._sub_axes = tuple(self._domain.axes[space])
        else:
            self._gain = conv_gain(sp, func)
        self._dev = None

    @property
    def gain(self):
        """the table the kernels use (numpy, full harmonic grid of the
        convolved space): kt with zero mode 1 on one space, the raw k on a
        product domain."""
        return self._gain

    @property
    def gain0(self):
        """k0, the raw kernel's zero mode."""
        return self._gain0

    # ---------------------------------------------------------------- device
    def _device(self):
        if self._dev is None and self._product:
            dev = config.device()
            nsub = int(np.prod(self._sub_shape))
            full = torch.from_numpy(self._gain / nsub).to(dev).contiguous()
            native, plan = False, None
            if self._space == 0 and len(self._sub_shape) == 2:
                n0, n1 = self._sub_shape
                ne = self._npix // nsub
                native = ne % 2 == 0 and _native.conv_space_supported(n0, n1, ne)
                if native:
                    plan = _native.conv_space_plan(n0, n1, ne, full, self._gain0)
            self._dev = dict(full=full, plan=plan, native=native, wide=None)
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
        """True where applications run nft_conv_apply_batched (on a product
        domain nft_conv_space_apply_batched)."""
        return self._device()["native"] and _native_wanted()

    def conv_plan(self):
        """the native plan (None on a product domain the native pipeline does
        not serve)"""
        return self._device()["plan"]

    def quad_blocks(self):
        """qpart columns of `apply_rows` (the two-transform path sums one)."""
        if not self.native:
            return 1
        if self._product:
            return _native.conv_space_quad_blocks(self.conv_plan())
        return _native.conv_quad_blocks(self.conv_plan())

    def _wide_table(self):
        """k / (pixels of S) broadcast over the other space, on the full
        domain's grid: the epilogue table of the two-transform path"""
        d = self._device()
        if d["wide"] is None:
            ones = (1,) * (len(self._shape) - len(self._sub_shape))
            t = d["full"].reshape(self._sub_shape + ones if self._space == 0 else ones + self._sub_shape)
            d["wide"] = t.expand(self._shape).contiguous()
        return d["wide"]

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
            run = _native.conv_space_apply if self._product else _native.conv_apply
            for a in range(0, k, _native.CONV_KMAX):
                b = min(k, a + _native.CONV_KMAX)
                run(d["plan"], X[a:b], out[a:b], colscale=cs, rowscale=rs, scale=scale,
                    qpart=None if qpart is None else qpart[a:b])
            return out
        if self._product:
            return self._apply_rows_product(X, cs, rs, scale, qpart, out)
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

    def _apply_rows_product(self, X, cs, rs, scale, qpart, out):
        """the two-transform path on a product domain: Hartley transforms over
        the axes of S only, then the mean term (1 - k0) * mean(colscale * x)"""
        axes = self._sub_axes
        table = self._wide_table()
        coef = (1. - self._gain0) / self._npix
        for v in range(X.shape[0]):
            xv = X[v].contiguous()
            x = xv.reshape(self._shape)
            h = torch.empty_like(x)
            if cs is None:
                _native.hartley_fused(h, axes, x=x, epi=dict(a=table))
                m = xv.sum()
            else:
                _native.hartley_fused(h, axes, pro=dict(a=cs.reshape(self._shape), x=x), epi=dict(a=table))
                m = torch.dot(cs, xv)
            t = torch.empty_like(x)
            _native.hartley_fused(t, axes, x=h)
            t.add_(m * coef)
            y = t * scale if rs is None else t * rs.reshape(self._shape) * scale
            out[v].copy_(y.reshape(-1))
            if qpart is not None:
                _native.dot(t.reshape(-1), y.reshape(-1).contiguous(), out=qpart[v, :1])
        return out

    # C is symmetric: both sides of the responses' row interface
    # (operators/middle.py) are apply_rows
    _fwd = _adj = apply_rows

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
        m = ResponseMiddle(self, dr, c, fct, fp32=False)
        m.conv_plan, m.conv_scales = self.conv_plan(), m.scales_as
        return m
