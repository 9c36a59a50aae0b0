"""Matern-kernel amplitude of the CorrelatedFieldMaker as a fused amplitude
model (src/library/correlated_fields.py:233-274 with the zero-mode and
volume factors of :360-384, :862-938).

On the PowerSpace the amplitude is a closed form in three scalar parameters
(plus the LogNormal zero mode):

    A_0 = V zm                                  (0 with the zero mode disabled)
    A_b = sqrt(V) s (1 + u_b)^(l/4),  u_b = k_b^2 / c^2,   b >= 1
    s = exp(lm_s + ls_s xi_scale), c = exp(lm_c + ls_c xi_cutoff),
    l = mu_l + sig_l xi_loglogslope, zm = exp(lm_o + ls_o xi_zeromode)

so its Jacobian has three columns (four with the zero mode), each a per-bin
vector finished at the linearisation point:

    dA_b/dxi_scale       = ls_s A_b
    dA_b/dxi_cutoff      = -(l ls_c / 2) A_b u_b / (1 + u_b)
    dA_b/dxi_loglogslope = (sig_l / 4) A_b log1p(u_b)
    dA_0/dxi_zeromode    = V zm ls_o

_MaternAmplitudeModel is an amplitude_base._AmplitudeBase (the `amp` of the
fused field, CFJacobian and geovi_batch._CFStage), as
correlated_fields_simple._AmplitudeModel is; its native passes are the
nft_matern_* kernels (csrc/nft_matern.hip): one streaming pass for the JVP, three dot
products for the VJP, no scans and no device-global state.  It has no
two-phase (amp2) form, so the carried CG iteration treats its keys as plain
segments (fused_cg._CarrySeg) and the solve storage stays fp64."""
import ctypes

import numpy as np
import torch

from .. import _native, config
from ..domain_tuple import DomainTuple
from ..domains import PowerSpace
from ..utilities import lognormal_moments
from .amplitude_base import DeviceLin, _AmplitudeBase


def _t(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=config.device())


class MaternLin(DeviceLin):
    """DeviceLin of _MaternAmplitudeModel.forward_rows: k device
    nft_matern_const (buf: the finished columns)"""

    def __init__(self, amp, a, buf, dconst, k):
        h = _native.MaternConst()
        h.B, h.has_zm = amp.B, int(amp.has_zm)
        super().__init__(h, a, buf, dconst, k)


class _MaternAmplitudeModel(_AmplitudeBase):
    """A(scale, cutoff, loglogslope[, zeromode]) on the PowerSpace, its JVP
    and VJP.  scale / cutoff: (mean, std) of LognormalTransforms, loglogslope:
    (mean, std) of a NormalTransform, offset_std: (mean, std) of the LogNormal
    zero mode or None; total_volume: the reference's `totvol`."""

    # the nft_matern kernels are fp64 and have no two-phase (amp2) form: the
    # base's defaults hold (fp64 storage under config.set_cg_precision("fp32"),
    # the 'seg' flavour of the carried iteration)

    def __init__(self, harmonic_partner, offset_std, scale, cutoff, loglogslope, total_volume, prefix,
                 zm_prefix=None):
        self.pspace = PowerSpace(harmonic_partner)
        self.B = self.pspace.shape[0]
        if self.B < 2:
            raise ValueError("the Matern amplitude needs at least two power bins")
        self.prefix = prefix
        zp = prefix if zm_prefix is None else zm_prefix
        self.k_scale, self.k_cutoff, self.k_slope = prefix + "scale", prefix + "cutoff", prefix + "loglogslope"
        self.k_zm = zp + "zeromode"
        self.keys = (self.k_scale, self.k_cutoff, self.k_slope, self.k_zm)   # nft_matern's pointer order
        self.has_zm = offset_std is not None
        self.lm_s, self.ls_s = (float(v) for v in lognormal_moments(*scale))
        self.lm_c, self.ls_c = (float(v) for v in lognormal_moments(*cutoff))
        self.mu_l, self.sig_l = float(loglogslope[0]), float(loglogslope[1])
        self.lm_o, self.ls_o = (float(v) for v in lognormal_moments(*offset_std)) if self.has_zm else (0., 0.)
        self.total_vol = float(total_volume)
        self.k2 = _t(self.pspace.k_lengths ** 2)
        dom = {k: DomainTuple.scalar_domain() for k in (self.k_scale, self.k_cutoff, self.k_slope)}
        if self.has_zm:
            dom[self.k_zm] = DomainTuple.scalar_domain()
        self.domain_dict = dom

    # ------------------------------------------------ torch restatement
    def forward(self, lat):
        """lat: dict key -> device tensor.  Returns (a, cache)."""
        s = torch.exp(self.lm_s + self.ls_s * lat[self.k_scale]).reshape(())
        cc = torch.exp(self.lm_c + self.ls_c * lat[self.k_cutoff]).reshape(())
        l = (self.mu_l + self.sig_l * lat[self.k_slope]).reshape(())
        u = self.k2 / (cc * cc)
        lp = torch.log1p(u)
        a = (self.total_vol ** 0.5) * s * torch.exp(0.25 * l * lp)
        a = torch.cat([a.new_zeros(1), a[1:]])
        c = dict(l=l)
        c["gs"] = self.ls_s * a
        c["gc"] = -(0.5 * l * self.ls_c) * a * (u / (1. + u))
        c["gl"] = (0.25 * self.sig_l) * a * lp
        if self.has_zm:
            zm = torch.exp(self.lm_o + self.ls_o * lat[self.k_zm]).reshape(())
            a = a + torch.cat([(self.total_vol * zm).reshape(1), a.new_zeros(self.B - 1)])
            c["zm"] = zm
        return a, c

    def jvp(self, c, t):
        da = (c["gs"] * t[self.k_scale].reshape(()) + c["gc"] * t[self.k_cutoff].reshape(())
              + c["gl"] * t[self.k_slope].reshape(()))
        if self.has_zm:
            dzm = (self.total_vol * c["zm"] * self.ls_o) * t[self.k_zm].reshape(1)
            da = da + torch.cat([dzm, da.new_zeros(self.B - 1)])
        return da

    def vjp(self, c, g):
        """g: (B,) cotangent of a.  Returns dict key -> cotangent tensors."""
        out = {self.k_scale: torch.sum(c["gs"] * g), self.k_cutoff: torch.sum(c["gc"] * g),
               self.k_slope: torch.sum(c["gl"] * g)}
        if self.has_zm:
            out[self.k_zm] = (self.total_vol * c["zm"] * self.ls_o) * g[0]
        return out

    # ------------------------------------------------------------ native
    def native_const(self, c):
        """(constant set, keep-alive) for the native JVP / VJP: a MaternLin is
        its own; a cache of `forward` becomes a host nft_matern_const that
        points at its column tensors"""
        if isinstance(c, MaternLin):
            return c, None
        keep = {n: c[n].contiguous() for n in ("gs", "gc", "gl")}
        k = _native.MaternConst()
        for n, v in keep.items():
            setattr(k, n, v.data_ptr())
        k.l = float(c["l"])
        k.zm = float(c["zm"]) if self.has_zm else 0.0
        k.ls_s, k.sig_l, k.ls_c, k.ls_o = self.ls_s, self.sig_l, self.ls_c, self.ls_o
        k.total_volume = self.total_vol
        k.B, k.has_zm = self.B, int(self.has_zm)
        return k, keep

    def native_model(self):
        """nft_matern_model of this amplitude"""
        nm = getattr(self, "_nm", None)
        if nm is None:
            k = _native.MaternModel()
            k.k2 = self.k2.data_ptr()
            for n in ("lm_s", "ls_s", "lm_c", "ls_c", "mu_l", "sig_l", "lm_o", "ls_o"):
                setattr(k, n, getattr(self, n))
            k.total_volume = self.total_vol
            k.B, k.has_zm = self.B, int(self.has_zm)
            nm = self._nm = k
        return nm

    def forward_rows(self, at, k, lat_stride, device):
        """Amplitude values and linearisations at k latent points in one
        native pass (nft_matern_forward_batched): at(key) -> device pointer of
        row 0's key or None, rows lat_stride elements apart.  Nothing is read
        back to the host."""
        lib = _native.load()
        nbuf = int(lib.nft_matern_forward_buf(self.B))
        a = torch.empty((k, self.B), dtype=torch.float64, device=device)
        buf = torch.empty((k, nbuf), dtype=torch.float64, device=device)
        dconst = torch.empty(k * ctypes.sizeof(_native.MaternConst), dtype=torch.uint8, device=device)
        P = ctypes.c_void_p
        _native._check(lib.nft_matern_forward_batched(
            ctypes.byref(self.native_model()), P(at(self.k_scale)), P(at(self.k_cutoff)), P(at(self.k_slope)),
            P(at(self.k_zm)), int(lat_stride), k, P(a.data_ptr()), self.B, P(buf.data_ptr()), nbuf,
            P(dconst.data_ptr()), _native.stream_ptr()))
        return MaternLin(self, a, buf, dconst, k)

    def _jvp(self, const, item_consts, t, lat_stride, da, da_stride, da_elem_stride, k):
        host, ic, mode = self._item_mode(const, item_consts)
        P = ctypes.c_void_p
        lib = _native.load()
        _native._check(lib.nft_matern_jvp_batched(ctypes.byref(host), P(ic), mode, t, int(lat_stride),
                                                  P(da.data_ptr()), int(da_stride), int(da_elem_stride), k, 0,
                                                  _native.stream_ptr()))
        return da

    def _vjp(self, const, item_consts, g, g_stride, out, d, lat_stride, shift, k):
        host, ic, mode = self._item_mode(const, item_consts)
        P = ctypes.c_void_p
        lib = _native.load()
        # sized for 8 right-hand sides at least (a few kB): solves of 1..8 RHS
        # share one buffer, so a captured iteration's workspace is never regrown
        ws = _native.workspace(max(k, 8) * lib.nft_matern_workspace(self.B), g.device, "matern")
        _native._check(lib.nft_matern_vjp_batched(ctypes.byref(host), P(ic), mode, P(g.data_ptr()), int(g_stride),
                                                  out, d, int(lat_stride), float(shift), P(ws.data_ptr()), k,
                                                  _native.stream_ptr()))

    def native_jvp_batched(self, const, D, off, da, interleave=False, item_consts=None):
        """da[b] = J_amp D[b] for the k rows of a packed batch D (k, size);
        interleave: da is (B, k), bin-major (one contiguous run per bin)."""
        k, size = D.shape
        if D.dtype != torch.float64 or da.dtype != torch.float64:
            raise _native.NativeError("the Matern amplitude JVP is fp64 only")
        _native.require_device(D, da)
        return self._jvp(const, item_consts, self._key_ptrs(D, off), size, da, 1 if interleave else self.B,
                         k if interleave else 1, k)

    def native_vjp_batched(self, const, g, Q, off, D=None, shift=0.0, item_consts=None):
        """Q[b] amplitude keys = shift * D[b] + J_amp^T g[b]."""
        k, size = Q.shape
        if g.dtype != torch.float64 or Q.dtype != torch.float64 or (D is not None and D.dtype != torch.float64):
            raise _native.NativeError("the Matern amplitude VJP is fp64 only")
        _native.require_device(g, Q, D)
        dk = self._key_ptrs(D, off) if (D is not None and shift != 0.0) else None
        self._vjp(const, item_consts, g, self.B, self._key_ptrs(Q, off), dk, size, shift, k)
        return Q

    def native_jvp(self, const, t, da):
        _native.require_device(da, *t.values())
        return self._jvp(const, None, self._dict_ptrs(t), 0, da, 0, 1, 1)

    def native_vjp(self, const, g, out, d=None, shift=0.0):
        """out/d: dict key -> contiguous device tensors; out = shift*d + J^T g."""
        _native.require_device(g)
        use_d = d is not None and shift != 0.0
        self._vjp(const, None, g, 0, self._dict_ptrs(out), self._dict_ptrs(d) if use_d else None, 0,
                  shift if use_d else 0.0, 1)
        return out
