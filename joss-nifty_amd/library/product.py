"""Product-spectrum correlated fields (two `add_fluctuations` components of
the CorrelatedFieldMaker on a product domain, src/library/correlated_fields.py:
764-823) as one fused field on the joint grid.

Two identities carry it.  With P_g the point mirror k -> -k on the grid axes
of sub-space g and

    R = (P1 + P2 + I - P1 P2) / 2      (symmetric, orthogonal, an involution)

the separable Hartley transform the reference applies is the joint one in a
rotated frame, H_1 (x) H_2 = R H_joint = H_joint R.  And the product of the
two distributed normalised amplitudes with the zero mode is a table over the
combined bins b = b1 * B2 + b2 (invariant under k_a -> -k_a on every axis):

    A[0,0] = z   A[b1,0] = a1[b1]   A[0,b2] = a2[b2]   A[b1,b2] = a1 a2 / z

with z = V1 V2 zm, a1 = V2 m1, a2 = V1 m2 for the components' amplitudes m_i
(_AmplitudeModel without a zero mode: V_i fl_i An_i) and the LogNormal zero
mode zm.  So

    s = offset_mean + c_h H_joint[ A[pindex] * (R xi) ],   c_h = dvol(h1) dvol(h2)

is a one-space fused field in the frame xi' = R xi: the prologue gather,
mirror fold, bin sums and the carried CG apply unchanged.  R is orthogonal and
the identity on the other keys, so a CG run on rotated buffers has the natural
run's iterates: fused_cg rotates b and x0 in once and x out once
(to_frame / from_frame), nothing per iteration.

The table, its JVP and VJP are the nft_prod_* kernels and R is nft_mirror_mix
(csrc/nft_prod.hip); the components' B_i-sized Jacobians stay the nft_amp
kernels.  No two-phase (amp2) form: the carried iteration runs the 'seg'
flavour and the solve storage stays fp64."""
import ctypes

import numpy as np
import torch

from .. import _native
from ..domain_tuple import DomainTuple
from ..utilities import lognormal_moments
from .amplitude_base import _AmplitudeBase
from .correlated_fields_simple import CFJacobian, _AmplitudeModel, _FusedFieldBase

_P = ctypes.c_void_p


class _CombinedBins:
    """what the fused field reads of a PowerSpace: the per-pixel bin index on
    the joint harmonic grid, pindex = p1 (x) B2 + p2"""

    def __init__(self, p1, p2):
        i1 = np.asarray(p1.pindex).reshape(p1.pindex.shape + (1,) * p2.pindex.ndim)
        self.pindex = np.ascontiguousarray(i1 * p2.shape[0] + np.asarray(p2.pindex))
        self.shape = (p1.shape[0] * p2.shape[0],)


class ProdLin:
    """One linearisation point: the components' constant sets, the table a
    (1, B) and the device constants of nft_prod_const_size doubles."""

    def __init__(self, c1, c2, a, cb, keep=None):
        self.c1, self.c2, self.a, self.cb, self.keep = c1, c2, a, cb, keep


class _ProductAmplitudeModel(_AmplitudeBase):
    """A(theta_1, theta_2, zeromode) over the combined bins, its JVP and VJP
    (an amplitude_base._AmplitudeBase whose native passes take the keys from
    its two components, so it sets no `keys` of its own).  comps: per
    component (sub-space, harmonic partner, fluctuations, flexibility,
    asperity, loglogavgslope, key prefix);
    offset_std: (mean, std) of the LogNormal zero mode keyed `zm_prefix`zeromode."""

    # the nft_prod kernels are fp64: the base's supports_fp32 = False holds (a
    # solve with this amplitude keeps fp64 storage under
    # config.set_cg_precision("fp32"))

    def __init__(self, comps, offset_std, zm_prefix):
        self.parts = tuple(_AmplitudeModel(t, h, None, fl, flex, asp, sl, pre) for t, h, fl, flex, asp, sl, pre in comps)
        m1, m2 = self.parts
        self.B1, self.B2 = m1.B, m2.B
        self.B = self.B1 * self.B2
        self.pspace = _CombinedBins(m1.pspace, m2.pspace)
        self.k_zm = zm_prefix + "zeromode"
        self.lm_o, self.ls_o = (float(v) for v in lognormal_moments(*offset_std))
        # z = s0 zm, a1 = s1 m1, a2 = s2 m2
        self.s0, self.s1, self.s2 = m1.total_vol * m2.total_vol, m2.total_vol, m1.total_vol
        dom = dict(m1.domain_dict)
        dom.update(m2.domain_dict)
        dom[self.k_zm] = DomainTuple.scalar_domain()
        self.domain_dict = dom

    # ------------------------------------------------ torch restatement
    def table(self, a1, a2, z):
        """the table (B,) of scaled component amplitudes a_i and z"""
        A = torch.outer(a1, a2) / z
        A[:, 0] = a1
        A[0, :] = a2
        A[0, 0] = z
        return A.reshape(-1)

    def forward(self, lat):
        """lat: dict key -> device tensor.  Returns (a, cache)."""
        m1, m2 = self.parts
        a1, c1 = m1.forward(lat)
        a2, c2 = m2.forward(lat)
        z = self.s0 * torch.exp(self.lm_o + self.ls_o * lat[self.k_zm]).reshape(())
        a1, a2 = self.s1 * a1, self.s2 * a2
        return self.table(a1, a2, z), dict(c1=c1, c2=c2, p1=a1 / z, p2=a2 / z, z=z)

    def jvp(self, c, t):
        m1, m2 = self.parts
        d1, d2 = self.s1 * m1.jvp(c["c1"], t), self.s2 * m2.jvp(c["c2"], t)
        dz = c["z"] * self.ls_o * t[self.k_zm].reshape(())
        p1, p2 = c["p1"], c["p2"]
        dA = torch.outer(d1, p2) + torch.outer(p1, d2) - torch.outer(p1, p2) * dz
        dA[:, 0] = d1
        dA[0, :] = d2
        dA[0, 0] = dz
        return dA.reshape(-1)

    def vjp(self, c, g):
        """g: (B,) cotangent of the table.  Returns dict key -> cotangents."""
        m1, m2 = self.parts
        G = g.reshape(self.B1, self.B2)
        p1, p2 = c["p1"], c["p2"]
        w1, w2 = p1.clone(), p2.clone()
        w1[0] = w2[0] = 1.
        g1, g2 = G @ w2, w1 @ G
        g1[0] = g2[0] = 0.
        out = m1.vjp(c["c1"], self.s1 * g1)
        out.update(m2.vjp(c["c2"], self.s2 * g2))
        out[self.k_zm] = c["z"] * self.ls_o * (G[0, 0] - p1[1:] @ G[1:, 1:] @ p2[1:])
        return out

    # ------------------------------------------------------------ native
    def _cb_size(self):
        return int(_native.load().nft_prod_const_size(self.B1, self.B2))

    def native_const(self, c):
        """(constant set, keep-alive): a ProdLin is its own; a cache of
        `forward` becomes one (the constants laid out as nft_prod_forward does)"""
        if isinstance(c, ProdLin):
            return c, None
        m1, m2 = self.parts
        k1, k2 = m1.native_const(c["c1"]), m2.native_const(c["c2"])
        cb = torch.zeros(self._cb_size(), dtype=torch.float64, device=c["p1"].device)
        cb[0], cb[1] = c["z"], c["z"] * self.ls_o
        o2 = 2 + ((self.B1 + 1) & ~1)
        cb[2:2 + self.B1], cb[o2:o2 + self.B2] = c["p1"], c["p2"]
        return ProdLin(k1[0], k2[0], None, cb, keep=(k1[1], k2[1], c)), None

    def forward_native(self, lat):
        """the table and its linearisation at one latent point (dict key ->
        tensor) in native passes: the components' nft_amp_forward_batched, then
        nft_prod_forward.  Nothing is read back to the host."""
        m1, m2 = self.parts
        l1, l2 = m1.forward_native(lat), m2.forward_native(lat)
        xz = lat[self.k_zm].contiguous()
        _native.require_device(xz)
        a = torch.empty((1, self.B), dtype=torch.float64, device=xz.device)
        cb = torch.empty(self._cb_size(), dtype=torch.float64, device=xz.device)
        _native._check(_native.load().nft_prod_forward(
            self.B1, self.B2, _P(l1.a.data_ptr()), self.B1, _P(l2.a.data_ptr()), self.B2, _P(xz.data_ptr()), 0,
            self.lm_o, self.ls_o, self.s0, self.s1, self.s2, 1, _P(a.data_ptr()), self.B, _P(cb.data_ptr()),
            cb.numel(), _native.stream_ptr()))
        return ProdLin(l1, l2, a, cb, keep=xz)

    def _jvp(self, const, d1, d2, tz, lat_stride, da, k):
        _native._check(_native.load().nft_prod_jvp_batched(
            self.B1, self.B2, _P(const.cb.data_ptr()), self.s1, self.s2, _P(d1.data_ptr()), self.B1,
            _P(d2.data_ptr()), self.B2, _P(tz.data_ptr()), int(lat_stride), _P(da.data_ptr()), k,
            _native.stream_ptr()))
        return da

    def _vjp(self, const, g, k, oz, dz, lat_stride, shift):
        """the components' cotangents (k, B1), (k, B2) of the bin sums g (k, B)
        and the zero-mode key's result at oz"""
        lib = _native.load()
        bufs = self.__dict__.setdefault("_gb", {})
        if k not in bufs:
            bufs[k] = tuple(torch.empty((k, b), dtype=torch.float64, device=g.device) for b in (self.B1, self.B2))
        g1, g2 = bufs[k]
        # sized for 8 right-hand sides at least: solves of 1..8 RHS share one
        # buffer, so a captured iteration's workspace is never regrown
        ws = _native.workspace(max(k, 8) * lib.nft_prod_workspace(self.B1, self.B2), g.device, "prod")
        _native._check(lib.nft_prod_vjp_batched(
            self.B1, self.B2, _P(const.cb.data_ptr()), self.s1, self.s2, _P(g.data_ptr()), self.B, _P(g1.data_ptr()),
            self.B1, _P(g2.data_ptr()), self.B2, _P(oz), _P(dz), int(lat_stride), float(shift), _P(ws.data_ptr()),
            k, _native.stream_ptr()))
        return g1, g2

    def _dbufs(self, k, device):
        bufs = self.__dict__.setdefault("_db", {})
        if k not in bufs:
            bufs[k] = tuple(torch.empty((k, b), dtype=torch.float64, device=device) for b in (self.B1, self.B2))
        return bufs[k]

    def native_jvp_batched(self, const, D, off, da, interleave=False, item_consts=None):
        """da (B, k), bin-major = J_amp D[b] for the k rows of a packed batch
        D (k, size): the components' tangents, then the table's"""
        k, size = D.shape
        if D.dtype != torch.float64 or da.dtype != torch.float64:
            raise _native.NativeError("the product amplitude JVP is fp64 only")
        if item_consts is not None or not (interleave or k == 1):
            raise _native.NativeError("the product amplitude JVP writes the bin-major layout of one constant set")
        _native.require_device(D, da)
        m1, m2 = self.parts
        d1, d2 = self._dbufs(k, D.device)
        m1.native_jvp_batched(const.c1, D, off, d1)
        m2.native_jvp_batched(const.c2, D, off, d2)
        return self._jvp(const, d1, d2, D[0, off[self.k_zm]:], size, da, k)

    def native_vjp_batched(self, const, g, Q, off, D=None, shift=0.0, item_consts=None):
        """Q[b] amplitude keys = shift * D[b] + J_amp^T g[b]."""
        k, size = Q.shape
        if g.dtype != torch.float64 or Q.dtype != torch.float64 or (D is not None and D.dtype != torch.float64):
            raise _native.NativeError("the product amplitude VJP is fp64 only")
        if item_consts is not None:
            raise _native.NativeError("the product amplitude VJP takes one constant set")
        _native.require_device(g, Q, D)
        m1, m2 = self.parts
        use_d = D is not None and shift != 0.0
        g1, g2 = self._vjp(const, g, k, Q[0, off[self.k_zm]:].data_ptr(),
                           D[0, off[self.k_zm]:].data_ptr() if use_d else None, size, shift)
        m1.native_vjp_batched(const.c1, g1, Q, off, D, shift)
        m2.native_vjp_batched(const.c2, g2, Q, off, D, shift)
        return Q

    def native_jvp(self, const, t, da):
        m1, m2 = self.parts
        _native.require_device(da, *t.values())
        d1, d2 = (torch.empty(b, dtype=torch.float64, device=da.device) for b in (self.B1, self.B2))
        m1.native_jvp(const.c1, t, d1)
        m2.native_jvp(const.c2, t, d2)
        return self._jvp(const, d1, d2, t[self.k_zm], 0, da, 1)

    def native_vjp(self, const, g, out, d=None, shift=0.0):
        """out/d: dict key -> contiguous device tensors; out = shift*d + J^T g."""
        m1, m2 = self.parts
        _native.require_device(g)
        use_d = d is not None and shift != 0.0
        g1, g2 = self._vjp(const, g, 1, out[self.k_zm].data_ptr(), d[self.k_zm].data_ptr() if use_d else None, 0,
                           shift if use_d else 0.0)
        m1.native_vjp(const.c1, g1[0], out, d, shift)
        m2.native_vjp(const.c2, g2[0], out, d, shift)
        return out

    # no two-phase (amp2) form of the table: the carried iteration runs the
    # 'seg' flavour; the components' constant-scan tables are made here, before
    # any graph capture uses them
    def amp2_table(self, const):
        for m, c in zip(self.parts, (const.c1, const.c2)):
            m.amp2_table(c)
        return None


class ProductJacobian(CFJacobian):
    """CFJacobian of the product field; its xi0 slot holds R xi.  The operator
    interface (_times_t, _adjoint_t, apply, sandwich_apply, lowering) is in
    the natural frame: the xi tangent is mixed on the way in, the xi cotangent
    on the way out.  The packed-buffer methods fused_cg calls
    (metric_flat(_batch), mv_*) are the base's: they work on buffers in the
    rotated frame, which to_frame / from_frame enter and leave with one
    batched launch each."""

    def _mix(self, x):
        m = self._m
        return _native.mirror_mix(x, torch.empty_like(x), m.grid, m.split)

    def _times_t(self, t):
        t = dict(t)
        t[self._m.k_xi] = self._mix(t[self._m.k_xi].contiguous())
        return self._times_frame(t)

    def _adjoint_t(self, g, out=None, d=None, shift=0.0):
        k_xi = self._m.k_xi
        res = self._adjoint_frame(g)
        res[k_xi] = self._mix(res[k_xi])
        if out is None:
            return res
        # a lowered metric (lowering.py: the per-sample geoVI refinement of this
        # field) asks for the natural-frame adjoint into packed views
        for k, r in res.items():
            if shift != 0.0:
                torch.add(r.reshape(out[k].shape), d[k], alpha=shift, out=out[k])
            else:
                out[k].copy_(r.reshape(out[k].shape))
        return out

    def to_frame(self, buf):
        """the xi segment of every row of the packed (k, size) buffer `buf`
        times R, in place, one launch (R is an involution: from_frame is the
        same map)"""
        m = self._m
        xo = self.layout.key_offsets[m.k_xi]
        k, size = buf.shape
        _native.mirror_mix(buf[0, xo:], buf[0, xo:], m.grid, m.split, rows=k, x_stride=size, y_stride=size)
        return buf

    from_frame = to_frame


class _ProductFieldModel(_FusedFieldBase):
    """The fused correlated field of TWO add_fluctuations components on a
    product domain with a LogNormal zero mode: the one-space engine on the
    joint grid in the frame R xi, with the combined-bin amplitude table."""

    _jacobian = ProductJacobian
    # packed buffers of its solves are in the frame R xi (geovi_batch's own
    # Jacobian passes do not know it and leave this field to the per-sample path)
    own_frame = True

    def __init__(self, comps, offset_mean, offset_std, xi_prefix):
        amp = _ProductAmplitudeModel(comps, offset_std, xi_prefix)
        targets, partners = tuple(c[0] for c in comps), tuple(c[1] for c in comps)
        hp = DomainTuple.make(partners)
        self.grid = tuple(int(n) for n in hp.shape)
        self.split = len(partners[0].shape)
        super().__init__(amp, targets, hp, offset_mean, xi_prefix,
                         c_h=float(partners[0].scalar_dvol) * float(partners[1].scalar_dvol))

    def _xi_frame(self, xi):
        xi = xi.contiguous()
        return _native.mirror_mix(xi, torch.empty_like(xi), self.grid, self.split)

    def __repr__(self):
        return f"Product-spectrum correlated field (fused) {self._target.shape}"
