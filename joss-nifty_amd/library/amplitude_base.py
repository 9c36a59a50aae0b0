"""What the amplitude models of the fused correlated field share
(correlated_fields_simple._AmplitudeModel, matern._MaternAmplitudeModel,
product._ProductAmplitudeModel): the device linearisation handle DeviceLin
and the base class _AmplitudeBase with the key-pointer helpers, the item-mode
rule and the capability defaults that CFJacobian, fused_cg and
geovi_batch._CFStage read."""
import ctypes

from .. import _native


class DeviceLin:
    """Linearisation points of an amplitude made on the device
    (forward_rows): values a (k, B), the per-row constant vectors (buf) and k
    device constant structs (dconst, bytes) pointing into them.  Stands in for
    the host constant struct wherever a native JVP / VJP takes one: `host`
    (a filled ctypes struct of the same type) carries B and the flags for the
    launch geometry, the kernels read every value from the device structs."""

    def __init__(self, host, a, buf, dconst, k, keep=None):
        self.host, self.a, self.buf, self.dconst, self.k, self.keep = host, a, buf, dconst, k, keep
        self.size = ctypes.sizeof(host)
        self._rep = {}

    @property
    def B(self):
        return self.host.B

    def row_bytes(self, r):
        return self.dconst[r * self.size:(r + 1) * self.size]

    def items(self, k, row=0):
        """device pointer of k consecutive structs: row `row` shared by k
        right-hand sides"""
        if self.k == 1 and k == 1:
            return self.dconst.data_ptr()
        key = (k, row)
        if key not in self._rep:
            self._rep[key] = self.row_bytes(row).repeat(k)
        return self._rep[key].data_ptr()

    def per_item(self, k):
        """device pointer of one struct per right-hand side: the k rows of
        their own, or the single point shared by all k"""
        return self.items(k) if self.k == 1 else self.dconst.data_ptr()


class _AmplitudeBase:
    """Base of the amplitude models.  A model sets `keys` (its latent keys in
    the order its native kernels take them), `B`, `domain_dict`, and provides
    forward / jvp / vjp (torch), native_const, native_jvp(_batched) and
    native_vjp(_batched); one with per-row device linearisations also
    forward_rows."""

    keys = ()

    # fp32 CG storage (config.set_cg_precision) only where the model's kernels
    # take it; otherwise a solve with this amplitude stays fp64
    supports_fp32 = False

    # no two-phase (amp2) form unless the model has one: the carried CG
    # iteration then runs the 'seg' flavour
    def amp2_table(self, const):
        return None

    def amp2_tiles(self, const, k):
        return 0

    def forward_native(self, lat):
        """forward_rows at one latent point given as a dict key -> tensor"""
        vals = {kk: v.contiguous() for kk, v in lat.items() if kk in self.domain_dict}
        _native.require_device(*vals.values())

        def at(key):
            return vals[key].data_ptr() if key in vals else None
        lin = self.forward_rows(at, 1, 0, next(iter(vals.values())).device)
        lin.keep = vals
        return lin

    def _ptrs(self, D, off):
        """base pointers of the amplitude keys of packed row 0 of D (or None)"""
        def at(key):
            if key not in off:
                return None
            return D[0, off[key]:].data_ptr()
        return at

    def _key_ptrs(self, T, off):
        """ctypes array of the pointers of `keys` in packed row 0 of T (NULL
        for absent keys), or NULL if T is None"""
        if T is None:
            return None
        return (ctypes.c_void_p * len(self.keys))(*[T[0, off[kk]:].data_ptr() if kk in off else None
                                                    for kk in self.keys])

    def _dict_ptrs(self, d):
        """the same array for a dict key -> contiguous tensor"""
        if d is None:
            return None
        return (ctypes.c_void_p * len(self.keys))(*[d[kk].data_ptr() if kk in d else None for kk in self.keys])

    @staticmethod
    def _item_mode(const, item_consts):
        """(host constant struct, item pointer, item_mode): a DeviceLin
        without per-item constants is ONE device constant set shared by every
        right-hand side (mode 2)"""
        if isinstance(const, DeviceLin):
            if item_consts is None:
                return const.host, const.items(1), 2
            return const.host, item_consts, 1
        return const, item_consts, (1 if item_consts else 0)
