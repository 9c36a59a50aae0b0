"""Fused conjugate gradient for sampling metrics  M = shift * 1 + J^T W J.

Same algorithm as ConjugateGradient.__call__ (src/minimization/
conjugate_gradient.py:48-126), on packed device vectors:

  q' = M' d                     fused model pipeline (core.metric_flat, M = shift + M')
  curv = d.(q' + shift d)       nft_cg_curv        -> sc[CURV]
  x -= a d ; r -= a (q' + s d)  nft_cg_update      -> sc[GAMMA]=r.r, x.r, x.b
  (every nreset-th step: r = M x - b exactly, nft_cg_residual)
The shift is applied element-wise inside the CG kernels (same arithmetic as
forming q = q' + shift d first), so the matvec never reads d a second time.
  host: guards + controller on (curv, gamma, value = (x.r - x.b)/2)
  d = max(0, g/g_prev) d + r    nft_cg_direction

All scalars stay on the device; one 16-double D2H read per iteration feeds the
host-side controller, exactly as the reference decides on host floats.
"""
import collections
import ctypes
import math
import os

import numpy as np
import torch

from .. import _native
from ..logger import logger
from .conjugate_gradient import ConjugateGradient


USE_GRAPHS = os.environ.get("NFT_NO_GRAPH") is None
# iterations run eagerly before the loop body is captured: capturing costs a
# few ms, which short solves (NewtonCG directions, ~5 steps) never win back
GRAPH_AFTER = 4


def fusable_metric(A):
    """(core, W, shift) if A = shift*1 + Sandwich(fused core, W), else None."""
    from ..operators.sandwich_operator import SandwichOperator
    from ..operators.scaling_operator import ScalingOperator
    from ..operators.sum_operator import SumOperator
    if isinstance(A, SandwichOperator):
        return None if A.fused is None else (A.fused[0], A.fused[1], 0.0)
    if isinstance(A, SumOperator):
        sands, shift = [], 0.0
        for op, neg in zip(A._ops, A._neg):
            if isinstance(op, SandwichOperator) and op.fused is not None and not neg:
                sands.append(op)
            elif isinstance(op, ScalingOperator) and complex(op._factor).imag == 0:
                shift += (-1 if neg else 1) * complex(op._factor).real
            else:
                return None
        if not sands:
            return None
        if len(sands) == 1:
            return sands[0].fused[0], sands[0].fused[1], shift
        # the metric of a joint likelihood (MGVI: lh1.metric + lh2.metric + 1):
        # sandwiches around one shared model Jacobian add their middles
        core = sands[0].fused[0]
        if any(s.fused[0] is not core for s in sands):
            return None
        joint = A.__dict__.get("_joint_fused")
        if joint is None:
            from ..operators.joint_middle import joint_middle
            joint = A.__dict__["_joint_fused"] = joint_middle(core, [s.fused[1] for s in sands])
        return core, joint, shift
    return None


class _State:
    """Energy-like view of the fused iterate for IterationControllers."""

    def __init__(self, value, gnorm, lazy):
        self._value, self.gradient_norm, self._lazy = value, gnorm, lazy

    @property
    def value(self):
        """the energy value (a callable is evaluated on first access)"""
        if callable(self._value):
            self._value = self._value()
        return self._value

    @property
    def position(self):
        return self._lazy()[0]

    @property
    def gradient(self):
        return self._lazy()[1]


def _stale():
    raise RuntimeError("CG energy value read after its iteration: the fused solve computes it "
                       "on demand only while the controller checks that iterate")


_CAPTURE_STREAM = None


def _capture(fn):
    """HIP graph of the launches fn makes.  Same capture as the
    torch.cuda.graph context manager, minus its device synchronize, gc.collect
    and empty_cache preamble (milliseconds per capture, paid per CG solve)."""
    global _CAPTURE_STREAM
    if _CAPTURE_STREAM is None:
        _CAPTURE_STREAM = torch.cuda.Stream()
    g = torch.cuda.CUDAGraph()
    cur = torch.cuda.current_stream()
    _CAPTURE_STREAM.wait_stream(cur)
    with torch.cuda.stream(_CAPTURE_STREAM):
        # thread-local capture: the background RNG thread may page-lock host
        # memory (random._pin) while the main thread captures
        g.capture_begin(capture_error_mode="thread_local")
        try:
            fn()
        finally:
            g.capture_end()
    cur.wait_stream(_CAPTURE_STREAM)
    return g


def _reads_value(ctl):
    """False for controllers that never look at the energy value (GradientNormController.check without a name
    and without an energy history, iteration_controllers.py:188-221).  A subclass may read it in an overridden
    check, so only the exact class qualifies.  (The decision trace reads values from scalars recorded beside
    the iteration, whichever runs.)"""
    from .iteration_controllers import GradientNormController
    return not (type(ctl) is GradientNormController and getattr(ctl, "_name", None) is None
                and getattr(ctl, "_history", None) is None)


# data-space curvature (nifty_amd.h "curvature from the data space"): shift * d.d summed while d is formed,
# (J d).W(J d) while the LOS forward reduces its lines -- no curvature pass over q and d (NFT_CURV_DATA=0: off)
CURV_DATA = os.environ.get("NFT_CURV_DATA", "1") != "0"
# ... also for value-driven controllers (energy deltas, gradient-norm tolerances; NFT_CURV_DATA_VALUE=1, off by
# default).  Equal in exact arithmetic, the data-space curvature rounds differently from the reference's
# d.(A d), and alpha = gamma / curv then no longer cancels d.r exactly in r -= alpha q: the CG energies leave
# the reference's trajectory (DESIGN.md section 1 has the measurement).  Value-driven controllers therefore
# keep d.q, and with it the separate update pass (the carried update needs alpha before the adjoint).
CURV_DATA_VALUE = os.environ.get("NFT_CURV_DATA_VALUE", "0") == "1"


def _count_only(ctl):
    """True for a controller whose decisions depend on the iteration count
    alone (GradientNormController without tolerances)."""
    from .iteration_controllers import GradientNormController
    return (type(ctl) is GradientNormController and ctl._tol_abs_gradnorm is None
            and ctl._tol_rel_gradnorm is None)


def _count_silent(ctl):
    """a count-only controller that logs nothing and keeps no energy history:
    its checks read no energy"""
    return (_count_only(ctl) and ctl._name is None and ctl._iteration_limit is not None
            and getattr(ctl, "_history", None) is None)


class _CountOnlyState:
    """energy stand-in for the checks of a queued chunk: count-only
    controllers read nothing from it (any read fails loudly)"""

    def __getattr__(self, name):
        raise RuntimeError(f"count-only controller read energy.{name} in a queued CG chunk")


_COUNT_ONLY_STATE = _CountOnlyState()

# queued CG iterations between host reads (NFT_CG_CHUNK=0: one read per step)
CHUNK = os.environ.get("NFT_CG_CHUNK", "1") != "0"
# The grid segment's CG update carried by the adjoint transform's epilogue (data-space curvature: alpha is known
# before the adjoint): q's grid segment is neither stored nor read back (NFT_CG_CARRY=0: separate update pass)
_CARRY = os.environ.get("NFT_CG_CARRY", "1") != "0"
# ... and its direction update inside the folded prologue (NFT_CG_CARRY_DIR=0: a separate direction pass)
_CARRY_DIR = os.environ.get("NFT_CG_CARRY_DIR", "1") != "0"
# the amplitude keys' direction with the JVP, their update + the finalize with the VJP in the two-phase
# amplitude kernels (NFT_CG_AMP2=0: separate launches)
_AMP2 = os.environ.get("NFT_CG_AMP2", "1") != "0"
# deferred iterate inside queued chunks of count-only solves (nft_hartley_fuse.lazy_*): the grid segment's
# directions go to ring slots, x is brought up to date once per chunk (nft_cg_lazy_flush, bitwise the per-step
# update); NFT_CG_LAZY=0: x updated every step
LAZY = os.environ.get("NFT_CG_LAZY", "1") != "0"
# compaction of the lock-step batch once right-hand sides stop (NFT_CG_COMPACT=0: frozen rows ride along)
COMPACT = os.environ.get("NFT_CG_COMPACT", "1") != "0"
# at most MAX_BATCH right-hand sides per loop (fused_cg_batch_or_none)
MAX_BATCH = 8
# which iterations the batched loop ran (tests assert the timed path ran) and its frame-hook launches
STATS = collections.Counter()


def _frame(core, hook, *bufs, copy=False):
    """the packed (k, size) buffers through the core's frame hook (to_frame / from_frame: one batched launch
    each, counted in STATS["frame_launches"]; on copies if asked); a core without the hook: as they are"""
    f = getattr(core, hook, None)
    if f is None:
        return bufs
    STATS["frame_launches"] += sum(b is not None for b in bufs)
    return tuple(b if b is None else f(b.clone() if copy else b) for b in bufs)


def _quad_blocks(core, W, dtype, controllers=()):
    """partials per RHS of the metric's data-space quadratic form, or 0"""
    if not CURV_DATA or dtype not in (torch.float64, torch.float32):
        return 0
    if dtype == torch.float32 and not (hasattr(core, "phases_fp32") and core.phases_fp32(1)):
        # fp32 storage: the data-space curvature rides in the carried
        # iteration only (its amplitude keys in the two-phase kernels)
        return 0
    if not CURV_DATA_VALUE and not all(_count_only(c) for c in controllers):
        return 0
    if not getattr(core, "supports_quad", False):
        return 0
    if torch.is_tensor(W):
        # pointwise W (Gaussian / Poisson): the forward transform's epilogue
        f = getattr(core, "pointwise_quad_blocks", None)
        return int(f(W)) if f is not None else 0
    return int(getattr(W, "quad_blocks", 0) or 0) if callable(W) else 0


def _carry_flavour(core, k, dtype=torch.float64):
    """'amp2' | 'seg': how the carried iteration (_CarryIteration) treats the
    amplitude keys, None where the adjoint's epilogue cannot carry the update.
    fp32 storage: 'amp2' only (the separate segment passes are fp64)."""
    if not (_CARRY and hasattr(core, "cg_blocks") and core.cg_blocks(k) > 0):
        return None
    if (_AMP2 and _CARRY_DIR and hasattr(core, "amp2_tiles") and core.amp2_tiles(k) > 0
            and hasattr(core, "dir_blocks") and core.dir_blocks(k) > 0):
        return "amp2" if dtype in (torch.float64, torch.float32) else None
    return "seg" if dtype == torch.float64 else None


# kind: plain (direction, matvec, curvature d.q, update) | quad (curvature
#   from the data space, nq partials per RHS) | carry (_CarryIteration, flavour
#   amp2 | seg); chunk: several graph replays per host read; lazy: the chunks
#   defer the iterate; need_value: a controller or the trace reads energies;
#   eager_only: the loop body is never captured; xb: x.b of the energy value
#   is streamed by the "update" kernel, a "dot" beside the carried iteration, or
#   formed on "demand" (also: no b); path: kind[+chunk] (FusedCGBatch.path)
IterationPlan = collections.namedtuple("IterationPlan", "kind nq flavour chunk lazy need_value eager_only xb path")


def plan_iteration(core, W, dtype, controllers, k, has_b, tracing, ring_bytes, free_bytes, live=None):
    """Which iteration k right-hand sides of this metric, storage dtype and
    controller set run: the one place that reads the switches and the core's
    capabilities.  `live`: the controllers still iterating when the solve
    starts (default: all) -- they alone decide the chunking.  ring_bytes: the
    deferred iterate's ring (nreset * k * n elements); free_bytes: free device
    memory, a number or a callable asked only where all else allows the ring.
    Value-driven solves are short (NewtonCG directions, ~7 iterations): their
    body stays eager (captured it measured 788 against 747 us per RHS iteration)."""
    eager_only = any(_reads_value(c) for c in controllers)
    need_value = bool(tracing) or eager_only
    nq = _quad_blocks(core, W, dtype, controllers)
    flavour = _carry_flavour(core, k, dtype) if nq else None
    kind = "carry" if flavour else "quad" if nq else "plain"
    chunk = bool(CHUNK and all(_count_silent(c) for c in (controllers if live is None else live)))
    xb = "demand" if not (need_value and has_b) else "dot" if flavour else "update"
    # deferred iterate: nothing reads x or x.r between a count-only chunk's host reads
    lazy = bool(LAZY and chunk and not need_value and flavour == "amp2"
                and getattr(core, "lazy_ok", lambda k: False)(k)
                and ring_bytes <= 0.5 * (free_bytes() if callable(free_bytes) else free_bytes))
    return IterationPlan(kind, nq, flavour, chunk, lazy, need_value, eager_only, xb, kind + ("+chunk" if chunk else ""))


def _worth_capturing(ctl, niter, min_left=4):
    """Capture only if the controller's iteration limit leaves at least
    `min_left` more iterations to replay (short solves, e.g. NewtonCG's first
    5-iteration direction, stay eager)."""
    lim = getattr(ctl, "_iteration_limit", None)
    return lim is None or lim - niter >= min_left


def fused_cg_or_none(energy, controller, nreset):
    from .quadratic_energy import QuadraticEnergy
    if type(energy) is not QuadraticEnergy:
        return None
    spec = fusable_metric(energy.metric)
    if spec is None:
        from ..lowering import lowered_metric
        lm = lowered_metric(energy.metric)
        if lm is None:
            return None
        spec = (lm, None, 0.0)
    core, W, shift = spec
    if energy.position.domain != core.domain or not core.device.type == "cuda":
        return None
    if mixed_precision(core, W):
        # fp32 storage runs in the batched loop (one right-hand side)
        return FusedCGBatch(core, W, shift, [controller], nreset).run([energy])[0]
    return FusedCG(core, W, shift, controller, nreset).run(energy)


def mixed_precision(core, W):
    """fp32 CG storage requested (config.set_cg_precision) and supported by
    the metric's native pipeline (else the solve stays fp64)."""
    from .. import config
    if config.cg_dtype() != torch.float32 or not getattr(core, "supports_fp32", False):
        return False
    return (not callable(W)) or getattr(W, "supports_fp32", False)


class FusedCG:
    """One fused solve: the batched loop (FusedCGBatch) with one right-hand
    side -- per RHS the batched kernels run exactly the single-solve
    arithmetic."""

    def __init__(self, core, W, shift, controller, nreset=20):
        self.core, self.W, self.shift = core, W, float(shift)
        self.controller = controller
        self.nreset = nreset
        self.layout = core.layout
        self.niter = 0

    def run(self, energy):
        cg = FusedCGBatch(self.core, self.W, self.shift, [self.controller], self.nreset)
        res = cg.run([energy])[0]
        self.niter = cg.niter
        self.path = getattr(cg, "path", None)
        return res


def batch_supported(core, W):
    """True if the fused metric can evaluate a batch of right-hand sides."""
    if not hasattr(core, "metric_flat_batch"):
        return False
    return (not callable(W)) or getattr(W, "supports_batch", False)


def fused_cg_batch_or_none(energies, controllers, nreset):
    """Solve several QuadraticEnergies with the SAME fused sampling metric in
    one batched loop (FusedCGBatch), or None if that does not apply."""
    from .quadratic_energy import QuadraticEnergy
    if len(energies) < 2 or any(type(e) is not QuadraticEnergy for e in energies):
        return None
    A = energies[0].metric
    if any(e.metric is not A for e in energies):
        return None
    if len({e._b is None for e in energies}) != 1:
        return None
    spec = fusable_metric(A)
    if spec is None:
        return None
    core, W, shift = spec
    if not batch_supported(core, W) or not core.device.type == "cuda":
        return None
    if any(e.position.domain != core.domain for e in energies):
        return None
    # at most MAX_BATCH right-hand sides per loop: the direction carried by
    # the folded prologue (and with it the rounding of the curvature) exists
    # for <= 8 items, so a rank holding 32 samples solves them in batches of
    # 8 with the per-RHS arithmetic of a rank holding 4 -- bit-identical KL
    # values on any rank count (tests/test_dist_ranks_gpu.py)
    out = []
    for i in range(0, len(energies), MAX_BATCH):
        out += FusedCGBatch(core, W, shift, controllers[i:i + MAX_BATCH], nreset).run(energies[i:i + MAX_BATCH])
    return out


class _CarryIteration:
    """One CG iteration (k RHS, count-only controllers, no energy values)
    with the update of the grid segment G (the 'xi' key) inside the adjoint
    transform's last pass:

      dir + d.d partials | amplitude JVP | forward transform, W (LOS with the
      (R J d).C(R J d) partials), curvature fold | adjoint transform whose
      epilogue updates x, r on G and writes its r.r, x.r partials per tile |
      bin sums, amplitude VJP | update of the amplitude segments | finalize

    The per-element arithmetic is that of the separate update; the dot
    partials are [amplitude keys before G][G's tiles][keys after G], folded
    in that order.  The same for k = 1 (FusedCG) and k > 1 (FusedCGBatch).
    Constructing it gives the core's flavour: _CarryAmp2 (na > 0) or _CarrySeg."""

    def __new__(cls, lib, core, W, n, k, nq, shift):
        if cls is _CarryIteration:
            cls = _CarryAmp2 if _carry_flavour(core, k) == "amp2" else _CarrySeg
        return object.__new__(cls)

    def __init__(self, lib, core, W, n, k, nq, shift):
        self.lib, self.core, self.W = lib, core, W
        self.n, self.k, self.nq, self.shift = n, k, nq, shift
        self.g0, self.g1 = core.grid_segment()
        self.tiles = core.cg_blocks(k)
        self._partials()
        self.PQ = torch.empty((k, self.nbd + nq), dtype=torch.float64, device=core.device)

    @staticmethod
    def supported(core, k, dtype=torch.float64):
        return _carry_flavour(core, k, dtype) is not None

    def _fold(self, SC):
        """the curvature fold of the d.d and data-space partials; .spec is the
        same call as arguments, for a W that carries it in its own launch"""
        lib, PQ, pstride, k = self.lib, self.PQ, self.nbd + self.nq, self.k
        curv = SC.data_ptr() + _native.CG_CURV * 8

        def fold():
            _native._check(lib.nft_fold_partials(_native.ptr(PQ), pstride, k, ctypes.c_void_p(curv),
                                                 _native.CG_NSCALARS, _native.stream_ptr()))
        fold.spec = (PQ, pstride, k, curv, _native.CG_NSCALARS)
        return fold


class _CarryAmp2(_CarryIteration):
    """the amplitude keys' direction / update carried by the two-phase
    amplitude kernels (nft_amp2_*): partials [amplitude tiles][prologue
    blocks] for d.d, [amplitude tiles] for r.r / x.r (each tile also folds a
    slice of the grid epilogue's partials, GP)"""

    def _partials(self):
        k, dev = self.k, self.core.device
        self.na = self.pro_blk0 = int(self.core.amp2_tiles(k))
        self.nbd = self.na + self.core.dir_blocks(k)
        self.UP = torch.empty((k, 2 * self.na), dtype=torch.float64, device=dev)
        self.GP = torch.empty((k, 3 * self.tiles), dtype=torch.float64, device=dev)

    def __call__(self, X, Rr, D, Q, SC, lazy=None):
        core, g0 = self.core, self.g0
        pstride = self.nbd + self.nq
        da = core.mv_amp_jvp_dir(D, Rr, SC, self.PQ, pstride, self.shift)
        pro_dir = dict(r=Rr[0, g0:], sc=SC, part=self.PQ, pstride=pstride, shift=self.shift, blk0=self.pro_blk0,
                       lazy=lazy)
        cg = dict(x=X[0, g0:], r=Rr[0, g0:], d=D[0, g0:], sc=SC, part=self.GP, stride=self.n, shift=self.shift,
                  nbtot=self.tiles, blk0=0, lazy=lazy)
        w = core.mv_grid(D, da, Q, self.W, 0.0, qpart=self.PQ[:, self.nbd:], after_w=self._fold(SC), cg=cg,
                         pro_dir=pro_dir)
        core.mv_amp_vjp_cg(X, Rr, D, w, SC, self.UP, 2 * self.na, self.GP, 3 * self.tiles, self.tiles, self.tiles,
                           self.shift)


class _CarrySeg(_CarryIteration):
    """the amplitude keys before and after G in direction / update passes of
    their own (fp64): one launch each for two segments, else one per segment"""

    def _partials(self):
        lib, core, n, k, g0, g1 = self.lib, self.core, self.n, self.k, self.g0, self.g1
        self.na = 0
        nb0 = int(lib.nft_cg_dd_blocks(g0)) if g0 > 0 else 0
        nb1 = int(lib.nft_cg_dd_blocks(n - g1)) if n > g1 else 0
        self.amp = [(o, e - o, blk) for (o, e), blk in (((0, g0), 0), ((g1, n), nb0 + self.tiles)) if e > o]
        self.tiles_blk0 = nb0
        self.nbtot = nb0 + self.tiles + nb1
        # the direction: the grid segment's inside the folded prologue (d.d partials
        # [keys before][prologue blocks][keys after]), else one pass over the whole vector
        pb = core.dir_blocks(k) if (_CARRY_DIR and hasattr(core, "dir_blocks")) else 0
        if pb:
            self.dirs = [(o, e - o, blk) for (o, e), blk in (((0, g0), 0), ((g1, n), nb0 + pb)) if e > o]
            self.pro_blk0 = nb0
            self.nbd = nb0 + pb + nb1
        else:
            self.dirs = None
            self.nbd = int(lib.nft_cg_dd_blocks(n))
        self.UP = torch.empty((k, 3 * self.nbtot), dtype=torch.float64, device=core.device)

    def __call__(self, X, Rr, D, Q, SC, lazy=None):
        if lazy is not None:
            raise RuntimeError("the deferred iterate needs the two-phase amplitude kernels")
        core, lib = self.core, self.lib
        P, Pv = _native.ptr, ctypes.c_void_p
        s_ = _native.stream_ptr()
        n, k, g0 = self.n, self.k, self.g0
        pstride = self.nbd + self.nq
        pro_dir = None
        if self.dirs is None:
            _native._check(lib.nft_cg_direction_dd_batched(P(D), P(Rr), n, n, k, 0, P(SC), self.shift, P(self.PQ),
                                                           pstride, s_))
        elif len(self.dirs) == 2 and self.dirs[0][0] == 0:
            (_, n1, _), (o2, n2, blk2) = self.dirs
            _native._check(lib.nft_cg_direction_dd2_batched(P(D), P(Rr), n1, o2, n2, n, k, 0, P(SC), self.shift,
                                                            P(self.PQ), blk2, pstride, s_))
        else:
            for o, ln, blk in self.dirs:
                _native._check(lib.nft_cg_direction_dd_batched(
                    Pv(D.data_ptr() + 8 * o), Pv(Rr.data_ptr() + 8 * o), ln, n, k, 0, P(SC), self.shift,
                    Pv(self.PQ.data_ptr() + 8 * blk), pstride, s_))
        if self.dirs is not None:
            pro_dir = dict(r=Rr[0, g0:], sc=SC, part=self.PQ, pstride=pstride, shift=self.shift,
                           blk0=self.pro_blk0)
        da = core.mv_amp_jvp(D)
        cg = dict(x=X[0, g0:], r=Rr[0, g0:], d=D[0, g0:], sc=SC, part=self.UP, stride=n, shift=self.shift,
                  nbtot=self.nbtot, blk0=self.tiles_blk0)
        w = core.mv_grid(D, da, Q, self.W, 0.0, qpart=self.PQ[:, self.nbd:], after_w=self._fold(SC), cg=cg,
                         pro_dir=pro_dir)
        core.mv_amp_vjp(D, w, Q, 0.0)
        if len(self.amp) == 2 and self.amp[0][0] == 0:
            (_, n1, blk1), (o2, n2, blk2) = self.amp
            _native._check(lib.nft_cg_update_seg2_batched(P(X), P(Rr), P(D), P(Q), n1, blk1, o2, n2, blk2, n, k, 0,
                                                          self.shift, P(SC), P(self.UP), self.nbtot, s_))
        else:
            for o, ln, blk in self.amp:
                e = 8 * o
                _native._check(lib.nft_cg_update_seg_batched(
                    Pv(X.data_ptr() + e), Pv(Rr.data_ptr() + e), Pv(D.data_ptr() + e), Pv(Q.data_ptr() + e),
                    Pv(0), ln, n, k, 0, self.shift, P(SC), P(self.UP), self.nbtot, blk, s_))
        _native._check(lib.nft_cg_finalize_batched(P(self.UP), self.nbtot, k, P(SC), s_))


def _guard_status(ctl, hj):
    """The reference's terminal guards on one RHS's scalars after a step
    (curvature / alpha, then gamma) with its log lines: ctl.ERROR,
    ctl.CONVERGED (gamma == 0), or None (the controller decides)."""
    curv, gamma = hj[_native.CG_CURV], float(hj[_native.CG_GAMMA])
    if hj[_native.CG_FLAG] != 0.0:
        logger.error("Error: ConjugateGradient: "
                     + ("curv==NaN" if np.isnan(curv) else "curv==0." if curv == 0. else "alpha<0."))
        return ctl.ERROR
    if np.isnan(gamma) or gamma < 0:
        logger.error("Error: ConjugateGradient: gamma==NaN" if np.isnan(gamma)
                     else "Positive definiteness of preconditioner violated!")
        return ctl.ERROR
    return ctl.CONVERGED if gamma == 0 else None


def _chunk_host(h, hist, iter_seen, active, pos, controllers):
    """The host's part of a queued chunk, on plain numpy: h the scalars read
    after it, hist the steps' recorded (gamma, x.r, x.b) (decision trace) or
    None, iter_seen the step counts before it.  Every live RHS's controller
    sees exactly the checks a one-step loop would have made, in order; a RHS
    the device froze on a terminal step (NFT_CG_DONE = 2) gets the guards'
    status, CONVERGED where they name none.  Returns {j: status where stopped}."""
    stopped = {}
    for j in active:
        ctl, hj, seen = controllers[j], h[pos[j]], iter_seen[pos[j]]
        p = int(round(hj[_native.CG_ITER] - seen))
        ConjugateGradient.iterations_total += p
        frozen = hj[_native.CG_DONE] == 2.0
        status = None
        for t in range(p - 1 if frozen else p):
            state = _COUNT_ONLY_STATE
            if hist is not None:
                g_, xr_, xb_ = hist[pos[j], (int(round(seen)) + t + 1) % hist.shape[1]]
                state = _State(0.5 * (float(xr_) - float(xb_)), math.sqrt(float(g_)), lambda: None)
            st = ctl.check(state)
            if st != ctl.CONTINUE:
                if t != p - 1:
                    raise RuntimeError("count-only controller stopped inside a queued chunk")
                status = st
        if frozen:
            status = _guard_status(ctl, hj)
            if status is None:
                status = ctl.CONVERGED
        if status is not None:
            stopped[j] = status
    return stopped


_chk, _P = _native._check, _native.ptr


class _BatchLoop:
    """The state of one FusedCGBatch.run_packed: the buffers (X, Rr, Bv, D,
    SC, host, HIST), the row maps (rows, pos, full_X, full_Rr), what setup()
    makes per batch size (plan, Q, AX, PQ, nbd, the carried iteration, the
    lazy ring) and the two HIP graphs.  It stores no callable that refers back
    to it, so it dies by reference count (a graph freed by the cyclic collector
    inside a later capture takes that capture down); run_packed drops the graphs."""

    def __init__(self, cg, X, Rr, Bv, active, results):
        self.cg, self.core, self.lib = cg, cg.core, _native.load()
        self.n, self.dt = cg.layout.size, _native.dtype_code(X.dtype)
        self.X = self.full_X = X
        self.Rr = self.full_Rr = Rr
        self.Bv, self.active, self.results = Bv, active, results
        k0, dev = X.shape[0], self.core.device
        self.rows = list(range(k0))          # buffer position -> original RHS index
        self.pos = {j: j for j in self.rows}  # original RHS index -> buffer position
        self.SC = torch.zeros((k0, _native.CG_NSCALARS), dtype=torch.float64, device=dev)
        self.host = torch.zeros((k0, _native.CG_NSCALARS), dtype=torch.float64).pin_memory()
        self.ws = _native.workspace(k0 * self.lib.nft_reduce_workspace(self.n), dev, "cgb")
        self.graph = self.lgraph = None

    def start(self):
        """gamma = r.r of the start residuals with the reference's checks on
        it, then the loop's state; False if no RHS is left to iterate"""
        cg, SC, Rr, n, results, dev = self.cg, self.SC, self.Rr, self.n, self.results, self.core.device
        k0 = Rr.shape[0]
        for j in range(k0):
            if results[j] is not None:
                SC[j, _native.CG_DONE] = 1.0
        _chk(self.lib.nft_dot_batched(_P(Rr), _P(Rr), n, n, k0, self.dt, _P(SC[:, _native.CG_GAMMA:]),
                                      _native.CG_NSCALARS, _P(self.ws), _native.stream_ptr()))
        self.host.copy_(SC)
        for j in list(self.active):
            g = float(self.host[j, _native.CG_GAMMA])
            if np.isnan(g):
                logger.error("Error: ConjugateGradient: previous_gamma==NaN")
                results[j] = (cg.controllers[j].ERROR, None)
            elif g == 0:
                results[j] = (cg.controllers[j].CONVERGED, None)
            if results[j] is not None:
                SC[j, _native.CG_DONE] = 1.0
                self.active.remove(j)
        if not self.active:
            return False
        # the decision trace records each step's gamma, x.r, x.b on the device
        # (HIST): tracing changes neither the iteration nor the chunking
        from . import trace
        self.tracing = trace.active()
        self.D = Rr.clone()
        self.HIST = torch.zeros((k0, cg.nreset + 1, 3), dtype=torch.float64, device=dev) if self.tracing else None
        self.hsel = torch.tensor([_native.CG_GAMMA, _native.CG_XR, _native.CG_XB], device=dev)
        self.live0 = [cg.controllers[j] for j in self.active]
        self.setup(k0)
        # a core without `subset` applies one metric to every row; a per-RHS
        # metric compacts only if it can restrict itself (subset not None)
        self.can_compact = COMPACT and getattr(self.core, "subset", True) is not None
        self.ii = self.eager = 0
        self.first = True
        self.iter_seen = np.zeros(k0)
        # which iteration this solve runs (diagnostics: tools/demo_profile.py)
        cg.path, cg.compactions = self.plan.path, 0
        return True

    def setup(self, k):
        """the k-dependent iteration state: plan, partials, carried iteration"""
        cg, core, lib, X, n, dev = self.cg, self.core, self.lib, self.X, self.n, self.core.device
        self.Q = torch.zeros_like(X)
        self.AX = None
        self.plan = plan = plan_iteration(core, cg.W, X.dtype, cg.controllers, k, self.Bv is not None, self.tracing,
                                          cg.nreset * k * n * X.element_size(),
                                          lambda: torch.cuda.mem_get_info(dev)[0], live=self.live0)
        # b as the update kernel streams it for x.b (None: x.b not summed there)
        self.Bu = self.Bv if plan.xb == "update" else None
        self.carried = self.lazy = None
        if plan.nq:
            self.nbd = int(lib.nft_cg_dd_blocks(n))
            self.PQ = torch.empty((k, self.nbd + plan.nq), dtype=torch.float64, device=dev)
            if plan.kind == "carry":
                self.carried = _CarryIteration(lib, core, cg.W, n, k, plan.nq, cg.shift)
        if plan.lazy:
            g0 = self.carried.g0
            ring = torch.empty((cg.nreset, k, n), dtype=X.dtype, device=dev)
            alpha = torch.empty((k, cg.nreset), dtype=torch.float64, device=dev)
            self.lazy = dict(ring=ring[0, 0, g0:], sstride=k * n, alpha=alpha, nslot=cg.nreset, buf=ring, g0=g0,
                             ng=core.grid_size())

    def record(self):
        """HIST[r, ITER % (nreset + 1)] = (gamma, x.r, x.b) of every live
        RHS after this step (device ops only: graph-capturable)"""
        HIST, SC = self.HIST, self.SC
        if HIST is None:
            return
        idx = (SC[:, _native.CG_ITER].long() % HIST.shape[1])
        rows = torch.arange(self.X.shape[0], device=SC.device)
        live = (SC[:, _native.CG_DONE] == 0.0).unsqueeze(1)
        cur = HIST[rows, idx]
        HIST[rows, idx] = torch.where(live, SC.index_select(1, self.hsel), cur)

    def _dq(self, with_dir, s_):
        """the plain iteration up to its curvature: d (but for the first step), q = M' d, d.(q + shift d)"""
        cg, D, Q, SC, n, dt, k = self.cg, self.D, self.Q, self.SC, self.n, self.dt, self.X.shape[0]
        if with_dir:
            _chk(self.lib.nft_cg_direction_batched(_P(D), _P(self.Rr), n, n, k, dt, _P(SC), s_))
        self.core.metric_flat_batch(D, Q, cg.W, 0.0)
        _chk(self.lib.nft_cg_curv_batched(_P(D), _P(Q), n, n, k, dt, cg.shift, _P(SC), _P(self.ws), s_))

    def body(self, with_dir, lazy=False):
        """one iteration's launches (graph-capturable)"""
        cg, lib, plan = self.cg, self.lib, self.plan
        X, Rr, D, Q, SC, n, dt = self.X, self.Rr, self.D, self.Q, self.SC, self.n, self.dt
        s_, k, NS = _native.stream_ptr(), X.shape[0], _native.CG_NSCALARS
        if with_dir and self.carried is not None:
            self.carried(X, Rr, D, Q, SC, self.lazy if lazy else None)
            if plan.xb == "dot":
                _chk(lib.nft_dot_batched(_P(X), _P(self.Bv), n, n, k, dt, _P(SC[:, _native.CG_XB:]), NS, _P(self.ws),
                                         s_))
            self.record()
            return
        if with_dir and plan.nq:
            # curvature from the data space: shift * d.d partials while d is
            # formed, (J d).W(J d) partials in the LOS forward reduce
            nbd, PQ, nq = self.nbd, self.PQ, plan.nq
            _chk(lib.nft_cg_direction_dd_batched(_P(D), _P(Rr), n, n, k, dt, _P(SC), cg.shift, _P(PQ), nbd + nq, s_))
            self.core.metric_flat_batch(D, Q, cg.W, 0.0, qpart=PQ[:, nbd:])
            _chk(lib.nft_fold_partials(_P(PQ), nbd + nq, k, _P(SC[:, _native.CG_CURV:]), NS, s_))
        else:
            self._dq(with_dir, s_)
        # the carried solve's first (direction-less) step runs this separate
        # update too: it streams b for x.b
        Bu = self.Bv if plan.xb == "dot" else self.Bu
        _chk(lib.nft_cg_update_batched(_P(X), _P(Rr), _P(D), _P(Q), _P(Bu), n, n, k, dt, cg.shift, _P(SC), _P(self.ws),
                                       s_))
        self.record()

    def refresh(self):
        """the nreset-th step: the plain iteration, then r = M x - b exactly"""
        lib, X, Rr, SC, n, dt, sh, ws = self.lib, self.X, self.Rr, self.SC, self.n, self.dt, self.cg.shift, self.ws
        sp, k = _native.stream_ptr(), X.shape[0]
        self._dq(not self.first, sp)
        self.first = False
        gp = SC[:, _native.CG_GAMMA].clone()
        _chk(lib.nft_cg_update_batched(_P(X), _P(Rr), _P(self.D), _P(self.Q), _P(self.Bu), n, n, k, dt, sh, _P(SC),
                                       _P(ws), sp))
        if self.AX is None:
            self.AX = torch.zeros_like(X)
        self.core.metric_flat_batch(X, self.AX, self.cg.W, 0.0)
        flag = SC[:, _native.CG_FLAG].clone()
        _chk(lib.nft_cg_residual_batched(_P(Rr), _P(self.AX), _P(X), _P(self.Bv), n, n, k, dt, sh, _P(SC), _P(ws), sp))
        live = SC[:, _native.CG_DONE] == 0.0
        SC[:, _native.CG_GPREV] = torch.where(live, gp, SC[:, _native.CG_GPREV])
        SC[:, _native.CG_FLAG] = torch.where(live, flag, SC[:, _native.CG_FLAG])
        self.record()
        self.ii = 0

    def step(self):
        """one iteration: eager, captured after GRAPH_AFTER eager ones, replayed, or the residual refresh"""
        cg = self.cg
        cg.niter += 1
        ConjugateGradient.iterations_total += len(self.active)
        self.ii += 1
        if self.ii >= cg.nreset:
            return self.refresh()
        first, self.first = self.first, False
        if not first and self.carried is not None:
            STATS["carry_iters"] += 1
        if first or not USE_GRAPHS or self.plan.eager_only or cg.niter <= GRAPH_AFTER or self.eager > 0:
            self.body(not first)
            self.eager = max(0, self.eager - 1)
        elif self.graph is not None:
            self.graph.replay()
        elif any(_worth_capturing(cg.controllers[j], cg.niter) for j in self.active):
            self.graph = _capture(lambda: self.body(True))
            self.graph.replay()
        else:
            self.body(True)

    def decide(self):
        """the per-step host read: guards, then each live controller's check"""
        cg, lay, X, Rr, Bv = self.cg, self.cg.layout, self.X, self.Rr, self.Bv
        self.host.copy_(self.SC, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        h = self.host.numpy()
        self.iter_seen = h[:, _native.CG_ITER].copy()
        # x.b of this step on the device: streamed by the update kernel, the
        # dot beside the carried iteration, or the residual refresh
        xb_dev = self.plan.xb != "demand" or self.ii == 0
        for j in list(self.active):
            ctl, p = cg.controllers[j], self.pos[j]
            hj = h[p]
            status = _guard_status(ctl, hj)
            if status is None:
                cache = {}

                def lazy(p=p, cache=cache, Xc=X, Rc=Rr):
                    if "v" not in cache:
                        xr_ = _frame(self.core, "from_frame", Xc[p:p + 1].double(), Rc[p:p + 1].double(), copy=True)
                        cache["v"] = (lay.unpack(xr_[0][0]), lay.unpack(xr_[1][0]))
                    return cache["v"]
                xr = float(hj[_native.CG_XR])
                value = 0.5 * (xr - float(hj[_native.CG_XB]))
                if not xb_dev and Bv is not None:
                    # x.b was not accumulated on the device: a dot, if the check reads the value
                    def value(p=p, xr=xr, Xc=X, Bc=Bv):
                        return 0.5 * (xr - float(torch.dot(Xc[p].double(), Bc[p].double())))
                state = _State(value, math.sqrt(float(hj[_native.CG_GAMMA])), lazy)
                sts = ctl.check(state)
                if callable(state._value):
                    # not read during the check: the buffers move on with the
                    # next iteration, so a later read would see another iterate
                    state._value = _stale
                if sts != ctl.CONTINUE:
                    status = sts
            if status is not None:
                self.finish(j, status)
                self.active.remove(j)

    def finish(self, j, status):
        self.results[j] = (status, True)
        self.SC[self.pos[j], _native.CG_DONE] = 1.0

    def chunk(self, m):
        """m queued iterations and one host read (FusedCGBatch._chunk); with the
        deferred iterate: ring slots from 0, x brought up to date before the read"""
        cg, lz, graph, flush = self.cg, self.lazy, self.graph, None
        if lz is not None:
            if self.lgraph is None:
                self.lgraph = _capture(lambda: self.body(True, lazy=True))
            graph = self.lgraph
            self.SC[:, _native.CG_LAZY] = 0.0

            def flush(m=m, lz=lz, X=self.X, D=self.D, n=self.n):
                g0 = lz["g0"]
                _native.cg_lazy_flush(X[0, g0:], D[0, g0:], lz["ring"], lz["sstride"], lz["alpha"], lz["nslot"], m,
                                      lz["ng"], n, X.shape[0])
        self.iter_seen = cg._chunk(graph, m, self.SC, self.host, self.iter_seen, self.active, self.finish, self.pos,
                                   self.HIST, flush)
        STATS["chunks"] += 1
        STATS["chunk_iters"] += m
        if self.carried is not None:
            STATS["carry_iters"] += m
        self.ii += m

    def advance(self):
        """up to the next host read -- a queued chunk while every live
        controller only counts, else one step -- and the compaction after it"""
        cg, active, m = self.cg, self.active, 0
        if self.plan.chunk and self.graph is not None and self.ii + 2 < cg.nreset:
            m = min(min(cg.controllers[j]._iteration_limit - cg.controllers[j]._itcount for j in active),
                    cg.nreset - 1 - self.ii)
        if m > 1:
            self.chunk(m)
        else:
            self.step()
            self.decide()
        if self.can_compact and _worth_compacting(cg.controllers, active, len(self.rows)):
            self.compact()

    def copy_back(self):
        """the compacted rows into the caller's buffers"""
        if self.X is not self.full_X:
            idx = torch.tensor(self.rows, device=self.core.device)
            self.full_X.index_copy_(0, idx, self.X)
            self.full_Rr.index_copy_(0, idx, self.Rr)

    def compact(self):
        """restrict the buffers, the scalars and the metric to the live RHS"""
        keep = sorted(self.pos[j] for j in self.active)
        self.copy_back()
        kt = torch.tensor(keep, device=self.core.device)
        self.X, self.Rr, self.D, self.SC = (t.index_select(0, kt) for t in (self.X, self.Rr, self.D, self.SC))
        if self.Bv is not None:
            self.Bv = self.Bv.index_select(0, kt)
        if self.HIST is not None:
            self.HIST = self.HIST.index_select(0, kt)
        self.host = torch.zeros((len(keep), _native.CG_NSCALARS), dtype=torch.float64).pin_memory()
        self.iter_seen = self.iter_seen[keep]
        self.rows = [self.rows[p] for p in keep]
        self.pos = {j: p for p, j in enumerate(self.rows)}
        sub = getattr(self.core, "subset", None)
        if sub is not None:
            # per-RHS metrics (NewtonCG directions): the live rows' metric
            self.core = sub(self.rows)
        self.setup(len(self.rows))
        # one eager iteration warms the new batch size's caches, then the
        # loop body is captured again
        self.graph = self.lgraph = None
        self.eager = 1
        self.cg.compactions += 1
        STATS["compactions"] += 1


class FusedCGBatch(FusedCG):
    """k independent conjugate-gradient solves with the same metric, run in
    lock step: every iteration is ONE batched matvec (the LOS matrix, the FFT
    passes and the amplitude kernels each launched once for all right-hand
    sides) and ONE set of batched CG kernels.  Each right-hand side keeps its
    own scalars, guards and controller (a deep copy of the caller's, started
    on its own energy, exactly as a sequential solve would); once it stops,
    sc[DONE] freezes it on the device.  Per right-hand side the arithmetic is
    bitwise that of FusedCG (and of solving the systems one after another)."""

    def __init__(self, core, W, shift, controllers, nreset=20):
        super().__init__(core, W, shift, controllers[0], nreset)
        self.controllers = controllers

    def run(self, energies):
        from .quadratic_energy import QuadraticEnergy
        lay, core, A = self.layout, self.core, energies[0].metric
        dt = torch.float32 if mixed_precision(core, self.W) else torch.float64
        X = torch.zeros((len(energies), lay.size), dtype=dt, device=core.device)
        Rr = torch.zeros_like(X)
        Bv = torch.zeros_like(X) if energies[0]._b is not None else None
        for j, e in enumerate(energies):
            lay.pack(e.position, out=X[j])
            lay.pack(e.gradient, out=Rr[j])
            if Bv is not None:
                lay.pack(e._b, out=Bv[j])
        # a core with a frame of its own (library/product.py) iterates in it
        _frame(core, "to_frame", X, Rr, Bv)
        X, status = self.run_packed(X, Rr, Bv, energies)
        X, Rr = _frame(core, "from_frame", X.double(), Rr.double())
        # (status, moved): moved is None for an energy returned as it came
        return [(e, st) if moved is None else (QuadraticEnergy(lay.unpack(X[j]), A, e._b, _grad=lay.unpack(Rr[j])), st)
                for j, (e, (st, moved)) in enumerate(zip(energies, status))]

    def run_packed(self, X, Rr, Bv, starts):
        """The batched loop on packed (k, n) buffers: X (iterates) and Rr
        (gradients A x - b) are updated in place, Bv is b (or None).
        `starts`: per RHS an energy-like object (value, gradient_norm) for the
        controller's start().  Returns (X, [(status, moved)]) -- moved is None
        for a RHS returned in its initial state.

        Once some right-hand sides have stopped, the live ones are compacted
        into smaller buffers (and a metric restricted to them, core.subset)
        when their controllers allow a few more iterations: the lock-step
        batch then stops paying matvecs for frozen rows.  Per RHS the
        arithmetic does not depend on the batch size (bitwise)."""
        results = [None] * X.shape[0]
        active = []
        for j, (e, ctl) in enumerate(zip(starts, self.controllers)):
            st = ctl.start(e)
            if st != ctl.CONTINUE:
                results[j] = (st, None)
            else:
                active.append(j)
        if not active:
            return X, results
        loop = _BatchLoop(self, X, Rr, Bv, active, results)
        try:
            if loop.start():
                while active:
                    loop.advance()
                loop.copy_back()
        finally:
            loop.graph = loop.lgraph = None
        return X, results

    def _chunk(self, graph, m, SC, host, iter_seen, active, finish, pos, HIST=None, flush=None):
        """m queued iterations (graph replays) and one host read.  A terminal
        step (guard tripped, gamma zero / negative / NaN) freezes its RHS on the
        device (NFT_CG_DONE = 2, with NFT_CG_AUTO set); _chunk_host maps the read."""
        SC[:, _native.CG_AUTO] = 1.0
        for _ in range(m):
            graph.replay()
        if flush is not None:
            flush()
        SC[:, _native.CG_AUTO] = 0.0
        self.niter += m
        host.copy_(SC, non_blocking=True)
        hh = HIST.cpu().numpy() if HIST is not None else None
        torch.cuda.current_stream().synchronize()
        h = host.numpy()
        for j, status in _chunk_host(h, hh, iter_seen, active, pos, self.controllers).items():
            finish(j, status)
            active.remove(j)
        return h[:, _native.CG_ITER].copy()


def _worth_compacting(controllers, active, k, min_left=3):
    """fewer live RHS than rows, and some live controller allows at least
    `min_left` more iterations (a compaction re-captures the loop body)"""
    def left(ctl):
        lim = getattr(ctl, "_iteration_limit", None)
        return lim is None or lim - getattr(ctl, "_itcount", 0) >= min_left
    return len(active) < k and any(left(controllers[j]) for j in active)
