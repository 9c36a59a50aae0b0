"""CPU: the host-side decisions of the batched CG driver (minimization/
fused_cg.py) -- which iteration a solve runs (plan_iteration), the terminal
guards on a step's scalars (_guard_status) and the host's reading of a queued
chunk (_chunk_host).  Stub cores carry only the capability attributes the
plan reads; nothing here touches a device."""
import logging

import numpy as np
import pytest
import torch

from test_cg_freeze_gpu import FLAVOURS

NAN = float("nan")
F64, F32 = torch.float64, torch.float32
RING = 1 << 20


class _Core:
    """a core with every capability of the CF model (correlated_fields_simple)"""
    supports_quad = True
    supports_fp32 = True

    def __init__(self, cg=16, amp2=7, dirb=33, lazy=True):
        self._cg, self._amp2, self._dir, self._lazy = cg, amp2, dirb, lazy

    def cg_blocks(self, k):
        return self._cg

    def amp2_tiles(self, k):
        return self._amp2

    def dir_blocks(self, k):
        return self._dir

    def lazy_ok(self, k):
        return self._lazy

    def phases_fp32(self, k):
        return self._amp2 > 0

    def pointwise_quad_blocks(self, W):
        return self._cg


class _MetricCoreShape:
    """geovi_batch._MetricCore: no supports_quad, no carried iteration"""


class _W:
    quad_blocks = 10

    def __call__(self, *a):
        raise AssertionError("the plan applies no operator")


@pytest.fixture()
def fcg(monkeypatch):
    """the module with every switch at its default, whatever the environment"""
    from nifty_amd.minimization import fused_cg
    for name in ("CURV_DATA", "_CARRY", "_CARRY_DIR", "_AMP2", "LAZY", "CHUNK"):
        monkeypatch.setattr(fused_cg, name, True)
    monkeypatch.setattr(fused_cg, "CURV_DATA_VALUE", False)
    return fused_cg


def _silent(ift_limit=30):
    from nifty_amd import GradientNormController
    return GradientNormController(iteration_limit=ift_limit)


def _plan(fcg, core=None, W=..., dtype=F64, ctls=None, k=4, has_b=False, tracing=False, ring=RING,
          free=1 << 40):
    return fcg.plan_iteration(_Core() if core is None else core, _W() if W is ... else W, dtype,
                              [_silent()] if ctls is None else ctls, k, has_b, tracing, ring, free)


def test_plan_table(fcg):
    from nifty_amd import AbsDeltaEnergyController, GradientNormController
    P = fcg.IterationPlan
    full = P(kind="carry", nq=10, flavour="amp2", chunk=True, lazy=True, need_value=False, eager_only=False,
             xb="demand", path="carry+chunk")
    assert _plan(fcg) == full
    assert _plan(fcg, has_b=True) == full
    # the ring may take half the free memory, no more; the reading is asked
    # for only here, where everything else allows the ring
    assert _plan(fcg, free=2 * RING) == full
    assert _plan(fcg, free=2 * RING - 1) == full._replace(lazy=False)
    assert _plan(fcg, free=lambda: 2 * RING - 1) == full._replace(lazy=False)

    def never():
        raise AssertionError("free memory read without a ring to place")
    assert _plan(fcg, core=_Core(lazy=False), free=never) == full._replace(lazy=False)
    # a decision trace reads values (recorded beside the same iteration)
    assert _plan(fcg, tracing=True, has_b=True, free=never) == full._replace(lazy=False, need_value=True, xb="dot")
    assert _plan(fcg, tracing=True, free=never) == full._replace(lazy=False, need_value=True)
    # count-only, but its log line reads the energy
    named = GradientNormController(iteration_limit=30, name="cg")
    assert _plan(fcg, ctls=[named], has_b=True, free=never) == P(
        "carry", 10, "amp2", False, False, True, True, "dot", "carry")
    # one value-driven controller in the batch decides for all
    assert _plan(fcg, ctls=[_silent(), AbsDeltaEnergyController(0.1, iteration_limit=30)], has_b=True,
                 free=never) == P("plain", 0, None, False, False, True, True, "update", "plain")
    assert _plan(fcg, ctls=[AbsDeltaEnergyController(0.1, iteration_limit=30)]).xb == "demand"
    # ... unless only the silent ones are still iterating when the solve starts
    mixed = [_silent(), named]
    assert not _plan(fcg, ctls=mixed).chunk
    assert fcg.plan_iteration(_Core(), _W(), F64, mixed, 4, False, False, RING, never, live=mixed[:1]).path == \
        "carry+chunk"
    # without the two-phase amplitude kernels: fp64 segment passes, no fp32 carry
    seg = full._replace(flavour="seg", lazy=False)
    assert _plan(fcg, core=_Core(amp2=0), free=never) == seg
    assert _plan(fcg, core=_Core(dirb=0), free=never) == seg
    assert _plan(fcg, core=_Core(amp2=0), dtype=F32, free=never) == P(
        "plain", 0, None, True, False, False, False, "demand", "plain+chunk")
    assert _plan(fcg, dtype=F32) == full
    assert _plan(fcg, core=_Core(dirb=0), dtype=F32, free=never) == full._replace(kind="quad", flavour=None,
                                                                                 lazy=False, path="quad+chunk")
    assert _plan(fcg, dtype=torch.float16).kind == "plain"
    # no CG-carrying epilogue at this grid
    assert _plan(fcg, core=_Core(cg=0), free=never) == full._replace(kind="quad", flavour=None, lazy=False,
                                                                    path="quad+chunk")
    # W: a pointwise weight takes the core's count, anything else none
    assert _plan(fcg, W=torch.ones(3)).nq == 16
    assert _plan(fcg, W=None).path == "plain+chunk"
    assert _plan(fcg, core=_MetricCoreShape(), W=None, has_b=True) == P(
        "plain", 0, None, True, False, False, False, "demand", "plain+chunk")


def test_plan_helpers_agree(fcg):
    """the names bench.py and the tests use answer from the same decisions"""
    core, W = _Core(), _W()
    assert fcg._quad_blocks(core, W, F64) == 10                     # no controllers: all count-only
    assert fcg._quad_blocks(core, W, F64, (_silent(),)) == 10
    assert fcg._quad_blocks(_Core(amp2=0), W, F32) == 0
    assert fcg._CarryIteration.supported(core, 4) and fcg._CarryIteration.supported(core, 4, F32)
    assert fcg._CarryIteration.supported(_Core(amp2=0), 4) and not fcg._CarryIteration.supported(_Core(amp2=0), 4, F32)
    assert not fcg._CarryIteration.supported(_Core(cg=0), 4)
    assert not fcg._CarryIteration.supported(_MetricCoreShape(), 4)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
def test_plan_follows_switches(fcg, flavour, monkeypatch):
    """each switch of test_cg_freeze_gpu.FLAVOURS, read at solve time"""
    switches, _, fp32, path = FLAVOURS[flavour]
    for name, val in switches.items():
        monkeypatch.setattr(fcg, name, val)
    plan = _plan(fcg, dtype=F32 if fp32 else F64)
    assert plan.path == path
    assert plan.flavour == (None if flavour in ("plain", "quad") else "seg" if flavour == "carry-seg" else "amp2")
    assert plan.nq == (0 if flavour == "plain" else 10)
    assert plan.lazy == switches.get("LAZY", False)


def test_plan_other_switches(fcg, monkeypatch):
    from nifty_amd import AbsDeltaEnergyController
    value = [AbsDeltaEnergyController(0.1, iteration_limit=30)]
    with monkeypatch.context() as mp:
        mp.setattr(fcg, "CHUNK", False)
        p = _plan(fcg)
        assert (p.path, p.chunk, p.lazy) == ("carry", False, False)
    with monkeypatch.context() as mp:
        mp.setattr(fcg, "_CARRY_DIR", False)
        assert _plan(fcg).flavour == "seg"
    with monkeypatch.context() as mp:
        mp.setattr(fcg, "CURV_DATA_VALUE", True)
        p = _plan(fcg, ctls=value, has_b=True)
        assert (p.kind, p.xb, p.eager_only, p.chunk) == ("carry", "dot", True, False)
    assert _plan(fcg, ctls=value, has_b=True).kind == "plain"


class _Log(logging.Handler):
    def __init__(self):
        super().__init__(logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append(record.getMessage())


@pytest.fixture()
def log():
    from nifty_amd.logger import logger
    h = _Log()
    logger.addHandler(h)
    yield h.lines
    logger.removeHandler(h)


def _row(**kw):
    from nifty_amd import _native as N
    r = np.zeros(N.CG_NSCALARS)
    for name, v in kw.items():
        r[getattr(N, "CG_" + name)] = v
    return r


def test_guard_status(fcg, log):
    c = _silent()
    cases = [(dict(FLAG=1.0, CURV=NAN, GAMMA=1.0), c.ERROR, "Error: ConjugateGradient: curv==NaN"),
             (dict(FLAG=1.0, CURV=0.0, GAMMA=1.0), c.ERROR, "Error: ConjugateGradient: curv==0."),
             (dict(FLAG=1.0, CURV=-3.0, GAMMA=1.0), c.ERROR, "Error: ConjugateGradient: alpha<0."),
             (dict(FLAG=1.0, CURV=2.0, GAMMA=NAN), c.ERROR, "Error: ConjugateGradient: alpha<0."),
             (dict(CURV=2.0, GAMMA=NAN), c.ERROR, "Error: ConjugateGradient: gamma==NaN"),
             (dict(CURV=2.0, GAMMA=-1e-30), c.ERROR, "Positive definiteness of preconditioner violated!"),
             (dict(CURV=2.0, GAMMA=0.0), c.CONVERGED, None),
             (dict(CURV=2.0, GAMMA=1e-300), None, None)]
    for kw, status, line in cases:
        del log[:]
        assert fcg._guard_status(c, _row(**kw)) == status, kw
        assert log == ([] if line is None else [line]), kw


def test_chunk_host_mapping(fcg, log):
    """the scalar rows of test_cg_freeze_gpu.test_chunk_host_mapping: DONE = 2
    rows by FLAG and GAMMA, a row frozen after p steps with p - 1 controller
    checks, a live row with m"""
    from nifty_amd import ConjugateGradient
    m, seen = 6, 7
    rows = [(3, dict(DONE=2.0, FLAG=1.0, CURV=0.0, GAMMA=1.5), "ERROR"),
            (2, dict(DONE=2.0, GAMMA=0.0), "CONVERGED"),
            (5, dict(DONE=2.0, GAMMA=-2.0), "ERROR"),
            (1, dict(DONE=2.0, GAMMA=NAN), "ERROR"),
            (m, dict(GAMMA=0.25), None),
            (4, dict(DONE=2.0, FLAG=1.0, CURV=NAN, GAMMA=1.5), "ERROR")]
    k = len(rows)
    ctls = [_silent(100) for _ in range(k)]
    for c in ctls:
        assert c.start(fcg._COUNT_ONLY_STATE) == c.CONTINUE
        for _ in range(seen):
            c.check(fcg._COUNT_ONLY_STATE)
    # buffer positions differ from the RHS indices (as after a compaction)
    pos = {j: k - 1 - j for j in range(k)}
    h = np.stack([_row(ITER=seen + p, **vals) for p, vals, _ in reversed(rows)])
    active = list(range(k))
    total = ConjugateGradient.iterations_total
    stopped = fcg._chunk_host(h, None, np.full(k, float(seen)), active, pos, ctls)
    assert ConjugateGradient.iterations_total - total == sum(p for p, _, _ in rows)
    assert active == list(range(k)), "the caller removes what stopped"
    assert [j for j in active if j not in stopped] == [4]
    for j, (p, _, status) in enumerate(rows):
        c = ctls[j]
        if status is None:
            assert c._itcount == seen + m
        else:
            assert stopped[j] == getattr(c, status), (j, stopped[j])
            assert c._itcount == seen + p - 1, (j, c._itcount)
    assert log == ["Error: ConjugateGradient: curv==0.", "Positive definiteness of preconditioner violated!",
                   "Error: ConjugateGradient: gamma==NaN", "Error: ConjugateGradient: curv==NaN"]


def test_chunk_host_limit_and_trace(fcg):
    """a controller whose limit ends the chunk stops on its last check; with a
    decision trace the checks see each step's recorded scalars; a stop before
    the last queued step is an error"""
    from nifty_amd import GradientNormController
    seen, p, nh = 18, 3, 21
    hist = np.zeros((1, nh, 3))
    for t in range(1, p + 1):
        hist[0, (seen + t) % nh] = (4.0 * t, 1.0, 0.5 + t)
    h = _row(ITER=seen + p, GAMMA=12.0)[None]

    class Spy(GradientNormController):
        seen_states = []

        def check(self, energy):
            if energy is not fcg._COUNT_ONLY_STATE:
                self.seen_states.append((energy.value, energy.gradient_norm))
            return super().check(energy)

    def started(limit):
        c = Spy(iteration_limit=limit)
        c.start(fcg._COUNT_ONLY_STATE)
        for _ in range(seen):
            c.check(fcg._COUNT_ONLY_STATE)
        return c
    c = started(seen + p)
    assert fcg._chunk_host(h, hist, np.array([float(seen)]), [0], {0: 0}, [c]) == {0: c.CONVERGED}
    assert Spy.seen_states == [(0.5 * (1.0 - (0.5 + t)), np.sqrt(4.0 * t)) for t in range(1, p + 1)]
    c = started(seen + p - 1)
    with pytest.raises(RuntimeError, match="stopped inside a queued chunk"):
        fcg._chunk_host(h, None, np.array([float(seen)]), [0], {0: 0}, [c])
    with pytest.raises(RuntimeError, match="count-only controller read energy.value"):
        fcg._COUNT_ONLY_STATE.value


def test_driver_shape():
    """the loop stays readable: no rebinding closures, short functions"""
    import ast
    import inspect
    from nifty_amd.minimization import fused_cg
    src = inspect.getsource(fused_cg)
    tree = ast.parse(src)
    assert not [n for n in ast.walk(tree) if isinstance(n, ast.Nonlocal)]
    sizes = {n.name: n.end_lineno - n.lineno + 1 for n in ast.walk(tree)
             if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef))}
    assert sizes["run_packed"] <= 60, sizes["run_packed"]
    assert max(sizes.values()) <= 100, max(sizes, key=sizes.get)
    assert len(src.splitlines()) <= 934
