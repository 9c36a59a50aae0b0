"""A right-hand side that freezes inside a queued chunk of the batched CG
(fused_cg.FusedCGBatch): the device sets NFT_CG_DONE = 2 on the tripping
step, the steps queued behind it leave the row alone, and the host maps the
frozen row to its controller's status with exactly the checks a one-step
loop would have made.

The trip is injected: between two graph replays of a chunk the device
scalars of one row are overwritten (a stream-ordered write, so every kernel
of the next step sees it).  NIFTy's ConjugateGradient.__call__ then returns
ERROR from the next iteration without moving x (alpha < 0, alpha NaN,
curvature NaN or zero), so the frozen row must be bitwise the solve of that
right-hand side alone stopped one iteration earlier, and the other rows
bitwise the batch without injection.
"""
import gc

import numpy as np
import pytest
import torch

from test_compact_gpu import _energies, _metric

pytestmark = pytest.mark.gpu

K, ROW, LIMIT = 4, 2, 30
NAN, INF = float("nan"), float("inf")
# injected GAMMA, and whether the row's residual is zeroed with it
SCENARIOS = {"alpha<0": (-1.0, False), "alpha NaN": (NAN, False), "gamma inf": (INF, False),
             "d=0 curv=0": (0.0, True)}
# (chunk number, replays before the write): strictly inside the first chunk,
# and inside the second one, which follows the residual refresh at nreset
PLACES = {"first": (0, 3), "second": (1, 3)}

# switches (fused_cg module attributes), NFT_PRO_R2C, fp32 storage, cg.path
FLAVOURS = {
    "plain": (dict(CURV_DATA=False), None, False, "plain+chunk"),
    "quad": (dict(_CARRY=False), None, False, "quad+chunk"),
    "carry-seg": (dict(_AMP2=False), None, False, "carry+chunk"),
    "carry-amp2": (dict(LAZY=False), None, False, "carry+chunk"),
    "lazy-rows": (dict(LAZY=True), "0", False, "carry+chunk"),
    "lazy": (dict(LAZY=True), None, False, "carry+chunk"),
    "lazy-fp32": (dict(LAZY=True), None, True, "carry+chunk"),
}


@pytest.fixture(scope="module")
def ift(dev):
    import nifty_amd
    return nifty_amd


@pytest.fixture(scope="module")
def problems(ift):
    out = {}
    for which in ("los", "gauss"):
        cf, A, spec = _metric(ift, which)
        out[which] = (cf, A, spec, _energies(ift, cf, A, K, 12))
    return out


class _Proxy:
    """stands in for the chunk's graph: replay() is the real one, and after
    the `after`-th replay the scalars of buffer row p are overwritten.  A
    plain instance (no class or closure made per chunk): it holds the HIP
    graph and must let go of it when _chunk returns -- garbage that only the
    cyclic collector frees could take the graph down inside a later capture."""

    def __init__(self, graph, after, SC, p, gamma, Rr):
        self.graph, self.after, self.SC, self.p, self.gamma, self.Rr = graph, after, SC, p, gamma, Rr
        self.count = 0

    def replay(self):
        from nifty_amd import _native
        self.graph.replay()
        self.count += 1
        if self.count == self.after:
            self.SC[self.p, _native.CG_GAMMA] = self.gamma
            if self.Rr is not None:
                self.Rr[self.p].zero_()


class _Injector:
    """wraps FusedCGBatch._chunk / run_packed: after `after` replays of chunk
    number `chunk`, GAMMA of row `row` := gamma (and its residual := 0)"""

    def __init__(self, monkeypatch, fused_cg, chunk, after, row, gamma, zero_r):
        self.hit = None
        self.nchunk = 0
        inj = self
        orig_chunk = fused_cg.FusedCGBatch._chunk
        orig_rp = fused_cg.FusedCGBatch.run_packed

        def run_packed(cg, X, Rr, Bv, starts):
            inj.Rr = Rr
            return orig_rp(cg, X, Rr, Bv, starts)

        def _chunk(cg, graph, m, SC, host, iter_seen, active, finish, pos, HIST=None, flush=None):
            c = inj.nchunk
            inj.nchunk += 1
            if c != chunk:
                return orig_chunk(cg, graph, m, SC, host, iter_seen, active, finish, pos, HIST, flush)
            # equal limits: nothing stopped, so nothing was compacted before
            assert cg.compactions == 0 and SC.shape[0] == inj.Rr.shape[0]
            p_ = pos[row]
            before = int(round(float(iter_seen[p_])))
            proxy = _Proxy(graph, after, SC, p_, gamma, inj.Rr if zero_r else None)
            out = orig_chunk(cg, proxy, m, SC, host, iter_seen, active, finish, pos, HIST, flush)
            del proxy
            inj.hit = dict(m=m, before=before, p=int(round(float(out[p_]))) - before, T=before + after,
                           sc=host.numpy()[p_].copy())
            return out
        monkeypatch.setattr(fused_cg.FusedCGBatch, "_chunk", _chunk)
        monkeypatch.setattr(fused_cg.FusedCGBatch, "run_packed", run_packed)


def _same_position(cf, e1, e2):
    for key in cf.domain.keys():
        a, b = e1.position[key].val.contiguous(), e2.position[key].val.contiguous()
        if not torch.equal(a.view(torch.int64), b.view(torch.int64)):
            return False
    return True


def _batch(ift, fused_cg, spec, es, limit=LIMIT):
    core, W, shift = spec
    cg = fused_cg.FusedCGBatch(core, W, shift, [ift.GradientNormController(iteration_limit=limit) for _ in es])
    return cg, cg.run(es)


@pytest.mark.parametrize("flavour", list(FLAVOURS))
@pytest.mark.parametrize("which", ["los", "gauss"])
def test_freeze_inside_chunk(ift, problems, which, flavour, monkeypatch):
    from nifty_amd import _native, config
    from nifty_amd.minimization import fused_cg
    # this test captures a few dozen graphs: whatever cyclic garbage earlier
    # tests left (it may hold HIP graphs) goes now, not inside a capture
    gc.collect()
    switches, r2c, fp32, path = FLAVOURS[flavour]
    cf, A, spec, es = problems[which]
    for name, val in switches.items():
        monkeypatch.setattr(fused_cg, name, val)
    if r2c is None:
        monkeypatch.delenv("NFT_PRO_R2C", raising=False)
    else:
        monkeypatch.setenv("NFT_PRO_R2C", r2c)
    lazy = switches.get("LAZY", False)
    flushes = []
    orig_flush = _native.cg_lazy_flush

    def spy(*a, **kw):
        flushes.append(a[6])
        return orig_flush(*a, **kw)
    monkeypatch.setattr(_native, "cg_lazy_flush", spy)
    if fp32:
        config.set_cg_precision("fp32")
    try:
        cg, base = _batch(ift, fused_cg, spec, es)
        assert cg.path == path, cg.path
        assert bool(flushes) == lazy
        assert all(s == cg.controllers[0].CONVERGED for _, s in base)
        solo = {}
        for place, (chunk, after) in PLACES.items():
            for scen, (gamma, zero_r) in SCENARIOS.items():
                what = (which, flavour, place, scen)
                runs = {}
                for on in ((True, False) if lazy else (lazy,)):
                    with monkeypatch.context() as mp:
                        mp.setattr(fused_cg, "LAZY", on)
                        inj = _Injector(mp, fused_cg, chunk, after, ROW, gamma, zero_r)
                        flushes.clear()
                        cg, res = _batch(ift, fused_cg, spec, es)
                    assert cg.path == path and bool(flushes) == on, what
                    runs[on] = res
                    hit = inj.hit
                    assert hit is not None, (what, "the chunk never ran")
                    # the trip falls strictly inside the chunk, on the step after the write
                    assert 1 < hit["p"] < hit["m"], (what, hit)
                    assert hit["p"] == after + 1, (what, hit)
                    assert (hit["before"] < cg.nreset) if place == "first" else (hit["before"] == cg.nreset), hit
                    assert hit["sc"][_native.CG_DONE] == 2.0 and hit["sc"][_native.CG_FLAG] == 1.0, (what, hit)
                    T = hit["T"]
                    ctl = cg.controllers[ROW]
                    assert res[ROW][1] == ctl.ERROR, what
                    assert ctl._itcount == T, (what, ctl._itcount, T)
                    for j in range(K):
                        if j != ROW:
                            assert res[j][1] == base[j][1], what
                            assert cg.controllers[j]._itcount == LIMIT
                            assert _same_position(cf, res[j][0], base[j][0]), (what, "live row", j)
                    if T not in solo:
                        core, W, shift = spec
                        solo[T] = fused_cg.FusedCG(core, W, shift, ift.GradientNormController(iteration_limit=T)
                                                   ).run(es[ROW])[0]
                    assert _same_position(cf, res[ROW][0], solo[T]), (what, "frozen row != solo solve of", T)
                    if place == "first":
                        # later chunks follow: the frozen row is dropped, its result copied back
                        assert cg.compactions >= 1, what
                if lazy:
                    for j in range(K):
                        assert runs[True][j][1] == runs[False][j][1], what
                        assert _same_position(cf, runs[True][j][0], runs[False][j][0]), (what, "lazy != eager", j)
    finally:
        if fp32:
            config.set_cg_precision("fp64")


class _NoGraph:
    """a graph whose replay does nothing but note NFT_CG_AUTO of row 0"""

    def __init__(self, SC):
        self.SC, self.auto = SC, []

    def replay(self):
        from nifty_amd import _native
        self.auto.append(float(self.SC[0, _native.CG_AUTO]))


def test_chunk_host_mapping(ift, problems):
    """_chunk's reading of the post-chunk scalars: DONE = 2 rows by FLAG and
    GAMMA, a row frozen after p steps with p - 1 controller checks, a live
    row with m"""
    from nifty_amd import _native as N
    from nifty_amd.minimization import fused_cg
    cf, A, (core, W, shift), es = problems["los"]
    m, seen = 6, 7
    # (steps in the chunk, scalars, status)
    rows = [(3, {N.CG_DONE: 2.0, N.CG_FLAG: 1.0, N.CG_CURV: 0.0, N.CG_GAMMA: 1.5}, "ERROR"),
            (2, {N.CG_DONE: 2.0, N.CG_GAMMA: 0.0}, "CONVERGED"),
            (5, {N.CG_DONE: 2.0, N.CG_GAMMA: -2.0}, "ERROR"),
            (1, {N.CG_DONE: 2.0, N.CG_GAMMA: NAN}, "ERROR"),
            (m, {N.CG_GAMMA: 0.25}, None),
            (4, {N.CG_DONE: 2.0, N.CG_FLAG: 1.0, N.CG_CURV: NAN, N.CG_GAMMA: 1.5}, "ERROR")]
    k = len(rows)
    ctls = [ift.GradientNormController(iteration_limit=100) for _ in range(k)]
    for c in ctls:
        assert c.start(fused_cg._COUNT_ONLY_STATE) == c.CONTINUE
        for _ in range(seen):
            c.check(fused_cg._COUNT_ONLY_STATE)
    cg = fused_cg.FusedCGBatch(core, W, shift, ctls)
    sc = np.zeros((k, N.CG_NSCALARS))
    for j, (p, vals, _) in enumerate(rows):
        sc[j, N.CG_ITER] = seen + p
        for idx, v in vals.items():
            sc[j, idx] = v
    SC = torch.from_numpy(sc).to(core.device)
    host = torch.zeros((k, N.CG_NSCALARS), dtype=torch.float64).pin_memory()
    done = {}
    graph = _NoGraph(SC)
    active = list(range(k))
    out = cg._chunk(graph, m, SC, host, np.full(k, float(seen)), active, done.__setitem__,
                    {j: j for j in range(k)})
    assert graph.auto == [1.0] * m, "AUTO is set while the steps are queued"
    assert float(SC[:, N.CG_AUTO].abs().max()) == 0.0
    assert np.array_equal(out, sc[:, N.CG_ITER])
    for j, (p, _, status) in enumerate(rows):
        c = ctls[j]
        if status is None:
            assert j in active and j not in done
            assert c._itcount == seen + m
        else:
            assert j not in active and done[j] == getattr(c, status), (j, done.get(j))
            assert c._itcount == seen + p - 1, (j, c._itcount)
