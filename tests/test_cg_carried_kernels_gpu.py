"""The replicas of the device CG state machine inside the fused transforms
(nft_hartley_fused with cg_* / dir_* / lazy_* set) against the plain
reference of tests/test_cg_primitives_gpu.py: the CG-carrying epilogue of the
adjoint transform, the direction-carrying folded prologue of the forward
one, and the deferred iterate (ring slots + nft_cg_lazy_flush) driven by
hand at kernel level.  Plus the argument checks of the carried fold.

Bounds: the element-wise and reduction forms derived in
test_cg_primitives_gpu.py.  r of the CG epilogue takes q = epi_a * h from
the transform itself, so it is held normwise with the transform tolerance
of tests/test_transforms_gpu.py (1e-13 fp64, 2e-6 fp32) on top.  The serial
chain L of a partial: an epilogue tile holds (elements per item) / tiles
values shared by at least one wave (``_chain``); a prologue block sums the
2^(d-1) mirror rows of its group one after the other, each strided over by
at least 64 threads (``_dir_chain``; the prologue fused with the R2C pass:
N / 8 threads, 8 positions of each of 2 rows, the same figure).
"""
import ctypes

import numpy as np
import pytest
import torch

import test_cg_primitives_gpu as prim
from test_cg_primitives_gpu import (ALPHA, AUTO, CURV, DONE, GAMMA, GPREV, GUARD_ROWS, ITER, LAZY, LD, NS, SENT,
                                    SHIFT, U, XB, XR, L, _bits, _draw, _same, assert_reduction, check_update_row,
                                    guard_expect, guard_scalars, nat)  # noqa: F401

pytestmark = pytest.mark.gpu

TOLH = {0: 1e-13, 1: 2e-6}
TT = {0: torch.float64, 1: torch.float32}
K = 8
GEOS = [((K, 64, 64), 0), ((K, 1024, 16), 0), ((K, 16, 16, 16), 0), ((K, 64, 64), 1)]
OFF, PAD = 5, 37


def _grid_rows(rng, k, N, dt):
    """(k, OFF + N + PAD) rows: the grid segment at OFF, sentinels around it"""
    a = np.full((k, OFF + N + PAD), SENT, prim.NP[dt])
    a[:, OFF:OFF + N] = _draw(rng, (k, N), dt)
    return a


def _chain(N, blocks):
    return -(-N // (blocks * 64))


def _dir_chain(grid):
    return 2 ** (len(grid) - 1) * -(-grid[-1] // 64)


MORE_ROWS = [("live", {}), GUARD_ROWS[8], GUARD_ROWS[9], GUARD_ROWS[10], ("live AUTO=1", dict(AUTO=1.0)),
             ("live", {}), ("live", {}), ("live", {})]


@pytest.mark.parametrize("shape,dt", GEOS)
@pytest.mark.parametrize("rows", [GUARD_ROWS[:8], MORE_ROWS], ids=["guards", "live"])
def test_cg_epilogue(L, shape, dt, rows):
    """cg=dict(...): x', r' and the tiles' partials of the adjoint's last pass
    against the reference update with q = epi_a * h"""
    nat_ = L.nat
    k, grid = shape[0], shape[1:]
    axes = tuple(range(1, len(shape)))
    N = int(np.prod(grid))
    tiles = nat_.hartley_cg_blocks(shape, axes, TT[dt])
    assert tiles > 0
    rng = np.random.default_rng(11 + N + dt)
    stride = OFF + N + PAD
    X, R, D = (_grid_rows(rng, k, N, dt) for _ in range(3))
    G = _draw(rng, shape, dt)
    A, Bw = (_draw(rng, grid, dt) for _ in range(2))
    SC = guard_scalars(rng, rows)
    scale = 1.0 / np.sqrt(N)
    blk0, nbtot = 2, tiles + 5
    x, r, d, g, a, bw, sc = (L.up(v) for v in (X, R, D, G, A, Bw, SC))
    part = torch.full((k, 3, nbtot), SENT, dtype=torch.float64, device=L.dev)
    out = torch.full((k, N + 3), SENT, dtype=TT[dt], device=L.dev)
    w2 = torch.full((k, N), SENT, dtype=TT[dt], device=L.dev)
    bt = dict(period=N, out=N + 3, out2=N)
    nat_.hartley_fused(out[0], axes, scale, x=g, epi=dict(a=a, b=bw, out2=w2), shape=shape, batch=bt,
                       cg=dict(x=x[0, OFF:], r=r[0, OFF:], d=d[0, OFF:], sc=sc, part=part, stride=stride, shift=SHIFT,
                               nbtot=nbtot, blk0=blk0))
    x1, r1, p1 = L.down(x), L.down(r), L.down(part)
    assert np.all(L.down(out) == SENT), "out is written although the CG epilogue replaces it"
    assert _same(L.down(sc), SC) and _same(L.down(d), D)
    # the un-carried call: out = a * h, out2 = b * h (the same transform)
    o0 = torch.full((k, N + 3), SENT, dtype=TT[dt], device=L.dev)
    w0 = torch.full((k, N), SENT, dtype=TT[dt], device=L.dev)
    nat_.hartley_fused(o0[0], axes, scale, x=g, epi=dict(a=a, b=bw, out2=w0), shape=shape, batch=bt)
    assert _same(L.down(w2), L.down(w0)), "out2 differs from the un-carried call"
    h = L.down(nat_.hartley(g, axes, scale=scale)).reshape(k, N)
    slots = np.ones(nbtot, bool)
    slots[blk0:blk0 + tiles] = False
    assert np.all(p1[:, :, slots] == SENT), "partial slots outside the tile range written"
    assert np.all(p1[:, 2, ~slots] == 0.0), "x.b partials of the epilogue are 0"
    part[:, :, torch.from_numpy(slots).to(L.dev)] = 0.0
    assert L.lib.nft_cg_finalize_batched(L.P(part), nbtot, k, L.P(sc), L.s()) == prim.OK
    sc1 = L.down(sc)
    u = U[dt]
    seg = slice(OFF, OFF + N)
    for j, (name, _) in enumerate(rows):
        what = f"{shape} {name}"
        assert _same(x1[j, :OFF], X[j, :OFF]) and _same(x1[j, OFF + N:], X[j, OFF + N:]), (what, "x padding")
        assert _same(r1[j, :OFF], R[j, :OFF]) and _same(r1[j, OFF + N:], R[j, OFF + N:]), (what, "r padding")
        applies = SC[j, DONE] == 0.0 and prim._guard_ok(SC[j])
        guard_expect(name.replace("live AUTO=1", "live"), SC[j], sc1[j])
        if not applies:
            assert _same(x1[j], X[j]) and _same(r1[j], R[j]), (what, "x or r moved")
            if SC[j, DONE] != 0.0:
                assert _same(sc1[j], SC[j]), what
            continue
        q = A.reshape(-1).astype(LD) * h[j].astype(LD)
        xn, rn, mx, mr = prim._ref_update(X[j, seg], R[j, seg], D[j, seg], q, SHIFT, SC[j])
        al = abs(float(prim._alpha64(SC[j])))
        ex = np.abs(x1[j, seg].astype(LD) - xn)
        assert np.all(ex <= 4 * u * mx), (what, "x", float(np.max(ex / mx)) / u)
        er = float(np.sqrt(np.sum((r1[j, seg].astype(LD) - rn) ** 2)))
        bound = (4 * u * float(np.sqrt(np.sum(mr ** 2)))
                 + al * float(np.max(np.abs(A))) * TOLH[dt] * float(np.sqrt(np.sum(h[j].astype(LD) ** 2))))
        assert er <= bound, (what, "r", er, bound)
        Lc = _chain(N, tiles)
        assert_reduction(sc1[j, GAMMA], r1[j, seg], r1[j, seg], Lc, what + " GAMMA")
        assert_reduction(sc1[j, XR], x1[j, seg], r1[j, seg], Lc, what + " XR")
        assert sc1[j, XB] == 0.0
        assert sc1[j, GPREV] == SC[j, GAMMA] and sc1[j, ITER] == SC[j, ITER] + 1


def _folded_prologue(L, shape, dt, rng):
    """operands of the folded batched prologue (tests/test_transforms_gpu.py:
    test_hartley_fused_folded_prologue): |k| bins of the harmonic grid"""
    from nifty_amd.operators.distributors import BinIndex
    k, grid = shape[0], shape[1:]
    kk = np.zeros(grid)
    for ax, n in enumerate(grid):
        f = np.fft.fftfreq(n) * n
        kk = kk + (f.reshape([-1 if a_ == ax else 1 for a_ in range(len(grid))]) * (1. + 0.1 * ax)) ** 2
    uq, pidx = np.unique(np.sqrt(kk), return_inverse=True)
    pidx = pidx.reshape(grid)
    bi = BinIndex(pidx, uq.size, L.dev, fold=True)
    assert bi.fold is not None
    a, b = (L.up(_draw(rng, grid, dt)) for _ in range(2))
    c = L.up(_draw(rng, (uq.size, k), dt))
    return dict(a=a, b=b, c=c, index=bi.fold["pindex"], fold=True)


@pytest.mark.parametrize("shape,dt", GEOS)
def test_direction_prologue(L, shape, dt):
    """pro["dir"]: d = max(0, gamma / gprev) d + r inside the folded prologue,
    its shift * d.d partials, and the transform of the updated d"""
    nat_ = L.nat
    k, grid = shape[0], shape[1:]
    axes = tuple(range(1, len(shape)))
    N = int(np.prod(grid))
    nbd = nat_.hartley_dir_blocks(grid)
    assert nbd > 0
    rng = np.random.default_rng(23 + N + dt)
    stride = OFF + N + PAD
    D, R = (_grid_rows(rng, k, N, dt) for _ in range(2))
    SC = prim._dir_scalars(rng, k)
    pro = _folded_prologue(L, shape, dt, rng)
    d, r, sc = L.up(D), L.up(R), L.up(SC)
    blk0, pstride = 3, nbd + 7
    part = torch.full((k, pstride), SENT, dtype=torch.float64, device=L.dev)
    bt = dict(period=N, x=stride, c=1, c_elem=k)
    scale = 1.0 / np.sqrt(N)
    out = torch.empty(shape, dtype=TT[dt], device=L.dev)
    nat_.hartley_fused(out, axes, scale, shape=shape, batch=bt,
                       pro=dict(pro, x=d[0, OFF:], dir=dict(r=r[0, OFF:], sc=sc, part=part, pstride=pstride,
                                                            shift=SHIFT, blk0=blk0)))
    d1, p1 = L.down(d), L.down(part)
    assert _same(L.down(sc), SC) and _same(L.down(r), R)
    ref = torch.empty(shape, dtype=TT[dt], device=L.dev)
    nat_.hartley_fused(ref, axes, scale, shape=shape, batch=bt, pro=dict(pro, x=d[0, OFF:]))
    assert _same(L.down(out), L.down(ref)), "transform != the un-carried call on the updated d"
    slots = np.ones(pstride, bool)
    slots[blk0:blk0 + nbd] = False
    assert np.all(p1[:, slots] == SENT), "partials outside the block range written"
    part[:, torch.from_numpy(slots).to(L.dev)] = 0.0
    folded = torch.full((k,), SENT, dtype=torch.float64, device=L.dev)
    assert L.lib.nft_fold_partials(L.P(part), pstride, k, L.P(folded), 1, L.s()) == prim.OK
    fo = L.down(folded)
    seg = slice(OFF, OFF + N)
    for j in range(k):
        what = f"{shape} item {j}"
        assert _same(d1[j, :OFF], D[j, :OFF]) and _same(d1[j, OFF + N:], D[j, OFF + N:]), (what, "padding")
        prim.check_dir_row(dt, N, D[j, seg], R[j, seg], SC[j], d1[j, seg], what)
        if SC[j, DONE] != 0.0:
            assert np.all(p1[j, ~slots] == 0.0) and fo[j] == 0.0, (what, "DONE item's partials")
        else:
            assert_reduction(fo[j], d1[j, seg], d1[j, seg], _dir_chain(grid), what + " d.d", scale=SHIFT)


@pytest.mark.parametrize("r2c", ["0", None], ids=["rows", "default"])
@pytest.mark.parametrize("shape,dt", [((K, 64, 64), 0), ((K, 16, 512), 0), ((K, 64, 64), 1)])
def test_lazy_ring_by_hand(L, shape, dt, r2c, monkeypatch):
    """m = 4 steps of prologue (dir + lazy) and adjoint (cg + lazy) with the
    scalars set by hand between them, then nft_cg_lazy_flush: bitwise the
    same steps without the ring in x, r and d; the recorded alphas finite
    where the step applied and NaN from the trip on.  (K, 16, 512) takes the
    prologue fused with the R2C pass unless NFT_PRO_R2C=0."""
    if r2c is None:
        monkeypatch.delenv("NFT_PRO_R2C", raising=False)
    else:
        monkeypatch.setenv("NFT_PRO_R2C", r2c)
    nat_ = L.nat
    k, grid = shape[0], shape[1:]
    axes = tuple(range(1, len(shape)))
    N = int(np.prod(grid))
    tiles, nbd = nat_.hartley_cg_blocks(shape, axes, TT[dt]), nat_.hartley_dir_blocks(grid)
    assert tiles > 0 and nbd > 0
    rng = np.random.default_rng(31 + N + dt)
    stride = OFF + N + PAD
    m, nslot = 4, 6
    X, R, D = (_grid_rows(rng, k, N, dt) for _ in range(3))
    pro = _folded_prologue(L, shape, dt, rng)
    bw = L.up(_draw(rng, grid, dt))
    # per step and item: gamma, gprev, curv > 0 with alpha = gamma / curv in
    # (0.05, 0.1]: the iterates stay O(1) over the four steps
    SCS = np.zeros((m, k, NS))
    for t in range(m):
        SCS[t, :, GAMMA] = rng.uniform(1.0, 2.0, k)
        SCS[t, :, GPREV] = rng.uniform(1.0, 2.0, k)
        SCS[t, :, CURV] = SCS[t, :, GAMMA] * rng.uniform(10.0, 20.0, k)
        SCS[t, :, LAZY] = t
        SCS[t, :, AUTO] = 1.0
        SCS[t, 2, DONE] = 1.0                   # item 2: stopped from the start
        if t == 2:
            SCS[t, 1, CURV] = 0.0               # item 1 trips at step 2 ...
        if t > 2:
            SCS[t, 1, DONE] = 2.0               # ... and is frozen afterwards
        SCS[t, 5, GAMMA] = -1.0 if t == 1 else SCS[t, 5, GAMMA]     # beta clamped, alpha < 0: one skipped step
    scs = L.up(SCS)
    scale = 1.0 / np.sqrt(N)
    res = {}
    for lazy in (False, True):
        x, r, d = L.up(X), L.up(R), L.up(D)
        sc = torch.zeros((k, NS), dtype=torch.float64, device=L.dev)
        s = torch.empty(shape, dtype=TT[dt], device=L.dev)
        w2 = torch.empty((k, N), dtype=TT[dt], device=L.dev)
        out = torch.full((k, N), SENT, dtype=TT[dt], device=L.dev)
        dpart = torch.zeros((k, nbd), dtype=torch.float64, device=L.dev)
        cpart = torch.zeros((k, 3, tiles), dtype=torch.float64, device=L.dev)
        ring = torch.full((nslot, k, stride), SENT, dtype=TT[dt], device=L.dev)
        alpha = torch.full((k, nslot), SENT, dtype=torch.float64, device=L.dev)
        lz = dict(ring=ring[0, 0, OFF:], sstride=k * stride, alpha=alpha, nslot=nslot) if lazy else None
        parts = []
        for t in range(m):
            sc.copy_(scs[t])
            with nat_.LaunchProfile() as prof:
                nat_.hartley_fused(s, axes, scale, shape=shape, batch=dict(period=N, x=stride, c=1, c_elem=k),
                                   pro=dict(pro, x=d[0, OFF:], dir=dict(r=r[0, OFF:], sc=sc, part=dpart, pstride=nbd,
                                                                        shift=SHIFT, blk0=0, lazy=lz)))
            # which prologue ran: fused with the R2C pass for rows of 512 unless switched off
            labels = {lab for lab, _ in prof.records}
            fused = r2c is None and grid[-1] == 512
            assert ("pro_r2c+dir" in labels) == fused and ("pro_fold+dir" in labels) == (not fused), sorted(labels)
            nat_.hartley_fused(out[0], axes, scale, x=s, epi=dict(a=pro["a"], b=bw, out2=w2), shape=shape,
                               batch=dict(period=N, out=N, out2=N),
                               cg=dict(x=x[0, OFF:], r=r[0, OFF:], d=d[0, OFF:], sc=sc, part=cpart, stride=stride,
                                       shift=SHIFT, nbtot=tiles, blk0=0, lazy=lz))
            parts.append((L.down(dpart).copy(), L.down(cpart)[:, 0].copy()))
        if lazy:
            ringh = L.down(ring)
            assert np.all(ringh[m:] == SENT), "ring slots past the last step written"
            assert np.all(ringh[:, :, :OFF] == SENT) and np.all(ringh[:, :, OFF + N:] == SENT), "ring padding"
            assert _same(L.down(x), X), "the deferred iterate moved x before the flush"
            nat_.cg_lazy_flush(x[0, OFF:], d[0, OFF:], ring[0, 0, OFF:], k * stride, alpha, nslot, m, N, stride, k)
        res[lazy] = (L.down(x), L.down(r), L.down(d), parts, L.down(alpha))
        assert np.all(L.down(out) == SENT)
    for name, a_, b_ in zip("xrd", res[True][:3], res[False][:3]):
        assert _same(a_, b_), f"lazy != eager in {name}"
    for t in range(m):
        assert _same(res[True][3][t][0], res[False][3][t][0]), ("d.d partials", t)
        assert _same(res[True][3][t][1], res[False][3][t][1]), ("r.r partials", t)
    al = res[True][4]
    assert np.all(al[:, m:] == SENT), "alphas past the last step written"
    for j in range(k):
        for t in range(m):
            applies = SCS[t, j, DONE] == 0.0 and prim._guard_ok(SCS[t, j])
            if applies:
                assert al[j, t] == SCS[t, j, GAMMA] / SCS[t, j, CURV], (j, t, al[j, t])
            else:
                assert np.isnan(al[j, t]), (j, t, al[j, t])
    assert not np.any(np.isnan(al[0, :m])) and np.all(np.isnan(al[1, 2:m])) and np.all(np.isnan(al[2, :m]))
    # stopped / tripped items: x, r, d as they entered
    xe, re_, de = res[False][:3]
    assert _same(xe[2], X[2]) and _same(re_[2], R[2]) and _same(de[2], D[2])
    assert not _same(xe[0], X[0]) and not _same(xe[1], X[1])


def test_carried_fold_rejects_bad_stride(L):
    """nft_hartley_fused: fold_ostride < 1 is NFT_ERR_ARG (as nft_los_adjoint_fold)"""
    nat_ = L.nat
    x = L.up(_draw(np.random.default_rng(3), (16, 256), 0))
    part = L.up(_draw(np.random.default_rng(4), (3, 40), 0))
    got = torch.full((3, 2), SENT, dtype=torch.float64, device=L.dev)
    h = torch.full_like(x, SENT)
    for bad in (0, -1):
        with pytest.raises(nat_.NativeError, match="fold_ostride"):
            nat_.hartley_fused(h, (0, 1), 1.0, x=x, fold=(part, 40, 3, got.data_ptr(), bad))
    assert np.all(L.down(got) == SENT) and np.all(L.down(h) == SENT), "a rejected call wrote"
    nat_.hartley_fused(h, (0, 1), 1.0, x=x, fold=(part, 40, 3, got.data_ptr(), 2))
    ref = torch.full((3, 2), SENT, dtype=torch.float64, device=L.dev)
    assert L.lib.nft_fold_partials(L.P(part), 40, 3, L.P(ref), 2, L.s()) == prim.OK
    assert _same(L.down(got), L.down(ref))


def test_los_adjoint_fold_without_boxes(L):
    """nft_los_adjoint_fold on a plan without boxes: no adjoint launch, the
    fold on its own, NFT_OK and `out` untouched (as nft_los_adjoint_batched).
    LOSResponse tiles the whole grid with boxes, so the plan is set by hand."""
    nat_ = L.nat
    plan = nat_.LosPlan()
    plan.H, plan.W, plan.bh, plan.bw, plan.nby, plan.nbx = 16, 16, 16, 16, 1, 1
    plan.nbox, plan.nlos, plan.nitems, plan.nseg = 0, 4, 0, 0
    part = L.up(_draw(np.random.default_rng(5), (3, 40), 0))
    y = L.up(_draw(np.random.default_rng(6), (2, 4), 0))
    out = torch.full((2, 256), SENT, dtype=torch.float64, device=L.dev)
    got = torch.full((3, 2), SENT, dtype=torch.float64, device=L.dev)
    ref = torch.full((3, 2), SENT, dtype=torch.float64, device=L.dev)
    args = (ctypes.byref(plan), L.P(y), None, None, L.P(out), 0, 1.0, 2, 4, 256, L.P(part), 40, 3)
    assert L.lib.nft_los_adjoint_fold(*args, L.P(got), 2, L.s()) == prim.OK
    assert L.lib.nft_fold_partials(L.P(part), 40, 3, L.P(ref), 2, L.s()) == prim.OK
    assert _same(L.down(got), L.down(ref))
    assert np.all(L.down(out) == SENT)
    assert L.lib.nft_los_adjoint_batched(ctypes.byref(plan), L.P(y), None, None, L.P(out), 0, 1.0, 2, 4, 256,
                                         L.s()) == prim.OK
    assert np.all(L.down(out) == SENT)
    assert L.lib.nft_los_adjoint_fold(*args, L.P(got), 0, L.s()) == prim.ERR_ARG
    assert L.lib.nft_los_adjoint_fold(*args[:5], 2, *args[6:], L.P(got), 2, L.s()) == prim.ERR_ARG
