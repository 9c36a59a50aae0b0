"""GPU: the tall-skinny Gram kernels of the block-Lanczos solver
(csrc/nft_eig.hip: nft_gram_dots, nft_gram_axpy) against exact references.

Shapes are the smallest at which the tiling can go wrong.  With T =
nft_gram_tile() the workgroup tile: n in 1, 63, 65, T - 1, T + 1, 2 T + 3 (a
lone element, around a wave, around a tile, three tiles with a ragged tail;
the kernels do not grid-stride, so there is no block cap to pass); m in 1, 2,
9, 33 basis rows; k = 1..8 block rows (every instantiation); row strides n
and n + 5 and a base one element off a 16-byte boundary.

Which load path a call takes (`vec16` below restates the library's rule: both
bases 16-byte aligned and the row strides of operands with more than one row
even): all six n are odd, so
'dense' (stride n) and 'offset' (base off by 8 bytes) take the 8-byte path
and 'padded' (stride n + 5, even) the 16-byte one.  The real-input and the
batch-independence tests add the even n = 2 T + 4, where 'dense' takes the
16-byte path and 'padded' the 8-byte one, and run every layout; each case of
them asserts that it saw both paths, and the cross-path check compares results of
calls whose paths differ.

Exact: integer-valued inputs in [-8, 8] make every product and sum exact in
fp64 (|sum| <= 2 T * 64 + 8 < 2^53), so both kernels must match numpy bitwise
whatever the summation order.
Real inputs (normal draws): |C - C_ref| <= n 2^-53 sum |v_i w_i| with C_ref
from math.fsum -- the standard bound for any summation order -- and
elementwise |dW| <= (m + 1) 2^-53 (|w| + sum_j |t_j v_j|) for the m fmas of
nft_gram_axpy, against an extended-precision reference.
Batch independence: bitwise, as the header promises."""
import ctypes
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

MS = (1, 2, 9, 33)
KS = tuple(range(1, 9))
U = 2.0 ** -53


@pytest.fixture(scope="module")
def nat(dev):
    from nifty_amd import _native
    _native.load()
    return _native


@pytest.fixture(scope="module")
def tile(nat):
    T = int(nat.load().nft_gram_tile())
    assert T >= 64 and nat.load().nft_gram_blocks(T) == 1 and nat.load().nft_gram_blocks(T + 1) == 2
    assert nat.load().nft_gram_workspace(3, 2, 2 * T + 3) == 3 * 2 * 3 * 8
    return T


def lengths(T):
    return (1, 63, 65, T - 1, T + 1, 2 * T + 3)


def rows(a, layout, dev):
    """device (r, n) rows of the host matrix `a`: layout 'dense' (stride n),
    'padded' (stride n + 5) or 'offset' (stride n + 5, base one element off)"""
    r, n = a.shape
    if layout == "dense":
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    buf = torch.full((r * (n + 5) + 2,), 777.0, dtype=torch.float64, device=dev)
    off = 1 if layout == "offset" else 0
    view = buf[off:off + r * (n + 5)].view(r, n + 5)[:, :n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(a)).to(dev))
    if layout == "offset":
        assert view.data_ptr() % 16 == 8
    return view


def ints(rng, shape):
    return rng.integers(-8, 9, size=shape).astype(np.float64)


LAYOUTS = ("dense", "padded", "offset")


def vec16(*views):
    """True where nft_gram_dots / nft_gram_axpy take their 16-byte loads for
    these operands: every base 16-byte aligned, the row stride of every
    operand with more than one row even (the rule of include/nifty_amd.h)"""
    return all(v.data_ptr() % 16 == 0 and (v.shape[0] == 1 or v.stride(0) % 2 == 0) for v in views)


def real_lengths(T):
    """the six lengths plus an even one: with it 'dense' rows are 16-byte rows"""
    return lengths(T) + (2 * T + 4,)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("ni", range(6))
def test_exact_integers_bitwise(nat, tile, dev, ni, layout):
    n = lengths(tile)[ni]
    rng = np.random.default_rng(100 + ni)
    Vh, Wh = ints(rng, (max(MS), n)), ints(rng, (8, n))
    Th = ints(rng, (max(MS), 8))
    for m in MS:
        V = rows(Vh[:m], layout, dev)
        for k in KS:
            W = rows(Wh[:k], layout, dev)
            C = nat.gram_dots(V, W).cpu().numpy()
            assert np.array_equal(C, Vh[:m] @ Wh[:k].T), (n, m, k, "dots")
            Td = torch.from_numpy(np.ascontiguousarray(Th[:m, :k])).to(dev)
            for beta in (1.0, 0.0):
                W2 = rows(Wh[:k], layout, dev)
                nat.gram_axpy(V, Td, W2, beta)
                assert np.array_equal(W2.cpu().numpy(), beta * Wh[:k] + Th[:m, :k].T @ Vh[:m]), (n, m, k, beta)
            if layout != "dense":
                # the padding between the rows is never written
                base = W2._base if W2._base is not None else W2
                flat = base.cpu().numpy().reshape(-1)
                off = 1 if layout == "offset" else 0
                pad = np.ones(flat.size, dtype=bool)
                for b in range(k):
                    pad[off + b * (n + 5): off + b * (n + 5) + n] = False
                assert np.all(flat[pad] == 777.0), (n, m, k)


@pytest.mark.parametrize("ni", range(7))
def test_real_inputs_within_summation_bounds(nat, tile, dev, ni):
    n = real_lengths(tile)[ni]
    rng = np.random.default_rng(200 + ni)
    seen = set()
    for layout in LAYOUTS:
        for m, k in ((1, 1), (2, 3), (9, 8), (33, 5)):
            Vh, Wh, Th = rng.standard_normal((m, n)), rng.standard_normal((k, n)), rng.standard_normal((m, k))
            V, W = rows(Vh, layout, dev), rows(Wh, layout, dev)
            seen.add(vec16(V, W))
            C = nat.gram_dots(V, W).cpu().numpy()
            worst = 0.0
            for j in range(m):
                for b in range(k):
                    ref = math.fsum(Vh[j] * Wh[b])       # products rounded once, their sum exact
                    bound = n * U * float(np.abs(Vh[j] * Wh[b]).sum())
                    worst = max(worst, abs(C[j, b] - ref) / bound)
                    assert abs(C[j, b] - ref) <= bound, (n, m, k, j, b, layout)
            Td = torch.from_numpy(Th).to(dev)
            nat.gram_axpy(V, Td, W, 1.0)
            ld = np.longdouble
            ref = Wh.astype(ld) + Th.astype(ld).T @ Vh.astype(ld)
            bound = (m + 1) * U * (np.abs(Wh) + np.abs(Th).T @ np.abs(Vh))
            err = np.abs(W.cpu().numpy().astype(ld) - ref)
            print(n, m, k, layout, "16-byte" if vec16(V, W) else "8-byte", "dots worst / bound", worst,
                  "axpy worst / bound", float((err / bound).max()))
            assert np.all(err <= bound), (n, m, k, layout)
    assert seen == {True, False}, (n, seen)      # both load paths ran at this n


@pytest.mark.parametrize("ni", (1, 4, 5, 6))
def test_batch_independence_bitwise(nat, tile, dev, ni):
    """column b of a k = 8 call equals the k = 1 call of that vector and the
    same vector at another place of the block: both kernels, every layout,
    hence both load paths at every n; then the results of the layouts against
    each other, which compares the 16-byte path with the 8-byte one"""
    n = real_lengths(tile)[ni]
    rng = np.random.default_rng(300 + ni)
    m = 9
    Vh, Wh, Th = rng.standard_normal((m, n)), rng.standard_normal((8, n)), rng.standard_normal((m, 8))
    seen, C_of, W_of = set(), {}, {}
    for layout in LAYOUTS:
        V = rows(Vh, layout, dev)
        Wd8 = rows(Wh, layout, dev)
        path = vec16(V, Wd8)
        seen.add(path)
        C8 = nat.gram_dots(V, Wd8)
        W8 = rows(Wh, layout, dev)
        nat.gram_axpy(V, torch.from_numpy(Th).to(dev), W8, 1.0)
        C_of[layout], W_of[layout] = (path, C8), (path, W8.contiguous())
        for b in (0, 3, 7):
            W1in = rows(Wh[b:b + 1], layout, dev)
            assert vec16(V, W1in) == path
            C1 = nat.gram_dots(V, W1in)
            assert torch.equal(C8[:, b], C1[:, 0]), (n, layout, b)
            W1 = rows(Wh[b:b + 1], layout, dev)
            nat.gram_axpy(V, torch.from_numpy(np.ascontiguousarray(Th[:, b:b + 1])).to(dev), W1, 1.0)
            assert torch.equal(W8[b], W1[0]), (n, layout, b)
            # the same vector at place 7 - b of a block of 5 .. 8 other rows
            for k in (5, 8):
                p = (7 - b) % k
                Wp, Tp = rng.standard_normal((k, n)), rng.standard_normal((m, k))
                Wp[p], Tp[:, p] = Wh[b], Th[:, b]
                Cp = nat.gram_dots(V, rows(Wp, layout, dev))
                assert torch.equal(Cp[:, p], C1[:, 0]), (n, layout, b, k)
                Wd = rows(Wp, layout, dev)
                nat.gram_axpy(V, torch.from_numpy(Tp).to(dev), Wd, 1.0)
                assert torch.equal(Wd[p], W1[0]), (n, layout, b, k)
    # the two load paths give the same bits: every pair of layouts, at least
    # one pair of which differs in its path
    assert seen == {True, False}, (n, seen)
    crossed = 0
    for la in LAYOUTS:
        for lb in LAYOUTS:
            if la < lb:
                crossed += C_of[la][0] != C_of[lb][0]
                assert torch.equal(C_of[la][1], C_of[lb][1]), (n, la, lb, "dots")
                assert torch.equal(W_of[la][1], W_of[lb][1]), (n, la, lb, "axpy")
    assert crossed >= 1


def test_bad_arguments_launch_nothing(nat, dev):
    lib = nat.load()
    P = lambda t: ctypes.c_void_p(t.data_ptr())     # noqa: E731
    n, m, k = 100, 4, 3
    V = torch.ones((m, n), dtype=torch.float64, device=dev)
    W = torch.ones((8, n), dtype=torch.float64, device=dev)
    T = torch.ones((m, 8), dtype=torch.float64, device=dev)
    C = torch.full((m * 9,), -5.0, dtype=torch.float64, device=dev)
    ws = torch.zeros(m * 9 * 8, dtype=torch.uint8, device=dev)
    s = nat.stream_ptr()

    def dots(m=m, k=k, dtype=0, n=n, vs=n, wsb=ws.numel(), C=C):
        return lib.nft_gram_dots(P(V), vs, m, P(W), n, k, n, dtype, P(C) if C is not None else None, P(ws),
                                 ctypes.c_size_t(wsb), s)

    def axpy(m=m, k=k, dtype=0, beta=1.0, W=W, T=T):
        return lib.nft_gram_axpy(P(V), n, m, P(T) if T is not None else None, P(W), n, k, n, dtype, beta, s)

    assert dots() == 0 and axpy() == 0
    torch.cuda.synchronize()
    C.fill_(-5.0)
    W.fill_(1.0)
    for bad in (dict(dtype=1), dict(k=0), dict(k=9), dict(m=0)):
        assert dots(**bad) == -1, bad
        assert b"nft_gram_dots" in lib.nft_last_error()
        assert axpy(**bad) == -1, bad
        assert b"nft_gram_axpy" in lib.nft_last_error()
    assert dots(n=0) == -1 and dots(vs=n - 1) == -1 and dots(wsb=m * k * 8 - 1) == -1 and dots(C=None) == -1
    assert axpy(beta=0.5) == -1 and axpy(T=None) == -1
    assert axpy(W=V) == -1                       # W may not alias V
    torch.cuda.synchronize()
    assert torch.all(C == -5.0) and torch.all(W == 1.0)
    # the wrappers refuse host tensors: there is no CPU fallback
    with pytest.raises(nat.NativeError):
        nat.gram_dots(V.cpu(), W[:k])
    with pytest.raises(nat.NativeError):
        nat.gram_axpy(V, T[:, :k].contiguous(), W[:k].cpu())
    with pytest.raises(nat.NativeError):
        nat.gram_dots(V.float(), W[:k].float())
