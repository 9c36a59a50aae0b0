"""GPU: every kernel template and instantiation of csrc/nft_cf.hip (power-bin
gather, scatter, mirror fold) against the exact references of
tests/bin_cases.py -- the documented summation order restated in numpy in the
kernel's storage type -- bit for bit, and additionally within the order-free
longdouble bound n * u * sum|terms| (which localises a failure; the bitwise
check is the requirement).

The layouts and fold shapes, and the regimes they are there for (bins of 63 /
64 / 65 positions, long and short bins crossing a chunk end at every chunk
size, chunks that own no bin, more than 512 bins in a chunk, rows longer than
a row kernel's first round), are asserted on the host by test_bin_cases.py,
which also shows that each reference with one detail turned wrong differs
bitwise on these inputs.

Kernel template, instantiation -> the test that holds it to an exact reference
(every one in T = double and float):
  bin_gather_kernel<T>                      test_gather, test_gather_folded_natural_grid,
                                            test_distributor_on_one_space_of_a_product_domain
  bin_scatter_kernel<T>                     test_scatter_generic, test_distributor_on_one_space_...
  bin_scatter_chunk<T, 1, false>            test_scatter_chunk (no table / table / gpix + gslot)
  bin_scatter_chunk<T, 1, true>             test_scatter_folded (no table / table)
  bin_scatter_il<T, 2 | 4 | 8, 1024 | 512 | 256>
                                            test_scatter_interleaved[*-2 | 4 | 8-*]
  bin_fold_kernel<T, unsigned>              test_fold_full, test_fold_full_wide_index[f32-32511-24]
  bin_fold_kernel<T, long long>             test_fold_full_wide_index[f32-32512-24], [f64-32512-48]
  bin_fold_half_flat_planar<T>              test_fold_half (NFT_FOLD_FLAT unset)
  bin_fold_half_rows<T>                     test_fold_half (NFT_FOLD_FLAT=0)
  bin_fold_half_flat<T, 1 | 2 | 4 | 8>      test_fold_half_sorted[*-pre] (NFT_FOLD_FLAT unset):
                                            PRE = 1: pre 1; 2: pre 2; 4: pre 3, 4; 8: pre 5..8
                                            (float: pre 1, 2, 3, 4, 8)
  bin_fold_half_sorted<T, 1 | 2 | 4 | 8>    the same cases, NFT_FOLD_FLAT=0
bin_scatter_chunk's K > 1 is instantiated by no entry point.

Every output is NaN before the call and sits between NaN guard elements:
afterwards no NaN remains inside and every guard is still NaN.  Every index
array handed to a kernel is checked on the host first (assert_valid_csr).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bin_cases as bc
from conftest import golden

pytestmark = pytest.mark.gpu

GUARD = 16      # elements; keeps the output 64-byte aligned, as the package's own buffers are
NP = {"f64": np.float64, "f32": np.float32}
TT = {"f64": torch.float64, "f32": torch.float32}
NITEM = 8       # items of the shared inputs; a test of pre items uses the first pre
ERR_ARG = -1    # NFT_ERR_ARG (include/nifty_amd.h)


@pytest.fixture(scope="module")
def nat(dev):
    import nifty_amd  # noqa: F401
    from nifty_amd import _native
    _native.load()
    return _native


class Guarded:
    """a NaN-filled output of `shape` between two runs of NaN guard elements"""

    def __init__(self, dev, dt, shape):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=TT[dt], device=dev)
        self.t = self.buf[GUARD:GUARD + n].view(shape)
        assert self.t.is_contiguous() and self.t.data_ptr() % 16 == 0

    def guards_intact(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf[:GUARD]).all() and torch.isnan(self.buf[self.buf.numel() - GUARD:]).all())

    def result(self):
        assert self.guards_intact(), "a guard element was written"
        assert not torch.isnan(self.t).any(), "an output element was not written"
        return self.t.cpu().numpy()

    def untouched(self):
        torch.cuda.synchronize()
        return bool(torch.isnan(self.buf).all())


def _up(a, dev):
    """upload a copy (the shared inputs are read-only)"""
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(dev)


def _exact(got, ref):
    assert got.dtype == ref.dtype and got.shape == ref.shape
    np.testing.assert_array_equal(got, ref)


def _bounded(got, ld, dt):
    ref, n, sa = ld
    assert np.all(np.abs(got.astype(np.longdouble) - ref) <= bc.bound(n, sa, NP[dt]))


# ------------------------------------------------- shared inputs, references
@functools.lru_cache(maxsize=None)
def host_layout(name):
    pindex, nb = bc.layout(name)
    perm, offs = bc.csr(pindex, nb)
    bc.assert_valid_csr(pindex, perm, offs, nb)
    assert len(pindex) < 2 ** 31 and nb < 2 ** 31
    return pindex, nb, perm, offs


@functools.lru_cache(maxsize=None)
def dev_layout(name, dev):
    pindex, nb, perm, offs = host_layout(name)
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a).astype(np.int32)).to(dev)   # noqa: E731
    return i32(pindex), i32(perm), i32(offs)


@functools.lru_cache(maxsize=None)
def planar_x(name, dt):
    """(NITEM, npix) items of a layout"""
    x = bc.values((NITEM, len(host_layout(name)[0])), NP[dt], 101)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_seq(name, dt):
    _, _, perm, offs = host_layout(name)
    return bc.scatter_seq(planar_x(name, dt)[:, :, None], perm, offs)[:, :, 0]


@functools.lru_cache(maxsize=None)
def ref_wave(name, dt):
    _, _, perm, offs = host_layout(name)
    return bc.scatter_wave(planar_x(name, dt), perm, offs)


@functools.lru_cache(maxsize=None)
def ref_planar_ld(name, dt):
    pindex, nb, _, _ = host_layout(name)
    s, n, sa = bc.scatter_ld(planar_x(name, dt)[:, :, None], pindex, nb)
    return s[:, :, 0], n[None, :], sa[:, :, 0]


@functools.lru_cache(maxsize=None)
def generic_x(name, dt):
    """(3, npix, 5): the generic scatter's input, (pre, post) blocks cut from it"""
    x = bc.values((3, len(host_layout(name)[0]), 5), NP[dt], 102)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def ref_generic(name, dt):
    pindex, nb, perm, offs = host_layout(name)
    s, n, sa = bc.scatter_ld(generic_x(name, dt), pindex, nb)
    return bc.scatter_seq(generic_x(name, dt), perm, offs), (s, n[None, :, None], sa)


@functools.lru_cache(maxsize=None)
def fold_inputs(shape, dt):
    w = bc.values((NITEM,) + shape, NP[dt], 103)
    H = bc.values((NITEM,) + bc.half_shape(shape), NP[dt], 104)
    w.setflags(write=False)
    H.setflags(write=False)
    return w, H


@functools.lru_cache(maxsize=None)
def ref_fold_full(shape, dt):
    w, _ = fold_inputs(shape, dt)
    return bc.fold_full(w), bc.fold_ld(w, shape)


@functools.lru_cache(maxsize=None)
def ref_fold_half(shape, dt):
    _, H = fold_inputs(shape, dt)
    return bc.fold_half(H, shape), bc.fold_ld(H, shape, half=True)


def _cut(ld, pre):
    s, n, sa = ld
    return s[:pre], n, sa[:pre]


def _chunk_table(name, ch, dev):
    from nifty_amd.operators.distributors import _chunk_bins
    pindex, nb, _, offs = host_layout(name)
    cb = _chunk_bins(offs, nb, len(pindex), ch)
    np.testing.assert_array_equal(cb, bc.chunk_bins_def(offs, nb, len(pindex), ch))
    return torch.from_numpy(cb).to(dev)


def test_chunk_sizes_are_the_library_s(nat):
    lib = nat.load()
    assert lib.nft_bin_chunk() == bc.CH_PLAIN
    for pre, ch in bc.CH_IL.items():
        assert lib.nft_bin_scatter_il_chunk(pre) == ch
    assert lib.nft_bin_scatter_il_chunk(3) == 0


# ------------------------------------------------------------------- gather
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre,post", [(1, 1), (3, 1), (1, 5), (3, 5)])
@pytest.mark.parametrize("name", ["A", "E"])
def test_gather(nat, dev, name, pre, post, dt):
    pindex, nb, _, _ = host_layout(name)
    src = bc.values((pre, nb, post), NP[dt], 110)
    out = Guarded(dev, dt, (pre, len(pindex), post))
    nat.bin_gather(torch.from_numpy(src).to(dev), dev_layout(name, dev)[0], out.t, pre, len(pindex), nb, post)
    _exact(out.result(), bc.gather(src, pindex, pre, nb, post))


@pytest.mark.parametrize("dt", ["f64", "f32"])
def test_gather_folded_natural_grid(nat, dev, dt):
    import nifty_amd as ift
    from nifty_amd.operators.distributors import BinIndex
    shape, k = (64, 64), 3
    grid = np.asarray(ift.PowerSpace(ift.RGSpace(shape, harmonic=True)).pindex)
    nb = int(grid.max()) + 1
    bi = BinIndex(grid, nb, dev, fold=True)
    assert bi.fold is not None
    cells = np.ascontiguousarray(grid[:33, :33]).ravel()
    np.testing.assert_array_equal(bi.fold["pindex"].cpu().numpy(), cells)
    src = bc.values((nb, k), NP[dt], 111)
    got = bi.gather_folded(torch.from_numpy(src).to(dev), k, interleaved=True)
    _exact(got.cpu().numpy(), bc.gather(src, cells, 1, nb, k)[0])
    srcp = np.ascontiguousarray(src.T)
    got = bi.gather_folded(torch.from_numpy(srcp).to(dev), k, interleaved=False)
    _exact(got.cpu().numpy(), bc.gather(srcp, cells, k, nb, 1)[:, :, 0])


# ------------------------------------------------------------------ scatter
@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre,post", [(1, 5), (3, 5), (2, 2)])
@pytest.mark.parametrize("name", ["A", "B2", "E"])
def test_scatter_generic(nat, dev, name, pre, post, dt):
    """bin_scatter_kernel (post != 1)"""
    pindex, nb, _, _ = host_layout(name)
    _, perm, offs = dev_layout(name, dev)
    x = np.ascontiguousarray(generic_x(name, dt)[:pre, :, :post])
    ref, (s, n, sa) = ref_generic(name, dt)
    out = Guarded(dev, dt, (pre, nb, post))
    nat.bin_scatter(_up(x, dev), perm, offs, out.t, pre, len(pindex), nb, post)
    got = out.result()
    _bounded(got, (s[:pre, :, :post], n, sa[:pre, :, :post]), dt)
    _exact(got, np.ascontiguousarray(ref[:pre, :, :post]))


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre", [1, 3])
@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_scatter_chunk(nat, dev, name, pre, dt):
    """bin_scatter_chunk<T, 1, false>: the kernel's own chunk search, the
    chunk -> first bin table, and the pixel-ordered gathers"""
    pindex, nb, hperm, _ = host_layout(name)
    _, perm, offs = dev_layout(name, dev)
    x = _up(planar_x(name, dt)[:pre], dev)
    cb = _chunk_table(name, bc.CH_PLAIN, dev)
    gpix, gslot = bc.pixel_order(hperm, bc.CH_PLAIN)
    assert np.array_equal(np.sort(gpix), np.arange(len(hperm))) and (len(gslot) == 0 or gslot.max() < bc.CH_PLAIN)
    gp = torch.from_numpy(gpix).to(dev)
    gs = torch.from_numpy(gslot.view(np.int16)).to(dev)        # the same bytes
    for order in (None, (None, None, cb), (gp, gs, cb)):
        out = Guarded(dev, dt, (pre, nb))
        nat.bin_scatter(x, perm, offs, out.t, pre, len(pindex), nb, 1, order=order)
        got = out.result()
        _bounded(got, _cut(ref_planar_ld(name, dt), pre), dt)
        _exact(got, ref_seq(name, dt)[:pre])
    for order in ((gp, None, cb), (None, gs, cb)):
        out = Guarded(dev, dt, (pre, nb))
        with pytest.raises(nat.NativeError, match=r"\(-1\): nft_bin_scatter_ordered"):
            nat.bin_scatter(x, perm, offs, out.t, pre, len(pindex), nb, 1, order=order)
        assert out.untouched()


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre", [1, 3, 5])
@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_scatter_folded(nat, dev, name, pre, dt):
    """bin_scatter_chunk<T, 1, true>: bins above 64 positions one wave each"""
    pindex, nb, _, _ = host_layout(name)
    _, perm, offs = dev_layout(name, dev)
    x = _up(planar_x(name, dt)[:pre], dev)
    for cb in (None, _chunk_table(name, bc.CH_PLAIN, dev)):
        out = Guarded(dev, dt, (pre, nb))
        nat.bin_scatter_folded(x, perm, offs, out.t, pre, len(pindex), nb, chunk_bins=cb)
        got = out.result()
        _bounded(got, _cut(ref_planar_ld(name, dt), pre), dt)
        _exact(got, ref_wave(name, dt)[:pre])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre", [2, 4, 8])
@pytest.mark.parametrize("name", bc.LAYOUTS)
def test_scatter_interleaved(nat, dev, name, pre, dt):
    """bin_scatter_il<T, PRE, CH>: input (npix, pre); row p is bitwise the
    folded scatter of item p"""
    pindex, nb, _, _ = host_layout(name)
    _, perm, offs = dev_layout(name, dev)
    xp = np.ascontiguousarray(planar_x(name, dt)[:pre])
    xi = _up(xp.T, dev)
    fol = Guarded(dev, dt, (pre, nb))
    nat.bin_scatter_folded(_up(xp, dev), perm, offs, fol.t, pre, len(pindex), nb)
    fol = fol.result()
    for cb in (None, _chunk_table(name, bc.CH_IL[pre], dev)):
        out = Guarded(dev, dt, (pre, nb))
        nat.bin_scatter_il(xi, perm, offs, out.t, pre, len(pindex), nb, chunk_bins=cb)
        got = out.result()
        _bounded(got, _cut(ref_planar_ld(name, dt), pre), dt)
        _exact(got, ref_wave(name, dt)[:pre])
        _exact(got, fol)


# -------------------------------------------------------------------- folds
def _flat_launches(monkeypatch):
    """NFT_FOLD_FLAT unset (one output per thread) and "0" (one workgroup per row)"""
    for flat in (None, "0"):
        if flat is None:
            monkeypatch.delenv("NFT_FOLD_FLAT", raising=False)
        else:
            monkeypatch.setenv("NFT_FOLD_FLAT", flat)
        yield flat


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre", [1, 3])
@pytest.mark.parametrize("shape", bc.FOLD_SHAPES)
def test_fold_full(nat, dev, shape, pre, dt):
    """bin_fold_kernel<T, unsigned>"""
    w, _ = fold_inputs(shape, dt)
    ref, ld = ref_fold_full(shape, dt)
    out = Guarded(dev, dt, (pre,) + bc.cell_shape(shape))
    nat.bin_fold(_up(w[:pre], dev), out.t, pre, shape)
    got = out.result()
    _bounded(got, _cut(ld, pre), dt)
    _exact(got, ref[:pre])


@pytest.mark.parametrize("dt", ["f64", "f32"])
@pytest.mark.parametrize("pre", [1, 3, 5])
@pytest.mark.parametrize("shape", bc.FOLD_SHAPES)
def test_fold_half(nat, dev, shape, pre, dt, monkeypatch):
    """bin_fold_half_flat_planar and bin_fold_half_rows"""
    _, H = fold_inputs(shape, dt)
    ref, ld = ref_fold_half(shape, dt)
    Ht = _up(H[:pre], dev)
    for flat in _flat_launches(monkeypatch):
        out = Guarded(dev, dt, (pre,) + bc.cell_shape(shape))
        nat.bin_fold_half(Ht, out.t, pre, shape)
        got = out.result()
        _bounded(got, _cut(ld, pre), dt)
        _exact(got, ref[:pre])


SORTED_PRE = [("f64", p) for p in range(1, 9)] + [("f32", p) for p in (1, 2, 3, 4, 8)]


@pytest.mark.parametrize("dt,pre", SORTED_PRE)
@pytest.mark.parametrize("shape", bc.FOLD_SHAPES)
def test_fold_half_sorted(nat, dev, shape, dt, pre, monkeypatch):
    """bin_fold_half_flat<T, PRE> and bin_fold_half_sorted<T, PRE>, PRE in
    1, 2, 4, 8; pre = 3, 5, 6, 7 take the scalar stores of pre < PRE; with
    and without the bin-sorted cell positions"""
    _, H = fold_inputs(shape, dt)
    Hp = np.ascontiguousarray(H[:pre])
    Ht = _up(Hp, dev)
    nf = int(np.prod(bc.cell_shape(shape)))
    cpos = bc.cell_perm(nf, 120)
    assert np.array_equal(np.sort(cpos), np.arange(nf))
    _, ld = ref_fold_half(shape, dt)
    for cp in (None, cpos):
        ref = bc.fold_half_sorted(Hp, shape, cp)
        cpt = None if cp is None else torch.from_numpy(cp).to(dev)
        for flat in _flat_launches(monkeypatch):
            out = Guarded(dev, dt, (nf * pre,))
            nat.bin_fold_half_sorted(Ht, out.t, cpt, pre, shape)
            got = out.result()
            # back in cell order: the planar fold's sums, within the bound
            back = got.reshape(nf, pre) if cp is None else got.reshape(nf, pre)[cp]
            _bounded(np.ascontiguousarray(back.T).reshape((pre,) + bc.cell_shape(shape)), _cut(ld, pre), dt)
            _exact(got, ref)


def test_fold_scatter_natural_grid_end_to_end(nat, dev):
    """BinIndex.fold_into(half=True) + scatter_from on a grid whose folded
    bins exceed 64 cells: bitwise scatter_wave(fold_half(.)) with the plan's
    own perm / offsets, and within n * u * sum|w| of the bin sums of the
    un-paired w on the full grid (n: the bin's grid pixels)"""
    import nifty_amd as ift
    from nifty_amd.operators.distributors import BinIndex, _ILFold
    shape, pre, dt = (64, 64, 64), 2, "f64"
    grid = np.asarray(ift.PowerSpace(ift.RGSpace(shape, harmonic=True)).pindex)
    nb = int(grid.max()) + 1
    bi = BinIndex(grid, nb, dev, fold=True)
    f = bi.fold
    assert f is not None and BinIndex.IL
    perm, offs = f["perm"].cpu().numpy().astype(np.int64), f["offsets"].cpu().numpy().astype(np.int64)
    cells = np.ascontiguousarray(grid[:33, :33, :33]).ravel()
    bc.assert_valid_csr(cells, perm, offs, nb)
    assert int(np.diff(offs).max()) > bc.LONGB
    w = bc.values((pre,) + shape, NP[dt], 130)
    H = bc.pair_sums(w)
    wf = Guarded(dev, dt, (f["nf"], pre))
    src = bi.fold_into(torch.from_numpy(H).to(dev), wf.t, pre, half=True)
    assert isinstance(src, _ILFold)
    out = Guarded(dev, dt, (pre, nb))
    bi.scatter_from(src, out.t, pre)
    _exact(wf.result(), bc.fold_half_sorted(H, shape).reshape(f["nf"], pre))
    got = out.result()
    s, n, sa = bc.scatter_ld(w.reshape(pre, -1, 1), grid.ravel(), nb)
    _bounded(got, (s[:, :, 0], n[None, :], sa[:, :, 0]), dt)
    _exact(got, bc.scatter_wave(bc.fold_half(H, shape).reshape(pre, -1), perm, offs))


# ---------------------------------------------------------- wide-index fold
def _fold_torch(w):
    """mirror fold of (s, n0, n1) over both axes in torch (exact for small integers)"""
    for ax in (2, 1):
        n = w.shape[ax]
        h = n // 2 + 1
        q = torch.arange(h, device=w.device)
        two = ((q != 0) & (n - q != q)).to(w.dtype)
        w = w.narrow(ax, 0, h) + w.index_select(ax, (n - q) % n) * (two if ax == 2 else two[:, None])
    return w


@pytest.mark.parametrize("dt,pre,need_gb", [("f32", 32511, 24), ("f32", 32512, 24), ("f64", 32512, 48)])
def test_fold_full_wide_index(nat, dev, dt, pre, need_gb):
    """bin_fold_kernel<T, long long> starts at pre * nin >= 2^31 - 2^24:
    (256, 256) with pre = 32512 is exactly there, 32511 the last 32-bit
    launch.  Small integers made on the device, so every sum is exact; the
    reference is torch's, slab by slab."""
    shape = (256, 256)
    nin, nout = 256 * 256, 129 * 129
    assert (pre * nin >= 2 ** 31 - 2 ** 24) == (pre == 32512)
    if torch.cuda.mem_get_info(dev)[0] < need_gb * 2 ** 30:
        pytest.skip(f"needs {need_gb} GB of free device memory")
    slab = 1024
    w = torch.empty((pre, nin), dtype=TT[dt], device=dev)
    for p0 in range(0, pre, slab):
        p1 = min(pre, p0 + slab)
        lin = torch.arange(p0 * nin, p1 * nin, dtype=torch.int64, device=dev)
        w[p0:p1] = ((lin * 2654435761 % 251) - 125).to(TT[dt]).view(p1 - p0, nin)
        del lin
    out = Guarded(dev, dt, (pre, nout))
    nat.bin_fold(w, out.t, pre, shape)
    assert out.guards_intact()
    for p0 in range(0, pre, slab):
        p1 = min(pre, p0 + slab)
        ref = _fold_torch(w[p0:p1].view(p1 - p0, 256, 256)).reshape(p1 - p0, nout)
        assert torch.equal(out.t[p0:p1], ref), (p0, p1)
    del w, out, ref
    torch.cuda.empty_cache()


# ------------------------------------------------- argument and empty paths
def _last(nat):
    return nat.load().nft_last_error().decode()


def test_empty_grid_gives_zeros(nat, dev):
    """npix = 0 with nbins > 0, all three chunked scatters"""
    nb = 5
    offs = torch.zeros(nb + 1, dtype=torch.int32, device=dev)
    one = torch.zeros(1, dtype=torch.int32, device=dev)         # a valid pointer; no element is read
    for dt in ("f64", "f32"):
        x = torch.zeros(8, dtype=TT[dt], device=dev)
        for call, pre in ((lambda o: nat.bin_scatter(x, one, offs, o, 3, 0, nb, 1), 3),
                          (lambda o: nat.bin_scatter_folded(x, one, offs, o, 3, 0, nb), 3),
                          (lambda o: nat.bin_scatter_il(x, one, offs, o, 4, 0, nb), 4)):
            out = Guarded(dev, dt, (pre, nb))
            call(out.t)
            assert np.all(out.result() == 0)


def test_nothing_to_do_writes_nothing(nat, dev):
    """nbins = 0 / pre = 0 / npix = 0: OK, nothing written"""
    offs0 = torch.zeros(1, dtype=torch.int32, device=dev)
    offs = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)
    perm = torch.arange(4, dtype=torch.int32, device=dev)
    for dt in ("f64", "f32"):
        x = torch.ones(16, dtype=TT[dt], device=dev)
        out = Guarded(dev, dt, (4,))
        nat.bin_scatter(x, perm, offs0, out.t, 1, 4, 0, 1)
        nat.bin_scatter(x, perm, offs0, out.t, 1, 4, 0, 2)
        nat.bin_scatter_folded(x, perm, offs0, out.t, 1, 4, 0)
        nat.bin_scatter_il(x, perm, offs0, out.t, 2, 4, 0)
        nat.bin_scatter(x, perm, offs, out.t, 0, 4, 2, 1)
        nat.bin_scatter(x, perm, offs, out.t, 0, 4, 2, 3)
        nat.bin_gather(x, perm, out.t, 0, 4, 4, 1)
        nat.bin_gather(x, perm, out.t, 1, 0, 4, 1)
        nat.bin_fold(x, out.t, 0, (4,))
        nat.bin_fold_half(x, out.t, 0, (4,))
        assert out.untouched()


def test_argument_errors(nat, dev):
    """host code only: every call below returns before a launch"""
    lib = nat.load()
    p, st = nat.ptr, nat.stream_ptr
    x = torch.ones(64, dtype=torch.float64, device=dev)
    out = Guarded(dev, "f64", (64,))
    perm = torch.arange(4, dtype=torch.int32, device=dev)
    offs = torch.tensor([0, 2, 4], dtype=torch.int32, device=dev)

    def sh(*s):
        return (ctypes.c_int64 * len(s))(*s)

    def err(status, name):
        assert status == ERR_ARG and _last(nat).startswith(name), (status, _last(nat))

    # item counts
    err(lib.nft_bin_scatter_il(p(x), p(perm), p(offs), None, p(out.t), 3, 4, 2, 0, st()), "nft_bin_scatter_il")
    err(lib.nft_bin_scatter_il(p(x), p(perm), p(offs), None, p(out.t), 0, 4, 2, 0, st()), "nft_bin_scatter_il")
    err(lib.nft_bin_scatter_folded(p(x), p(perm), p(offs), None, p(out.t), 0, 4, 2, 0, st()),
        "nft_bin_scatter_folded")
    err(lib.nft_bin_fold_half_sorted(p(x), p(out.t), None, 9, 1, sh(4), 0, st()), "nft_bin_fold_half_sorted")
    err(lib.nft_bin_fold_half_sorted(p(x), p(out.t), None, 0, 1, sh(4), 0, st()), "nft_bin_fold_half_sorted")
    # shapes: ndim = 4, ndim = 0, a zero extent
    for fn, name in ((lib.nft_bin_fold, "nft_bin_fold"), (lib.nft_bin_fold_half, "nft_bin_fold_half")):
        err(fn(p(x), p(out.t), 1, 4, sh(2, 2, 2, 2), 0, st()), name)
        err(fn(p(x), p(out.t), 1, 0, sh(2), 0, st()), name)
        err(fn(p(x), p(out.t), 1, 2, sh(4, 0), 0, st()), name)
        err(fn(p(x), p(out.t), 1, 1, sh(4), 2, st()), name)            # dtype code 2
    err(lib.nft_bin_fold_half_sorted(p(x), p(out.t), None, 1, 4, sh(2, 2, 2, 2), 0, st()), "nft_bin_fold_half_sorted")
    err(lib.nft_bin_fold_half_sorted(p(x), p(out.t), None, 1, 2, sh(0, 4), 0, st()), "nft_bin_fold_half_sorted")
    err(lib.nft_bin_fold_half_sorted(p(x), p(out.t), None, 1, 1, sh(4), 2, st()), "nft_bin_fold_half_sorted")
    # dtype code 2
    err(lib.nft_bin_gather(p(x), p(perm), p(out.t), 1, 4, 4, 1, 2, st()), "nft_bin_gather")
    err(lib.nft_bin_scatter(p(x), p(perm), p(offs), p(out.t), 1, 4, 2, 1, 2, st()), "nft_bin_scatter")
    err(lib.nft_bin_scatter(p(x), p(perm), p(offs), p(out.t), 1, 4, 2, 3, 2, st()), "nft_bin_scatter")
    err(lib.nft_bin_scatter_folded(p(x), p(perm), p(offs), None, p(out.t), 1, 4, 2, 2, st()),
        "nft_bin_scatter_folded")
    err(lib.nft_bin_scatter_il(p(x), p(perm), p(offs), None, p(out.t), 2, 4, 2, 2, st()), "nft_bin_scatter_il")
    # missing index arrays
    err(lib.nft_bin_scatter_folded(p(x), None, p(offs), None, p(out.t), 1, 4, 2, 0, st()), "nft_bin_scatter_folded")
    err(lib.nft_bin_scatter_il(p(x), p(perm), None, None, p(out.t), 2, 4, 2, 0, st()), "nft_bin_scatter_il")
    assert out.untouched()


# ------------------------------------------- the operators on a middle space
@pytest.mark.parametrize("tag", ["mid", "first", "last"])
def test_distributor_on_one_space_of_a_product_domain(nat, dev, tag):
    """PowerDistributor / DOFDistributor with pre > 1 and / or post > 1
    (bin_gather_kernel, bin_scatter_kernel) against the reference's times and
    adjoint_times (tests/golden/distributor.npz), bit for bit: the adjoint
    sums in ascending pixel order, as the reference's special_add_at
    (np.bincount) does"""
    import nifty_amd as ift
    G = golden("distributor.npz")
    h = ift.RGSpace(tuple(int(s) for s in G["shape"]), distances=tuple(G["pos_dist"])).get_default_codomain()
    a, b = ift.UnstructuredDomain(int(G["na"])), ift.UnstructuredDomain(int(G["nb"]))
    dom, space = {"mid": ((a, h, b), 1), "first": ((h, b), 0), "last": ((a, h), 1)}[tag]
    pd = ift.PowerDistributor(ift.DomainTuple.make(dom), space=space)
    assert (pd._pre, pd._post) == {"mid": (3, 4), "first": (1, 4), "last": (3, 1)}[tag]
    np.testing.assert_array_equal(np.asarray(pd._dofdex_np), G["pindex"])
    x, y = G[f"{tag}_x"], G[f"{tag}_y"]
    assert x.shape == pd.domain.shape and y.shape == pd.target.shape
    got = pd(ift.makeField(pd.domain, x)).val.cpu().numpy()
    np.testing.assert_array_equal(got, G[f"{tag}_times"])
    got = pd.adjoint_times(ift.makeField(pd.target, y)).val.cpu().numpy()
    np.testing.assert_array_equal(got, G[f"{tag}_adjoint_times"])
    dd = ift.DOFDistributor(ift.makeField(h, G["pindex"]), target=ift.DomainTuple.make(dom), space=space)
    np.testing.assert_array_equal(dd.adjoint_times(ift.makeField(dd.target, y)).val.cpu().numpy(),
                                  G[f"{tag}_adjoint_times"])
    np.testing.assert_array_equal(dd(ift.makeField(dd.domain, x)).val.cpu().numpy(), G[f"{tag}_times"])
    for op in (pd, dd):
        u = ift.from_random(op.domain, "normal")
        v = ift.from_random(op.target, "normal")
        l, r = op.times(u).s_vdot(v), u.s_vdot(op.adjoint_times(v))
        assert abs(l - r) <= 1e-12 * max(abs(l), abs(r), 1.)
